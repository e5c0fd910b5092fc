// The C++ host adapter's plaintext methods (gemini-seal_amd/host/evaluator.hpp: transform_to_ntt(_inplace) of a
// plaintext, mod_switch_to(_inplace) / mod_switch_to_next(_inplace) of an NTT-form plaintext). On a host-only context:
// the reference's host checks and messages. With a device (argv[1] = ordinal): digests of the outputs, which the Python
// test compares with the C ABI's outputs on the same inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

int main(int argc, char **argv)
{
    const auto throws_invalid = [](auto &&f, const char *msg) { return throws_exact<std::invalid_argument>(f, msg); };
    // cfg1 of BASELINE.json: BFV N=4096, {36,36,37}, t = 786433
    const std::uint64_t mods[3] = { 68719230977ULL, 68719403009ULL, 137438822401ULL };
    const std::uint64_t t = 786433;
    const std::size_t n = 4096, cc = 3000;
    sealhip_params p{ SEALHIP_SCHEME_BFV, 12, 3, 1, mods, t, SEALHIP_MODE_PARITY, argc > 1 ? std::atoi(argv[1]) : -1 };
    try
    {
        Context ctx(p);
        Evaluator<HostCiphertext> ev(ctx);
        std::uint64_t state = 0x9A17 + 5;
        std::vector<std::uint64_t> plain(cc);
        for (auto &v : plain)
            v = splitmix(state) % t;
        if (p.device < 0)
        {
            bool ok = true;
            std::vector<std::uint64_t> out(3 * n), big(n + 1, 0), bad = plain;
            bad[17] = t;
            bool ntt = false, ntt_true = true;
            ok &= throws_invalid([&] { ev.transform_to_ntt(bad.data(), bad.size(), 2, out.data()); },
                                 "plain is not valid for encryption parameters");
            ok &= throws_invalid([&] { ev.transform_to_ntt(big.data(), big.size(), 2, out.data()); },
                                 "plain is not valid for encryption parameters");
            ok &= throws_invalid([&] { ev.transform_to_ntt(plain.data(), plain.size(), 4, out.data()); },
                                 "parms_id is not valid for the current context");
            std::vector<std::uint64_t> copy = plain;
            ok &= throws_invalid([&] { ev.transform_to_ntt_inplace(copy, 2, ntt_true); }, "plain is already in NTT form");
            std::vector<std::uint64_t> two(2 * n, 0), odd(2 * n + 1, 0);
            ok &= throws_invalid([&] { ev.mod_switch_to_inplace(two, false, 1); }, "plain is not in NTT form");
            ok &= throws_invalid([&] { ev.mod_switch_to_inplace(two, true, 3); }, "cannot switch to higher level modulus");
            ok &= throws_invalid([&] { ev.mod_switch_to_inplace(two, true, 0); }, "parms_id is not valid for encryption parameters");
            ok &= throws_invalid([&] { ev.mod_switch_to_inplace(odd, true, 1); }, "plain is not valid for encryption parameters");
            std::vector<std::uint64_t> one(n, 0), dst;
            ok &= throws_invalid([&] { ev.mod_switch_to_next_inplace(one, true); }, "end of modulus switching chain reached");
            ok &= throws_invalid([&] { ev.mod_switch_to_next(two, false, dst); }, "plain is not in NTT form");
            // a valid call reaches the ABI, which has no CPU fallback
            bool refused = false;
            try
            {
                ev.transform_to_ntt_inplace(copy, 2, ntt);
            }
            catch (const std::logic_error &e)
            {
                refused = std::strstr(e.what(), "host-only") != nullptr && !ntt && copy == plain;
            }
            ok &= refused;
            if (!ok)
                return 1;
            std::printf("host-only plain checks ok\n");
            return 0;
        }
        for (std::size_t k = 1; k <= 3; k++)
        {
            std::vector<std::uint64_t> out(k * n);
            ev.transform_to_ntt(plain.data(), cc, k, out.data());
            std::printf("transform_to_ntt k=%zu digest %016llx\n", k, static_cast<unsigned long long>(digest(out)));
        }
        std::vector<std::uint64_t> in_place = plain;
        bool ntt = false;
        ev.transform_to_ntt_inplace(in_place, 3, ntt);
        std::printf("transform_to_ntt_inplace k=3 digest %016llx words %zu ntt %d\n",
                    static_cast<unsigned long long>(digest(in_place)), in_place.size(), ntt ? 1 : 0);
        std::vector<std::uint64_t> next, to1;
        ev.mod_switch_to_next(in_place, true, next);
        ev.mod_switch_to(in_place, true, 1, to1);
        std::printf("mod_switch_to_next digest %016llx words %zu\n", static_cast<unsigned long long>(digest(next)), next.size());
        std::printf("mod_switch_to k=1 digest %016llx words %zu\n", static_cast<unsigned long long>(digest(to1)), to1.size());
        ev.mod_switch_to_next_inplace(in_place, true);
        ev.mod_switch_to_inplace(in_place, true, 1);
        std::printf("in-place switches %s\n", in_place == to1 ? "agree" : "DIFFER");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
