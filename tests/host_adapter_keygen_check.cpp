// The C++ host adapter's KeyGenerator (gemini-seal_amd/host/evaluator.hpp). On a host-only context: the reference's host
// checks and messages (keygenerator.cpp:146-240), duplicate elements dropped before any sample is drawn, and the samples
// asked for in the reference's order. With a device (argv[1] = ordinal): digests of the saved keys and of the public key,
// which the Python test compares with the C ABI's outputs for the same samples.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static std::uint64_t save_digest(const Context &ctx, const std::vector<const sealhip_kswitch_key *> &keys)
{
    std::size_t need = 0, written = 0;
    throw_on(sealhip_kswitch_keys_save(ctx.get(), keys.data(), std::uint32_t(keys.size()), nullptr, 0, &need));
    std::vector<unsigned char> buf(need);
    throw_on(sealhip_kswitch_keys_save(ctx.get(), keys.data(), std::uint32_t(keys.size()), buf.data(), need, &written));
    return digest(buf.data(), written);
}

int main(int argc, char **argv)
{
    // BFV N=256, {30, 40, 60, 60}, nsp = 2 (k = 2: one digit), t = 786433 (batching)
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    const int device = argc > 1 ? std::atoi(argv[1]) : -1;
    sealhip_params p{ SEALHIP_SCHEME_BFV, 8, 4, 2, mods, 786433, SEALHIP_MODE_PARITY, device };
    try
    {
        Context ctx(p);
        std::vector<std::uint64_t> sk(4 * n);
        std::uint64_t state = 0x5EC2E7;
        fill_rows(sk.data(), 4, n, mods, 4, state);
        std::uint64_t sample_state = 0xCAFE;
        std::size_t asked = 0;
        KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *seed, std::int32_t *noise) {
            asked++;
            for (int i = 0; i < 8; i++)
                seed[i] = splitmix(sample_state);
            for (std::size_t i = 0; i < n; i++)
                noise[i] = static_cast<std::int32_t>(splitmix(sample_state) % 83) - 41;
        });
        if (device < 0)
        {
            bool ok = true;
            ok &= throws_exact<std::invalid_argument>([&] { kg.relin_keys(0); }, "invalid count");
            ok &= throws_exact<std::invalid_argument>([&] { kg.relin_keys(15); }, "invalid count");
            ok &= throws_exact<std::invalid_argument>([&] { kg.galois_keys(std::vector<std::uint32_t>{ 3, 4 }); },
                                                "Galois element is not valid");
            ok &= throws_exact<std::invalid_argument>([&] { kg.galois_keys(std::vector<std::uint32_t>{ 3, 2 * n + 1 }); },
                                                "Galois element is not valid");
            ok &= throws_exact<std::invalid_argument>([&] { kg.galois_keys(std::vector<int>{ 1, int(n / 2) }); }, "step count too large");
            ok &= asked == 0; // nothing sampled for rejected arguments
            sealhip_params nb = p;
            nb.plain_modulus = 65539; // prime, not 1 mod 2N
            Context ctx_nb(nb);
            KeyGenerator kg_nb(ctx_nb, sk.data(), [](std::uint64_t *, std::int32_t *) {});
            ok &= throws_exact<std::logic_error>([&] { kg_nb.galois_keys(std::vector<std::uint32_t>{ 3 }); },
                                           "encryption parameters do not support batching");
            // get_elts_all: 2N - 1 first, 2 (log N - 1) + 1 entries, 5^(N/4) twice
            const std::vector<std::uint32_t> all = kg.elts_all();
            ok &= all.size() == 15 && all[0] == 2 * n - 1 && all[1] == 5 && all[13] == all[14];
            // valid arguments reach the ABI, which has no CPU fallback; duplicates draw no samples (one digit per key here)
            bool refused = false;
            try
            {
                kg.galois_keys(std::vector<std::uint32_t>{ 3, 5, 3, 2 * n - 1, 5 });
            }
            catch (const std::logic_error &e)
            {
                refused = std::strstr(e.what(), "host-only") != nullptr;
            }
            ok &= refused && asked == 3;
            if (!ok)
                return 1;
            std::printf("host-only keygen checks ok\n");
            return 0;
        }
        const std::uint64_t pid[4] = { 0x1111, 0x2222, 0x3333, 0x4444 };
        throw_on(sealhip_context_set_parms_id(ctx.get(), 4, pid));
        auto rk = kg.relin_keys(2, false);
        std::printf("relin_keys(2) digest %016llx\n",
                    static_cast<unsigned long long>(save_digest(ctx, { rk[0]->get(), rk[1]->get() })));
        auto gk = kg.galois_keys(std::vector<int>{ 1, -1 });
        std::vector<const sealhip_kswitch_key *> by_elt;
        for (auto &kv : gk)
            by_elt.push_back(kv.second->get());
        std::printf("galois_keys(steps 1, -1) digest %016llx elts %u %u\n",
                    static_cast<unsigned long long>(save_digest(ctx, by_elt)), gk.begin()->first, gk.rbegin()->first);
        const std::vector<std::uint64_t> pk = kg.public_key();
        std::printf("public_key digest %016llx\n",
                    static_cast<unsigned long long>(digest(reinterpret_cast<const unsigned char *>(pk.data()), pk.size() * 8)));
        std::printf("samples asked %zu\n", asked);
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
