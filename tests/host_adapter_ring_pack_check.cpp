// The C++ host adapter's ring packing (gemini-seal_amd/host/evaluator.hpp: LweSamples, Evaluator::extract_lwe / pack_lwes).
// argv[1] = "host": on a host-only context, the checks the adapter makes itself and their exception classes.
// argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 4096, one special prime): digests of the samples and
// of the packed ciphertext for seeded inputs, which the Python test compares with the C ABI's output for the same inputs,
// and the exceptions of the refusals that reach the ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 2, mods, 0ULL, SEALHIP_MODE_STRICT, -1 };
    Context ctx(p);
    Evaluator<HostCiphertext> ev(ctx);
    const std::map<std::uint32_t, const KSwitchKeys *> none;
    bool ok = true;
    DeviceCiphertext d(ctx), out(ctx);
    LweSamples s(ctx);
    ok &= throws<std::invalid_argument>([&] { ev.extract_lwe(d, { 0 }, s); }, "encrypted size must be 2");
    ok &= throws<std::invalid_argument>([&] { ev.pack_lwes(s, none, out); }, "samples are empty");
    ok &= s.size() == 0 && out.size() == 0;
    if (!ok)
        return 1;
    std::printf("host-only ring pack checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    try
    {
        if (argc < 2 || std::strcmp(argv[1], "host") == 0)
            return host_checks();
        if (argc < 6)
            return 2;
        const int device = std::atoi(argv[1]);
        std::uint64_t mods[4];
        parse_moduli(argv, 2, 4, mods);
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, 0, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x27ACC;
        HostCiphertext ct = host_ct(2, k, n, true);
        ct.scale_ = 1048576.0;
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        for (std::uint32_t elt : { 3u, 5u })
        {
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elt] = keys.back().get();
        }
        Evaluator<HostCiphertext> ev(ctx);
        DeviceCiphertext d(ctx);
        d.upload(ct);
        LweSamples s(ctx);
        ev.extract_lwe(d, { 7, 0, 4095, 7 }, s);
        std::vector<std::uint64_t> a(4 * k * n), b(4 * k);
        throw_on(sealhip_memcpy_d2h(ctx.get(), a.data(), s.a(), a.size() * 8));
        throw_on(sealhip_memcpy_d2h(ctx.get(), b.data(), s.b(), b.size() * 8));
        print_digest("device extract_lwe", digest(digest(a), b.data(), b.size()),
                     s.size() == 4 && s.coeff_modulus_size() == k && s.scale() == ct.scale());
        DeviceCiphertext out(ctx);
        ev.pack_lwes(s, gk, out, false, true);
        HostCiphertext back;
        out.download(back);
        print_digest("device pack_lwes", digest(back.words),
                     back.size() == 2 && back.coeff_modulus_size() == k && back.is_ntt_form() && back.scale() == ct.scale());
        // the refusals that reach the ABI: E_INVALIDARG arrives as std::invalid_argument
        bool ok = throws<std::invalid_argument>([&] { ev.pack_lwes(s, gk, out, true, false); }, "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.extract_lwe(d, { 4096 }, s); }, "index out of range");
        ok &= s.size() == 4; // (a refused call leaves the destination alone)
        std::printf("refusals %s\n", ok ? "ok" : "wrong");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
