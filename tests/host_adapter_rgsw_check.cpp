// The C++ host adapter's RGSW ciphertexts (gemini-seal_amd/host/evaluator.hpp: RgswCiphertext, KeyGenerator::rgsw,
// Evaluator::external_product / cmux / select).
// argv[1] = "host": on a host-only context, the checks the adapter makes itself and their exception classes.
// argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 4096, one special prime): digests of the results for
// seeded inputs, on resident and on host operands, which the Python test compares with the C ABI's output for the same
// inputs, and the exceptions of the refusals that reach the ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 2, mods, 0ULL, SEALHIP_MODE_STRICT, -1 };
    Context ctx(p);
    Evaluator<HostCiphertext> ev(ctx);
    RgswCiphertext none(ctx, static_cast<sealhip_rgsw *>(nullptr)); // (a handle cannot exist without a device: never followed)
    bool ok = true;
    DeviceCiphertext d(ctx), other(ctx), out(ctx);
    ok &= throws<std::invalid_argument>([&] { ev.external_product(d, none, out); }, "CKKS encrypted must be in NTT form");
    ok &= throws<std::invalid_argument>([&] { ev.cmux(d, other, none, out); }, "CKKS encrypted must be in NTT form");
    d.is_ntt_form() = true;
    ok &= throws<std::invalid_argument>([&] { ev.external_product(d, none, out); }, "encrypted size must be 2");
    HostCiphertext a = host_ct(2, 2, n, true), b = host_ct(2, 1, n, true), c = host_ct(2, 2, n, false), r;
    ok &= throws<std::invalid_argument>([&] { ev.cmux(a, b, none, r); }, "differ in size, level or form");
    ok &= throws<std::invalid_argument>([&] { ev.external_product(a, none, r, &c); }, "differ in size, level or form");
    std::vector<HostCiphertext> three{ a, a, a }, two{ a, a };
    ok &= throws<std::invalid_argument>([&] { ev.select(three, { &none, &none }, r); }, "2^l ciphertexts for l RGSW bits");
    ok &= throws<std::invalid_argument>([&] { ev.select(two, { nullptr }, r); }, "null entry");
    ok &= throws<std::logic_error>([&] { ev.select(two, { &none }, r); }, "host-only"); // (staging needs a device)
    std::vector<std::uint64_t> sk(4 * n, 1);
    std::size_t asked = 0;
    KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *, std::int32_t *) { asked++; });
    const std::vector<std::int32_t> m(n, 0), too_short(n - 1, 0);
    ok &= throws_exact<std::invalid_argument>([&] { kg.rgsw({}); }, "invalid count");
    ok &= throws_exact<std::invalid_argument>([&] { kg.rgsw({ too_short }); }, "an rgsw message has N coefficients");
    ok &= throws_exact<std::invalid_argument>([&] { kg.rgsw({ m }, 3); }, "level k out of range");
    ok &= asked == 0; // nothing sampled for rejected arguments
    ok &= throws<std::logic_error>([&] { kg.rgsw({ m }); }, "host-only");
    if (!ok)
        return 1;
    std::printf("host-only rgsw checks ok\n");
    return 0;
}

template <class C>
static std::uint64_t words_digest(C &c, bool &meta, std::size_t k, double scale)
{
    HostCiphertext back;
    c.download(back);
    meta = back.size() == 2 && back.coeff_modulus_size() == k && back.is_ntt_form() && back.scale() == scale;
    return digest(back.words.data(), back.words.size());
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
        std::uint64_t state = 0x29A5;
        std::vector<HostCiphertext> host;
        std::vector<DeviceCiphertext> dev;
        dev.reserve(4);
        for (int i = 0; i < 4; i++)
        {
            host.push_back(host_ct(2, k, n, true, 1048576.0));
            fill_rows(host.back().words.data(), 2 * k, n, mods, k, state);
            dev.emplace_back(ctx);
            dev.back().upload(host.back());
        }
        auto kb = seeded_key(ctx, nd, nk, n, mods, state), ka = seeded_key(ctx, nd, nk, n, mods, state);
        RgswCiphertext g(ctx, *kb, *ka), g2(ctx, *ka, *kb);
        Evaluator<HostCiphertext> ev(ctx);
        bool meta = false;
        std::uint64_t h;
        {
            DeviceCiphertext out(ctx);
            ev.external_product(dev[0], g, out, &dev[1]);
            h = words_digest(out, meta, k, 1048576.0);
            print_digest("device external_product", h, meta);
            HostCiphertext hout;
            ev.external_product(host[0], g, hout, &host[1]);
            print_digest("host external_product", digest(hout.words), hout.size() == 2 && hout.is_ntt_form() && hout.scale() == 1048576.0);
            auto halves = g.export_keys();
            RgswCiphertext again(ctx, *halves.first, *halves.second);
            DeviceCiphertext out2(ctx);
            ev.external_product(dev[0], again, out2, &dev[1]);
            print_digest("device external_product recreated", words_digest(out2, meta, k, 1048576.0), meta);
            DeviceCiphertext out3(ctx);
            ev.external_product(dev[0], g, out3);
            print_digest("device external_product no base", words_digest(out3, meta, k, 1048576.0), meta);
        }
        {
            DeviceCiphertext out(ctx);
            ev.cmux(dev[0], dev[1], g, out);
            print_digest("device cmux", words_digest(out, meta, k, 1048576.0), meta);
            HostCiphertext hout;
            ev.cmux(host[0], host[1], g, hout);
            print_digest("host cmux", digest(hout.words), hout.size() == 2 && hout.is_ntt_form());
        }
        {
            DeviceCiphertext out(ctx);
            ev.select(dev, { &g, &g2 }, out);
            print_digest("device select", words_digest(out, meta, k, 1048576.0), meta);
            HostCiphertext hout;
            ev.select(host, { &g, &g2 }, hout);
            print_digest("host select", digest(hout.words), hout.size() == 2 && hout.is_ntt_form());
            std::vector<DeviceCiphertext> one;
            one.emplace_back(ctx);
            one.back().upload(host[2]);
            DeviceCiphertext copy(ctx);
            ev.select(one, {}, copy);
            print_digest("device select l0", words_digest(copy, meta, k, 1048576.0), meta);
        }
        {
            // KeyGenerator::rgsw: the samples of 2 x nd encrypt_zero_symmetric calls from the seeded stream, K_b's digits first
            std::vector<std::uint64_t> sk(nk * n);
            fill_rows(sk.data(), nk, n, mods, nk, state);
            std::uint64_t sample_state = 0xCAFE29;
            KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *seed, std::int32_t *noise) {
                for (int i = 0; i < 8; i++)
                    seed[i] = splitmix(sample_state);
                for (std::size_t i = 0; i < n; i++)
                    noise[i] = static_cast<std::int32_t>(splitmix(sample_state) % 83) - 41;
            });
            std::vector<std::int32_t> m(n, 0);
            m[3] = -1;
            m[0] = 1;
            auto made = kg.rgsw({ m });
            DeviceCiphertext out(ctx);
            ev.external_product(dev[0], *made[0], out);
            print_digest("device external_product generated", words_digest(out, meta, k, 1048576.0), meta && made.size() == 1);
        }
        // the refusals: E_INVALIDARG arrives as std::invalid_argument, and a refused call leaves the destination alone
        auto short_key = seeded_key(ctx, 2, nk, n, mods, state);
        bool ok = throws<std::invalid_argument>([&] { RgswCiphertext bad(ctx, *kb, *short_key); }, "same digit count and level");
        RgswCiphertext low(ctx, *short_key, *short_key);
        DeviceCiphertext untouched(ctx);
        ok &= throws<std::invalid_argument>([&] { ev.external_product(dev[0], low, untouched); }, "rgsw is not valid for encryption parameters");
        ok &= throws<std::invalid_argument>([&] { ev.cmux(dev[0], dev[1], low, untouched); }, "rgsw is not valid for encryption parameters");
        ok &= throws<std::invalid_argument>([&] { ev.select(dev, { &g, &low }, untouched); }, "rgsw is not valid for encryption parameters");
        ok &= untouched.size() == 0;
        std::printf("refusals %s\n", ok ? "ok" : "wrong");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
