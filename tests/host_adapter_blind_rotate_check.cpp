// The C++ host adapter's blind rotation (gemini-seal_amd/host/evaluator.hpp: BlindRotationKeys, lut_test_vector,
// KeyGenerator::blind_rotation_keys, Evaluator::multiply_monomial / blind_rotate).
// argv[1] = "host": on a host-only context, the checks the adapter makes itself and their exception classes.
// argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 4096, one special prime): digests of the results for
// seeded inputs, on resident and on host operands, which the Python test compares with the C ABI's output for the same
// inputs.
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
    BlindRotationKeys none({}, false);
    bool ok = true;
    DeviceCiphertext d(ctx), out(ctx);
    ok &= throws<std::invalid_argument>([&] { ev.multiply_monomial(d, 3, out); }, "CKKS encrypted must be in NTT form");
    ok &= throws<std::invalid_argument>([&] { ev.blind_rotate(d, { 3 }, none, out); }, "CKKS encrypted must be in NTT form");
    d.is_ntt_form() = true;
    ok &= throws<std::invalid_argument>([&] { ev.multiply_monomial(d, 3, out, true); }, "encrypted size must be 2");
    HostCiphertext a = host_ct(2, 2, n, true), r;
    ok &= throws<std::invalid_argument>([&] { ev.blind_rotate(a, { 3, 4 }, none, r); }, "one exponent and one more per key");
    ok &= throws<std::invalid_argument>([&] { ev.blind_rotate(a, {}, none, r); }, "one exponent and one more per key");
    ok &= throws<std::logic_error>([&] { ev.blind_rotate(a, { 3 }, none, r); }, "host-only"); // (staging needs a device)
    ok &= throws<std::logic_error>([&] { ev.multiply_monomial(a, 3, r); }, "host-only");
    std::vector<std::uint64_t> sk(4 * n, 1);
    std::size_t asked = 0;
    KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *, std::int32_t *) { asked++; });
    ok &= throws_exact<std::invalid_argument>([&] { kg.blind_rotation_keys({}, true); }, "invalid count");
    ok &= throws<std::invalid_argument>([&] { kg.blind_rotation_keys({ 1, 2 }, true); }, "coefficients in {-1, 0, 1}");
    ok &= throws<std::invalid_argument>([&] { kg.blind_rotation_keys({ 1, -1 }, false); }, "coefficients in {-1, 0, 1}");
    ok &= throws_exact<std::invalid_argument>([&] { kg.blind_rotation_keys({ 1, -1 }, true, 3); }, "level k out of range");
    ok &= asked == 0; // nothing sampled for rejected arguments
    ok &= throws<std::logic_error>([&] { kg.blind_rotation_keys({ 1, -1 }, true); }, "host-only");
    const auto tv = lut_test_vector([](std::uint64_t m) { return (3 * m + 1) % 8; }, 8, 32);
    ok &= tv.size() == 32;
    for (std::size_t j = 0; j < tv.size(); j++)
        ok &= tv[j] == (3 * (j / 8) + 1) % 8;
    if (!ok)
        return 1;
    std::printf("host-only blind rotation checks ok\n");
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
        const std::size_t n = 4096, k = 3, nk = 4;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, 0, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x30A5;
        HostCiphertext host = host_ct(2, k, n, true, 1048576.0);
        fill_rows(host.words.data(), 2 * k, n, mods, k, state);
        DeviceCiphertext dev(ctx);
        dev.upload(host);
        std::vector<std::uint64_t> sk(nk * n);
        fill_rows(sk.data(), nk, n, mods, nk, state);
        std::uint64_t sample_state = 0xCAFE30;
        KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *seed, std::int32_t *noise) {
            for (int i = 0; i < 8; i++)
                seed[i] = splitmix(sample_state);
            for (std::size_t i = 0; i < n; i++)
                noise[i] = static_cast<std::int32_t>(splitmix(sample_state) % 83) - 41;
        });
        auto keys = kg.blind_rotation_keys({ 1, -1, 0 }, true);
        const std::vector<std::uint32_t> exps{ 5, 4097, 8191, 1, 0, 77, 4096 };
        Evaluator<HostCiphertext> ev(ctx);
        bool meta = false;
        {
            DeviceCiphertext out(ctx);
            ev.multiply_monomial(dev, 4099, out, true);
            std::uint64_t h = words_digest(out, meta, k, 1048576.0); // (meta is set by the call: not in one argument list)
            print_digest("device multiply_monomial", h, meta);
            HostCiphertext hout;
            ev.multiply_monomial(host, 4099, hout, true);
            print_digest("host multiply_monomial", digest(hout.words), hout.size() == 2 && hout.is_ntt_form() && hout.scale() == 1048576.0);
        }
        {
            DeviceCiphertext out(ctx);
            ev.blind_rotate(dev, exps, *keys, out);
            std::uint64_t h = words_digest(out, meta, k, 1048576.0);
            print_digest("device blind_rotate", h, meta && keys->n_steps() == 6 && keys->ternary());
            HostCiphertext hout;
            ev.blind_rotate(host, exps, *keys, hout);
            print_digest("host blind_rotate", digest(hout.words), hout.size() == 2 && hout.is_ntt_form() && hout.scale() == 1048576.0);
            ev.blind_rotate(dev, exps, *keys, dev); // the destination may be the operand
            h = words_digest(dev, meta, k, 1048576.0);
            print_digest("device blind_rotate in place", h, meta);
        }
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
