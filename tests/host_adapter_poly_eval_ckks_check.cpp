// The C++ host adapter's CKKS polynomial evaluation (gemini-seal_amd/host/evaluator.hpp: evaluate_polynomial with doubles,
// DESIGN.md section 21). argv[1] = "host": on a host-only context, the checks on the operand with their messages, the plan's
// refusals passed through, and a valid call reaching the ABI (which has no CPU fallback).
// argv[1] = device ordinal, argv[2..10] = nine key primes (N = 4096, eight data primes and one special prime): digests of a
// degree-7 polynomial of a seeded ciphertext at the scale 2^40 in the monomial and in the Chebyshev basis (the latter with
// scale_out = 2^38), on the host ciphertext type and on DeviceCiphertext; the Python test compares them with the words of
// tests/poly_eval_ckks_ref.py for the same inputs. meta: size 2, NTT form, the plan's level and the requested scale.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

using Doubles = std::vector<double>;
using Keys = std::vector<const KSwitchKeys *>;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    bool ok = true;
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, -1 }; // first level 3
    Context ctx(p);
    Evaluator<HostCiphertext> ev(ctx);
    HostCiphertext out = host_ct(3, 1, n, false);
    const double scale = 1099511627776.0; // 2^40
    const HostCiphertext good = host_ct(2, 3, n, true, scale), coeff_form = host_ct(2, 3, n, false, scale),
                         three = host_ct(3, 3, n, true, scale), low = host_ct(2, 1, n, true, scale),
                         unscaled = host_ct(2, 3, n, true, 0.0);
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(coeff_form, Doubles{ 1, 2 }, Keys{}, out); }, "must be in NTT form");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(three, Doubles{ 1, 2 }, Keys{}, out); }, "encrypted size must be 2");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(good, Doubles{}, Keys{}, out); }, "must not be empty");
    // the plan's refusals come through before anything is staged
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(unscaled, Doubles{ 1, 2 }, Keys{}, out); }, "scale out of bounds");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(good, Doubles{ 1, 2 }, Keys{}, out, 2); }, "basis");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(good, Doubles{ 5, 0 }, Keys{}, out); }, "constant");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(low, Doubles{ 1, 2 }, Keys{}, out); }, "end of modulus switching chain");
    ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(good, Doubles(8, 0.5), Keys{}, out, 1); },
                                        "end of modulus switching chain"); // (degree 7 takes four levels)
    // a valid call reaches the device (the operand is staged before the ABI looks at the keys): in both bases and with a
    // scale of its own
    ok &= throws<std::logic_error>([&] { ev.evaluate_polynomial(good, Doubles{ 1, 2 }, Keys{}, out); }, "host-only");
    ok &= throws<std::logic_error>([&] { ev.evaluate_polynomial(good, Doubles{ 1, 2 }, Keys{}, out, 1, 1048576.0); }, "host-only");
    ok &= out.size() == 3 && out.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
    if (!ok)
        return 1;
    std::printf("host-only poly_eval_ckks checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    try
    {
        if (argc < 2 || std::strcmp(argv[1], "host") == 0)
            return host_checks();
        if (argc < 11)
            return 2;
        const int device = std::atoi(argv[1]);
        const std::size_t n = 4096, k = 8, nk = 9, nd = 8;
        std::uint64_t mods[nk];
        parse_moduli(argv, 2, int(nk), mods);
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, std::uint32_t(nk), 1, mods, 0ULL, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4021;
        const double scale = 1099511627776.0, scale_out = 274877906944.0; // 2^40, 2^38
        HostCiphertext ct = host_ct(2, k, n, true, scale);
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        const std::unique_ptr<KSwitchKeys> seeded = seeded_key(ctx, nd, nk, n, mods, state);
        const KSwitchKeys &key = *seeded;
        const Keys keys{ &key };
        const Doubles coeffs{ 0.5, -0.25, 0.125, 0.75, -0.5, 0.0625, 0.3125, -0.875 };
        sealhip_poly_plan plan{};
        if (sealhip_evaluator_polynomial_plan_ckks(ctx.get(), std::uint32_t(k), scale, coeffs.data(), 7, 0, 0, 0.0, &plan, nullptr,
                                                   nullptr) != 0)
            return 3;
        Evaluator<HostCiphertext> ev(ctx);
        auto report = [&](const char *what, const HostCiphertext &c, double want_scale) {
            const std::uint64_t h = digest(c.words);
            const bool meta = c.size() == 2 && c.coeff_modulus_size() == plan.out_level && c.is_ntt_form() &&
                              c.words.size() == 2 * plan.out_level * n && c.scale() == want_scale;
            print_digest(what, h, meta);
        };
        HostCiphertext out;
        ev.evaluate_polynomial(ct, coeffs, keys, out);
        report("host monomial", out, scale);
        ev.evaluate_polynomial(ct, coeffs, keys, out, 1, scale_out);
        report("host chebyshev", out, scale_out);
        DeviceCiphertext dct(ctx), dout(ctx);
        dct.upload(ct);
        HostCiphertext back;
        ev.evaluate_polynomial(dct, coeffs, keys, dout);
        dout.download(back);
        report("device monomial", back, scale);
        ev.evaluate_polynomial(dct, coeffs, keys, dout, 1, scale_out);
        dout.download(back);
        report("device chebyshev", back, scale_out);
        // in place: the operand becomes p(operand), at the plan's level and scale
        DeviceCiphertext x(dct);
        ev.evaluate_polynomial_inplace(x, coeffs, keys, 1, scale_out);
        HostCiphertext again;
        x.download(again);
        if (again.words != back.words || again.scale() != scale_out || again.coeff_modulus_size() != plan.out_level)
        {
            std::printf("error: the in-place form differs\n");
            return 1;
        }
        dct.download(back);
        if (back.words != ct.words)
        {
            std::printf("error: the operand was modified\n");
            return 1;
        }
        ev.synchronize(); // (the deferred transparency checks of the resident calls: random inputs are not transparent)
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
