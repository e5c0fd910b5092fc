// The C++ host adapter's linear combination and polynomial evaluation (gemini-seal_amd/host/evaluator.hpp:
// linear_combination, evaluate_polynomial). argv[1] = "host": on host-only contexts, the checks on the term list, the weights
// and the operand with their messages, and a valid call reaching the ABI (which has no CPU fallback).
// argv[1] = device ordinal, argv[2] = "ckks" or "bfv", argv[3..6] = four key primes (N = 4096, one special prime; BFV in
// STRICT mode with t = 65537): digests of the linear combination of three seeded terms -- BFV scalars mod t, CKKS doubles at
// the scale 2^30 -- and, for BFV, of a degree-4 polynomial of the first term, on the host ciphertext type and on
// DeviceCiphertext; the Python test compares them with the oracle's words for the same inputs. meta: the size, level, form
// and, for CKKS, the scale (the product of the terms' scale and the weights').
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

using Terms = std::vector<HostCiphertext>;
using Scalars = std::vector<std::uint64_t>;
using Doubles = std::vector<double>;
using Keys = std::vector<const KSwitchKeys *>;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    bool ok = true;
    for (std::uint32_t scheme : { SEALHIP_SCHEME_BFV, SEALHIP_SCHEME_CKKS })
    {
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        sealhip_params p{ scheme, 8, 4, 2, mods, bfv ? 786433ULL : 0ULL, SEALHIP_MODE_STRICT, -1 };
        Context ctx(p);
        Evaluator<HostCiphertext> ev(ctx);
        HostCiphertext out = host_ct(3, 1, n, false);
        const HostCiphertext good = host_ct(2, 2, n, !bfv, 4.0), wrong_form = host_ct(2, 2, n, bfv, 4.0),
                             three = host_ct(3, 2, n, !bfv, 4.0), one = host_ct(1, 2, n, !bfv, 4.0),
                             below = host_ct(2, 1, n, !bfv, 4.0), scaled = host_ct(2, 2, n, !bfv, 8.0);
        const char *form = bfv ? "cannot be in NTT form" : "must be in NTT form";
        // one call shape per scheme; the other scheme's overload is refused
        auto lin = [&](const Terms &t, std::size_t n_weights) {
            if (bfv)
                ev.linear_combination(t, Scalars(n_weights, 5), out);
            else
                ev.linear_combination(t, Doubles(n_weights, 0.5), 1024.0, out);
        };
        if (bfv)
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Doubles{ 1.0 }, 2.0, out); }, "for CKKS");
        else
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Scalars{ 1 }, out); }, "for BFV");
        ok &= throws<std::invalid_argument>([&] { lin(Terms{}, 0); }, "non-zero number of entries");
        ok &= throws<std::invalid_argument>([&] { lin(Terms{ good, good }, 1); }, "non-zero number of entries");
        ok &= throws<std::invalid_argument>([&] { lin(Terms{ good, wrong_form }, 2); }, form);
        ok &= throws<std::invalid_argument>([&] { lin(Terms{ good, three }, 2); }, "one size");
        ok &= throws<std::invalid_argument>([&] { lin(Terms{ one }, 1); }, "one size");
        ok &= throws<std::invalid_argument>([&] { lin(Terms{ good, below }, 2); }, "parameter mismatch");
        if (bfv)
        {
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Scalars{ 786433 }, out); },
                                                "below the plain modulus");
            ok &= throws<std::logic_error>([&] { lin(Terms{ good, scaled }, 2); }, "host-only"); // (BFV has no scales)
            // polynomial evaluation: the operand's form and size, an empty list; the rest is the ABI's
            ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(wrong_form, Scalars{ 1, 2 }, Keys{}, out); }, form);
            ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(three, Scalars{ 1, 2 }, Keys{}, out); },
                                                "encrypted size must be 2");
            ok &= throws<std::invalid_argument>([&] { ev.evaluate_polynomial(good, Scalars{}, Keys{}, out); }, "must not be empty");
            ok &= throws<std::logic_error>([&] { ev.evaluate_polynomial(good, Scalars{ 1, 2 }, Keys{}, out); }, "host-only");
        }
        else
        {
            ok &= throws<std::invalid_argument>([&] { lin(Terms{ good, scaled }, 2); }, "scale mismatch");
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Doubles{ 1.0 }, 0.0, out); },
                                                "scale out of bounds");
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Doubles{ 4.0 }, 1152921504606846976.0, out); },
                                                "too large"); // 4 * 2^60 = 2^62
            ok &= throws<std::invalid_argument>([&] { ev.linear_combination(Terms{ good }, Doubles{ -4.0 }, 1152921504606846976.0, out); },
                                                "too large");
            ok &= throws<std::logic_error>([&] { ev.linear_combination(Terms{ good }, Doubles{ -3.9 }, 1152921504606846976.0, out); },
                                           "host-only");
            ok &= throws<std::logic_error>([&] { ev.evaluate_polynomial(good, Scalars{ 1, 2 }, Keys{}, out); }, "unsupported scheme");
        }
        ok &= out.size() == 3 && out.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        // valid calls reach the device; sizes above 2 are served
        ok &= throws<std::logic_error>([&] { lin(Terms{ good, good, good }, 3); }, "host-only");
        ok &= throws<std::logic_error>([&] { lin(Terms{ three, three }, 2); }, "host-only");
    }
    if (!ok)
        return 1;
    std::printf("host-only poly_eval checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    try
    {
        if (argc < 2 || std::strcmp(argv[1], "host") == 0)
            return host_checks();
        if (argc < 7)
            return 2;
        const int device = std::atoi(argv[1]);
        const bool bfv = std::strcmp(argv[2], "bfv") == 0;
        std::uint64_t mods[4];
        parse_moduli(argv, 3, 4, mods);
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3, n_terms = 3;
        sealhip_params p{ bfv ? SEALHIP_SCHEME_BFV : SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, bfv ? 65537ULL : 0ULL,
                          bfv ? SEALHIP_MODE_STRICT : SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4020;
        const double ct_scale = bfv ? 1.0 : 1048576.0, w_scale = 1073741824.0; // 2^20, 2^30
        Terms terms;
        for (std::size_t t = 0; t < n_terms; t++)
        {
            HostCiphertext ct = host_ct(2, k, n, !bfv, ct_scale);
            fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
            terms.push_back(ct);
        }
        const std::unique_ptr<KSwitchKeys> seeded = seeded_key(ctx, nd, nk, n, mods, state);
        const KSwitchKeys &key = *seeded;
        const Keys keys{ &key };
        const Scalars scalars{ 3, 65536, 40000 }, coeffs{ 7, 0, 65530, 5, 9 };
        const Doubles values{ 1.5, -2.25, 0.0078125 };
        Evaluator<HostCiphertext> ev(ctx);
        auto report = [&](const char *what, const HostCiphertext &c, double scale) {
            const std::uint64_t h = digest(c.words);
            const bool meta = c.size() == 2 && c.coeff_modulus_size() == k && c.is_ntt_form() == !bfv &&
                              c.words.size() == 2 * k * n && (bfv || c.scale() == scale);
            print_digest(what, h, meta);
        };
        HostCiphertext out;
        if (bfv)
            ev.linear_combination(terms, scalars, out);
        else
            ev.linear_combination(terms, values, w_scale, out);
        report("host lincomb", out, ct_scale * w_scale);
        if (bfv)
        {
            ev.evaluate_polynomial(terms[0], coeffs, keys, out);
            report("host poly", out, 1.0);
        }
        std::vector<DeviceCiphertext> dt;
        for (std::size_t t = 0; t < n_terms; t++)
        {
            dt.emplace_back(ctx);
            dt.back().upload(terms[t]);
        }
        DeviceCiphertext dout(ctx);
        HostCiphertext back;
        if (bfv)
            ev.linear_combination(dt, scalars, dout);
        else
            ev.linear_combination(dt, values, w_scale, dout);
        dout.download(back);
        report("device lincomb", back, ct_scale * w_scale);
        if (bfv)
        {
            ev.evaluate_polynomial(dt[0], coeffs, keys, dout);
            dout.download(back);
            report("device poly", back, 1.0);
            // in place: the operand becomes p(operand)
            DeviceCiphertext x(dt[0]);
            ev.evaluate_polynomial_inplace(x, coeffs, keys);
            HostCiphertext again;
            x.download(again);
            if (again.words != back.words)
            {
                std::printf("error: the in-place form differs\n");
                return 1;
            }
        }
        // the operands are still what was uploaded
        for (std::size_t t = 0; t < n_terms; t++)
        {
            dt[t].download(back);
            if (back.words != terms[t].words)
            {
                std::printf("error: an operand was modified\n");
                return 1;
            }
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
