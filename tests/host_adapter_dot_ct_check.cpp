// The C++ host adapter's ciphertext inner product (gemini-seal_amd/host/evaluator.hpp: dot_product). argv[1] = "host": on
// host-only contexts, the checks on the term lists and their messages (empty or unequal lists, the form, the size, a level
// or a scale that differs from the first term's) and a valid call reaching the ABI (which has no CPU fallback).
// argv[1] = device ordinal, argv[2] = "ckks" or "bfv", argv[3..6] = four key primes (N = 4096, one special prime; BFV in
// STRICT mode with t = 65537): digests of the size-3 sum and of the relinearized sum on the host ciphertext type and on
// DeviceCiphertext for seeded inputs, which the Python test compares with the C ABI's output for the same inputs; the size,
// level, form and scale (the product of the two sides' scales) of the result.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

using Terms = std::vector<HostCiphertext>;

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
                             three = host_ct(3, 2, n, !bfv, 4.0), below = host_ct(2, 1, n, !bfv, 4.0),
                             scaled = host_ct(2, 2, n, !bfv, 8.0);
        const char *form = bfv ? "cannot be in NTT form" : "must be in NTT form";
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{}, Terms{}, out); }, "non-zero number of terms");
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, good }, Terms{ good }, out); },
                                            "non-zero number of terms");
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, wrong_form }, Terms{ good, good }, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, good }, Terms{ good, three }, out); },
                                            "encrypted size must be 2");
        // a level that differs inside a term, and one that differs from the first term's
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, good }, Terms{ good, below }, out); },
                                            "parameter mismatch");
        ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, below }, Terms{ good, below }, out); },
                                            "parameter mismatch");
        // scales: one per side (BFV has none: the call goes on to the device, which a host-only context does not have)
        if (bfv)
            ok &= throws<std::logic_error>([&] { ev.dot_product(Terms{ good, scaled }, Terms{ good, good }, out); }, "host-only");
        else
        {
            ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, scaled }, Terms{ good, good }, out); },
                                                "scale mismatch");
            ok &= throws<std::invalid_argument>([&] { ev.dot_product(Terms{ good, good }, Terms{ scaled, good }, out); },
                                                "scale mismatch");
        }
        ok &= out.size() == 3 && out.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        // valid calls reach the device; the two sides may differ in scale
        ok &= throws<std::logic_error>([&] { ev.dot_product(Terms{ good, good }, Terms{ scaled, scaled }, out); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.dot_product(Terms{ good }, Terms{ good }, out); }, "host-only");
    }
    if (!ok)
        return 1;
    std::printf("host-only dot_ct checks ok\n");
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
        std::uint64_t state = 0x4018;
        const double sa = bfv ? 1.0 : 1048576.0, sb = bfv ? 1.0 : 1024.0;
        Terms a, b;
        for (std::size_t t = 0; t < 2 * n_terms; t++)
        {
            HostCiphertext ct = host_ct(2, k, n, !bfv, t < n_terms ? sa : sb);
            fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
            (t < n_terms ? a : b).push_back(ct);
        }
        const std::unique_ptr<KSwitchKeys> seeded = seeded_key(ctx, nd, nk, n, mods, state);
        const KSwitchKeys &key = *seeded;
        Evaluator<HostCiphertext> ev(ctx);
        auto report = [&](const char *what, const HostCiphertext &c, std::size_t size) {
            const std::uint64_t h = digest(c.words);
            const bool meta = c.size() == size && c.coeff_modulus_size() == k && c.is_ntt_form() == !bfv &&
                              c.words.size() == size * k * n && (bfv || c.scale() == sa * sb);
            print_digest(what, h, meta);
        };
        HostCiphertext out;
        ev.dot_product(a, b, out);
        report("host size3", out, 3);
        ev.dot_product(a, b, key, out);
        report("host relin", out, 2);
        std::vector<DeviceCiphertext> da, db;
        for (std::size_t t = 0; t < n_terms; t++)
        {
            da.emplace_back(ctx);
            da.back().upload(a[t]);
            db.emplace_back(ctx);
            db.back().upload(b[t]);
        }
        DeviceCiphertext dout(ctx);
        HostCiphertext back;
        ev.dot_product(da, db, dout);
        dout.download(back);
        report("device size3", back, 3);
        ev.dot_product(da, db, key, dout);
        dout.download(back);
        report("device relin", back, 2);
        // the operands are still what was uploaded
        for (std::size_t t = 0; t < n_terms; t++)
        {
            da[t].download(back);
            if (back.words != a[t].words)
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
