// The C++ host adapter's baby-step/giant-step matrix-vector product (gemini-seal_amd/host/evaluator.hpp:
// apply_galois_bsgs_plain, rotate_vector_bsgs_plain, rotate_rows_bsgs_plain). argv[1] = "host": on host-only contexts, the
// operand and plaintext checks and their messages, the missing key on either axis, the wrong scheme, and a valid call
// reaching the ABI (which has no CPU fallback). argv[1] = device ordinal, argv[2] = "ckks" or "bfv", argv[3..6] = four key
// primes (N = 4096, one special prime; BFV in STRICT mode with t = 65537): digests of the result on the host ciphertext type
// and on DeviceCiphertext / DevicePlaintext for seeded inputs, which the Python test compares with the C ABI's output for
// the same inputs; the level, form and scale of the result.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

using Plains = std::vector<std::vector<HostPlaintext>>;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256, n_key = 4;
    bool ok = true;
    for (std::uint32_t scheme : { SEALHIP_SCHEME_BFV, SEALHIP_SCHEME_CKKS })
    {
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        sealhip_params p{ scheme, 8, 4, 2, mods, bfv ? 786433ULL : 0ULL, SEALHIP_MODE_STRICT, -1 };
        Context ctx(p);
        Evaluator<HostCiphertext> ev(ctx);
        const std::map<std::uint32_t, const KSwitchKeys *> none;
        HostCiphertext out = host_ct(3, 1, n, false);
        const HostCiphertext good = host_ct(2, 2, n, !bfv), wrong_form = host_ct(2, 2, n, bfv), three = host_ct(3, 2, n, !bfv);
        const HostPlaintext w = host_plain(n_key, n, true, 4.0);
        const Plains one{ { w } }, two{ { w, w } }, square{ { w, w }, { w, w } };
        const char *form = bfv ? "BFV encrypted cannot be in NTT form" : "CKKS encrypted must be in NTT form";
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(wrong_form, { 1 }, { 1 }, none, one, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(three, { 1 }, { 1 }, none, one, out); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 3 }, { 1 }, none, one, out); },
                                            "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 3 }, none, one, out); },
                                            "Galois key not present");
        // element 1 needs no key on either axis: the call gets past the key lookup (to the missing device); element 3 next
        // to it does not, on the baby axis or on the giant axis
        ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 1 }, none, one, out); }, "host-only");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1, 3 }, { 1 }, none, two, out); },
                                            "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 1, 3 }, none, Plains{ { w }, { w } }, out); },
                                            "Galois key not present");
        // the plaintexts: rows per giant, a ragged row, a level below the key level, coefficient form, unequal scales (CKKS)
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1, 1 }, { 1 }, none, square, out); },
                                            "one row of plaintexts per giant element");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 1 }, none, two, out); },
                                            "one plaintext per Galois element");
        ok &= throws<std::invalid_argument>(
            [&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 1 }, none, Plains{ { host_plain(2, n, true, 4.0) } }, out); },
            "NTT form at the key level");
        ok &= throws<std::invalid_argument>(
            [&] { ev.apply_galois_bsgs_plain(good, { 1 }, { 1 }, none, Plains{ { host_plain(n_key, n, false, 4.0) } }, out); },
            "NTT form at the key level");
        const Plains scales{ { w, host_plain(n_key, n, true, 8.0) } };
        if (bfv) // (BFV plaintexts have no scale: the call goes on to the device, which a host-only context does not have)
            ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain(good, { 1, 1 }, { 1 }, none, scales, out); },
                                           "host-only");
        else
            ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain(good, { 1, 1 }, { 1 }, none, scales, out); },
                                                "scale mismatch");
        // the steps forms name their scheme
        if (bfv)
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_bsgs_plain(good, { 0 }, { 0 }, none, one, out); },
                                           "unsupported scheme");
        else
            ok &= throws<std::logic_error>([&] { ev.rotate_rows_bsgs_plain(good, { 0 }, { 0 }, none, one, out); },
                                           "unsupported scheme");
        ok &= out.size() == 3 && out.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        // a valid call (step 0 needs no key) reaches the device, which a host-only context does not have
        if (bfv)
            ok &= throws<std::logic_error>([&] { ev.rotate_rows_bsgs_plain(good, { 0 }, { 0 }, none, one, out); }, "host-only");
        else
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_bsgs_plain(good, { 0 }, { 0 }, none, one, out); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain(good, { 1, 1 }, { 1, 1 }, none, square, out); },
                                       "host-only");
    }
    if (!ok)
        return 1;
    std::printf("host-only bsgs checks ok\n");
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
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3, n_giant = 3, n_baby = 2;
        sealhip_params p{ bfv ? SEALHIP_SCHEME_BFV : SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, bfv ? 65537ULL : 0ULL,
                          bfv ? SEALHIP_MODE_STRICT : SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4017;
        HostCiphertext ct = host_ct(2, k, n, !bfv);
        ct.scale_ = bfv ? 1.0 : 1048576.0;
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        const int steps[3] = { 1, -2, 4 };
        std::uint32_t elts[3];
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        for (int e = 0; e < 3; e++)
        {
            throw_on(sealhip_galois_elt_from_step(ctx.get(), steps[e], &elts[e]));
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elts[e]] = keys.back().get();
        }
        const double pscale = bfv ? 1.0 : 1024.0;
        Plains plains(n_giant, std::vector<HostPlaintext>(n_baby));
        std::vector<std::vector<DevicePlaintext>> dplains(n_giant);
        for (std::size_t s = 0; s < n_giant; s++)
            for (std::size_t e = 0; e < n_baby; e++)
            {
                HostPlaintext &w = plains[s][e];
                w.words.resize(nk * n);
                w.k = nk;
                w.ntt_form = true;
                w.scale = pscale;
                fill_rows(w.words.data(), nk, n, mods, nk, state);
                dplains[s].emplace_back(ctx);
                dplains[s].back().upload(w.words, true);
                dplains[s].back().scale() = pscale;
            }
        Evaluator<HostCiphertext> ev(ctx);
        // babies: step 1 and the identity; giants: the identity, steps -2 and 4
        const std::vector<std::uint32_t> baby{ elts[0], 1 }, giant{ 1, elts[1], elts[2] };
        const std::vector<int> baby_steps{ 1, 0 }, giant_steps{ 0, -2, 4 };
        auto report = [&](const char *what, const HostCiphertext &c) {
            const std::uint64_t h = digest(c.words);
            const bool meta = c.size() == 2 && c.coeff_modulus_size() == k && c.is_ntt_form() == !bfv &&
                              (bfv || c.scale() == ct.scale() * pscale);
            print_digest(what, h, meta);
        };
        HostCiphertext out;
        ev.apply_galois_bsgs_plain(ct, baby, giant, gk, plains, out);
        report("host apply_galois_bsgs_plain", out);
        if (bfv)
            ev.rotate_rows_bsgs_plain(ct, baby_steps, giant_steps, gk, plains, out);
        else
            ev.rotate_vector_bsgs_plain(ct, baby_steps, giant_steps, gk, plains, out);
        report("host steps", out);
        DeviceCiphertext d(ctx), dout(ctx);
        d.upload(ct);
        HostCiphertext back;
        ev.apply_galois_bsgs_plain(d, baby, giant, gk, dplains, dout);
        dout.download(back);
        report("device apply_galois_bsgs_plain", back);
        if (bfv)
            ev.rotate_rows_bsgs_plain(d, baby_steps, giant_steps, gk, dplains, dout);
        else
            ev.rotate_vector_bsgs_plain(d, baby_steps, giant_steps, gk, dplains, dout);
        dout.download(back);
        report("device steps", back);
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
