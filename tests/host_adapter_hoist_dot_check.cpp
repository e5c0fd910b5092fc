// The C++ host adapter's plaintext-weighted sums of rotations (gemini-seal_amd/host/evaluator.hpp: apply_galois_dot_plain,
// rotate_vector_dot_plain, rotate_rows_dot_plain). argv[1] = "host": on host-only contexts, the operand and plaintext checks
// and their messages, the missing key, the wrong scheme, and a valid call reaching the ABI (which has no CPU fallback).
// argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 4096, one special prime): digests of the results on the
// host ciphertext type and on DeviceCiphertext / DevicePlaintext for seeded inputs, which the Python test compares with the C
// ABI's output for the same inputs; the scale of the results; the deferred transparency exception; and that a warm
// resident call takes every block from the pool.
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
        std::vector<HostCiphertext> out(3);
        const HostCiphertext good = host_ct(2, 2, n, !bfv), wrong_form = host_ct(2, 2, n, bfv), three = host_ct(3, 2, n, !bfv);
        const HostPlaintext w = host_plain(n_key, n, true, 4.0);
        const Plains one{ { w } }, two{ { w, w } };
        const char *form = bfv ? "BFV encrypted cannot be in NTT form" : "CKKS encrypted must be in NTT form";
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(wrong_form, { 1 }, none, one, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(three, { 1 }, none, one, out); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(good, { 3 }, none, one, out); },
                                            "Galois key not present");
        // element 1 needs no key: the call gets past the key lookup (to the missing device); element 3 next to it does not
        ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain(good, { 1 }, none, one, out); }, "host-only");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(good, { 1, 3 }, none, two, out); },
                                            "Galois key not present");
        // the plaintexts: a ragged matrix, a level below the key level, coefficient form, unequal scales (CKKS)
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(good, { 1 }, none, two, out); },
                                            "one plaintext per Galois element");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(good, { 1, 1 }, none, Plains{ { w, w }, { w } }, out); },
                                            "one plaintext per Galois element");
        ok &= throws<std::invalid_argument>(
            [&] { ev.apply_galois_dot_plain(good, { 1 }, none, Plains{ { host_plain(2, n, true, 4.0) } }, out); },
            "NTT form at the key level");
        ok &= throws<std::invalid_argument>(
            [&] { ev.apply_galois_dot_plain(good, { 1 }, none, Plains{ { host_plain(n_key, n, false, 4.0) } }, out); },
            "NTT form at the key level");
        const Plains scales{ { w, host_plain(n_key, n, true, 8.0) } };
        if (bfv) // (BFV plaintexts have no scale: the call goes on to the device, which a host-only context does not have)
            ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain(good, { 1, 1 }, none, scales, out); }, "host-only");
        else
            ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain(good, { 1, 1 }, none, scales, out); },
                                                "scale mismatch");
        // the steps forms name their scheme
        if (bfv)
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_dot_plain(good, { 0 }, none, one, out); }, "unsupported scheme");
        else
            ok &= throws<std::logic_error>([&] { ev.rotate_rows_dot_plain(good, { 0 }, none, one, out); }, "unsupported scheme");
        ok &= out.size() == 3; // (a refused call leaves the destinations alone)
        // a valid call (step 0 needs no key) reaches the device, which a host-only context does not have
        if (bfv)
            ok &= throws<std::logic_error>([&] { ev.rotate_rows_dot_plain(good, { 0 }, none, one, out); }, "host-only");
        else
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_dot_plain(good, { 0 }, none, one, out); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain(good, { 1, 1 }, none, two, out); }, "host-only");
    }
    if (!ok)
        return 1;
    std::printf("host-only hoist dot checks ok\n");
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
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3, n_sums = 2, n_elts = 3;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, 0, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4016;
        HostCiphertext ct = host_ct(2, k, n, true);
        ct.scale_ = 1048576.0;
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        std::uint32_t elts[2];
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &elts[0]));
        throw_on(sealhip_galois_elt_from_step(ctx.get(), -2, &elts[1]));
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        for (int e = 0; e < 2; e++)
        {
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elts[e]] = keys.back().get();
        }
        const double pscale = 1024.0;
        Plains plains(n_sums, std::vector<HostPlaintext>(n_elts));
        std::vector<std::vector<DevicePlaintext>> dplains(n_sums);
        for (std::size_t s = 0; s < n_sums; s++)
            for (std::size_t e = 0; e < n_elts; e++)
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
        const std::vector<std::uint32_t> ge{ elts[0], 1, elts[1] };
        const std::vector<int> steps{ 1, 0, -2 };
        auto report = [&](const char *what, const std::vector<HostCiphertext> &out) {
            std::uint64_t h = kFnvBasis;
            bool meta = true;
            for (auto &c : out)
            {
                h = digest(h, c.data(), c.words.size());
                meta = meta && c.size() == 2 && c.coeff_modulus_size() == k && c.is_ntt_form() &&
                       c.scale() == ct.scale() * pscale;
            }
            std::printf("%s digest %016llx count %zu meta %d\n", what, static_cast<unsigned long long>(h), out.size(), int(meta));
        };
        std::vector<HostCiphertext> out;
        ev.apply_galois_dot_plain(ct, ge, gk, plains, out);
        report("host apply_galois_dot_plain", out);
        ev.rotate_vector_dot_plain(ct, steps, gk, plains, out);
        report("host rotate_vector_dot_plain", out);
        DeviceCiphertext d(ctx);
        d.upload(ct);
        std::vector<DeviceCiphertext> dout;
        auto down = [&](const char *what) {
            std::vector<HostCiphertext> back(dout.size());
            for (std::size_t i = 0; i < dout.size(); i++)
                dout[i].download(back[i]);
            report(what, back);
        };
        ev.apply_galois_dot_plain(d, ge, gk, dplains, dout);
        down("device apply_galois_dot_plain");
        ev.rotate_vector_dot_plain(d, steps, gk, dplains, dout);
        down("device rotate_vector_dot_plain");
        // a warm resident call takes every block from the pool: no hipMalloc, no hipFree between the two snapshots
        struct sealhip_pool_stats before{}, after{};
        throw_on(sealhip_pool_stats(ctx.get(), &before));
        ev.apply_galois_dot_plain(d, ge, gk, dplains, dout);
        ev.synchronize();
        throw_on(sealhip_pool_stats(ctx.get(), &after));
        std::printf("warm call pool mallocs %llu frees %llu\n",
                    static_cast<unsigned long long>(after.device_mallocs - before.device_mallocs),
                    static_cast<unsigned long long>(after.device_frees - before.device_frees));
        // the deferred transparency check: a resident operand with c1 = 0 gives transparent sums, reported at the next
        // host-visible point
        HostCiphertext z = ct;
        std::fill(z.words.begin() + k * n, z.words.end(), 0);
        DeviceCiphertext dz(ctx);
        dz.upload(z);
        ev.apply_galois_dot_plain(dz, ge, gk, dplains, dout);
        const bool late = throws<std::logic_error>([&] { ev.synchronize(); }, "result ciphertext is transparent");
        std::printf("deferred transparency %s\n", late ? "ok" : "missing");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
