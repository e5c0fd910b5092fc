// The C++ host adapter's bootstrap (gemini-seal_amd/host/evaluator.hpp: Bootstrapper, Evaluator::mod_raise, double_angle,
// eval_mod, bootstrap). argv[1] = "host": on host-only contexts the plans' refusals arrive as std::invalid_argument before the
// missing device does as std::logic_error. argv[1] = device ordinal, argv[2..12] = eleven key primes (N = 256, q_0, nine primes
// near 2 q_0, one special prime, CKKS): on seeded inputs the host-ciphertext form and the DeviceCiphertext form give the words
// of the C ABI called directly, at the plans' levels and scales; then the operand checks and their messages.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    bool ok = true;
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, -1 };
    Context ctx(p);
    using V = std::vector<std::uint32_t>;
    ok &= throws<std::invalid_argument>([&] { Bootstrapper b(ctx, 3, V{ 4, 2 }, V{ 7 }, 2, 0, 1); }, "sum to log2(N/2)");
    ok &= throws<std::invalid_argument>([&] { Bootstrapper b(ctx, 4, V{ 7 }, V{ 7 }, 2, 0, 1); }, "level k out of range");
    ok &= throws<std::invalid_argument>([&] { Bootstrapper b(ctx, 3, V{ 7 }, V{ 7 }, 0, 0, 1); }, "K must be at least 1");
    ok &= throws<std::invalid_argument>([&] { Bootstrapper b(ctx, 3, V{ 7 }, V{ 7 }, 2, 9, 1); }, "r must be at most 8");
    ok &= throws<std::invalid_argument>([&] { Bootstrapper b(ctx, 3, V{ 7 }, V{ 7 }, 2, 1, 3); }, "end of modulus switching chain");
    sealhip_params b{ SEALHIP_SCHEME_BFV, 8, 4, 1, mods, 786433ULL, SEALHIP_MODE_STRICT, -1 };
    Context bfv(b);
    ok &= throws<std::invalid_argument>([&] { Bootstrapper bb(bfv, 3, V{ 7 }, V{ 7 }, 2, 0, 1); }, "CKKS only");
    Evaluator<HostCiphertext> ev(ctx);
    HostCiphertext ct = host_ct(2, 1, 256, true), keep = host_ct(3, 1, 256, false);
    ct.scale_ = 1048576.0;
    ok &= throws<std::invalid_argument>([&] { ev.mod_raise(ct, 1, keep); }, "at least 2");
    ok &= throws<std::invalid_argument>([&] { ev.mod_raise(host_ct(2, 1, 256, false), 2, keep); }, "must be in NTT form");
    ok &= throws<std::invalid_argument>([&] { ev.double_angle(ct, {}, keep); }, "not enough relinearization keys");
    ok &= throws<std::invalid_argument>([&] { ev.eval_mod(ct, 2, 9, 7, {}, keep); }, "r must be at most 8");
    ok &= throws<std::logic_error>([&] { ev.mod_raise(ct, 3, keep); }, "host-only");
    ok &= keep.size() == 3 && keep.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
    if (!ok)
        return 1;
    std::printf("host-only bootstrap checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    try
    {
        if (argc < 2 || std::strcmp(argv[1], "host") == 0)
            return host_checks();
        if (argc < 13)
            return 2;
        const int device = std::atoi(argv[1]);
        std::uint64_t mods[11];
        parse_moduli(argv, 2, 11, mods);
        const std::size_t n = 256, k_top = 10, nk = 11, nd = 10;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 11, 1, mods, 0ULL, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        // ModRaise to 10, CoeffToSlot [4,3] to 8, EvalMod (K 2, r 1, degree 7) to 3, SlotToCoeff [4,3] to 1
        const std::vector<std::uint32_t> stages{ 4, 3 };
        const std::uint32_t K = 2, r = 1, degree = 7;
        Bootstrapper boot(ctx, k_top, stages, stages, K, r, degree);
        const sealhip_bootstrap_plan &bp = boot.plan();
        bool ok = bp.c2s_out_level == 8 && bp.evalmod_out_level == 3 && boot.out_level() == 1 && !boot.key_steps().empty() &&
                  bp.raise_scale == double(mods[0]) * K;
        std::uint64_t state = 0x4024;
        auto random_ct = [&](std::size_t k, double scale) {
            HostCiphertext c = host_ct(2, k, n, true);
            c.scale_ = scale;
            fill_rows(c.words.data(), 2 * k, n, mods, k, state);
            return c;
        };
        auto random_key = [&] {
            return seeded_key(ctx, nd, nk, n, mods, state);
        };
        std::vector<std::uint32_t> elts{ std::uint32_t(2 * n - 1) };
        for (std::uint32_t step : boot.key_steps())
        {
            std::uint32_t elt = 0;
            throw_on(sealhip_galois_elt_from_step(ctx.get(), int(step), &elt));
            elts.push_back(elt);
        }
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        std::vector<const sealhip_kswitch_key *> raw;
        for (std::uint32_t elt : elts)
        {
            keys.push_back(random_key());
            gk[elt] = keys.back().get();
            raw.push_back(keys.back()->get());
        }
        const std::unique_ptr<KSwitchKeys> relin = random_key();
        const std::vector<const KSwitchKeys *> rk{ relin.get() };
        const sealhip_kswitch_key *relin_raw = relin->get();
        const double delta = 1048576.0;
        const HostCiphertext low = random_ct(2, delta), mid = random_ct(6, double(mods[0]) * K);

        // the C ABI, called directly
        sealhip_evalmod_plan ep{};
        throw_on(sealhip_evaluator_evalmod_plan(ctx.get(), 6, mid.scale(), K, r, degree, 0, 0.0, &ep));
        ok &= ep.out_level == 1;
        std::uint64_t *d_low = nullptr, *d_mid = nullptr, *d_o = nullptr;
        throw_on(sealhip_malloc(ctx.get(), 2 * 2 * n * 8, reinterpret_cast<void **>(&d_low)));
        throw_on(sealhip_malloc(ctx.get(), 2 * 6 * n * 8, reinterpret_cast<void **>(&d_mid)));
        throw_on(sealhip_malloc(ctx.get(), 2 * k_top * n * 8, reinterpret_cast<void **>(&d_o)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_low, low.data(), 2 * 2 * n * 8));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_mid, mid.data(), 2 * 6 * n * 8));
        auto fetch = [&](std::size_t k) {
            std::vector<std::uint64_t> w(2 * k * n);
            throw_on(sealhip_synchronize(ctx.get()));
            throw_on(sealhip_memcpy_d2h(ctx.get(), w.data(), d_o, w.size() * 8));
            return w;
        };
        throw_on(sealhip_evaluator_mod_raise(ctx.get(), 2, d_low, 1, 5, d_o));
        const std::vector<std::uint64_t> want_raise = fetch(5);
        double da_scale = 0.0;
        throw_on(sealhip_evaluator_double_angle(ctx.get(), 6, d_mid, 1, mid.scale(), &relin_raw, 1, d_o, &da_scale));
        const std::vector<std::uint64_t> want_da = fetch(5);
        throw_on(sealhip_evaluator_eval_mod(ctx.get(), 6, d_mid, 1, mid.scale(), K, r, degree, 0, 0.0, &relin_raw, 1, d_o, nullptr,
                                            nullptr));
        const std::vector<std::uint64_t> want_em = fetch(1);
        throw_on(sealhip_evaluator_bootstrap(ctx.get(), boot.get(), 2, d_low, 1, elts.data(), raw.data(), std::uint32_t(elts.size()),
                                             &relin_raw, 1, d_o));
        const std::vector<std::uint64_t> want_boot = fetch(1);
        for (std::uint64_t *ptr : { d_low, d_mid, d_o })
            throw_on(sealhip_free(ctx.get(), ptr));
        auto same = [&](const char *what, const HostCiphertext &c, std::size_t k, double scale, const std::vector<std::uint64_t> &want) {
            const bool good = c.size() == 2 && c.coeff_modulus_size() == k && c.is_ntt_form() && c.scale() == scale &&
                              c.words.size() == want.size() && std::memcmp(c.data(), want.data(), want.size() * 8) == 0;
            if (!good)
                std::printf("%s: the adapter's result differs from the C ABI's\n", what);
            return good;
        };
        Evaluator<HostCiphertext> ev(ctx);
        HostCiphertext out;
        ev.mod_raise(low, 5, out);
        ok &= same("host mod_raise", out, 5, delta, want_raise);
        ev.double_angle(mid, rk, out);
        ok &= same("host double_angle", out, 5, da_scale, want_da) && da_scale == mid.scale() * mid.scale() / double(mods[5]);
        ev.eval_mod(mid, K, r, degree, rk, out);
        ok &= same("host eval_mod", out, 1, ep.scales[r], want_em);
        ev.bootstrap(low, boot, gk, rk, out);
        ok &= same("host bootstrap", out, 1, delta, want_boot);
        DeviceCiphertext d_l(ctx), d_m(ctx), d_out(ctx);
        d_l.upload(low);
        d_m.upload(mid);
        HostCiphertext back;
        ev.mod_raise(d_l, 5, d_out);
        d_out.download(back);
        ok &= same("device mod_raise", back, 5, delta, want_raise);
        ev.double_angle(d_m, rk, d_out);
        d_out.download(back);
        ok &= same("device double_angle", back, 5, da_scale, want_da);
        ev.eval_mod(d_m, K, r, degree, rk, d_out);
        d_out.download(back);
        ok &= same("device eval_mod", back, 1, ep.scales[r], want_em);
        ev.bootstrap(d_l, boot, gk, rk, d_out);
        d_out.download(back);
        ok &= same("device bootstrap", back, 1, delta, want_boot);
        // the operand checks
        const std::map<std::uint32_t, const KSwitchKeys *> none;
        HostCiphertext keep = host_ct(3, 1, n, false);
        ok &= throws<std::invalid_argument>([&] { ev.bootstrap(host_ct(2, 2, n, false), boot, gk, rk, keep); },
                                            "CKKS encrypted must be in NTT form");
        ok &= throws<std::invalid_argument>([&] { ev.bootstrap(host_ct(3, 2, n, true), boot, gk, rk, keep); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.bootstrap(low, boot, none, rk, keep); }, "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.bootstrap(low, boot, gk, {}, keep); }, "not enough relinearization keys");
        ok &= throws<std::invalid_argument>([&] { ev.mod_raise(low, 1, keep); }, "at least 2");
        ok &= throws<std::invalid_argument>([&] { ev.eval_mod(low, K, 3, degree, rk, keep); }, "end of modulus switching chain");
        ok &= keep.size() == 3 && keep.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        if (!ok)
            return 1;
        std::printf("bootstrap adapter checks ok\n");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
