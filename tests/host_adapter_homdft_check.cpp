// The C++ host adapter's homomorphic DFT (gemini-seal_amd/host/evaluator.hpp: HomomorphicDFT, Evaluator::coeffs_to_slots,
// Evaluator::slots_to_coeffs). argv[1] = "host": on host-only contexts the plan's refusals arrive as std::invalid_argument
// before the missing device does as std::logic_error. argv[1] = device ordinal, argv[2..6] = five key primes (N = 256, one
// special prime, CKKS): on seeded inputs the host-ciphertext form and the DeviceCiphertext form give the words of the C ABI
// called directly, at the plan's level and the operand's scale; then the operand checks and their messages.
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
    for (std::uint32_t dir : { SEALHIP_DFT_COEFFS_TO_SLOTS, SEALHIP_DFT_SLOTS_TO_COEFFS })
    {
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 4, 2 }); }, "sum to log2(N/2)");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 7, 0 }); }, "zero layers");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 3, 2, 2 }); }, "more stages than levels");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 4, V{ 4, 3 }); }, "level k out of range");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 4, 3 }, V{ 3, 2 }); }, "n_baby");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 4, 3 }, V{ 2 }); }, "differ in length");
        ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 4, 3 }, V{}, 0.0); }, "gain");
        ok &= throws<std::logic_error>([&] { HomomorphicDFT d(ctx, dir, 3, V{ 4, 3 }); }, "host-only");
    }
    sealhip_params b{ SEALHIP_SCHEME_BFV, 8, 4, 1, mods, 786433ULL, SEALHIP_MODE_STRICT, -1 };
    Context bfv(b);
    ok &= throws<std::invalid_argument>([&] { HomomorphicDFT d(bfv, SEALHIP_DFT_COEFFS_TO_SLOTS, 3, V{ 4, 3 }); }, "CKKS only");
    if (!ok)
        return 1;
    std::printf("host-only homdft checks ok\n");
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
        std::uint64_t mods[5];
        parse_moduli(argv, 2, 5, mods);
        const std::size_t n = 256, k = 4, nk = 5, nd = 4;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 5, 1, mods, 0ULL, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        const std::vector<std::uint32_t> stages{ 4, 3 };
        HomomorphicDFT c2s(ctx, SEALHIP_DFT_COEFFS_TO_SLOTS, k, stages), s2c(ctx, SEALHIP_DFT_SLOTS_TO_COEFFS, k, stages);
        const std::size_t ko = c2s.out_level();
        bool ok = ko == 2 && s2c.out_level() == 2 && c2s.plan().needs_conjugation == 1 && !c2s.key_steps().empty();
        std::uint64_t state = 0x4023;
        auto random_ct = [&] {
            HostCiphertext c = host_ct(2, k, n, true);
            c.scale_ = 1048576.0;
            fill_rows(c.words.data(), 2 * k, n, mods, k, state);
            return c;
        };
        const HostCiphertext ct = random_ct(), ct2 = random_ct();
        std::vector<std::uint32_t> elts{ std::uint32_t(2 * n - 1) };
        for (const HomomorphicDFT *d : { &c2s, &s2c })
            for (std::uint32_t step : d->key_steps())
            {
                std::uint32_t elt = 0;
                throw_on(sealhip_galois_elt_from_step(ctx.get(), int(step), &elt));
                if (std::find(elts.begin(), elts.end(), elt) == elts.end())
                    elts.push_back(elt);
            }
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        std::vector<const sealhip_kswitch_key *> raw;
        for (std::uint32_t elt : elts)
        {
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elt] = keys.back().get();
            raw.push_back(keys.back()->get());
        }
        // the C ABI, called directly
        const std::size_t in_words = 2 * k * n, out_words = 2 * ko * n;
        std::uint64_t *d_a = nullptr, *d_b = nullptr, *d_o = nullptr;
        throw_on(sealhip_malloc(ctx.get(), in_words * 8, reinterpret_cast<void **>(&d_a)));
        throw_on(sealhip_malloc(ctx.get(), in_words * 8, reinterpret_cast<void **>(&d_b)));
        throw_on(sealhip_malloc(ctx.get(), 2 * out_words * 8, reinterpret_cast<void **>(&d_o)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_a, ct.data(), in_words * 8));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_b, ct2.data(), in_words * 8));
        std::vector<std::uint64_t> want_re(out_words), want_im(out_words), want_out(out_words);
        throw_on(sealhip_evaluator_coeffs_to_slots(ctx.get(), c2s.get(), d_a, 1, elts.data(), raw.data(), std::uint32_t(elts.size()),
                                                   d_o, d_o + out_words));
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), want_re.data(), d_o, out_words * 8));
        throw_on(sealhip_memcpy_d2h(ctx.get(), want_im.data(), d_o + out_words, out_words * 8));
        throw_on(sealhip_evaluator_slots_to_coeffs(ctx.get(), s2c.get(), d_a, d_b, 1, elts.data(), raw.data(),
                                                   std::uint32_t(elts.size()), d_o));
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), want_out.data(), d_o, out_words * 8));
        for (std::uint64_t *ptr : { d_a, d_b, d_o })
            throw_on(sealhip_free(ctx.get(), ptr));
        auto same = [&](const char *what, const HostCiphertext &c, const std::vector<std::uint64_t> &want) {
            const bool good = c.size() == 2 && c.coeff_modulus_size() == ko && c.is_ntt_form() && c.scale() == ct.scale() &&
                              c.words.size() == want.size() && std::memcmp(c.data(), want.data(), want.size() * 8) == 0;
            if (!good)
                std::printf("%s: the adapter's result differs from the C ABI's\n", what);
            return good;
        };
        Evaluator<HostCiphertext> ev(ctx);
        HostCiphertext re, im, out;
        ev.coeffs_to_slots(ct, c2s, gk, re, im);
        ok &= same("host re", re, want_re) && same("host im", im, want_im);
        ev.slots_to_coeffs(ct, ct2, s2c, gk, out);
        ok &= same("host out", out, want_out);
        DeviceCiphertext d(ctx), d2(ctx), dre(ctx), dim(ctx), dout(ctx);
        d.upload(ct);
        d2.upload(ct2);
        HostCiphertext back;
        ev.coeffs_to_slots(d, c2s, gk, dre, dim);
        dre.download(back);
        ok &= same("device re", back, want_re);
        dim.download(back);
        ok &= same("device im", back, want_im);
        ev.slots_to_coeffs(d, d2, s2c, gk, dout);
        dout.download(back);
        ok &= same("device out", back, want_out);
        // the operand checks
        const std::map<std::uint32_t, const KSwitchKeys *> none;
        HostCiphertext keep = host_ct(3, 1, n, false);
        ok &= throws<std::invalid_argument>([&] { ev.coeffs_to_slots(host_ct(2, 3, n, true), c2s, gk, keep, keep); },
                                            "not at the level of the DFT tables");
        ok &= throws<std::invalid_argument>([&] { ev.coeffs_to_slots(host_ct(2, k, n, false), c2s, gk, keep, keep); },
                                            "CKKS encrypted must be in NTT form");
        ok &= throws<std::invalid_argument>([&] { ev.coeffs_to_slots(host_ct(3, k, n, true), c2s, gk, keep, keep); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.coeffs_to_slots(ct, s2c, gk, keep, keep); }, "other direction");
        ok &= throws<std::invalid_argument>([&] { ev.slots_to_coeffs(ct, ct2, c2s, gk, keep); }, "other direction");
        ok &= throws<std::invalid_argument>([&] { ev.coeffs_to_slots(ct, c2s, none, keep, keep); }, "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.slots_to_coeffs(ct, ct2, s2c, none, keep); }, "Galois key not present");
        HostCiphertext other = ct2;
        other.scale_ = 2.0;
        ok &= throws<std::invalid_argument>([&] { ev.slots_to_coeffs(ct, other, s2c, gk, keep); }, "scale mismatch");
        ok &= keep.size() == 3 && keep.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        if (!ok)
            return 1;
        std::printf("homdft adapter checks ok\n");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
