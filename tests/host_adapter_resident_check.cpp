// The resident overloads of the C++ host adapter (gemini-seal_amd/host/evaluator.hpp: DeviceCiphertext, the pooled
// Evaluator overloads, the deferred transparency check). Without a device it only checks that everything compiles and links
// and that a host-only context refuses resident work. With a device (argv[1] = ordinal) it prints one line per check; the
// Python test (tests/test_gpu_adapter_resident.py) reads them.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

namespace
{
    unsigned long long digest(const HostCiphertext &ct)
    {
        return (unsigned long long)adapter_check::digest(ct.words);
    }

    HostCiphertext down(const DeviceCiphertext &d)
    {
        HostCiphertext h;
        d.download(h);
        return h;
    }

    DeviceCiphertext up(const Context &c, const HostCiphertext &h)
    {
        DeviceCiphertext d(c);
        d.upload(h);
        return d;
    }

    bool same(const HostCiphertext &h, const DeviceCiphertext &d)
    {
        const HostCiphertext g = down(d);
        return g.words == h.words && g.size() == h.size() && g.coeff_modulus_size() == h.coeff_modulus_size() &&
               g.is_ntt_form() == h.is_ntt_form();
    }

    struct sealhip_pool_stats stats(const Context &c)
    {
        struct sealhip_pool_stats s{};
        throw_on(sealhip_pool_stats(c.get(), &s));
        return s;
    }

    // the words of a random size-2 ciphertext at level k
    HostCiphertext random_ct(std::uint64_t &state, const std::uint64_t *mods, std::size_t n, std::size_t k, bool ntt)
    {
        HostCiphertext ct = host_ct(2, k, n, ntt);
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        return ct;
    }

    template <class F>
    bool throws_transparent(F &&f)
    {
        try
        {
            f();
        }
        catch (const std::logic_error &e)
        {
            return std::strcmp(e.what(), "result ciphertext is transparent") == 0;
        }
        return false;
    }

    // every resident method and destination-taking variant against its host overload, word for word
    bool resident_equals_host(const Context &ctx, std::uint32_t scheme, const std::uint64_t *mods, std::size_t n,
                              std::size_t k, const KSwitchKeys &rk, std::uint64_t seed)
    {
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        std::uint64_t st = seed;
        const HostCiphertext x = random_ct(st, mods, n, k, !bfv), y = random_ct(st, mods, n, k, !bfv);
        Evaluator<HostCiphertext> ev(ctx);
        const DeviceCiphertext dx = up(ctx, x), dy = up(ctx, y);
        bool ok = true;
        const auto expect = [&](const char *what, const HostCiphertext &h, const DeviceCiphertext &d) {
            if (!same(h, d))
            {
                std::printf("mismatch: %s (scheme %u, k %zu)\n", what, scheme, k);
                ok = false;
            }
        };
        const std::vector<const KSwitchKeys *> rks{ &rk };
        std::uint32_t e1 = 0, ec = 0;
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &e1));
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 0, &ec));
        const std::map<std::uint32_t, const KSwitchKeys *> gks{ { e1, &rk }, { ec, &rk } };
        {
            HostCiphertext h = x;
            DeviceCiphertext d = dx;
            ev.negate_inplace(h);
            ev.negate_inplace(d);
            expect("negate_inplace", h, d);
            HostCiphertext hd;
            DeviceCiphertext dd(ctx);
            ev.negate(x, hd);
            ev.negate(dx, dd);
            expect("negate", hd, dd);
        }
        for (int sub = 0; sub < 2; sub++)
        {
            HostCiphertext h = x, ha, hb = y;
            DeviceCiphertext d = dx, da(ctx), db = dy;
            if (sub)
            {
                ev.sub_inplace(h, y);
                ev.sub_inplace(d, dy);
                ev.sub(x, y, ha);
                ev.sub(dx, dy, da);
                ev.sub(x, hb, hb); // destination aliases encrypted2
                ev.sub(dx, db, db);
            }
            else
            {
                ev.add_inplace(h, y);
                ev.add_inplace(d, dy);
                ev.add(x, y, ha);
                ev.add(dx, dy, da);
                ev.add(x, hb, hb);
                ev.add(dx, db, db);
            }
            expect(sub ? "sub_inplace" : "add_inplace", h, d);
            expect(sub ? "sub" : "add", ha, da);
            expect(sub ? "sub aliased" : "add aliased", hb, db);
        }
        {
            HostCiphertext hm, hs, hr, hms, hmt, hb = y;
            DeviceCiphertext dm(ctx), ds(ctx), dr(ctx), dms(ctx), dmt(ctx), db = dy;
            ev.multiply(x, y, hm);
            ev.multiply(dx, dy, dm);
            expect("multiply", hm, dm);
            ev.multiply(x, hb, hb);
            ev.multiply(dx, db, db);
            expect("multiply aliased", hb, db);
            ev.square(x, hs);
            ev.square(dx, ds);
            expect("square", hs, ds);
            DeviceCiphertext dxx = dx;
            ev.multiply_inplace(dxx, dx);
            expect("square == multiply(x, x)", down(dxx), ds);
            ev.relinearize(hm, rks, hr);
            ev.relinearize(dm, rks, dr);
            expect("relinearize", hr, dr);
            if (k > 1)
            {
                if (bfv)
                {
                    ev.mod_switch_to_next(hr, hms);
                    ev.mod_switch_to_next(dr, dms);
                    expect("mod_switch_to_next", hms, dms);
                    ev.mod_switch_to(hr, 1, hmt);
                    ev.mod_switch_to(dr, 1, dmt);
                    expect("mod_switch_to", hmt, dmt);
                }
                else
                {
                    ev.rescale_to_next(hr, hms);
                    ev.rescale_to_next(dr, dms);
                    expect("rescale_to_next", hms, dms);
                    ev.rescale_to(hr, 1, hmt);
                    ev.rescale_to(dr, 1, dmt);
                    expect("rescale_to", hmt, dmt);
                }
            }
        }
        {
            HostCiphertext ha, hmm, hex;
            DeviceCiphertext da(ctx), dmm(ctx), dex(ctx);
            ev.add_many({ x, y, x }, ha);
            ev.add_many(std::vector<DeviceCiphertext>{ dx, dy, dx }, da);
            expect("add_many", ha, da);
            if (bfv)
            {
                ev.multiply_many({ x, y, x }, rks, hmm);
                ev.multiply_many(std::vector<DeviceCiphertext>{ dx, dy, dx }, rks, dmm);
                expect("multiply_many", hmm, dmm);
                ev.exponentiate(x, 3, rks, hex);
                ev.exponentiate(dx, 3, rks, dex);
                expect("exponentiate", hex, dex);
            }
        }
        {
            std::vector<std::uint64_t> plain(bfv ? n : k * n);
            for (std::size_t i = 0; i < plain.size(); i++)
                plain[i] = bfv ? splitmix(st) % ctx.plain_modulus() : splitmix(st) % mods[i / n];
            HostCiphertext hp, ha, hs;
            DeviceCiphertext dp(ctx), da(ctx), ds(ctx);
            ev.multiply_plain(x, plain.data(), !bfv, hp);
            ev.multiply_plain(dx, plain.data(), !bfv, dp);
            expect("multiply_plain", hp, dp);
            ev.add_plain(x, plain.data(), !bfv, ha);
            ev.add_plain(dx, plain.data(), !bfv, da);
            expect("add_plain", ha, da);
            ev.sub_plain(x, plain.data(), !bfv, hs);
            ev.sub_plain(dx, plain.data(), !bfv, ds);
            expect("sub_plain", hs, ds);
        }
        {
            HostCiphertext h1, h2;
            DeviceCiphertext d1(ctx), d2(ctx);
            if (bfv)
            {
                ev.transform_to_ntt(x, h1);
                ev.transform_to_ntt(dx, d1);
                expect("transform_to_ntt", h1, d1);
                ev.transform_from_ntt(h1, h2);
                ev.transform_from_ntt(d1, d2);
                expect("transform_from_ntt", h2, d2);
                ev.rotate_rows(x, 1, gks, h1);
                ev.rotate_rows(dx, 1, gks, d1);
                expect("rotate_rows", h1, d1);
                ev.rotate_columns(x, gks, h2);
                ev.rotate_columns(dx, gks, d2);
                expect("rotate_columns", h2, d2);
            }
            else
            {
                ev.transform_from_ntt(x, h1);
                ev.transform_from_ntt(dx, d1);
                expect("transform_from_ntt", h1, d1);
                ev.rotate_vector(x, 1, gks, h1);
                ev.rotate_vector(dx, 1, gks, d1);
                expect("rotate_vector", h1, d1);
                ev.complex_conjugate(x, gks, h2);
                ev.complex_conjugate(dx, gks, d2);
                expect("complex_conjugate", h2, d2);
            }
            HostCiphertext hg;
            DeviceCiphertext dg(ctx);
            ev.apply_galois(x, e1, rk, hg);
            ev.apply_galois(dx, e1, rk, dg);
            expect("apply_galois", hg, dg);
            if (bfv)
                std::printf("apply_galois %u digest %016llx\n", k == 2 ? 1u : 0u, digest(hg));
        }
        ev.synchronize();
        return ok;
    }

    // A client on a context: ternary secret key (NTT form, made with the context's own transform), public, relinearization
    // and Galois keys from the adapter's KeyGenerator, deterministic samplers. Checks the resident Encryptor / Decryptor
    // overloads against the host ones (same samples: same words), the round trip, DevicePlaintext operations against host
    // plaintexts, and that a second pass of encrypt -> multiply -> relinearize -> mod_switch -> rotate -> decrypt makes no
    // pool hipMalloc / hipFree.
    bool client_side(const Context &ctx, const std::uint64_t *mods, std::size_t nk, const char *tag)
    {
        const std::size_t n = ctx.n(), k = nk - 1;
        std::uint64_t st = 0xC11E47 + nk;
        std::vector<std::uint64_t> sk(nk * n);
        for (std::size_t c = 0; c < n; c++)
        {
            const int v = int(splitmix(st) % 3) - 1;
            for (std::size_t r = 0; r < nk; r++)
                sk[r * n + c] = v < 0 ? mods[r] - 1 : std::uint64_t(v);
        }
        {
            Staged d(ctx, nk * n);
            d.up(sk.data(), nk * n);
            throw_on(sealhip_ntt_negacyclic_harvey(ctx.get(), d.ptr(), 1, std::uint32_t(k), SEALHIP_BASE_KEY));
            d.down(sk.data(), nk * n);
        }
        std::uint64_t sample_state = 1;
        const auto reset = [&] { sample_state = 0xABCDEF; };
        const auto noise = [&](std::int32_t *e) {
            for (std::size_t i = 0; i < n; i++)
                e[i] = std::int32_t(splitmix(sample_state) % 7) - 3;
        };
        KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *seed, std::int32_t *e) {
            for (int i = 0; i < 8; i++)
                seed[i] = splitmix(sample_state);
            noise(e);
        });
        const std::vector<std::uint64_t> pk = kg.public_key();
        auto relin = kg.relin_keys(1);
        auto galois = kg.galois_keys(std::vector<int>{ 1 });
        std::map<std::uint32_t, const KSwitchKeys *> gks;
        for (auto &kv : galois)
            gks[kv.first] = kv.second.get();
        const std::vector<const KSwitchKeys *> rks{ relin[0].get() };
        Encryptor<HostCiphertext> enc(ctx, pk.data(), sk.data(),
                                      [&](std::int32_t *u, std::int32_t *e0, std::int32_t *e1) {
                                          for (std::size_t i = 0; i < n; i++)
                                              u[i] = std::int32_t(splitmix(sample_state) % 3) - 1;
                                          noise(e0);
                                          noise(e1);
                                      },
                                      [&](std::uint64_t *seed, std::int32_t *e) {
                                          for (int i = 0; i < 8; i++)
                                              seed[i] = splitmix(sample_state);
                                          noise(e);
                                      });
        Decryptor<HostCiphertext> dec(ctx, sk.data());
        Evaluator<HostCiphertext> ev(ctx);
        HostPlaintext m{ std::vector<std::uint64_t>(n), 0, false, 1.0 };
        for (auto &v : m.words)
            v = splitmix(st) % ctx.plain_modulus();
        bool ok = true;
        // the same samples give the same words, host or resident, public or secret key
        for (int sym = 0; sym < 2; sym++)
        {
            HostCiphertext h; // (a HostCiphertext destination of the host Encryptor carries its N)
            h.n_ = n;
            DeviceCiphertext d(ctx);
            reset();
            sym ? enc.encrypt_symmetric(m, h) : enc.encrypt(m, h);
            reset();
            sym ? enc.encrypt_symmetric(m, d) : enc.encrypt(m, d);
            std::vector<std::uint64_t> ph, pd;
            dec.decrypt(h, ph);
            dec.decrypt(d, pd);
            ph.resize(n, 0);
            pd.resize(n, 0);
            ok = ok && same(h, d) && ph == pd && ph == m.words && dec.invariant_noise_budget(h) == dec.invariant_noise_budget(d) &&
                 dec.invariant_noise_budget(d) > 0;
            HostCiphertext hz;
            hz.n_ = n;
            DeviceCiphertext dz(ctx);
            reset();
            enc.encrypt_zero(hz);
            reset();
            enc.encrypt_zero(dz);
            ok = ok && same(hz, dz);
        }
        std::printf("client %s %s\n", tag, ok ? "ok" : "FAILED");
        // DevicePlaintext: plain operations, transform_to_ntt and mod_switch_to against the host plaintext forms
        {
            DeviceCiphertext d(ctx);
            HostCiphertext h;
            h.n_ = n;
            reset();
            enc.encrypt(m, h);
            d.upload(h);
            DevicePlaintext dp(ctx);
            dp.upload(m.words, false);
            HostCiphertext hm = h, ha = h;
            DeviceCiphertext dm = d, da = d;
            ev.multiply_plain_inplace(hm, m.words.data(), false);
            ev.multiply_plain_inplace(dm, dp);
            ev.add_plain_inplace(ha, m.words.data(), false);
            ev.add_plain_inplace(da, dp);
            std::vector<std::uint64_t> hn = m.words, hs;
            bool is_ntt = false;
            ev.transform_to_ntt_inplace(hn, k, is_ntt);
            DevicePlaintext dn(ctx);
            ev.transform_to_ntt(dp, k, dn);
            std::vector<std::uint64_t> dn_words, ds_words;
            dn.download(dn_words);
            ev.mod_switch_to(hn, true, 1, hs);
            DevicePlaintext ds(ctx);
            ev.mod_switch_to(dn, 1, ds);
            ds.download(ds_words);
            const bool pl = same(hm, dm) && same(ha, da) && dn_words == hn && ds_words == hs && ds.coeff_modulus_size() == 1;
            std::printf("device plaintext %s %s\n", tag, pl ? "ok" : "FAILED");
            ok = ok && pl;
        }
        // the chain twice; the second pass makes no allocator call
        struct sealhip_pool_stats before{}, after{};
        std::vector<std::uint64_t> out;
        for (int iter = 0; iter < 2; iter++)
        {
            if (iter == 1)
            {
                ev.synchronize();
                before = stats(ctx);
            }
            DeviceCiphertext a(ctx), b(ctx);
            enc.encrypt(m, a);
            enc.encrypt(m, b);
            ev.multiply_inplace(a, b);
            ev.relinearize_inplace(a, rks);
            ev.mod_switch_to_next_inplace(a);
            ev.rotate_rows_inplace(a, 1, gks);
            dec.decrypt(a, out);
            ev.synchronize();
        }
        after = stats(ctx);
        const bool warm = after.device_mallocs == before.device_mallocs && after.device_frees == before.device_frees;
        std::printf("warm chain %s %s (mallocs %llu, hits %llu)\n", tag, warm ? "ok" : "FAILED",
                    (unsigned long long)after.device_mallocs, (unsigned long long)after.hits);
        return ok && warm;
    }
} // namespace

int main(int argc, char **argv)
{
    // cfg1 of BASELINE.json: BFV N=4096, {36,36,37}
    const std::uint64_t mods[3] = { 68719230977ULL, 68719403009ULL, 137438822401ULL };
    sealhip_params p{ SEALHIP_SCHEME_BFV, 12, 3, 1, mods, 786433, SEALHIP_MODE_PARITY, argc > 1 ? std::atoi(argv[1]) : -1 };
    try
    {
        Context ctx(p);
        if (p.device < 0)
        {
            // resident work needs a device: the pool refuses a host-only context
            bool refused = false;
            try
            {
                DeviceCiphertext d(ctx);
                d.resize(2);
            }
            catch (const std::logic_error &)
            {
                refused = true;
            }
            struct sealhip_pool_stats s{};
            throw_on(sealhip_pool_stats(ctx.get(), &s));
            std::printf("host-only resident checks %s\n", refused && s.device_mallocs == 0 ? "ok" : "FAILED");
            return refused ? 0 : 1;
        }
        const std::size_t n = 4096, k = 2;
        std::uint64_t state = 0xC0FFEE + 1;
        // the survey generator's fill order (keys first), as tests/host_adapter_check.cpp
        std::vector<std::uint64_t> key(2 * 2 * 3 * n);
        fill_rows(key.data(), 2 * 2 * 3, n, mods, 3, state);
        const HostCiphertext a = random_ct(state, mods, n, k, false), b = random_ct(state, mods, n, k, false);
        Evaluator<HostCiphertext> ev(ctx);
        KSwitchKeys rk(ctx, key.data(), 2);

        // the cfg1 golden chain on resident ciphertexts
        DeviceCiphertext da = up(ctx, a), db = up(ctx, b);
        ev.multiply_inplace(da, db);
        ev.relinearize_inplace(da, { &rk });
        ev.mod_switch_to_next_inplace(da);
        std::printf("resident modswitch digest %016llx\n", digest(down(da)));

        // every method and destination-taking variant, BFV and CKKS, two levels, nsp 1 and 2
        bool eq = true;
        for (std::size_t kk : { std::size_t(2), std::size_t(1) })
            eq = resident_equals_host(ctx, SEALHIP_SCHEME_BFV, mods, n, kk, rk, 11 + kk) && eq;
        {
            sealhip_params pc{ SEALHIP_SCHEME_CKKS, 12, 3, 1, mods, 0, SEALHIP_MODE_PARITY, p.device };
            Context cctx(pc);
            KSwitchKeys gk(cctx, key.data(), 2);
            for (std::size_t kk : { std::size_t(2), std::size_t(1) })
                eq = resident_equals_host(cctx, SEALHIP_SCHEME_CKKS, mods, n, kk, gk, 21 + kk) && eq;
        }
        {
            // nsp = 2: one ciphertext prime, two special primes; the key has one digit of 1 + 2 rows
            sealhip_params p2{ SEALHIP_SCHEME_BFV, 12, 3, 2, mods, 786433, SEALHIP_MODE_PARITY, p.device };
            Context ctx2(p2);
            KSwitchKeys rk2(ctx2, key.data(), 1);
            eq = resident_equals_host(ctx2, SEALHIP_SCHEME_BFV, mods, n, 1, rk2, 31) && eq;
        }
        std::printf("resident equals host %s\n", eq ? "ok" : "FAILED");

        // after one warm-up pass, the same chain makes no allocator call
        {
            std::uint32_t e1 = 0;
            throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &e1));
            const std::map<std::uint32_t, const KSwitchKeys *> gks{ { e1, &rk } };
            struct sealhip_pool_stats before{}, after{};
            for (int iter = 0; iter < 2; iter++)
            {
                if (iter == 1)
                {
                    ev.synchronize();
                    before = stats(ctx);
                }
                DeviceCiphertext x = up(ctx, a), y = up(ctx, b);
                ev.multiply_inplace(x, y);
                ev.relinearize_inplace(x, { &rk });
                ev.mod_switch_to_next_inplace(x);
                ev.rotate_rows_inplace(x, 1, gks);
                ev.synchronize();
            }
            after = stats(ctx);
            const bool warm = after.device_mallocs == before.device_mallocs && after.device_frees == before.device_frees &&
                              after.hits > before.hits;
            std::printf("warm pool %s (mallocs %llu, hits %llu)\n", warm ? "ok" : "FAILED",
                        (unsigned long long)after.device_mallocs, (unsigned long long)after.hits);
            eq = eq && warm;
        }

        // transparency: late, on the resident path only
        {
            DeviceCiphertext x = up(ctx, a), z(ctx);
            ev.sub(x, x, z); // no exception yet: the check is deferred
            const bool late = throws_transparent([&] { ev.synchronize(); });
            DeviceCiphertext w(ctx);
            ev.sub(x, x, w);
            HostCiphertext sink;
            const bool at_download = throws_transparent([&] { w.download(sink); });
            bool normal = true;
            try
            {
                DeviceCiphertext m = up(ctx, a), m2 = up(ctx, b);
                ev.multiply_inplace(m, m2);
                ev.relinearize_inplace(m, { &rk });
                ev.synchronize();
            }
            catch (const std::exception &)
            {
                normal = false;
            }
            bool host_silent = true;
            try
            {
                HostCiphertext h = a, hz;
                ev.sub(h, h, hz);
                ev.synchronize();
            }
            catch (const std::exception &)
            {
                host_silent = false;
            }
            // multiply_many over transparent inputs: the composite entry, caught through sealhip_transparency_note
            HostCiphertext t = a;
            std::fill(t.words.begin() + std::ptrdiff_t(k * n), t.words.end(), 0);
            const DeviceCiphertext dt = up(ctx, t);
            DeviceCiphertext prod(ctx);
            ev.multiply_many(std::vector<DeviceCiphertext>{ dt, dt }, { &rk }, prod);
            const bool many = throws_transparent([&] { ev.synchronize(); });
            const bool tr = late && at_download && normal && host_silent && many;
            std::printf("transparency %s (%d %d %d %d %d)\n", tr ? "ok" : "FAILED", late, at_download, normal, host_silent, many);
            eq = eq && tr;
        }

        // wire format: save of a resident ciphertext == sealhip_ciphertext_save of the same words; load evaluates like upload
        {
            for (std::size_t kk = 1; kk <= 3; kk++)
            {
                const std::uint64_t pid[4] = { 0x1000 + kk, 2, 3, 4 };
                ctx.set_parms_id(kk, pid);
            }
            const DeviceCiphertext x = up(ctx, b);
            std::vector<std::uint8_t> saved;
            x.save(saved);
            sealhip_ciphertext_info info{};
            info.parms_id[0] = 0x1000 + k;
            info.parms_id[1] = 2;
            info.parms_id[2] = 3;
            info.parms_id[3] = 4;
            info.is_ntt_form = 0;
            info.size = 2;
            info.coeff_modulus_size = std::uint32_t(k);
            info.poly_modulus_degree = n;
            info.scale = 1.0;
            Staged s(ctx, 2 * k * n);
            s.up(b.data(), 2 * k * n);
            std::size_t need = 0, written = 0;
            throw_on(sealhip_ciphertext_save_size(ctx.get(), 2, std::uint32_t(k), &need));
            std::vector<std::uint8_t> raw(need);
            throw_on(sealhip_ciphertext_save(ctx.get(), &info, s.ptr(), raw.data(), need, &written));
            raw.resize(written);
            DeviceCiphertext loaded(ctx), uploaded = up(ctx, a);
            loaded.load(saved.data(), saved.size());
            DeviceCiphertext via_upload = up(ctx, b);
            ev.multiply_inplace(uploaded, loaded);
            DeviceCiphertext again = up(ctx, a);
            ev.multiply_inplace(again, via_upload);
            const bool wire = saved == raw && same(down(again), uploaded);
            std::printf("wire %s\n", wire ? "ok" : "FAILED");
            eq = eq && wire;
        }
        // the client side on cfg1, and on cfg3 when its primes are given (argv[2..])
        eq = client_side(ctx, mods, 3, "cfg1") && eq;
        if (argc > 3)
        {
            std::vector<std::uint64_t> m3;
            for (int i = 2; i < argc; i++)
                m3.push_back(std::strtoull(argv[i], nullptr, 10));
            sealhip_params p3{ SEALHIP_SCHEME_BFV, 15, std::uint32_t(m3.size()), 1, m3.data(), 786433, SEALHIP_MODE_PARITY,
                               p.device };
            Context ctx3(p3);
            eq = client_side(ctx3, m3.data(), m3.size(), "cfg3") && eq;
        }
        return eq ? 0 : 1;
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
