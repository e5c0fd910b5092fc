// The C++ host adapter's merged mod-down and rescale (gemini-seal_amd/host/evaluator.hpp: relinearize_rescale,
// dot_product_rescale, apply_galois_dot_plain_rescale, rotate_vector_dot_plain_rescale, apply_galois_bsgs_plain_rescale,
// rotate_vector_bsgs_plain_rescale). argv[1] = "host": on host-only contexts, the scheme, the operand
// checks of the unmerged methods, "end of modulus switching chain reached" at the last level, and a valid call reaching the
// ABI (which has no CPU fallback); the methods that take a key object stop where one is needed (a key cannot exist without
// a device). argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 256, one special prime): digests of every
// method's result on the host ciphertext type and on DeviceCiphertext / DevicePlaintext for seeded inputs, which the Python
// test compares with the C ABI's output for the same inputs; the size, level, form and scale of the result.
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
        ok &= ctx.key_modulus(1) == mods[1];
        Evaluator<HostCiphertext> ev(ctx);
        const std::map<std::uint32_t, const KSwitchKeys *> none;
        const std::vector<const KSwitchKeys *> no_keys;
        HostCiphertext out = host_ct(3, 1, n, false);
        std::vector<HostCiphertext> outs(1, out);
        const HostCiphertext good = host_ct(2, 2, n, !bfv), wrong_form = host_ct(2, 2, n, bfv), three = host_ct(3, 2, n, !bfv);
        const HostCiphertext last = host_ct(2, 1, n, !bfv), last3 = host_ct(3, 1, n, !bfv);
        const HostPlaintext w = host_plain(n_key, n, true, 4.0);
        const Plains one{ { w } }, two{ { w, w } };
        if (bfv)
        {
            // the merged rescale is a CKKS operation (rescale_to_next: "unsupported scheme")
            ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain_rescale(good, { 1 }, none, one, outs); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_dot_plain_rescale(good, { 0 }, none, one, outs); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain_rescale(good, { 1 }, { 1 }, none, one, out); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.rotate_vector_bsgs_plain_rescale(good, { 0 }, { 0 }, none, one, out); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.relinearize_rescale(three, no_keys, out); }, "unsupported scheme");
            // an operand at the last level breaks two rules: the scheme's refusal comes first
            ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain_rescale(last, { 1 }, none, one, outs); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain_rescale(last, { 1 }, { 1 }, none, one, out); },
                                           "unsupported scheme");
            ok &= throws<std::logic_error>([&] { ev.relinearize_rescale(last3, no_keys, out); }, "unsupported scheme");
            ok &= out.size() == 3 && out.coeff_modulus_size() == 1 && outs.size() == 1;
            continue;
        }
        // the unmerged methods' operand checks
        const char *form = "CKKS encrypted must be in NTT form";
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(wrong_form, { 1 }, none, one, outs); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(wrong_form, { 1 }, { 1 }, none, one, out); },
                                            form);
        ok &= throws<std::invalid_argument>([&] { ev.relinearize_rescale(host_ct(3, 2, n, false), no_keys, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(three, { 1 }, none, one, outs); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(three, { 1 }, { 1 }, none, one, out); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.relinearize_rescale(good, no_keys, out); }, "encrypted size must be 3");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(good, { 3 }, none, one, outs); },
                                            "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(good, { 1 }, { 3 }, none, one, out); },
                                            "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(good, { 1 }, none, two, outs); },
                                            "one plaintext per Galois element");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(good, { 1 }, { 1 }, none, two, out); },
                                            "one plaintext per Galois element");
        ok &= throws<std::invalid_argument>([&] { ev.relinearize_rescale(three, no_keys, out); },
                                            "not enough relinearization keys");
        // the last level has nothing to rescale to
        const char *chain = "end of modulus switching chain reached";
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(last, { 1 }, none, one, outs); }, chain);
        ok &= throws<std::invalid_argument>([&] { ev.rotate_vector_dot_plain_rescale(last, { 0 }, none, one, outs); }, chain);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(last, { 1 }, { 1 }, none, one, out); }, chain);
        ok &= throws<std::invalid_argument>([&] { ev.rotate_vector_bsgs_plain_rescale(last, { 0 }, { 0 }, none, one, out); }, chain);
        ok &= throws<std::invalid_argument>([&] { ev.relinearize_rescale(last3, no_keys, out); }, chain);
        // a coefficient-form operand at the last level breaks two rules: the form's refusal comes first
        const HostCiphertext last_coeff = host_ct(2, 1, n, false), last3_coeff = host_ct(3, 1, n, false);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_dot_plain_rescale(last_coeff, { 1 }, none, one, outs); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_bsgs_plain_rescale(last_coeff, { 1 }, { 1 }, none, one, out); },
                                            form);
        ok &= throws<std::invalid_argument>([&] { ev.relinearize_rescale(last3_coeff, no_keys, out); }, form);
        ok &= out.size() == 3 && out.coeff_modulus_size() == 1 && outs.size() == 1; // (a refused call leaves the destinations alone)
        // a valid call (element 1 / step 0 needs no key) reaches the device, which a host-only context does not have
        ok &= throws<std::logic_error>([&] { ev.apply_galois_dot_plain_rescale(good, { 1 }, none, one, outs); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.rotate_vector_dot_plain_rescale(good, { 0 }, none, one, outs); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.apply_galois_bsgs_plain_rescale(good, { 1 }, { 1 }, none, one, out); }, "host-only");
        ok &= throws<std::logic_error>([&] { ev.rotate_vector_bsgs_plain_rescale(good, { 0 }, { 0 }, none, one, out); },
                                       "host-only");
    }
    if (!ok)
        return 1;
    std::printf("host-only ks rescale checks ok\n");
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
        const std::size_t n = 256, k = 3, nk = 4, nd = 3;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4019;
        const double scale = 1099511627776.0, pscale = 1024.0;
        auto fill_ct = [&](std::size_t size) {
            HostCiphertext c = host_ct(size, k, n, true);
            c.scale_ = scale;
            fill_rows(c.words.data(), size * k, n, mods, k, state);
            return c;
        };
        auto fill_key = [&] {
            return seeded_key(ctx, nd, nk, n, mods, state);
        };
        // (the order of the Python test's draws: a, b, the size-3 ciphertext, the relinearization key, the keys of steps 1
        //  and 2, the 2 x 2 plaintexts)
        const HostCiphertext a = fill_ct(2), b = fill_ct(2), c3 = fill_ct(3);
        const std::unique_ptr<KSwitchKeys> relin = fill_key();
        std::uint32_t g1 = 0, g2 = 0;
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &g1));
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 2, &g2));
        const std::unique_ptr<KSwitchKeys> k1 = fill_key(), k2 = fill_key();
        const std::map<std::uint32_t, const KSwitchKeys *> gk{ { g1, k1.get() }, { g2, k2.get() } };
        Plains plains(2, std::vector<HostPlaintext>(2));
        std::vector<std::vector<DevicePlaintext>> dplains(2);
        for (std::size_t s = 0; s < 2; s++)
            for (std::size_t e = 0; e < 2; e++)
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
        const double q_last = double(mods[k - 1]);
        auto report = [&](const char *side, const char *what, const std::vector<HostCiphertext> &cs, double want_scale) {
            std::uint64_t h = kFnvBasis;
            bool meta = true;
            for (const HostCiphertext &c : cs)
            {
                h = digest(h, c.data(), c.words.size());
                meta = meta && c.size() == 2 && c.coeff_modulus_size() == k - 1 && c.is_ntt_form() && c.scale() == want_scale &&
                       c.words.size() == 2 * (k - 1) * n;
            }
            std::printf("%s %s digest %016llx meta %d\n", side, what, static_cast<unsigned long long>(h), int(meta));
        };
        const std::vector<std::uint32_t> baby{ g1, 1 }, giant{ 1, g2 };
        const std::vector<const KSwitchKeys *> relin_keys{ relin.get() };
        {
            HostCiphertext out;
            std::vector<HostCiphertext> outs;
            ev.relinearize_rescale(c3, relin_keys, out);
            report("host", "relinearize", { out }, scale / q_last);
            ev.dot_product_rescale(std::vector<HostCiphertext>{ a }, std::vector<HostCiphertext>{ b }, *relin, out);
            report("host", "dot_product", { out }, scale * scale / q_last);
            ev.apply_galois_dot_plain_rescale(a, baby, gk, plains, outs);
            report("host", "dot_plain", outs, scale * pscale / q_last);
            ev.rotate_vector_dot_plain_rescale(a, { 1, 0 }, gk, plains, outs);
            report("host", "dot_plain", outs, scale * pscale / q_last);
            ev.apply_galois_bsgs_plain_rescale(a, baby, giant, gk, plains, out);
            report("host", "bsgs", { out }, scale * pscale / q_last);
            ev.rotate_vector_bsgs_plain_rescale(a, { 1, 0 }, { 0, 2 }, gk, plains, out);
            report("host", "bsgs", { out }, scale * pscale / q_last);
        }
        {
            std::vector<DeviceCiphertext> da, db;
            da.emplace_back(ctx);
            db.emplace_back(ctx);
            da[0].upload(a);
            db[0].upload(b);
            DeviceCiphertext d3(ctx), dout(ctx);
            d3.upload(c3);
            std::vector<DeviceCiphertext> douts;
            auto back = [&](const std::vector<const DeviceCiphertext *> &ds) {
                std::vector<HostCiphertext> hs(ds.size());
                for (std::size_t i = 0; i < ds.size(); i++)
                    ds[i]->download(hs[i]);
                return hs;
            };
            ev.relinearize_rescale(d3, relin_keys, dout);
            report("device", "relinearize", back({ &dout }), scale / q_last);
            ev.dot_product_rescale(da, db, *relin, dout);
            report("device", "dot_product", back({ &dout }), scale * scale / q_last);
            ev.apply_galois_dot_plain_rescale(da[0], baby, gk, dplains, douts);
            report("device", "dot_plain", back({ &douts[0], &douts[1] }), scale * pscale / q_last);
            ev.rotate_vector_dot_plain_rescale(da[0], { 1, 0 }, gk, dplains, douts);
            report("device", "dot_plain", back({ &douts[0], &douts[1] }), scale * pscale / q_last);
            ev.apply_galois_bsgs_plain_rescale(da[0], baby, giant, gk, dplains, dout);
            report("device", "bsgs", back({ &dout }), scale * pscale / q_last);
            ev.rotate_vector_bsgs_plain_rescale(da[0], { 1, 0 }, { 0, 2 }, gk, dplains, dout);
            report("device", "bsgs", back({ &dout }), scale * pscale / q_last);
        }
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
