// adapter_latency.cpp -- latency of one call through the C++ adapter (gemini-seal_amd/host/evaluator.hpp), per operation of
// the reference's timing loops (native/examples/7_performance.cpp: bfv_performance_test's add, multiply, multiply_plain,
// square, relinearize, rotate_rows one step, rotate_columns; ckks_performance_test's multiply, square, relinearize,
// rescale, rotate_vector one step, complex_conjugate), restated here, plus multiply + relinearize as one row.
//   usage: adapter_latency DEVICE SCHEME LOGN NSP T PRIME...
// Columns, each the mean of 10 calls after 2 warm-up calls, in ms: the host overload on pageable HostCiphertext words, the
// resident overload on DeviceCiphertext, and the raw ABI on pool blocks (the same entries, same run). The inputs are
// uniformly random words (the timing does not depend on them); the keys come from the adapter's KeyGenerator with
// deterministic samples. tools/adapter_latency.py adds the one-thread CPU oracle column and writes the profile.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../gemini-seal_amd/host/evaluator.hpp"

using namespace sealhip_host;

namespace
{
    std::uint64_t splitmix(std::uint64_t &s)
    {
        std::uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }

    template <class F, class S>
    double mean_ms(F &&op, S &&sync)
    {
        for (int i = 0; i < 2; i++)
            op();
        sync();
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < 10; i++)
            op();
        sync();
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / 10;
    }

    std::uint64_t *block(const Context &c, std::size_t words)
    {
        void *p = nullptr;
        throw_on(sealhip_pool_alloc(c.get(), words * 8, &p));
        return static_cast<std::uint64_t *>(p);
    }
} // namespace

int main(int argc, char **argv)
{
    if (argc < 7)
    {
        std::fprintf(stderr, "usage: %s DEVICE SCHEME LOGN NSP T PRIME...\n", argv[0]);
        return 2;
    }
    std::vector<std::uint64_t> mods;
    for (int i = 6; i < argc; i++)
        mods.push_back(std::strtoull(argv[i], nullptr, 10));
    const std::uint32_t scheme = std::uint32_t(std::atoi(argv[2])), logn = std::uint32_t(std::atoi(argv[3]));
    const std::uint32_t nsp = std::uint32_t(std::atoi(argv[4]));
    sealhip_params p{ scheme, logn, std::uint32_t(mods.size()), nsp, mods.data(), std::strtoull(argv[5], nullptr, 10),
                      SEALHIP_MODE_PARITY, std::atoi(argv[1]) };
    try
    {
        Context ctx(p);
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        const std::size_t n = std::size_t(1) << logn, nk = mods.size(), k = nk - nsp;
        std::uint64_t st = 0x5EED0000 + logn;
        std::vector<std::uint64_t> sk(nk * n);
        for (std::size_t r = 0; r < nk; r++)
            for (std::size_t c = 0; c < n; c++)
                sk[r * n + c] = splitmix(st) % mods[r];
        KeyGenerator kg(ctx, sk.data(), [&](std::uint64_t *seed, std::int32_t *noise) {
            for (int i = 0; i < 8; i++)
                seed[i] = splitmix(st);
            for (std::size_t i = 0; i < n; i++)
                noise[i] = std::int32_t(splitmix(st) % 7) - 3;
        });
        auto relin = kg.relin_keys(1);
        auto galois = kg.galois_keys(std::vector<int>{ 1, 0 });
        const std::vector<const KSwitchKeys *> rks{ relin[0].get() };
        std::map<std::uint32_t, const KSwitchKeys *> gks;
        for (auto &kv : galois)
            gks[kv.first] = kv.second.get();
        std::uint32_t e1 = 0, e0 = 0;
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &e1));
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 0, &e0));

        HostCiphertext x, y;
        for (HostCiphertext *ct : { &x, &y })
        {
            ct->n_ = n;
            ct->resize_raw(2, k);
            for (std::size_t s = 0; s < 2; s++)
                for (std::size_t r = 0; r < k; r++)
                    for (std::size_t c = 0; c < n; c++)
                        ct->words[(s * k + r) * n + c] = splitmix(st) % mods[r];
            ct->is_ntt_form() = !bfv;
        }
        std::vector<std::uint64_t> plain(n);
        for (auto &v : plain)
            v = splitmix(st) % (bfv ? p.plain_modulus : 2);
        Evaluator<HostCiphertext> ev(ctx);
        DeviceCiphertext dx(ctx), dy(ctx);
        dx.upload(x);
        dy.upload(y);
        DevicePlaintext dplain(ctx);
        if (bfv) // (multiply_plain is timed on BFV only, as in bfv_performance_test)
            dplain.upload(plain, false);
        HostCiphertext x3;
        ev.multiply(x, y, x3);
        DeviceCiphertext dx3(ctx);
        dx3.upload(x3);

        const std::size_t w2 = 2 * k * n, w3 = 3 * k * n;
        std::uint64_t *rx = block(ctx, w2), *ry = block(ctx, w2), *r3 = block(ctx, w3), *rt = block(ctx, w3),
                      *ro = block(ctx, w3), *rp = block(ctx, n);
        throw_on(sealhip_memcpy_h2d(ctx.get(), rx, x.data(), w2 * 8));
        throw_on(sealhip_memcpy_h2d(ctx.get(), ry, y.data(), w2 * 8));
        throw_on(sealhip_memcpy_h2d(ctx.get(), r3, x3.data(), w3 * 8));
        throw_on(sealhip_memcpy_h2d(ctx.get(), rp, plain.data(), n * 8));
        const sealhip_kswitch_key *rk_raw = rks[0]->get();
        const auto none = [] {};
        const auto dsync = [&] { ev.synchronize(); };
        const auto rsync = [&] { throw_on(sealhip_synchronize(ctx.get())); };
        HostCiphertext ho;
        DeviceCiphertext dout(ctx), dt(ctx);
        HostCiphertext ht;
        const auto row = [](const char *name, double h, double d, double r) {
            std::printf("%s %.4f %.4f %.4f\n", name, h, d, r);
            std::fflush(stdout);
        };
        const std::uint32_t K = std::uint32_t(k);
        if (bfv)
            row("add", mean_ms([&] { ev.add(x, y, ho); }, none), mean_ms([&] { ev.add(dx, dy, dout); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_add(ctx.get(), K, rx, 2, ry, 2, 1, ro)); }, rsync));
        row("multiply", mean_ms([&] { ev.multiply(x, y, ho); }, none), mean_ms([&] { ev.multiply(dx, dy, dout); }, dsync),
            mean_ms([&] { throw_on(sealhip_evaluator_multiply(ctx.get(), K, rx, 2, ry, 2, 1, ro)); }, rsync));
        if (bfv)
        {
            ht = x;
            dt = dx;
            throw_on(sealhip_memcpy_d2d(ctx.get(), rt, rx, w2 * 8));
            row("multiply_plain", mean_ms([&] { ev.multiply_plain_inplace(ht, plain.data(), false); }, none),
                mean_ms([&] { ev.multiply_plain_inplace(dt, dplain); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_multiply_plain(ctx.get(), K, rt, 2, 1, rp, 0)); }, rsync));
        }
        row("square", mean_ms([&] { ev.square(x, ho); }, none), mean_ms([&] { ev.square(dx, dout); }, dsync),
            mean_ms([&] { throw_on(sealhip_evaluator_square(ctx.get(), K, rx, 2, 1, ro)); }, rsync));
        row("relinearize", mean_ms([&] { ev.relinearize(x3, rks, ho); }, none),
            mean_ms([&] { ev.relinearize(dx3, rks, dout); }, dsync), mean_ms([&] {
                throw_on(sealhip_memcpy_d2d(ctx.get(), rt, r3, w3 * 8));
                throw_on(sealhip_evaluator_relinearize(ctx.get(), K, rt, 3, 1, &rk_raw, 1));
            }, rsync));
        if (!bfv)
            row("rescale", mean_ms([&] { ev.rescale_to_next(x, ho); }, none), mean_ms([&] { ev.rescale_to_next(dx, dout); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_rescale_to_next(ctx.get(), K, rx, 2, 1, ro)); }, rsync));
        ht = x;
        dt = dx;
        throw_on(sealhip_memcpy_d2d(ctx.get(), rt, rx, w2 * 8));
        const sealhip_kswitch_key *g1 = gks.at(e1)->get(), *g0 = gks.at(e0)->get();
        if (bfv)
        {
            row("rotate_rows", mean_ms([&] { ev.rotate_rows_inplace(ht, 1, gks); }, none),
                mean_ms([&] { ev.rotate_rows_inplace(dt, 1, gks); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_apply_galois(ctx.get(), K, rt, 1, e1, g1)); }, rsync));
            row("rotate_columns", mean_ms([&] { ev.rotate_columns_inplace(ht, gks); }, none),
                mean_ms([&] { ev.rotate_columns_inplace(dt, gks); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_apply_galois(ctx.get(), K, rt, 1, e0, g0)); }, rsync));
        }
        else
        {
            row("rotate_vector", mean_ms([&] { ev.rotate_vector_inplace(ht, 1, gks); }, none),
                mean_ms([&] { ev.rotate_vector_inplace(dt, 1, gks); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_apply_galois(ctx.get(), K, rt, 1, e1, g1)); }, rsync));
            row("complex_conjugate", mean_ms([&] { ev.complex_conjugate_inplace(ht, gks); }, none),
                mean_ms([&] { ev.complex_conjugate_inplace(dt, gks); }, dsync),
                mean_ms([&] { throw_on(sealhip_evaluator_apply_galois(ctx.get(), K, rt, 1, e0, g0)); }, rsync));
        }
        // multiply_inplace + relinearize_inplace on one ciphertext (the resident operand is refreshed by a device copy, the
        // raw path writes a separate product buffer)
        row("multiply+relinearize", mean_ms([&] {
                ht = x;
                ev.multiply_inplace(ht, y);
                ev.relinearize_inplace(ht, rks);
            }, none),
            mean_ms([&] {
                dt = dx;
                ev.multiply_inplace(dt, dy);
                ev.relinearize_inplace(dt, rks);
            }, dsync),
            mean_ms([&] {
                throw_on(sealhip_evaluator_multiply(ctx.get(), K, rx, 2, ry, 2, 1, ro));
                throw_on(sealhip_evaluator_relinearize(ctx.get(), K, ro, 3, 1, &rk_raw, 1));
            }, rsync));
        for (std::uint64_t *b : { rx, ry, r3, rt, ro, rp })
            throw_on(sealhip_pool_release(ctx.get(), b));
        ev.synchronize();
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
