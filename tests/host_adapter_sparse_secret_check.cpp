// The C++ host adapter's sparse-secret surface (gemini-seal_amd/host/evaluator.hpp: KeyGenerator::generate_sparse_secret_key
// and switching_keys, Evaluator::switch_secret, the Bootstrapper overload of Evaluator::bootstrap that takes the two keys).
// argv[1] = "host": the checks that need no device, on a host-only context. argv[1] = device ordinal, argv[2..12] = eleven key
// primes (N = 256, q_0, nine primes near 2 q_0, one special prime, CKKS; the shape of host_adapter_bootstrap_check.cpp): from
// a counting SeedSource to digests of the sparse secret key, the two switching keys and a switched ciphertext, which the
// Python test compares with the C ABI's outputs for the same seeds; and the host-ciphertext and DeviceCiphertext forms of
// switch_secret and of the encapsulated bootstrap against the C ABI called directly.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

// seed number i: word j = (0x5EED000000000000 + i + j) * 0x9E3779B97F4A7C15 (tests/test_gpu_sparse_secret.py restates it)
static SeedSource counting_source(std::size_t &drawn)
{
    return [&drawn](std::uint64_t *seed) {
        for (std::uint64_t j = 0; j < 8; j++)
            seed[j] = (0x5EED000000000000ULL + drawn + j) * 0x9E3779B97F4A7C15ULL;
        drawn++;
    };
}

static std::uint64_t save_digest(const Context &ctx, const sealhip_kswitch_key *key)
{
    std::size_t need = 0, written = 0;
    throw_on(sealhip_kswitch_keys_save(ctx.get(), &key, 1, nullptr, 0, &need));
    std::vector<unsigned char> buf(need);
    throw_on(sealhip_kswitch_keys_save(ctx.get(), &key, 1, buf.data(), need, &written));
    return digest(buf.data(), written);
}

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, -1 };
    Context ctx(p);
    std::size_t drawn = 0;
    const SeedSource source = counting_source(drawn);
    bool ok = true;
    ok &= throws_exact<std::invalid_argument>([&] { KeyGenerator::generate_sparse_secret_key(ctx, source, 0); }, "h must be 1 .. N");
    ok &= throws_exact<std::invalid_argument>([&] { KeyGenerator::generate_sparse_secret_key(ctx, source, n + 1); }, "h must be 1 .. N");
    ok &= drawn == 0; // nothing drawn for a refused weight
    ok &= throws<std::logic_error>([&] { KeyGenerator::generate_sparse_secret_key(ctx, source, 32); }, "host-only");
    ok &= drawn == 1;
    std::vector<std::uint64_t> sk(4 * n, 1), other(4 * n, 2);
    KeyGenerator kg(ctx, sk.data(), source);
    ok &= throws_exact<std::invalid_argument>([&] { kg.switching_keys(other.data(), 0); }, "invalid count");
    ok &= throws_exact<std::invalid_argument>([&] { kg.switching_keys(other.data(), 15); }, "invalid count");
    ok &= throws_exact<std::invalid_argument>([&] { kg.switching_keys(nullptr, 1); }, "from_secret_keys_ntt is null");
    ok &= throws_exact<std::invalid_argument>([&] { kg.switching_keys(other.data(), 1, 4); }, "level k out of range");
    ok &= drawn == 1;
    ok &= throws<std::logic_error>([&] { kg.switching_keys(other.data(), 1, 1); }, "host-only");
    ok &= drawn == 1 + 2 * 3; // three digits, a public and a noise seed each
    if (!ok)
        return 1;
    std::printf("host-only sparse secret checks ok\n");
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
        const std::uint64_t pid[4] = { 0x1111, 0x2222, 0x3333, 0x4444 };
        throw_on(sealhip_context_set_parms_id(ctx.get(), std::uint32_t(nk), pid));
        std::size_t drawn = 0;
        const SeedSource source = counting_source(drawn);
        // seed 0: the dense secret; seed 1: the weight-16 one; then a public and a noise seed per digit of each key
        const std::vector<std::uint64_t> dense = KeyGenerator::generate_secret_key(ctx, source);
        const std::vector<std::uint64_t> sparse = KeyGenerator::generate_sparse_secret_key(ctx, source, 16);
        bool ok = drawn == 2 && dense.size() == nk * n && sparse.size() == nk * n;
        KeyGenerator kg_sparse(ctx, sparse.data(), source), kg_dense(ctx, dense.data(), source);
        KeyGenerator::Keys to_sparse = kg_sparse.switching_keys(dense.data(), 1, 1);
        ok &= drawn == 2 + 2 * nd;
        KeyGenerator::Keys to_dense = kg_dense.switching_keys(sparse.data(), 1);
        ok &= drawn == 2 + 4 * nd && to_sparse.size() == 1 && to_dense.size() == 1;
        std::printf("sparse_sk digest %016llx\n", static_cast<unsigned long long>(digest(sparse)));
        std::printf("to_sparse digest %016llx\n", static_cast<unsigned long long>(save_digest(ctx, to_sparse[0]->get())));
        std::printf("to_dense digest %016llx\n", static_cast<unsigned long long>(save_digest(ctx, to_dense[0]->get())));

        std::uint64_t state = 0x5A25E;
        auto random_ct = [&](std::size_t k, double scale) {
            HostCiphertext c = host_ct(2, k, n, true);
            c.scale_ = scale;
            fill_rows(c.words.data(), 2 * k, n, mods, k, state);
            return c;
        };
        const double delta = 1048576.0;
        const HostCiphertext top = random_ct(k_top, delta), low = random_ct(2, delta), one = random_ct(1, delta);
        Evaluator<HostCiphertext> ev(ctx);
        HostCiphertext out, back;
        ev.switch_secret(top, *to_dense[0], out);
        ok &= out.size() == 2 && out.coeff_modulus_size() == k_top && out.is_ntt_form() && out.scale() == delta;
        std::printf("switch_secret digest %016llx\n", static_cast<unsigned long long>(digest(out.words)));
        DeviceCiphertext d_top(ctx), d_low(ctx), d_out(ctx);
        d_top.upload(top);
        ev.switch_secret(d_top, *to_dense[0], d_out);
        d_out.download(back);
        ok &= back.words == out.words && back.coeff_modulus_size() == k_top;
        ev.switch_secret(one, *to_sparse[0], out); // the level-1 key at level 1
        ok &= out.coeff_modulus_size() == 1;
        ok &= throws<std::invalid_argument>([&] { ev.switch_secret(low, *to_sparse[0], back); }, "not valid for encryption parameters");
        ok &= throws<std::invalid_argument>([&] { ev.switch_secret(host_ct(3, 2, n, true), *to_dense[0], back); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.switch_secret(host_ct(2, 2, n, false), *to_dense[0], back); },
                                            "CKKS encrypted must be in NTT form");

        // the encapsulated bootstrap: ModRaise to 10, CoeffToSlot [4,3] to 8, EvalMod (K 2, r 1, degree 7) to 3, SlotToCoeff
        // [4,3] to 1; Galois and relinearization keys are seeded words (the words do not depend on what they encrypt)
        const std::vector<std::uint32_t> stages{ 4, 3 };
        Bootstrapper boot(ctx, k_top, stages, stages, 2, 1, 7);
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
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elt] = keys.back().get();
            raw.push_back(keys.back()->get());
        }
        const std::unique_ptr<KSwitchKeys> relin = seeded_key(ctx, nd, nk, n, mods, state);
        const std::vector<const KSwitchKeys *> rk{ relin.get() };
        const sealhip_kswitch_key *relin_raw = relin->get();
        std::uint64_t *d_in = nullptr, *d_o = nullptr;
        throw_on(sealhip_malloc(ctx.get(), 2 * 2 * n * 8, reinterpret_cast<void **>(&d_in)));
        throw_on(sealhip_malloc(ctx.get(), 2 * n * 8, reinterpret_cast<void **>(&d_o)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_in, low.data(), 2 * 2 * n * 8));
        throw_on(sealhip_evaluator_bootstrap_encapsulated(ctx.get(), boot.get(), 2, d_in, 1, elts.data(), raw.data(),
                                                          std::uint32_t(elts.size()), &relin_raw, 1, to_sparse[0]->get(),
                                                          to_dense[0]->get(), d_o));
        std::vector<std::uint64_t> want(2 * n), plain(2 * n);
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), want.data(), d_o, want.size() * 8));
        throw_on(sealhip_evaluator_bootstrap(ctx.get(), boot.get(), 2, d_in, 1, elts.data(), raw.data(), std::uint32_t(elts.size()),
                                             &relin_raw, 1, d_o));
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), plain.data(), d_o, plain.size() * 8));
        for (std::uint64_t *ptr : { d_in, d_o })
            throw_on(sealhip_free(ctx.get(), ptr));
        ok &= want != plain; // (the two keys are used)
        ev.bootstrap(low, boot, gk, rk, *to_sparse[0], *to_dense[0], out);
        ok &= out.size() == 2 && out.coeff_modulus_size() == 1 && out.scale() == delta && out.words == want;
        d_low.upload(low);
        ev.bootstrap(d_low, boot, gk, rk, *to_sparse[0], *to_dense[0], d_out);
        d_out.download(back);
        ok &= back.words == want && back.coeff_modulus_size() == 1;
        ev.bootstrap(low, boot, gk, rk, out);
        ok &= out.words == plain;
        HostCiphertext keep = host_ct(3, 1, n, false);
        ok &= throws<std::invalid_argument>([&] { ev.bootstrap(low, boot, gk, rk, *to_sparse[0], *to_sparse[0], keep); },
                                            "not valid for encryption parameters");
        ok &= keep.size() == 3 && keep.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)
        if (!ok)
            return 1;
        std::printf("sparse secret adapter checks ok\n");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
