// The C++ host adapter's matrix-vector product (gemini-seal_amd/host/evaluator.hpp: LinearTransform,
// Evaluator::linear_transform). argv[1] = "host": on host-only contexts the argument refusals arrive as
// std::invalid_argument before the missing device does as std::logic_error. argv[1] = device ordinal, argv[2..5] = four key
// primes (N = 1024, one special prime, CKKS): LinearTransform made from a host vector and from device memory holds the same
// tables; on an encryption under real keys the host-ciphertext form and the DeviceCiphertext form give the words of the C ABI
// called directly, with and without the merged rescale, at the level and scale the header documents; a missing key throws;
// and the decrypted, decoded result is printed against M z.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;
using Cx = std::complex<double>;

static std::vector<Cx> seeded_matrix(std::size_t d, std::uint64_t &state)
{
    std::vector<Cx> m(d * d);
    for (Cx &v : m)
    {
        const double re = double(splitmix(state) >> 11) / 9007199254740992.0 - 0.5;
        const double im = double(splitmix(state) >> 11) / 9007199254740992.0 - 0.5;
        v = Cx(re, im);
    }
    return m;
}

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    bool ok = true;
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, -1 };
    Context ctx(p);
    std::uint64_t state = 1;
    const std::vector<Cx> m8 = seeded_matrix(8, state);
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, m8, 4, 1048576.0); }, "d x d entries");
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, seeded_matrix(6, state), 6, 1048576.0); }, "power of two");
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, m8, 8, 1048576.0, 3); }, "n1");
    ok &= throws<std::logic_error>([&] { LinearTransform t(ctx, m8, 8, 1048576.0); }, "host-only");
    const double *p8 = reinterpret_cast<const double *>(m8.data());
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, p8, 8, 1048576.0, 16); }, "n1");
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, p8, 8, 1048576.0, 0, 0.0); }, "gain");
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(ctx, reinterpret_cast<const double *>(m8.data()) + 1, 8, 1048576.0); },
                                        "16-byte aligned");
    ok &= throws<std::logic_error>([&] { LinearTransform t(ctx, reinterpret_cast<const double *>(m8.data()), 8, 1048576.0); },
                                   "host-only");
    sealhip_params b{ SEALHIP_SCHEME_BFV, 8, 4, 1, mods, 786433ULL, SEALHIP_MODE_STRICT, -1 };
    Context bfv(b);
    ok &= throws<std::invalid_argument>([&] { LinearTransform t(bfv, reinterpret_cast<const double *>(m8.data()), 8, 1048576.0); },
                                        "CKKS only");
    if (!ok)
        return 1;
    std::printf("host-only lintrans checks ok\n");
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
        const std::size_t N = 1024, n = N / 2, k = 3, nk = 4, d = 16;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 10, 4, 1, mods, 0ULL, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x26;
        const std::vector<Cx> M = seeded_matrix(d, state);
        const double delta = 1099511627776.0, table_scale = double(mods[k - 1]); // 2^40; q_2, the prime the rescale drops

        // the tables: from the host vector, and from device memory
        LinearTransform from_host(ctx, M, d, table_scale);
        double *d_m = nullptr;
        throw_on(sealhip_malloc(ctx.get(), d * d * 16, reinterpret_cast<void **>(&d_m)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_m, M.data(), d * d * 16));
        LinearTransform lt(ctx, d_m, d, table_scale);
        bool ok = lt.plan().d == d && lt.plan().n_diagonals == d && lt.plan().n1 == 8 && lt.plan().n_baby == 8 &&
                  lt.plan().n_giant == 2 && lt.scale() == table_scale && lt.key_steps().size() == 8 &&
                  lt.plan().table_words == 16 * nk * N && from_host.plan().table_words == lt.plan().table_words &&
                  from_host.baby_steps() == lt.baby_steps() && from_host.giant_steps() == lt.giant_steps();
        std::vector<std::uint64_t> t1(lt.plan().table_words), t2(t1.size());
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), t1.data(), lt.plain_ntt(), t1.size() * 8));
        throw_on(sealhip_memcpy_d2h(ctx.get(), t2.data(), from_host.plain_ntt(), t2.size() * 8));
        ok &= t1 == t2;
        print_digest("tables", digest(t1), t1 == t2);

        // real keys: the secret, the Galois keys of the plan's steps
        std::size_t drawn = 0;
        const SeedSource source = [&drawn](std::uint64_t *seed) {
            for (std::uint64_t j = 0; j < 8; j++)
                seed[j] = (0x11A7000000000000ULL + drawn + j) * 0x9E3779B97F4A7C15ULL;
            drawn++;
        };
        const std::vector<std::uint64_t> sk = KeyGenerator::generate_secret_key(ctx, source);
        KeyGenerator kg(ctx, sk.data(), source);
        const KeyGenerator::GaloisKeys made = kg.galois_keys(std::vector<int>(lt.key_steps().begin(), lt.key_steps().end()));
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        std::vector<std::uint32_t> elts;
        std::vector<const sealhip_kswitch_key *> raw;
        for (const auto &kv : made)
        {
            gk[kv.first] = kv.second.get();
            elts.push_back(kv.first);
            raw.push_back(kv.second->get());
        }
        ok &= gk.size() == lt.key_steps().size();

        // z: a vector of d values tiled n / d times, encoded on the device at level k and 2^40, encrypted under the secret
        std::vector<Cx> tile(d), z(n);
        for (Cx &v : tile)
            v = Cx(double(splitmix(state) >> 11) / 9007199254740992.0 - 0.5, double(splitmix(state) >> 11) / 9007199254740992.0 - 0.5);
        for (std::size_t i = 0; i < n; i++)
            z[i] = tile[i % d];
        double *d_v = nullptr;
        std::uint64_t *d_p = nullptr;
        throw_on(sealhip_malloc(ctx.get(), n * 16, reinterpret_cast<void **>(&d_v)));
        throw_on(sealhip_malloc(ctx.get(), k * N * 8, reinterpret_cast<void **>(&d_p)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_v, z.data(), n * 16));
        throw_on(sealhip_ckks_encode(ctx.get(), std::uint32_t(k), d_v, n, 1, delta, d_p));
        HostPlaintext plain;
        plain.words.resize(k * N);
        plain.k = k;
        plain.ntt_form = true;
        plain.scale = delta;
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), plain.words.data(), d_p, k * N * 8));
        Encryptor<HostCiphertext> enc(ctx, nullptr, sk.data(), source);
        HostCiphertext ct = host_ct(2, k, N, true, delta);
        enc.encrypt_symmetric(plain, ct);
        ct.ntt_form_ = true;
        ct.scale_ = delta;
        ok &= ct.size() == 2 && ct.coeff_modulus_size() == k && ct.is_ntt_form();

        // the C ABI, called directly
        const std::size_t in_words = 2 * k * N;
        std::uint64_t *d_a = nullptr, *d_o = nullptr;
        throw_on(sealhip_malloc(ctx.get(), in_words * 8, reinterpret_cast<void **>(&d_a)));
        throw_on(sealhip_malloc(ctx.get(), in_words * 8, reinterpret_cast<void **>(&d_o)));
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_a, ct.data(), in_words * 8));
        std::vector<std::uint64_t> want[2];
        for (int rescale = 0; rescale < 2; rescale++)
        {
            want[rescale].resize(2 * (k - rescale) * N);
            throw_on(sealhip_evaluator_linear_transform(ctx.get(), lt.get(), std::uint32_t(k), d_a, 1, elts.data(), raw.data(),
                                                        std::uint32_t(elts.size()), rescale, d_o));
            throw_on(sealhip_synchronize(ctx.get()));
            throw_on(sealhip_memcpy_d2h(ctx.get(), want[rescale].data(), d_o, want[rescale].size() * 8));
            print_digest(rescale ? "abi rescale" : "abi", digest(want[rescale]), true);
        }

        // the adapter: host ciphertexts and resident ones, tables from either source
        Evaluator<HostCiphertext> ev(ctx);
        auto same = [&](const char *what, const HostCiphertext &c, int rescale) {
            const double scale = rescale ? delta * table_scale / double(mods[k - 1]) : delta * table_scale;
            const bool good = c.size() == 2 && c.coeff_modulus_size() == k - rescale && c.is_ntt_form() && c.scale() == scale &&
                              c.words.size() == want[rescale].size() &&
                              std::memcmp(c.data(), want[rescale].data(), want[rescale].size() * 8) == 0;
            print_digest(what, digest(c.words), good);
            return good;
        };
        HostCiphertext out, rescaled, back;
        ev.linear_transform(ct, lt, gk, out);
        ok &= same("host", out, 0);
        ev.linear_transform(ct, from_host, gk, out);
        ok &= same("host, tables from a host vector", out, 0);
        ev.linear_transform(ct, lt, gk, rescaled, true);
        ok &= same("host rescale", rescaled, 1) && rescaled.scale() == delta;
        DeviceCiphertext dc(ctx), dout(ctx);
        dc.upload(ct);
        ev.linear_transform(dc, lt, gk, dout);
        dout.download(back);
        ok &= same("device", back, 0);
        ev.linear_transform(dc, from_host, gk, dout, true);
        dout.download(back);
        ok &= same("device rescale", back, 1);

        // a missing key; the operand checks
        std::map<std::uint32_t, const KSwitchKeys *> fewer = gk;
        fewer.erase(fewer.begin());
        HostCiphertext keep = host_ct(3, 1, N, false);
        ok &= throws<std::invalid_argument>([&] { ev.linear_transform(ct, lt, fewer, keep); }, "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.linear_transform(host_ct(2, k, N, false), lt, gk, keep); },
                                            "CKKS encrypted must be in NTT form");
        ok &= throws<std::invalid_argument>([&] { ev.linear_transform(host_ct(3, k, N, true), lt, gk, keep); },
                                            "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.linear_transform(host_ct(2, 1, N, true, delta), lt, gk, keep, true); },
                                            "end of modulus switching chain reached");
        // an operand that breaks two rules gets the first one's message: the form before the end of the chain, and on a BFV
        // context (host-only: the call stops at the scheme) "unsupported scheme" before any form message
        ok &= throws<std::invalid_argument>([&] { ev.linear_transform(host_ct(2, 1, N, false, delta), lt, gk, keep, true); },
                                            "CKKS encrypted must be in NTT form");
        sealhip_params b{ SEALHIP_SCHEME_BFV, 10, 4, 1, mods, 786433ULL, SEALHIP_MODE_STRICT, -1 };
        Context bfv(b);
        Evaluator<HostCiphertext> ev_bfv(bfv);
        ok &= throws<std::logic_error>([&] { ev_bfv.linear_transform(host_ct(2, k, N, true), lt, gk, keep, true); },
                                       "unsupported scheme");
        ok &= keep.size() == 3 && keep.coeff_modulus_size() == 1; // (a refused call leaves the destination alone)

        // decrypted and decoded against M z
        Decryptor<HostCiphertext> dec(ctx, sk.data());
        std::vector<std::uint64_t> msg;
        dec.decrypt(rescaled, msg);
        ok &= msg.size() == (k - 1) * N;
        throw_on(sealhip_memcpy_h2d(ctx.get(), d_p, msg.data(), msg.size() * 8));
        throw_on(sealhip_ckks_decode(ctx.get(), std::uint32_t(k - 1), d_p, 1, rescaled.scale(), d_v));
        std::vector<Cx> got(n);
        throw_on(sealhip_synchronize(ctx.get()));
        throw_on(sealhip_memcpy_d2h(ctx.get(), got.data(), d_v, n * 16));
        double err = 0, size = 0;
        for (std::size_t i = 0; i < n; i++)
        {
            Cx s = 0;
            for (std::size_t j = 0; j < d; j++)
                s += M[(i % d) * d + j] * tile[j];
            err = std::max(err, std::abs(got[i] - s));
            size = std::max(size, std::abs(s));
        }
        std::printf("decrypted against M z: max slot error %.3g, max |M z| %.3g\n", err, size);
        ok &= err < std::ldexp(size, -16);
        for (void *ptr : { static_cast<void *>(d_m), static_cast<void *>(d_v), static_cast<void *>(d_p), static_cast<void *>(d_a),
                           static_cast<void *>(d_o) })
            throw_on(sealhip_free(ctx.get(), ptr));
        if (!ok)
            return 1;
        std::printf("lintrans adapter checks ok\n");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
