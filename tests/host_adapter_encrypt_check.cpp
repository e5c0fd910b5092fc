// The C++ host adapter's Encryptor (gemini-seal_amd/host/evaluator.hpp). Without arguments, on host-only contexts: the
// reference's checks and messages (encryptor.cpp:106-259). With a device (argv[1] = ordinal, argv[2] = input file written by
// tests/test_gpu_encryptor.py, argv[3] = output path of the seeded stream): a BFV batch encrypted with the public key, one
// with the secret key and one seeded encryption, all at the first level, the samples handed to the samplers from the file
// in the reference's order. It prints FNV-1a digests of the ciphertext words, which the test compares with the oracle, and
// checks that the adapter's Decryptor returns the plaintexts.
//
// Input file, little-endian 64-bit words: scheme, log_n, n_key, nsp, t, key moduli [n_key], secret key (NTT form)
// [n_key x N], public key [2 x n_key x N], count, plaintexts [count x N], public-key samples [count x 3 x N] (u, e_0, e_1
// as signed words), secret-key samples [(count + 1) x (8 + N)] (seed, e), parms_id of the first level [4].
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

// (not host_ct: no polynomials at all, the state a destination has before its first use)
static HostCiphertext empty_ct(std::size_t n)
{
    HostCiphertext ct;
    ct.n_ = n;
    return ct;
}

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    sealhip_params bp{ SEALHIP_SCHEME_BFV, 8, 4, 2, mods, 786433, SEALHIP_MODE_PARITY, -1 };
    sealhip_params cp{ SEALHIP_SCHEME_CKKS, 8, 4, 2, mods, 0, SEALHIP_MODE_PARITY, -1 };
    Context bfv(bp), ckks(cp);
    std::vector<std::uint64_t> sk(4 * n, 1), pk(2 * 4 * n, 1);
    auto asym = [&](std::int32_t *u, std::int32_t *e0, std::int32_t *e1) {
        std::fill(u, u + n, 0);
        std::fill(e0, e0 + n, 0);
        std::fill(e1, e1 + n, 0);
    };
    auto sym = [&](std::uint64_t *seed, std::int32_t *e) {
        std::fill(seed, seed + 8, 1);
        std::fill(e, e + n, 0);
    };
    Encryptor<HostCiphertext> none(bfv, nullptr, nullptr, asym, sym);
    Encryptor<HostCiphertext> eb(bfv, pk.data(), sk.data(), asym, sym), ec(ckks, pk.data(), sk.data(), asym, sym);
    HostCiphertext ct = empty_ct(n);
    HostPlaintext ok_plain{ std::vector<std::uint64_t>(n / 2, 5), 0, false, 1.0 };
    HostPlaintext ntt_plain{ std::vector<std::uint64_t>(n, 5), 0, true, 1.0 };
    HostPlaintext long_plain{ std::vector<std::uint64_t>(n + 1, 5), 0, false, 1.0 };
    HostPlaintext big_plain{ std::vector<std::uint64_t>(n, 786433), 0, false, 1.0 };
    HostPlaintext ckks_coeff{ std::vector<std::uint64_t>(2 * n, 5), 2, false, 4.0 };
    HostPlaintext ckks_key{ std::vector<std::uint64_t>(4 * n, 5), 4, true, 4.0 };
    HostPlaintext ckks_short{ std::vector<std::uint64_t>(n, 5), 2, true, 4.0 };
    HostPlaintext ckks_ok{ std::vector<std::uint64_t>(2 * n, 5), 2, true, 4.0 };
    const char *invalid = "plain is not valid for encryption parameters";
    const std::uint64_t pid[4] = { 1, 2, 3, 4 };
    bool ok = true;
    ok &= throws_prefix<std::logic_error>([&] { none.encrypt(ok_plain, ct); }, "public key is not set");
    ok &= throws_prefix<std::logic_error>([&] { none.encrypt_zero(ct); }, "public key is not set");
    ok &= throws_prefix<std::logic_error>([&] { none.encrypt_symmetric(ok_plain, ct); }, "secret key is not set");
    ok &= throws_prefix<std::logic_error>([&] { none.encrypt_zero_symmetric(ct); }, "secret key is not set");
    ok &= throws_prefix<std::logic_error>([&] { none.encrypt_symmetric_seeded(ok_plain, pid); }, "secret key is not set");
    ok &= throws_prefix<std::invalid_argument>([&] { eb.encrypt(ntt_plain, ct); }, "plain cannot be in NTT form");
    ok &= throws_prefix<std::invalid_argument>([&] { eb.encrypt(long_plain, ct); }, invalid);
    ok &= throws_prefix<std::invalid_argument>([&] { eb.encrypt_symmetric(big_plain, ct); }, invalid);
    ok &= throws_prefix<std::invalid_argument>([&] { ec.encrypt(ckks_coeff, ct); }, "plain must be in NTT form");
    ok &= throws_prefix<std::invalid_argument>([&] { ec.encrypt(ckks_key, ct); }, invalid);
    ok &= throws_prefix<std::invalid_argument>([&] { ec.encrypt_symmetric(ckks_short, ct); }, invalid);
    for (std::size_t bad : { std::size_t(0), std::size_t(5) })
    {
        ok &= throws_prefix<std::invalid_argument>([&] { eb.encrypt_zero(bad, ct); }, "parms_id is not valid for encryption parameters");
        ok &= throws_prefix<std::invalid_argument>([&] { ec.encrypt_zero_symmetric(bad, ct); },
                                            "parms_id is not valid for encryption parameters");
    }
    // valid arguments reach the device: a host-only context refuses them
    ok &= throws_prefix<std::logic_error>([&] { eb.encrypt(ok_plain, ct); }, "host-only");
    ok &= throws_prefix<std::logic_error>([&] { eb.encrypt_zero(4, ct); }, "host-only");
    ok &= throws_prefix<std::logic_error>([&] { ec.encrypt(ckks_ok, ct); }, "host-only");
    ok &= throws_prefix<std::logic_error>([&] { ec.encrypt_symmetric(ckks_ok, ct); }, "host-only");
    if (!ok)
        return 1;
    std::printf("host-only encrypt checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4)
        return host_checks();
    try
    {
        std::FILE *f = std::fopen(argv[2], "rb");
        if (!f)
            return 2;
        std::vector<std::uint64_t> in;
        std::uint64_t w;
        while (std::fread(&w, 8, 1, f) == 1)
            in.push_back(w);
        std::fclose(f);
        std::size_t at = 0;
        auto next = [&] { return in.at(at++); };
        const std::uint32_t scheme = std::uint32_t(next()), log_n = std::uint32_t(next());
        const std::uint32_t n_key = std::uint32_t(next()), nsp = std::uint32_t(next());
        const std::uint64_t t = next();
        std::vector<std::uint64_t> mods(n_key);
        for (auto &m : mods)
            m = next();
        const std::size_t n = std::size_t(1) << log_n, k = n_key - nsp;
        sealhip_params p{ scheme, log_n, n_key, nsp, mods.data(), t, SEALHIP_MODE_PARITY, std::atoi(argv[1]) };
        Context ctx(p);
        const std::uint64_t *sk = in.data() + at;
        at += n_key * n;
        const std::uint64_t *pk = in.data() + at;
        at += 2 * n_key * n;
        const std::size_t count = next();
        std::vector<HostPlaintext> plains(count);
        for (std::size_t i = 0; i < count; i++)
        {
            plains[i].words.assign(in.data() + at, in.data() + at + n);
            at += n;
        }
        // the first plaintext is handed over short (its upper half is zero): the Encryptor pads it
        plains[0].words.resize(n / 2);
        std::size_t asym_at = at, sym_at = at + count * 3 * n;
        const std::size_t pid_at = sym_at + (count + 1) * (8 + n);
        auto asym = [&](std::int32_t *u, std::int32_t *e0, std::int32_t *e1) {
            for (std::int32_t *dst : { u, e0, e1 })
                for (std::size_t c = 0; c < n; c++)
                    dst[c] = static_cast<std::int32_t>(static_cast<std::int64_t>(in.at(asym_at++)));
        };
        auto sym = [&](std::uint64_t *seed, std::int32_t *e) {
            for (int j = 0; j < 8; j++)
                seed[j] = in.at(sym_at++);
            for (std::size_t c = 0; c < n; c++)
                e[c] = static_cast<std::int32_t>(static_cast<std::int64_t>(in.at(sym_at++)));
        };
        std::uint64_t pid[4];
        for (int j = 0; j < 4; j++)
            pid[j] = in.at(pid_at + j);
        throw_on(sealhip_context_set_parms_id(ctx.get(), std::uint32_t(k), pid));
        Encryptor<HostCiphertext> enc(ctx, pk, sk, asym, sym);
        Decryptor<HostCiphertext> dec(ctx, sk);
        std::vector<const HostPlaintext *> pp;
        for (auto &pl : plains)
            pp.push_back(&pl);
        std::vector<HostCiphertext> ca(count, empty_ct(n)), cs(count, empty_ct(n));
        std::vector<HostCiphertext *> da, ds;
        for (std::size_t i = 0; i < count; i++)
        {
            da.push_back(&ca[i]);
            ds.push_back(&cs[i]);
        }
        enc.encrypt(pp, da);
        enc.encrypt_symmetric(pp, ds);
        HostCiphertext seeded = empty_ct(n);
        const std::vector<unsigned char> stream = enc.encrypt_symmetric_seeded(plains[1], pid, &seeded);
        std::FILE *o = std::fopen(argv[3], "wb");
        if (!o || std::fwrite(stream.data(), 1, stream.size(), o) != stream.size())
            return 3;
        std::fclose(o);
        bool ok = true;
        for (std::size_t i = 0; i < count; i++)
        {
            std::printf("asym %zu %llu\n", i, static_cast<unsigned long long>(digest(ca[i].data(), 2 * k * n)));
            std::printf("sym %zu %llu\n", i, static_cast<unsigned long long>(digest(cs[i].data(), 2 * k * n)));
            ok &= ca[i].coeff_modulus_size() == k && !ca[i].is_ntt_form() && cs[i].size() == 2;
        }
        std::printf("seeded %llu\n", static_cast<unsigned long long>(digest(seeded.data(), 2 * k * n)));
        // the adapter's Decryptor returns the plaintexts (trimmed like bfv_decrypt)
        auto trimmed = [&](const HostPlaintext &pl) {
            std::vector<std::uint64_t> v(pl.words);
            v.resize(n, 0);
            while (v.size() > 1 && v.back() == 0)
                v.pop_back();
            return v;
        };
        bool dec_a = true, dec_s = true;
        for (std::size_t i = 0; i < count; i++)
        {
            std::vector<std::uint64_t> out;
            dec.decrypt(ca[i], out);
            dec_a &= out == trimmed(plains[i]);
            dec.decrypt(cs[i], out);
            dec_s &= out == trimmed(plains[i]);
        }
        std::vector<std::uint64_t> out;
        dec.decrypt(seeded, out);
        std::printf("decrypt_asym=%s\ndecrypt_sym=%s\ndecrypt_seeded=%s\nmeta=%s\n", dec_a ? "ok" : "bad", dec_s ? "ok" : "bad",
                    out == trimmed(plains[1]) ? "ok" : "bad", ok ? "ok" : "bad");
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
