// The C++ host adapter with a seed source (gemini-seal_amd/host/evaluator.hpp: SeedSource, the Encryptor and KeyGenerator
// constructors that take one, KeyGenerator::generate_secret_key). Without arguments, on a host-only context: what needs
// no device. With a device (argv[1] = ordinal, argv[2] = input file written by tests/test_gpu_sample.py): a
// secret key, a public key and one relinearization key from seeds alone, then one resident public-key and one resident
// secret-key encryption. The seed source hands out seed number i = { base + i, base + i + 1, ..., base + i + 7 } x a
// constant, so the test knows every seed by its position. Checked here: how many seeds each operation draws and in which
// order they are used (c_1's before the noise seed), that a repeated seed is refused, that no noise seed appears in the
// seeded save of the keys while every c_1 seed does, and that the sample scratch reads back zero. Printed for the test:
// FNV-1a digests of the key and ciphertext words.
//
// Input file, little-endian 64-bit words: scheme, log_n, n_key, nsp, t, key moduli [n_key], parms_id of the key level [4],
// plaintext [N (BFV) or k x N (CKKS)].
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static const std::uint64_t kBase = 0x5EED000000000000ULL, kStep = 0x9E3779B97F4A7C15ULL;

static void seed_number(std::size_t i, std::uint64_t *seed)
{
    for (int j = 0; j < 8; j++)
        seed[j] = (kBase + i + j) * kStep;
}

#define REQUIRE(cond)                                          \
    do                                                         \
    {                                                          \
        if (!(cond))                                           \
        {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            return 1;                                          \
        }                                                      \
    } while (0)

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    sealhip_params bp{ SEALHIP_SCHEME_BFV, 8, 4, 2, mods, 786433, SEALHIP_MODE_PARITY, -1 };
    Context bfv(bp);
    std::vector<std::uint64_t> sk(4 * n, 1), pk(2 * 4 * n, 1);
    std::size_t drawn = 0;
    SeedSource counting = [&](std::uint64_t *seed) { seed_number(drawn++, seed); };
    // an empty source is refused at construction
    REQUIRE(throws<std::invalid_argument>([&] { Encryptor<HostCiphertext> e(bfv, pk.data(), sk.data(), SeedSource()); }));
    REQUIRE(throws<std::invalid_argument>([&] { KeyGenerator g(bfv, sk.data(), SeedSource()); }));
    // a pair is drawn public seed first, noise seed second, and a source that repeats itself is refused
    std::uint64_t a[8], b[8], want[8];
    detail::draw_seed_pair(counting, a, b);
    REQUIRE(drawn == 2);
    seed_number(0, want);
    REQUIRE(std::equal(a, a + 8, want));
    seed_number(1, want);
    REQUIRE(std::equal(b, b + 8, want));
    SeedSource stuck = [&](std::uint64_t *seed) { seed_number(7, seed); };
    REQUIRE(throws<std::logic_error>([&] { detail::draw_seed_pair(stuck, a, b); }));
    // generate_secret_key draws one seed; there is no host fallback behind it
    drawn = 0;
    REQUIRE(throws<std::logic_error>([&] { (void)KeyGenerator::generate_secret_key(bfv, counting); }));
    REQUIRE(drawn == 1);
    // the key generator draws before any device work, as it asks its sampler: two seeds for the public key, two per digit
    // of a key (this context: 2 digits at nsp = 2), and only then is refused for want of a device
    KeyGenerator gen(bfv, sk.data(), counting);
    drawn = 0;
    REQUIRE(throws<std::logic_error>([&] { (void)gen.public_key(); }));
    REQUIRE(drawn == 2);
    std::uint32_t k_first = 0, digits = 0;
    throw_on(sealhip_context_first_level(bfv.get(), &k_first));
    throw_on(sealhip_kswitch_digits(bfv.get(), k_first, &digits));
    drawn = 0;
    REQUIRE(throws<std::logic_error>([&] { (void)gen.relin_keys(2); }));
    REQUIRE(drawn == 2 * 2 * std::size_t(digits));
    // the sampler constructors are what they were
    Encryptor<HostCiphertext> old(bfv, pk.data(), sk.data(), [](std::int32_t *, std::int32_t *, std::int32_t *) {},
                                  [](std::uint64_t *, std::int32_t *) {});
    REQUIRE(old.last_sample_scratch().empty());
    std::printf("host-only sample checks ok\n");
    return 0;
}

static bool contains(const std::vector<unsigned char> &hay, const std::uint64_t *seed)
{
    const unsigned char *s = reinterpret_cast<const unsigned char *>(seed);
    for (std::size_t i = 0; i + 64 <= hay.size(); i++)
        if (std::memcmp(hay.data() + i, s, 64) == 0)
            return true;
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 3)
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
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        sealhip_params p{ scheme, log_n, n_key, nsp, mods.data(), t, SEALHIP_MODE_PARITY, std::atoi(argv[1]) };
        Context ctx(p);
        std::uint64_t pid[4];
        for (auto &v : pid)
            v = next();
        throw_on(sealhip_context_set_parms_id(ctx.get(), n_key, pid));
        HostPlaintext plain;
        plain.words.assign(in.begin() + at, in.begin() + at + (bfv ? n : k * n));
        plain.k = k;
        plain.ntt_form = !bfv;
        plain.scale = bfv ? 1.0 : 1073741824.0;

        std::size_t drawn = 0;
        SeedSource source = [&](std::uint64_t *seed) { seed_number(drawn++, seed); };

        // seed 0: the secret key
        const std::vector<std::uint64_t> sk = KeyGenerator::generate_secret_key(ctx, source);
        REQUIRE(drawn == 1);
        std::printf("sk digest %016llx\n", (unsigned long long)digest(sk.data(), sk.size()));
        // seeds 1, 2: the public key (c_1, noise)
        KeyGenerator gen(ctx, sk.data(), source);
        const std::vector<std::uint64_t> pk = gen.public_key();
        REQUIRE(drawn == 3);
        std::printf("pk digest %016llx\n", (unsigned long long)digest(pk.data(), pk.size()));
        // seeds 3 .. 2 + 2d: one relinearization key, digit by digit (c_1, noise)
        std::uint32_t digits = 0;
        throw_on(sealhip_kswitch_digits(ctx.get(), std::uint32_t(k), &digits));
        KeyGenerator::Keys rk = gen.relin_keys(1, true);
        REQUIRE(drawn == 3 + 2 * std::size_t(digits));
        const sealhip_kswitch_key *raw[1] = { rk[0]->get() };
        std::size_t need = 0, written = 0;
        throw_on(sealhip_kswitch_keys_save_seeded(ctx.get(), raw, 1, nullptr, 0, &need));
        std::vector<unsigned char> stream(need);
        throw_on(sealhip_kswitch_keys_save_seeded(ctx.get(), raw, 1, stream.data(), need, &written));
        stream.resize(written);
        for (std::size_t j = 0; j < digits; j++)
        {
            std::uint64_t c1[8], noise[8];
            seed_number(3 + 2 * j, c1);
            seed_number(4 + 2 * j, noise);
            REQUIRE(contains(stream, c1));     // the public seed of digit j is what the seeded save stores
            REQUIRE(!contains(stream, noise)); // its noise seed is nowhere in it
        }
        std::uint64_t other[8];
        for (std::size_t i = 0; i < 3; i++) // nor the seeds of the secret key and of the public key
        {
            seed_number(i, other);
            REQUIRE(!contains(stream, other));
        }
        throw_on(sealhip_kswitch_keys_save(ctx.get(), raw, 1, nullptr, 0, &need));
        std::vector<unsigned char> full(need);
        throw_on(sealhip_kswitch_keys_save(ctx.get(), raw, 1, full.data(), need, &written));
        std::printf("rk digest %016llx\n", (unsigned long long)digest(reinterpret_cast<const std::uint64_t *>(full.data()), written / 8));
        std::printf("seeded save ok\n");

        // the next seed: a resident public-key encryption; the two after it: a resident secret-key encryption
        const std::size_t before = drawn;
        Encryptor<HostCiphertext> enc(ctx, pk.data(), sk.data(), source);
        auto scratch_is_zero = [&](std::size_t blocks) { // (u and the noise: 2; the noise alone: 1)
            throw_on(sealhip_synchronize(ctx.get()));
            if (enc.last_sample_scratch().size() != blocks)
                return false;
            for (const auto &blk : enc.last_sample_scratch())
            {
                std::vector<unsigned char> host(blk.second, 1);
                throw_on(sealhip_memcpy_d2h(ctx.get(), host.data(), blk.first, blk.second));
                for (unsigned char c : host)
                    if (c)
                        return false;
            }
            return true;
        };
        DeviceCiphertext ca(ctx), cs(ctx);
        enc.encrypt(plain, ca);
        REQUIRE(drawn == before + 1);
        REQUIRE(scratch_is_zero(2));
        enc.encrypt_symmetric(plain, cs);
        REQUIRE(drawn == before + 3);
        REQUIRE(scratch_is_zero(1));
        HostCiphertext host;
        ca.download(host);
        REQUIRE(host.size() == 2 && host.coeff_modulus_size() == k);
        std::printf("asym digest %016llx\n", (unsigned long long)digest(host.data(), 2 * k * n));
        cs.download(host);
        std::printf("sym digest %016llx\n", (unsigned long long)digest(host.data(), 2 * k * n));
        std::printf("scratch zero ok\n");
        std::printf("seeds drawn %zu\n", drawn);
        std::printf("sample adapter ok\n");
        return 0;
    }
    catch (const std::exception &e)
    {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
}
