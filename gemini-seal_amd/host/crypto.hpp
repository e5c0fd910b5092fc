// crypto.hpp -- the client side of the C++ host adapter (include evaluator.hpp, which pulls this in): Decryptor,
// HostPlaintext, Encryptor and KeyGenerator over the sealhip C ABI, with the reference's method names, checks and
// exceptions (decryptor.h, encryptor.h, keygenerator.h).
#pragma once

#include "adapter_core.hpp"

namespace sealhip_host
{
    // Decryptor (decryptor.h / decryptor.cpp) over a context and the secret key in NTT form (n_key x N words, host). The powers
    // s^1..s^m live on the device and grow on demand, as compute_secret_key_array does (:152-216), by dyadic products on the
    // device. A plaintext is a vector of words: BFV, the coefficients mod t trimmed like bfv_decrypt (:112-116); CKKS, the
    // k x N words in NTT form. The batch overloads decrypt runs of ciphertexts of equal level and size with one call each.
    template <class CT>
    class Decryptor
    {
    public:
        Decryptor(const Context &context, const std::uint64_t *secret_key_ntt)
            : ctx_(context), sk_(secret_key_ntt, secret_key_ntt + context.n_key() * context.n())
        {}

        // decrypt (:51-75). The DeviceCiphertext overloads read the resident words in place (no upload) and are a
        // host-visible point of the Evaluator's deferred transparency check.
        template <class C>
        using IfCt = typename std::enable_if<std::is_same<C, CT>::value || std::is_same<C, DeviceCiphertext>::value, int>::type;
        template <class C, IfCt<C> = 0>
        void decrypt(const C &encrypted, std::vector<std::uint64_t> &destination)
        {
            std::vector<std::vector<std::uint64_t>> out;
            decrypt(std::vector<const C *>{ &encrypted }, out);
            destination.swap(out[0]);
        }
        // invariant_noise_budget (:269-325)
        template <class C, IfCt<C> = 0>
        int invariant_noise_budget(const C &encrypted)
        {
            return invariant_noise_budget(std::vector<const C *>{ &encrypted })[0];
        }
        template <class C, IfCt<C> = 0>
        void decrypt(const std::vector<const C *> &encrypted, std::vector<std::vector<std::uint64_t>> &destination)
        {
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            for (const C *ct : encrypted)
            {
                check_valid(*ct);
                if (bfv && ct->is_ntt_form())
                    throw std::invalid_argument("encrypted cannot be in NTT form"); // :79-82
                if (!bfv && !ct->is_ntt_form())
                    throw std::invalid_argument("encrypted must be in NTT form"); // :124-127
            }
            destination.assign(encrypted.size(), {});
            for_runs(encrypted, [&](std::size_t first, std::size_t count, std::size_t k, std::size_t size, const std::uint64_t *c,
                                    const std::uint64_t *powers) {
                const std::size_t n = ctx_.n(), words = bfv ? n : k * n;
                Staged o(ctx_, count * words);
                throw_on(sealhip_decryptor_decrypt(ctx_.get(), std::uint32_t(k), c, std::uint32_t(size), count, powers,
                                                   bfv ? 0 : 1, o.ptr()));
                std::vector<std::uint64_t> all(count * words);
                o.down(all.data(), all.size());
                for (std::size_t i = 0; i < count; i++)
                {
                    const std::uint64_t *p = all.data() + i * words;
                    std::size_t keep = words;
                    if (bfv) // get_significant_uint64_count_uint, at least one coefficient (:112-116)
                    {
                        while (keep > 1 && p[keep - 1] == 0)
                            keep--;
                    }
                    destination[first + i].assign(p, p + keep);
                }
            });
        }

        template <class C, IfCt<C> = 0>
        std::vector<int> invariant_noise_budget(const std::vector<const C *> &encrypted)
        {
            for (const C *ct : encrypted)
            {
                check_valid(*ct);
                if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                    throw std::logic_error("unsupported scheme"); // :276-279
                if (ct->is_ntt_form())
                    throw std::invalid_argument("encrypted cannot be in NTT form"); // :280-283
            }
            std::vector<int> out(encrypted.size(), 0);
            for_runs(encrypted, [&](std::size_t first, std::size_t count, std::size_t k, std::size_t size, const std::uint64_t *c,
                                    const std::uint64_t *powers) {
                std::vector<std::int32_t> b(count);
                throw_on(sealhip_decryptor_invariant_noise_budget(ctx_.get(), std::uint32_t(k), c, std::uint32_t(size), count,
                                                                  powers, b.data()));
                std::copy(b.begin(), b.end(), out.begin() + static_cast<std::ptrdiff_t>(first));
            });
            return out;
        }

    private:
        // is_valid_for (valcheck.cpp), the metadata the ABI cannot see
        template <class C>
        void check_valid(const C &ct) const
        {
            if (ct.size() < 2 || ct.size() > 16 || ct.coeff_modulus_size() < 1 || ct.coeff_modulus_size() > ctx_.n_key() ||
                ct.poly_modulus_degree() != ctx_.n())
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
        }

        // compute_secret_key_array (:152-216): s^1..s^max_power on the device, kept, and rebuilt longer on demand
        const std::uint64_t *powers(std::size_t max_power)
        {
            if (max_power <= n_powers_)
                return powers_->ptr();
            const std::size_t poly = ctx_.n_key() * ctx_.n();
            std::uint32_t k_first = 0; // the key base of the first data level: all n_key key primes
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            auto next = std::make_unique<Staged>(ctx_, max_power * poly);
            next->up(sk_.data(), poly);
            for (std::size_t i = 1; i < max_power; i++)
                throw_on(sealhip_dyadic_product_coeffmod(ctx_.get(), next->ptr() + (i - 1) * poly, next->ptr(), 1, k_first,
                                                         SEALHIP_BASE_KEY, next->ptr() + i * poly));
            powers_ = std::move(next);
            n_powers_ = max_power;
            return powers_->ptr();
        }

        // resident ciphertexts: each is its own run, read in place
        template <class F>
        void for_runs(const std::vector<const DeviceCiphertext *> &encrypted, F &&body)
        {
            ctx_.check_transparency();
            for (std::size_t i = 0; i < encrypted.size(); i++)
            {
                const DeviceCiphertext &c = *encrypted[i];
                const std::uint64_t *pw = powers(c.size() - 1);
                body(i, 1, c.coeff_modulus_size(), c.size(), c.data(), pw);
            }
        }
        // calls body(first, count, k, size, device ciphertexts, device powers) for each run of equal level and size
        template <class F>
        void for_runs(const std::vector<const CT *> &encrypted, F &&body)
        {
            for (std::size_t first = 0; first < encrypted.size();)
            {
                const std::size_t k = encrypted[first]->coeff_modulus_size(), size = encrypted[first]->size();
                std::size_t end = first + 1;
                while (end < encrypted.size() && encrypted[end]->coeff_modulus_size() == k && encrypted[end]->size() == size)
                    end++;
                const std::size_t words = size * k * ctx_.n(), count = end - first;
                const std::uint64_t *pw = powers(size - 1);
                Staged c(ctx_, count * words);
                for (std::size_t i = 0; i < count; i++)
                    throw_on(sealhip_memcpy_h2d(ctx_.get(), c.ptr() + i * words, encrypted[first + i]->data(), words * 8));
                body(first, count, k, size, c.ptr(), pw);
                first = end;
            }
        }

        const Context &ctx_;
        std::vector<std::uint64_t> sk_;
        std::unique_ptr<Staged> powers_;
        std::size_t n_powers_ = 0;
    };

    // A plaintext as Encryptor takes it: BFV, up to N coefficients < t in coefficient form (shorter is zero-padded);
    // CKKS, the k x N words of an NTT-form plaintext at level k, with its scale.
    struct HostPlaintext
    {
        std::vector<std::uint64_t> words;
        std::size_t k = 0; // CKKS: the level (coeff_modulus_size); BFV: unused
        bool ntt_form = false;
        double scale = 1.0;
    };

    // Encryptor (encryptor.h / encryptor.cpp:106-259) over a context and an optional public key (2 x n_key x N host words,
    // as KeyGenerator::public_key() returns) and an optional secret key (n_key x N, NTT form). Sampling stays with the
    // caller: asym_sampler(u, e0, e1) is asked once per public-key encryption for the N ternary values of
    // u and the N + N values of e_0, e_1; sym_sampler(seed, noise) once per secret-key encryption for the 8-word
    // BlakePRNGFactory().create() seed of c_1 and the N values of e. Ciphertexts are made on the device
    // (sealhip_encryptor_encrypt, sealhip_encryptor_encrypt_symmetric); the batch overloads make one call per run of equal
    // level. The seeded forms return the Serializable<Ciphertext> stream (the level's parms_id must be registered with
    // sealhip_context_set_parms_id). Built with a SeedSource instead of the samplers, it draws u and the noise on the device
    // from seeds: the library's own streams, the reference's noise law.
    template <class CT>
    class Encryptor
    {
    public:
        using AsymSampler = std::function<void(std::int32_t *u, std::int32_t *e0, std::int32_t *e1)>;
        using SymSampler = std::function<void(std::uint64_t *seed, std::int32_t *noise)>;

        Encryptor(const Context &context, const std::uint64_t *public_key, const std::uint64_t *secret_key_ntt,
                  AsymSampler asym_sampler, SymSampler sym_sampler)
            : ctx_(context), asym_(std::move(asym_sampler)), sym_(std::move(sym_sampler))
        {
            const std::size_t n = context.n(), nk = context.n_key();
            if (public_key)
                pk_.assign(public_key, public_key + 2 * nk * n);
            if (secret_key_ntt)
                sk_.assign(secret_key_ntt, secret_key_ntt + nk * n);
            std::uint32_t k_first = 0;
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            k_first_ = k_first;
        }
        // The samples drawn on the device: a public-key encryption asks `seeds` for one seed and samples (1, 2) = u, e_0,
        // e_1 from it; a secret-key encryption asks for two, c_1's seed and then a separate noise seed sampled as (0, 1) --
        // c_1's seed is public in a seeded stream, the noise seed never leaves this call. The scratch that held the samples
        // is erased before it goes back to the pool.
        Encryptor(const Context &context, const std::uint64_t *public_key, const std::uint64_t *secret_key_ntt, SeedSource seeds)
            : Encryptor(context, public_key, secret_key_ntt, AsymSampler(), SymSampler())
        {
            if (!seeds)
                throw std::invalid_argument("seed source is empty");
            seeds_ = std::move(seeds);
        }
        // where the samples of the last seed-source encryption lay on the device (pointer, bytes), for tests: the blocks
        // are back in the pool, erased
        const std::vector<std::pair<const void *, std::size_t>> &last_sample_scratch() const { return scratch_; }
        void set_public_key(const std::uint64_t *public_key)
        {
            pk_.assign(public_key, public_key + 2 * ctx_.n_key() * ctx_.n());
            dpk_.reset();
        }
        void set_secret_key(const std::uint64_t *secret_key_ntt)
        {
            sk_.assign(secret_key_ntt, secret_key_ntt + ctx_.n_key() * ctx_.n());
            dsk_.reset();
        }

        // A destination is a host ciphertext, or a resident one: the words then stay on the device (the samples still come
        // from the samplers)
        template <class D>
        using IfCt = typename std::enable_if<std::is_same<D, CT>::value || std::is_same<D, DeviceCiphertext>::value, int>::type;

        // encrypt (:205-253) / encrypt_zero() at the first level / encrypt_zero(parms_id) at level k
        template <class D, IfCt<D> = 0>
        void encrypt(const HostPlaintext &plain, D &destination) { run_one(true, &plain, destination, 0); }
        template <class D, IfCt<D> = 0>
        void encrypt_zero(D &destination) { run_one(true, nullptr, destination, k_first_); }
        template <class D, IfCt<D> = 0>
        void encrypt_zero(std::size_t k, D &destination) { run_one(true, nullptr, destination, k); }
        void encrypt(const std::vector<const HostPlaintext *> &plain, std::vector<CT *> destination)
        {
            run(true, plain, destination, 0, false);
        }
        void encrypt_zero(std::size_t k, std::vector<CT *> destination) { run(true, {}, destination, k, false); }

        // encrypt_symmetric / encrypt_zero_symmetric (rlwe.cpp:204-300)
        template <class D, IfCt<D> = 0>
        void encrypt_symmetric(const HostPlaintext &plain, D &destination) { run_one(false, &plain, destination, 0); }
        template <class D, IfCt<D> = 0>
        void encrypt_zero_symmetric(D &destination) { run_one(false, nullptr, destination, k_first_); }
        template <class D, IfCt<D> = 0>
        void encrypt_zero_symmetric(std::size_t k, D &destination) { run_one(false, nullptr, destination, k); }
        void encrypt_symmetric(const std::vector<const HostPlaintext *> &plain, std::vector<CT *> destination)
        {
            run(false, plain, destination, 0, false);
        }
        void encrypt_zero_symmetric(std::size_t k, std::vector<CT *> destination) { run(false, {}, destination, k, false); }

        // encrypt_symmetric(plain) returning Serializable<Ciphertext> (encryptor.h:371-376): the stream of c_0 and the seed.
        // parms_id: that of the ciphertext's level (it is written into the stream and must be registered with
        // sealhip_context_set_parms_id); destination (optional) receives the ciphertext with c_1 expanded.
        std::vector<unsigned char> encrypt_symmetric_seeded(const HostPlaintext &plain, const std::uint64_t parms_id[4],
                                                            CT *destination = nullptr)
        {
            return seeded(&plain, k_first_, parms_id, destination);
        }
        std::vector<unsigned char> encrypt_zero_symmetric_seeded(std::size_t k, const std::uint64_t parms_id[4],
                                                                 CT *destination = nullptr)
        {
            return seeded(nullptr, k, parms_id, destination);
        }

    private:
        // one encryption (plain null: of zero, at level k_zero)
        template <class D>
        void run_one(bool asymmetric, const HostPlaintext *plain, D &destination, std::size_t k_zero)
        {
            std::vector<D *> d{ &destination };
            run(asymmetric, std::vector<const HostPlaintext *>(plain ? 1 : 0, plain), d, k_zero, false);
        }

        // is_metadata_valid_for / the form checks of encrypt_internal (:185-238) on the host; returns the level
        std::size_t check_plain(const HostPlaintext &p) const
        {
            const std::size_t n = ctx_.n();
            if (ctx_.scheme() == SEALHIP_SCHEME_BFV)
            {
                if (p.words.size() > n || std::any_of(p.words.begin(), p.words.end(),
                                                      [&](std::uint64_t v) { return v >= ctx_.plain_modulus(); }))
                    throw std::invalid_argument("plain is not valid for encryption parameters");
                if (p.ntt_form)
                    throw std::invalid_argument("plain cannot be in NTT form");
                return k_first_;
            }
            if (p.k < 1 || p.k > k_first_ || p.words.size() != p.k * n)
                throw std::invalid_argument("plain is not valid for encryption parameters");
            if (!p.ntt_form)
                throw std::invalid_argument("plain must be in NTT form");
            return p.k;
        }
        void check_keys(bool asymmetric) const
        {
            if (asymmetric && pk_.empty())
                throw std::logic_error("public key is not set");
            if (!asymmetric && sk_.empty())
                throw std::logic_error("secret key is not set");
        }

        // one device call per run of plaintexts of equal level (plain empty: destination.size() zero encryptions at k)
        // the key on the device, uploaded once and kept across calls
        const std::uint64_t *device_key(bool asymmetric)
        {
            const std::size_t words = (asymmetric ? 2 : 1) * ctx_.n_key() * ctx_.n();
            std::unique_ptr<Staged> &key = asymmetric ? dpk_ : dsk_;
            if (!key)
            {
                std::unique_ptr<Staged> up(new Staged(ctx_, words));
                up->up(asymmetric ? pk_.data() : sk_.data(), words);
                key = std::move(up);
            }
            return key->ptr();
        }
        // item i of the `count` encryptions in `ct` becomes the destination's words
        void deliver(CT &d, Staged &ct, std::size_t i, std::size_t count, std::size_t words, std::size_t k)
        {
            (void)count;
            d.resize_raw(2, k);
            throw_on(sealhip_memcpy_d2h(ctx_.get(), d.data(), ct.ptr() + i * words, words * 8));
        }
        void deliver(DeviceCiphertext &d, Staged &ct, std::size_t i, std::size_t count, std::size_t words, std::size_t k)
        {
            d.adopt_result(ct, i, count, words, 2, k);
        }

        template <class D>
        void run(bool asymmetric, const std::vector<const HostPlaintext *> &plain, std::vector<D *> &destination,
                 std::size_t k_zero, bool save_seed, std::vector<std::uint64_t> *seeds_out = nullptr)
        {
            check_keys(asymmetric);
            const bool zero = plain.empty();
            if (!zero && plain.size() != destination.size())
                throw std::invalid_argument("destination count does not match");
            if (zero && (k_zero < 1 || k_zero > ctx_.n_key()))
                throw std::invalid_argument("parms_id is not valid for encryption parameters");
            std::vector<std::size_t> level(destination.size(), k_zero);
            for (std::size_t i = 0; !zero && i < plain.size(); i++)
                level[i] = check_plain(*plain[i]);
            const std::size_t n = ctx_.n();
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            const std::uint64_t *key = device_key(asymmetric);
            for (std::size_t first = 0; first < destination.size();)
            {
                const std::size_t k = level[first];
                std::size_t end = first + 1;
                while (end < destination.size() && level[end] == k)
                    end++;
                const std::size_t count = end - first, words = 2 * k * n;
                const std::size_t pw = bfv ? n : k * n; // plaintext words per item
                std::vector<std::uint64_t> host_plain(zero ? 0 : count * pw, 0);
                for (std::size_t i = 0; !zero && i < count; i++) // BFV plaintexts shorter than N are zero-padded
                    std::copy(plain[first + i]->words.begin(), plain[first + i]->words.end(), host_plain.begin() + i * pw);
                std::unique_ptr<Staged> dp(zero ? nullptr : new Staged(ctx_, host_plain.size()));
                if (dp)
                    dp->up(host_plain.data(), host_plain.size());
                Staged ct(ctx_, count * words);
                if (seeds_)
                {
                    std::vector<std::uint64_t> seeds(count * 8), noise_seeds(asymmetric ? 0 : count * 8);
                    for (std::size_t i = 0; i < count; i++)
                    {
                        if (asymmetric)
                            seeds_(seeds.data() + 8 * i);
                        else
                            detail::draw_seed_pair(seeds_, seeds.data() + 8 * i, noise_seeds.data() + 8 * i);
                    }
                    ZeroedStaged du(ctx_, asymmetric ? (count * n + 1) / 2 : 0), de(ctx_, (count * (asymmetric ? 2 : 1) * n + 1) / 2);
                    auto *u32 = reinterpret_cast<std::int32_t *>(du.ptr()), *e32 = reinterpret_cast<std::int32_t *>(de.ptr());
                    scratch_.assign({ { de.ptr(), de.words() * 8 } });
                    if (asymmetric)
                        scratch_.push_back({ du.ptr(), du.words() * 8 });
                    if (asymmetric)
                    {
                        throw_on(sealhip_sample_polys_split(ctx_.get(), seeds.data(), count, 1, 2, u32, e32));
                        throw_on(sealhip_encryptor_encrypt(ctx_.get(), std::uint32_t(k), key, dp ? dp->ptr() : nullptr, pw, u32,
                                                           e32, count, ct.ptr()));
                        std::fill(seeds.begin(), seeds.end(), 0); // (u and the noise follow from them)
                    }
                    else
                    {
                        throw_on(sealhip_sample_polys(ctx_.get(), noise_seeds.data(), count, 0, 1, e32, 0));
                        throw_on(sealhip_encryptor_encrypt_symmetric(ctx_.get(), std::uint32_t(k), key,
                                                                     dp ? dp->ptr() : nullptr, pw, seeds.data(), e32,
                                                                     save_seed ? 1 : 0, count, ct.ptr()));
                        std::fill(noise_seeds.begin(), noise_seeds.end(), 0);
                        if (seeds_out) // c_1's seeds only: the noise seeds stay here
                            seeds_out->insert(seeds_out->end(), seeds.begin(), seeds.end());
                    }
                }
                else if (asymmetric)
                {
                    std::vector<std::int32_t> u(count * n), e(count * 2 * n);
                    for (std::size_t i = 0; i < count; i++)
                        asym_(u.data() + i * n, e.data() + 2 * i * n, e.data() + (2 * i + 1) * n);
                    Staged du(ctx_, (u.size() + 1) / 2), de(ctx_, (e.size() + 1) / 2);
                    throw_on(sealhip_memcpy_h2d(ctx_.get(), du.ptr(), u.data(), u.size() * 4));
                    throw_on(sealhip_memcpy_h2d(ctx_.get(), de.ptr(), e.data(), e.size() * 4));
                    throw_on(sealhip_encryptor_encrypt(ctx_.get(), std::uint32_t(k), key, dp ? dp->ptr() : nullptr, pw,
                                                       reinterpret_cast<const std::int32_t *>(du.ptr()),
                                                       reinterpret_cast<const std::int32_t *>(de.ptr()), count, ct.ptr()));
                }
                else
                {
                    std::vector<std::uint64_t> seeds(count * 8);
                    std::vector<std::int32_t> e(count * n);
                    for (std::size_t i = 0; i < count; i++)
                        sym_(seeds.data() + 8 * i, e.data() + i * n);
                    Staged de(ctx_, (e.size() + 1) / 2);
                    throw_on(sealhip_memcpy_h2d(ctx_.get(), de.ptr(), e.data(), e.size() * 4));
                    throw_on(sealhip_encryptor_encrypt_symmetric(ctx_.get(), std::uint32_t(k), key,
                                                                 dp ? dp->ptr() : nullptr, pw, seeds.data(),
                                                                 reinterpret_cast<const std::int32_t *>(de.ptr()),
                                                                 save_seed ? 1 : 0, count, ct.ptr()));
                    if (seeds_out)
                        seeds_out->insert(seeds_out->end(), seeds.begin(), seeds.end());
                }
                for (std::size_t i = 0; i < count; i++)
                {
                    D &d = *destination[first + i];
                    deliver(d, ct, i, count, words, k);
                    d.is_ntt_form() = !bfv;
                    // encrypt_zero_* set 1.0; CKKS encrypt takes the plaintext's scale (:252)
                    d.scale() = (!zero && !bfv) ? plain[first + i]->scale : 1.0;
                }
                first = end;
            }
        }

        std::vector<unsigned char> seeded(const HostPlaintext *plain, std::size_t k, const std::uint64_t *pid, CT *destination)
        {
            CT local{};
            CT &d = destination ? *destination : local;
            if (!destination)
                prepare(local);
            std::vector<CT *> dst{ &d };
            std::vector<std::uint64_t> seed;
            if (plain)
                run(false, std::vector<const HostPlaintext *>{ plain }, dst, 0, true, &seed);
            else
                run(false, {}, dst, k, true, &seed);
            const std::size_t kk = d.coeff_modulus_size(), n = ctx_.n();
            if (kk * n < 9) // rlwe.cpp:225-230: the reference drops save_seed and saves both polynomials
                throw std::logic_error("polynomial is too small to store a seed");
            sealhip_ciphertext_info info{};
            std::copy(pid, pid + 4, info.parms_id);
            info.is_ntt_form = d.is_ntt_form() ? 1 : 0;
            info.size = 2;
            info.coeff_modulus_size = std::uint32_t(kk);
            info.poly_modulus_degree = n;
            info.scale = d.scale();
            Staged c(ctx_, 2 * kk * n);
            c.up(d.data(), 2 * kk * n);
            std::size_t need = 0;
            throw_on(sealhip_ciphertext_save_seeded(ctx_.get(), &info, c.ptr(), seed.data(), nullptr, 0, &need));
            std::vector<unsigned char> bytes(need);
            std::size_t written = 0;
            throw_on(sealhip_ciphertext_save_seeded(ctx_.get(), &info, c.ptr(), seed.data(), bytes.data(), need, &written));
            bytes.resize(written);
            return bytes;
        }
        template <class C = CT>
        auto prepare(C &c) -> decltype(c.n_ = 0, void()) { c.n_ = ctx_.n(); }
        void prepare(...) {}

        const Context &ctx_;
        std::vector<std::uint64_t> pk_, sk_;
        std::unique_ptr<Staged> dpk_, dsk_; // the keys on the device (device_key)
        AsymSampler asym_;
        SymSampler sym_;
        SeedSource seeds_; // set: the samples are drawn on the device
        std::vector<std::pair<const void *, std::size_t>> scratch_;
        std::size_t k_first_ = 0;
    };

    // KeyGenerator (keygenerator.h / keygenerator.cpp:105-240) over a context and a secret key in NTT form (n_key x N words,
    // host). Sampling stays with the caller: `sampler(seed, noise)` is asked once per encrypt_zero_symmetric, in the
    // reference's order (key by key, digit by digit), for the 8-word BlakePRNGFactory().create() seed of c_1 and the N
    // signed values of sample_poly_normal. The keys are made on the device (sealhip_generate_*_keys).
    // Built with a SeedSource instead of the sampler, it draws the noise on the device from seeds.
    class KeyGenerator
    {
    public:
        using Sampler = std::function<void(std::uint64_t *seed, std::int32_t *noise)>;
        using Keys = std::vector<std::unique_ptr<KSwitchKeys>>;
        using GaloisKeys = std::map<std::uint32_t, std::unique_ptr<KSwitchKeys>>; // galois_elt -> key (GaloisKeys::get_index)

        KeyGenerator(const Context &context, const std::uint64_t *secret_key_ntt, Sampler sampler)
            : ctx_(context), sk_(secret_key_ntt, secret_key_ntt + context.n_key() * context.n()), sampler_(std::move(sampler))
        {}
        // The noise drawn on the device: every encrypt_zero_symmetric (a key digit, the public key) asks `seeds` for two
        // seeds, c_1's and then a separate noise seed sampled as (0, 1). save_seed keeps c_1's seeds only.
        KeyGenerator(const Context &context, const std::uint64_t *secret_key_ntt, SeedSource seeds)
            : ctx_(context), sk_(secret_key_ntt, secret_key_ntt + context.n_key() * context.n()), seeds_(std::move(seeds))
        {
            if (!seeds_)
                throw std::invalid_argument("seed source is empty");
        }

        // generate_sk (keygenerator.cpp:66-103) on the device from one seed of `seeds` (sealhip_generate_secret_key): the
        // n_key x N words of the secret key in NTT form
        static std::vector<std::uint64_t> generate_secret_key(const Context &context, const SeedSource &seeds)
        {
            return secret_key(context, seeds, 0);
        }
        // the same with the fixed-weight polynomial of Hamming weight h, 1 .. N, in place of the ternary one
        // (sealhip_generate_sparse_secret_key)
        static std::vector<std::uint64_t> generate_sparse_secret_key(const Context &context, const SeedSource &seeds, std::uint32_t h)
        {
            if (h < 1 || h > context.n())
                throw std::invalid_argument("h must be 1 .. N");
            return secret_key(context, seeds, h);
        }

        // Key-switch keys from OTHER secrets to this generator's (sealhip_generate_switching_keys): keys[i] switches what is
        // encrypted under from_secret_keys_ntt[i] (count x n_key x N words, NTT form) to the secret key this generator was
        // built with. level 0 or n_ct: the full key; a smaller level: a key for key switches at levels <= level only, which
        // publishes nothing above it and cannot keep its seeds (encapsulation's dense -> sparse key takes level 1). Samples
        // are drawn as for relin_keys, key by key, digit by digit.
        Keys switching_keys(const std::uint64_t *from_secret_keys_ntt, std::size_t count, std::size_t level = 0,
                            bool save_seed = false)
        {
            if (!count || count > 14)
                throw std::invalid_argument("invalid count");
            if (!from_secret_keys_ntt)
                throw std::invalid_argument("from_secret_keys_ntt is null");
            std::uint32_t k_first = 0;
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            if (level > k_first)
                throw std::invalid_argument("level k out of range");
            return generate(nullptr, count, save_seed, from_secret_keys_ntt, level ? level : k_first);
        }

        // RGSW encryptions of small polynomials under this generator's secret key (sealhip_generate_rgsw, DESIGN.md section
        // 29): messages[i] holds the N signed coefficients of m_i. level as switching_keys. Samples are drawn as for
        // relin_keys: message by message, K_b's digits before K_a's.
        std::vector<std::unique_ptr<RgswCiphertext>> rgsw(const std::vector<std::vector<std::int32_t>> &messages, std::size_t level = 0)
        {
            const std::size_t n = ctx_.n(), nk = ctx_.n_key(), count = messages.size();
            if (!count)
                throw std::invalid_argument("invalid count");
            for (const auto &m : messages)
                if (m.size() != n)
                    throw std::invalid_argument("an rgsw message has N coefficients");
            std::uint32_t k_first = 0, digits = 0;
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            if (level > k_first)
                throw std::invalid_argument("level k out of range");
            throw_on(sealhip_kswitch_digits(ctx_.get(), k_first, &digits));
            const std::size_t items = count * 2 * digits;
            std::vector<std::uint64_t> seeds(items * 8);
            Drawn drawn = draw(seeds.data(), items);
            Staged sk(ctx_, nk * n);
            ZeroedStaged e(ctx_, (items * n + 1) / 2), mm(ctx_, (count * n + 1) / 2);
            sk.up(sk_.data(), nk * n);
            to_device(drawn, items, e);
            for (std::size_t i = 0; i < count; i++)
                throw_on(sealhip_memcpy_h2d(ctx_.get(), reinterpret_cast<std::int32_t *>(mm.ptr()) + i * n, messages[i].data(),
                                            n * sizeof(std::int32_t)));
            std::vector<sealhip_rgsw *> raw(count, nullptr);
            throw_on(sealhip_generate_rgsw(ctx_.get(), sk.ptr(), reinterpret_cast<const std::int32_t *>(mm.ptr()), std::uint32_t(count),
                                           std::uint32_t(level ? level : k_first), seeds.data(),
                                           reinterpret_cast<const std::int32_t *>(e.ptr()), raw.data()));
            std::vector<std::unique_ptr<RgswCiphertext>> out;
            for (auto *h : raw)
                out.push_back(std::make_unique<RgswCiphertext>(ctx_, h));
            return out;
        }

        // The keys of a blind rotation under this generator's secret key (sealhip_generate_blind_rotation_keys, DESIGN.md
        // section 30) for an LWE secret with coefficients in {-1, 0, 1} (binary: {0, 1}): n_steps = lwe_secret.size(), or twice
        // that with `ternary`. level as switching_keys. Samples are drawn as for rgsw: step by step, K_b's digits before
        // K_a's. The staged secret is erased in stream order.
        std::unique_ptr<BlindRotationKeys> blind_rotation_keys(const std::vector<std::int32_t> &lwe_secret, bool ternary,
                                                               std::size_t level = 0)
        {
            const std::size_t n = ctx_.n(), nk = ctx_.n_key(), n_lwe = lwe_secret.size(), count = n_lwe * (ternary ? 2 : 1);
            if (!n_lwe)
                throw std::invalid_argument("invalid count");
            for (std::int32_t s : lwe_secret)
                if (s > 1 || s < (ternary ? -1 : 0))
                    throw std::invalid_argument("an LWE secret has coefficients in {-1, 0, 1} (binary: {0, 1})");
            std::uint32_t k_first = 0, digits = 0;
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            if (level > k_first)
                throw std::invalid_argument("level k out of range");
            throw_on(sealhip_kswitch_digits(ctx_.get(), k_first, &digits));
            const std::size_t items = count * 2 * digits;
            std::vector<std::uint64_t> seeds(items * 8);
            Drawn drawn = draw(seeds.data(), items);
            Staged sk(ctx_, nk * n);
            ZeroedStaged e(ctx_, (items * n + 1) / 2), ss(ctx_, (n_lwe + 1) / 2);
            sk.up(sk_.data(), nk * n);
            to_device(drawn, items, e);
            throw_on(sealhip_memcpy_h2d(ctx_.get(), ss.ptr(), lwe_secret.data(), n_lwe * sizeof(std::int32_t)));
            std::vector<sealhip_rgsw *> raw(count, nullptr);
            throw_on(sealhip_generate_blind_rotation_keys(ctx_.get(), sk.ptr(), reinterpret_cast<const std::int32_t *>(ss.ptr()),
                                                          std::uint32_t(n_lwe), ternary ? 1 : 0, std::uint32_t(level ? level : k_first),
                                                          seeds.data(), reinterpret_cast<const std::int32_t *>(e.ptr()), raw.data()));
            std::vector<std::unique_ptr<RgswCiphertext>> made;
            for (auto *h : raw)
                made.push_back(std::make_unique<RgswCiphertext>(ctx_, h));
            return std::make_unique<BlindRotationKeys>(std::move(made), ternary);
        }

    private:
        // h = 0: the ternary polynomial
        static std::vector<std::uint64_t> secret_key(const Context &context, const SeedSource &seeds, std::uint32_t h)
        {
            std::uint64_t seed[8];
            seeds(seed);
            const std::size_t words = context.n_key() * context.n();
            ZeroedStaged sk(context, words);
            throw_on(h ? sealhip_generate_sparse_secret_key(context.get(), seed, h, sk.ptr())
                       : sealhip_generate_secret_key(context.get(), seed, sk.ptr()));
            std::fill(seed, seed + 8, 0);
            std::vector<std::uint64_t> out(words);
            sk.down(out.data(), words);
            return out;
        }

    public:
        // relin_keys(count, save_seed) (:146-175): keys[i] is the key of sk^(i+2) (RelinKeys::get_index(i + 2) = i)
        Keys relin_keys(std::size_t count, bool save_seed = false)
        {
            if (!count || count > 14) // SEAL_CIPHERTEXT_SIZE_MAX - 2
                throw std::invalid_argument("invalid count");
            return generate(nullptr, count, save_seed);
        }

        // galois_keys(galois_elts, save_seed) (:177-240): invalid elements throw before any sample is drawn; an element that
        // is already present is skipped and draws no samples (has_key)
        GaloisKeys galois_keys(const std::vector<std::uint32_t> &galois_elts, bool save_seed = false)
        {
            std::int32_t batching = 0;
            throw_on(sealhip_context_using_batching(ctx_.get(), &batching));
            if (!batching && ctx_.scheme() == SEALHIP_SCHEME_BFV)
                throw std::logic_error("encryption parameters do not support batching");
            std::vector<std::uint32_t> elts;
            for (std::uint32_t elt : galois_elts)
            {
                if (!(elt & 1) || elt >= 2 * ctx_.n())
                    throw std::invalid_argument("Galois element is not valid");
                if (std::find(elts.begin(), elts.end(), elt) == elts.end())
                    elts.push_back(elt);
            }
            Keys made = generate(elts.data(), elts.size(), save_seed);
            GaloisKeys out;
            for (std::size_t i = 0; i < elts.size(); i++)
                out.emplace(elts[i], std::move(made[i]));
            return out;
        }
        // galois_keys(steps) (keygenerator.h:180-208): GaloisTool::get_elts_from_steps
        GaloisKeys galois_keys(const std::vector<int> &steps, bool save_seed = false)
        {
            std::vector<std::uint32_t> elts;
            for (int step : steps)
            {
                std::uint32_t elt = 0;
                throw_on(sealhip_galois_elt_from_step(ctx_.get(), step, &elt));
                elts.push_back(elt);
            }
            return galois_keys(elts, save_seed);
        }
        // galois_keys() (keygenerator.h:224-247): GaloisTool::get_elts_all (galois.cpp:102-127), in its order
        GaloisKeys galois_keys(bool save_seed = false) { return galois_keys(elts_all(), save_seed); }

        // generate_pk (keygenerator.cpp:105-136): encrypt_zero_symmetric at the key level in NTT form, no seed kept; returns
        // the 2 x n_key x N words of the public key
        std::vector<std::uint64_t> public_key()
        {
            const std::size_t n = ctx_.n(), nk = ctx_.n_key();
            std::uint64_t seed[8];
            Drawn drawn = draw(seed, 1);
            Staged sk(ctx_, nk * n), a(ctx_, nk * n), ct(ctx_, 2 * nk * n);
            ZeroedStaged e(ctx_, (n + 1) / 2);
            sk.up(sk_.data(), nk * n);
            to_device(drawn, 1, e);
            throw_on(sealhip_expand_seed(ctx_.get(), std::uint32_t(nk), seed, 1, a.ptr(), 0));
            throw_on(sealhip_encrypt_zero_symmetric(ctx_.get(), std::uint32_t(nk), 1, a.ptr(),
                                                    reinterpret_cast<const std::int32_t *>(e.ptr()), sk.ptr(), 1, ct.ptr()));
            std::vector<std::uint64_t> pk(2 * nk * n);
            ct.down(pk.data(), pk.size());
            return pk;
        }

        std::vector<std::uint32_t> elts_all() const
        {
            const std::uint64_t m = 2 * static_cast<std::uint64_t>(ctx_.n());
            std::uint64_t pos = 5, neg = 1; // neg = 5^-1 mod m = 5^(N/2 - 1): the order of 5 is N/2
            for (std::size_t i = 0; i + 1 < ctx_.n() / 2; i++)
                neg = (neg * 5) & (m - 1);
            std::vector<std::uint32_t> out{ static_cast<std::uint32_t>(m - 1) };
            for (std::size_t i = 0; (std::size_t(2) << i) < ctx_.n(); i++) // coeff_count_power - 1 rounds
            {
                out.push_back(static_cast<std::uint32_t>(pos));
                pos = (pos * pos) & (m - 1);
                out.push_back(static_cast<std::uint32_t>(neg));
                neg = (neg * neg) & (m - 1);
            }
            return out;
        }

    private:
        // from (n_keys x n_key x N, with elts == nullptr): switching keys from those secrets at `level`
        Keys generate(const std::uint32_t *elts, std::size_t n_keys, bool save_seed, const std::uint64_t *from = nullptr,
                      std::size_t level = 0)
        {
            Keys out;
            if (!n_keys)
                return out;
            std::uint32_t k_first = 0, digits = 0;
            throw_on(sealhip_context_first_level(ctx_.get(), &k_first));
            throw_on(sealhip_kswitch_digits(ctx_.get(), k_first, &digits));
            const std::size_t n = ctx_.n(), nk = ctx_.n_key(), d = digits, items = n_keys * d;
            std::vector<std::uint64_t> seeds(items * 8);
            Drawn drawn = draw(seeds.data(), items);
            Staged sk(ctx_, nk * n);
            ZeroedStaged e(ctx_, (items * n + 1) / 2);
            sk.up(sk_.data(), nk * n);
            to_device(drawn, items, e);
            std::vector<sealhip_kswitch_key *> raw(n_keys, nullptr);
            const auto *en = reinterpret_cast<const std::int32_t *>(e.ptr());
            if (from)
            {
                ZeroedStaged other(ctx_, n_keys * nk * n);
                other.up(from, n_keys * nk * n);
                throw_on(sealhip_generate_switching_keys(ctx_.get(), sk.ptr(), other.ptr(), std::uint32_t(n_keys),
                                                         std::uint32_t(level), seeds.data(), en, save_seed ? 1 : 0, raw.data()));
            }
            else if (elts)
                throw_on(sealhip_generate_galois_keys(ctx_.get(), sk.ptr(), elts, std::uint32_t(n_keys), seeds.data(), en,
                                                      save_seed ? 1 : 0, raw.data()));
            else
                throw_on(sealhip_generate_relin_keys(ctx_.get(), sk.ptr(), std::uint32_t(n_keys), seeds.data(), en,
                                                     save_seed ? 1 : 0, raw.data()));
            for (auto *h : raw)
                out.push_back(std::make_unique<KSwitchKeys>(ctx_, h));
            return out;
        }

        // What `items` encrypt_zero_symmetric calls draw on the host, item by item in the reference's order, before any
        // device work: c_1's seed (into seeds, 8 words per item) and either the N noise values from the sampler, or a second
        // seed from the seed source, from which to_device samples them as (0, 1) and which is dropped there
        struct Drawn
        {
            std::vector<std::int32_t> noise;
            std::vector<std::uint64_t> noise_seeds;
        };
        Drawn draw(std::uint64_t *seeds, std::size_t items)
        {
            Drawn d;
            const std::size_t n = ctx_.n();
            if (seeds_)
            {
                d.noise_seeds.resize(items * 8);
                for (std::size_t i = 0; i < items; i++)
                    detail::draw_seed_pair(seeds_, seeds + 8 * i, d.noise_seeds.data() + 8 * i);
                return d;
            }
            d.noise.resize(items * n);
            for (std::size_t i = 0; i < items; i++)
                sampler_(seeds + 8 * i, d.noise.data() + n * i);
            return d;
        }
        void to_device(Drawn &d, std::size_t items, Staged &e)
        {
            auto *e32 = reinterpret_cast<std::int32_t *>(e.ptr());
            if (seeds_)
            {
                throw_on(sealhip_sample_polys(ctx_.get(), d.noise_seeds.data(), items, 0, 1, e32, 0));
                std::fill(d.noise_seeds.begin(), d.noise_seeds.end(), 0);
            }
            else
                throw_on(sealhip_memcpy_h2d(ctx_.get(), e32, d.noise.data(), d.noise.size() * sizeof(std::int32_t)));
        }

        const Context &ctx_;
        std::vector<std::uint64_t> sk_;
        Sampler sampler_;
        SeedSource seeds_; // set: the noise is drawn on the device
    };
} // namespace sealhip_host
