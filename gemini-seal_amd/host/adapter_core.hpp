// adapter_core.hpp -- what the classes of the C++ host adapter share (include evaluator.hpp, which pulls this in): the
// translation of the ABI's result codes into the reference's exceptions (throw_on), the plain HostCiphertext, the Context,
// the pool-block owner and the stagings on it (PoolBlock, Staged, ZeroedStaged), the resident DeviceCiphertext and
// DevicePlaintext, and the handles of keys, RGSW ciphertexts, tables and LWE samples.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/sealhip.h"

namespace sealhip_host
{
    inline void throw_on(long hr)
    {
        if (hr == SEALHIP_S_OK)
            return;
        const std::string msg = sealhip_last_error_string();
        if (hr == SEALHIP_E_INVALIDARG || hr == SEALHIP_E_POINTER)
            throw std::invalid_argument(msg);
        if (hr == SEALHIP_COR_E_INVALIDOPERATION)
            throw std::logic_error(msg);
        if (hr == SEALHIP_E_OUTOFMEMORY)
            throw std::bad_alloc();
        throw std::runtime_error(msg);
    }

    // Plain stand-in with the reference's layout (ciphertext.h:359-368): size x k x N uint64, row-major.
    struct HostCiphertext
    {
        std::vector<std::uint64_t> words;
        std::size_t size_ = 0, k_ = 0, n_ = 0;
        bool ntt_form_ = false;
        double scale_ = 1.0;
        std::uint64_t *data() { return words.data(); }
        const std::uint64_t *data() const { return words.data(); }
        std::size_t size() const { return size_; }
        std::size_t coeff_modulus_size() const { return k_; }
        std::size_t poly_modulus_degree() const { return n_; }
        bool &is_ntt_form() { return ntt_form_; }
        bool is_ntt_form() const { return ntt_form_; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        void resize_raw(std::size_t size, std::size_t k)
        {
            // like IntArray::resize: keeps the leading words, zero-fills the rest (ciphertext.cpp:84-133)
            std::vector<std::uint64_t> next(size * k * n_, 0);
            const std::size_t polys = size < size_ ? size : size_;
            const std::size_t rows = k < k_ ? k : k_;
            for (std::size_t s = 0; s < polys; s++)
                for (std::size_t r = 0; r < rows; r++)
                    for (std::size_t c = 0; c < n_; c++)
                        next[(s * k + r) * n_ + c] = words[(s * k_ + r) * n_ + c];
            words.swap(next);
            size_ = size;
            k_ = k;
        }
    };

    class Context
    {
    public:
        explicit Context(const sealhip_params &p)
            : scheme_(p.scheme), n_(std::size_t(1) << p.log_n), t_(p.plain_modulus), n_key_(p.n_key_moduli),
              key_moduli_(p.key_moduli ? p.key_moduli : nullptr, p.key_moduli ? p.key_moduli + p.n_key_moduli : nullptr)
        {
            throw_on(sealhip_context_create(&p, &ctx_));
        }
        ~Context()
        {
            if (ctx_)
                sealhip_context_destroy(ctx_); // (frees every pool block, the transparency rings' included)
        }
        Context(const Context &) = delete;
        Context &operator=(const Context &) = delete;
        sealhip_context *get() const { return ctx_; }
        std::uint32_t scheme() const { return scheme_; }
        std::size_t n() const { return n_; }
        std::uint64_t plain_modulus() const { return t_; }
        std::size_t n_key() const { return n_key_; } // the highest level the ABI names (key level)
        std::uint64_t key_modulus(std::size_t i) const { return key_moduli_.at(i); } // q_i; the special primes come last

        // SEALContext's parms_id of level k (sealhip_context_set_parms_id), kept for DeviceCiphertext::save
        void set_parms_id(std::size_t k, const std::uint64_t parms_id[4])
        {
            throw_on(sealhip_context_set_parms_id(ctx_, std::uint32_t(k), parms_id));
            std::lock_guard<std::mutex> lock(mu_);
            std::copy(parms_id, parms_id + 4, parms_ids_[k].begin());
        }
        bool parms_id(std::size_t k, std::uint64_t out[4]) const
        {
            std::lock_guard<std::mutex> lock(mu_);
            auto it = parms_ids_.find(k);
            if (it == parms_ids_.end())
                return false;
            std::copy(it->second.begin(), it->second.end(), out);
            return true;
        }

        // The deferred transparency check of the resident Evaluator overloads (SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT,
        // evaluator.cpp:265-271 and the other #ifdef blocks): a ring of flag words in a pool block per (Evaluator, calling
        // thread). Each checked operation gets its own slot as the lane's transparency sink; the sink writes a non-zero word
        // for a result that is NOT transparent. The slots are read at the thread's next host-visible point.
        static constexpr std::size_t kRingSlots = 256;
        // (count consecutive slots for an operation with that many results: the hoisted rotations)
        std::uint32_t *transparency_slot(const void *evaluator, std::size_t count = 1) const
        {
            if (count > kRingSlots)
                throw std::invalid_argument("too many results for one checked operation");
            Ring &r = ring(evaluator);
            if (r.used + count > kRingSlots)
                check_transparency(); // a full ring is a host-visible point
            std::uint32_t *slot = r.flags + r.used;
            r.used += count;
            return slot;
        }
        void transparency_unslot(const void *evaluator, std::size_t count = 1) const // the operation failed before its result existed
        {
            Ring &r = ring(evaluator);
            r.used -= count < r.used ? count : r.used;
        }
        // reads the calling thread's rings (one synchronisation each); throws the reference's std::logic_error when a
        // checked result was transparent
        void check_transparency() const
        {
            std::vector<std::pair<std::uint32_t *, std::size_t>> todo;
            {
                std::lock_guard<std::mutex> lock(mu_);
                for (auto &kv : rings_)
                    if (kv.first.second == std::this_thread::get_id() && kv.second.used)
                    {
                        todo.emplace_back(kv.second.flags, kv.second.used);
                        kv.second.used = 0;
                    }
            }
            bool transparent = false;
            for (auto &t : todo)
            {
                std::vector<std::uint32_t> host(t.second);
                throw_on(sealhip_memcpy_d2h(ctx_, host.data(), t.first, host.size() * sizeof(std::uint32_t)));
                transparent = transparent || std::find(host.begin(), host.end(), 0u) != host.end();
            }
            if (transparent)
                throw std::logic_error("result ciphertext is transparent");
        }
        // The Evaluator goes away: its rings go back to the pool. Every lane is waited for first (no stream still writes a
        // flag into them); flags not yet read are dropped unread -- a destructor does not throw, so call
        // Evaluator::synchronize() before destroying an Evaluator whose resident results must be checked.
        void drop_transparency(const void *evaluator) const
        {
            bool any = false;
            {
                std::lock_guard<std::mutex> lock(mu_);
                for (auto &kv : rings_)
                    any = any || kv.first.first == evaluator;
            }
            if (any)
                (void)sealhip_synchronize(ctx_);
            std::lock_guard<std::mutex> lock(mu_);
            for (auto it = rings_.begin(); it != rings_.end();)
                if (it->first.first == evaluator)
                {
                    sealhip_pool_release(ctx_, it->second.flags);
                    it = rings_.erase(it);
                }
                else
                    ++it;
        }

    private:
        struct Ring
        {
            std::uint32_t *flags = nullptr;
            std::size_t used = 0;
        };
        Ring &ring(const void *evaluator) const
        {
            std::lock_guard<std::mutex> lock(mu_);
            Ring &r = rings_[{ evaluator, std::this_thread::get_id() }];
            if (!r.flags)
            {
                void *p = nullptr;
                throw_on(sealhip_pool_alloc(ctx_, kRingSlots * sizeof(std::uint32_t), &p));
                r.flags = static_cast<std::uint32_t *>(p);
            }
            return r;
        }

        sealhip_context *ctx_ = nullptr;
        std::uint32_t scheme_;
        std::size_t n_;
        std::uint64_t t_;
        std::size_t n_key_;
        std::vector<std::uint64_t> key_moduli_;
        mutable std::mutex mu_;
        std::map<std::size_t, std::array<std::uint64_t, 4>> parms_ids_;
        mutable std::map<std::pair<const void *, std::thread::id>, Ring> rings_;
    };

    // The owner of one block of a context's pool: (context, device pointer, capacity in words). Staged, DeviceCiphertext and
    // DevicePlaintext hold one and keep only their metadata; every sealhip_pool_alloc / sealhip_pool_release of an object's
    // words is here. Movable by swap; a default-constructed one has no context and owns nothing.
    class PoolBlock
    {
    public:
        explicit PoolBlock(const Context *context = nullptr) : ctx_(context) {}
        PoolBlock(const PoolBlock &) = delete;
        PoolBlock &operator=(const PoolBlock &) = delete;
        ~PoolBlock() { release(); }
        const Context *context() const { return ctx_; }
        std::uint64_t *ptr() const { return ptr_; }
        std::size_t cap() const { return cap_; }
        // room for `words` words: the block is kept when it is large enough
        void reserve(std::size_t words)
        {
            if (words <= cap_ && ptr_)
                return;
            void *p = nullptr;
            throw_on(sealhip_pool_alloc(ctx_->get(), (words ? words : 1) * 8, &p));
            release();
            ptr_ = static_cast<std::uint64_t *>(p);
            cap_ = words;
        }
        void release() // stream-ordered
        {
            if (ptr_ && ctx_)
                sealhip_pool_release(ctx_->get(), ptr_);
            ptr_ = nullptr;
            cap_ = 0;
        }
        // `block` (a pool block of cap_words words) replaces this one, which is released
        void adopt(void *block, std::size_t cap_words)
        {
            release();
            ptr_ = static_cast<std::uint64_t *>(block);
            cap_ = cap_words;
        }
        // the block changes owner; cap() still tells its size
        void *detach()
        {
            void *p = ptr_;
            ptr_ = nullptr;
            return p;
        }
        // the leading `words` words of `o`, by a stream-ordered device copy; a block of another context goes back to the
        // pool it came from first
        void copy_from(const PoolBlock &o, std::size_t words)
        {
            if (ctx_ != o.ctx_)
            {
                release();
                ctx_ = o.ctx_;
            }
            reserve(words);
            if (words)
                throw_on(sealhip_memcpy_d2d(ctx_->get(), ptr_, o.ptr_, words * 8));
        }
        void swap(PoolBlock &o) noexcept
        {
            std::swap(ctx_, o.ctx_);
            std::swap(ptr_, o.ptr_);
            std::swap(cap_, o.cap_);
        }

    private:
        const Context *ctx_ = nullptr;
        std::uint64_t *ptr_ = nullptr;
        std::size_t cap_ = 0;
    };

    // device staging of one host object, in a block of the context's pool (sealhip_pool_alloc): released stream-ordered,
    // so the host path makes no allocator call once the pool is warm
    class Staged
    {
    public:
        Staged(const Context &c, std::size_t words) : block_(&c) { block_.reserve(words); }
        Staged(const Staged &) = delete;
        Staged &operator=(const Staged &) = delete;
        void up(const std::uint64_t *h, std::size_t words) { throw_on(sealhip_memcpy_h2d(ctx(), ptr(), h, words * 8)); }
        void down(std::uint64_t *h, std::size_t words) { throw_on(sealhip_memcpy_d2h(ctx(), h, ptr(), words * 8)); }
        std::uint64_t *ptr() { return block_.ptr(); }
        std::size_t words() const { return block_.cap(); }
        void *release() { return block_.detach(); } // the block changes owner (a DeviceCiphertext adopts it)

    private:
        sealhip_context *ctx() const { return block_.context()->get(); }
        PoolBlock block_;
    };

    // Staging that held secret samples (u, the noise, a secret key in coefficient form): erased in stream order before the
    // block goes back to the pool, as the reference's clear_on_destruction pool does (util/rlwe.cpp:141)
    class ZeroedStaged : public Staged
    {
    public:
        ZeroedStaged(const Context &c, std::size_t words) : Staged(c, words), ctx_(c) {}
        ~ZeroedStaged() { sealhip_memset_zero(ctx_.get(), ptr(), (words() ? words() : 1) * 8); }

    private:
        const Context &ctx_;
    };

    // Where the random samples come from when they are drawn on the device (sealhip_sample_polys): the
    // source is asked for one 64-byte seed at a time (a CSPRNG's output; never reuse one). Only seeds cross from the host.
    using SeedSource = std::function<void(std::uint64_t *seed8)>;

    namespace detail
    {
        // two seeds from the source, in order; the second (a noise seed, secret) must not be the first (c_1's, public)
        inline void draw_seed_pair(const SeedSource &source, std::uint64_t *public_seed, std::uint64_t *noise_seed)
        {
            source(public_seed);
            source(noise_seed);
            if (std::equal(public_seed, public_seed + 8, noise_seed))
                throw std::logic_error("the seed source returned the same seed twice");
        }

        // HostCiphertext needs its N before resize_raw; seal::Ciphertext gets it from its parms_id
        template <class C>
        auto prepare_host(C &c, std::size_t n) -> decltype(c.n_ = n, void())
        {
            c.n_ = n;
        }
        inline void prepare_host(...) {}
    } // namespace detail

    // A ciphertext resident on the device: size x k x N words in a block of the context's pool, with the
    // metadata of seal::Ciphertext the adapter uses (size, level k, N, NTT form, scale). Copies take a pool block and a
    // stream-ordered device copy; moves swap. Only download / save / load synchronise (the host-visible points).
    class DeviceCiphertext
    {
    public:
        explicit DeviceCiphertext(const Context &context) : block_(&context), n_(context.n()) {}
        DeviceCiphertext(const DeviceCiphertext &o) : block_(o.block_.context()), n_(o.n_) { *this = o; }
        DeviceCiphertext(DeviceCiphertext &&o) noexcept { swap(o); }
        DeviceCiphertext &operator=(const DeviceCiphertext &o)
        {
            if (this == &o)
                return *this;
            n_ = o.n_;
            block_.copy_from(o.block_, o.words());
            size_ = o.size_;
            k_ = o.k_;
            ntt_ = o.ntt_;
            scale_ = o.scale_;
            return *this;
        }
        DeviceCiphertext &operator=(DeviceCiphertext &&o) noexcept
        {
            swap(o); // o releases what this held
            return *this;
        }
        void swap(DeviceCiphertext &o) noexcept
        {
            block_.swap(o.block_);
            std::swap(size_, o.size_);
            std::swap(k_, o.k_);
            std::swap(n_, o.n_);
            std::swap(ntt_, o.ntt_);
            std::swap(scale_, o.scale_);
        }

        std::uint64_t *data() { return block_.ptr(); } // a DEVICE pointer
        const std::uint64_t *data() const { return block_.ptr(); }
        std::size_t size() const { return size_; }
        std::size_t coeff_modulus_size() const { return k_; }
        std::size_t poly_modulus_degree() const { return n_; }
        bool &is_ntt_form() { return ntt_; }
        bool is_ntt_form() const { return ntt_; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        const Context &context() const { return *ctx(); }

        // host ciphertext -> device (one synchronous copy)
        template <class H>
        void upload(const H &h)
        {
            if (h.poly_modulus_degree() != n_)
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            const std::size_t words = h.size() * h.coeff_modulus_size() * n_;
            block_.reserve(words);
            if (words)
                throw_on(sealhip_memcpy_h2d(ctx()->get(), block_.ptr(), h.data(), words * 8));
            size_ = h.size();
            k_ = h.coeff_modulus_size();
            ntt_ = h.is_ntt_form();
            scale_ = h.scale();
        }
        // device -> host ciphertext; a host-visible point of the calling thread's deferred transparency checks
        template <class H>
        void download(H &h) const
        {
            ctx()->check_transparency();
            detail::prepare_host(h, n_);
            h.resize_raw(size_, k_);
            if (words())
                throw_on(sealhip_memcpy_d2h(ctx()->get(), h.data(), block_.ptr(), words() * 8));
            h.is_ntt_form() = ntt_;
            h.scale() = scale_;
        }
        // Ciphertext::load (ciphertext.cpp:228-330) straight into the block (sealhip_ciphertext_load)
        void load(const void *bytes, std::size_t len)
        {
            sealhip_ciphertext_info info{};
            throw_on(sealhip_ciphertext_peek(bytes, len, &info));
            if (info.poly_modulus_degree != n_)
                throw std::logic_error("ciphertext data is invalid");
            block_.reserve(std::size_t(info.size) * info.coeff_modulus_size * n_);
            throw_on(sealhip_ciphertext_load(ctx()->get(), bytes, len, &info, block_.ptr(), block_.cap()));
            size_ = info.size;
            k_ = info.coeff_modulus_size;
            ntt_ = info.is_ntt_form != 0;
            scale_ = info.scale;
        }
        // Ciphertext::save (compr_mode_type::none) straight from the block (sealhip_ciphertext_save); the level's parms_id
        // comes from Context::set_parms_id. A host-visible point.
        void save(std::vector<std::uint8_t> &out) const
        {
            ctx()->check_transparency();
            sealhip_ciphertext_info info{};
            if (!ctx()->parms_id(k_, info.parms_id))
                throw std::logic_error("the level's parms_id is not registered (Context::set_parms_id)");
            info.is_ntt_form = ntt_ ? 1 : 0;
            info.size = std::uint32_t(size_);
            info.coeff_modulus_size = std::uint32_t(k_);
            info.poly_modulus_degree = n_;
            info.scale = scale_;
            std::size_t need = 0, written = 0;
            throw_on(sealhip_ciphertext_save_size(ctx()->get(), std::uint32_t(size_), std::uint32_t(k_), &need));
            out.resize(need);
            throw_on(sealhip_ciphertext_save(ctx()->get(), &info, block_.ptr(), out.data(), need, &written));
            out.resize(written);
        }
        // Ciphertext::resize (ciphertext.cpp:84-133): polynomials it adds are zero (sealhip_ciphertext_resize)
        void resize(std::size_t size)
        {
            if (size == size_)
                return;
            if ((size < 2 && size != 0) || size > 16)
                throw std::invalid_argument("invalid size");
            Staged next(*ctx(), size * k_ * n_);
            throw_on(sealhip_ciphertext_resize(ctx()->get(), std::uint32_t(k_), block_.ptr() ? block_.ptr() : next.ptr(), std::uint32_t(size_),
                                               next.ptr(), std::uint32_t(size), 1));
            adopt(next.release(), next.words(), size, k_);
        }

        // (Evaluator) the result in `block` (a pool block of cap_words words) replaces the words; the old block is
        // released stream-ordered
        void adopt(void *block, std::size_t cap_words, std::size_t size, std::size_t k)
        {
            block_.adopt(block, cap_words);
            size_ = size;
            k_ = k;
        }
        // (Evaluator, Encryptor) result i of the `count` results of `words` words each that lie back to back in `results`
        // becomes these words: `size` polynomials at level k. Every resident ciphertext owns a pool block of its own, so
        // the result is copied once more on the device (stream-ordered); a single result takes over the block itself.
        void adopt_result(Staged &results, std::size_t i, std::size_t count, std::size_t words, std::size_t size, std::size_t k)
        {
            if (count == 1)
            {
                const std::size_t cap = results.words();
                return adopt(results.release(), cap, size, k);
            }
            Staged one(*ctx(), words);
            throw_on(sealhip_memcpy_d2d(ctx()->get(), one.ptr(), results.ptr() + i * words, words * 8));
            adopt(one.release(), words, size, k);
        }
        void set_size(std::size_t size) { size_ = size; } // (Evaluator) fewer polynomials, the leading words kept
        void copy_meta(const DeviceCiphertext &o) // (Evaluator) NTT form and scale, not the words
        {
            ntt_ = o.ntt_;
            scale_ = o.scale_;
        }

    private:
        const Context *ctx() const { return block_.context(); }
        std::size_t words() const { return size_ * k_ * n_; }

        PoolBlock block_;
        std::size_t size_ = 0, k_ = 0, n_ = 0;
        bool ntt_ = false;
        double scale_ = 1.0;
    };

    // A plaintext resident on the device, in a pool block: coefficient form (N words, each below t; a shorter plaintext is
    // zero-padded) or NTT form at level k (k x N words). It serves the plain operations of the resident Evaluator overloads,
    // transform_to_ntt and mod_switch_to(_next) of plaintexts. upload checks the words like is_valid_for (coefficient form:
    // every word below t) and is the only call that synchronises.
    class DevicePlaintext
    {
    public:
        explicit DevicePlaintext(const Context &context) : block_(&context) {}
        DevicePlaintext(const DevicePlaintext &o) : block_(o.block_.context()) { *this = o; }
        DevicePlaintext(DevicePlaintext &&o) noexcept { swap(o); }
        DevicePlaintext &operator=(const DevicePlaintext &o)
        {
            if (this == &o)
                return *this;
            block_.copy_from(o.block_, o.words_);
            words_ = o.words_;
            k_ = o.k_;
            ntt_ = o.ntt_;
            scale_ = o.scale_;
            return *this;
        }
        DevicePlaintext &operator=(DevicePlaintext &&o) noexcept
        {
            swap(o);
            return *this;
        }
        void swap(DevicePlaintext &o) noexcept
        {
            block_.swap(o.block_);
            std::swap(words_, o.words_);
            std::swap(k_, o.k_);
            std::swap(ntt_, o.ntt_);
            std::swap(scale_, o.scale_);
        }
        // coefficient form: up to N coefficients below t; NTT form: k x N words (k = words.size() / N)
        void upload(const std::vector<std::uint64_t> &words, bool ntt_form)
        {
            const Context &ctx = *block_.context();
            const std::size_t n = ctx.n();
            std::vector<std::uint64_t> padded;
            const std::uint64_t *src = words.data();
            std::size_t count = words.size(), k = 0;
            if (ntt_form)
            {
                k = count / n;
                if (count % n != 0 || k < 1 || k > ctx.n_key())
                    throw std::invalid_argument("plain is not valid for encryption parameters");
            }
            else
            {
                if (count > n || std::any_of(words.begin(), words.end(),
                                             [&](std::uint64_t v) { return v >= ctx.plain_modulus(); }))
                    throw std::invalid_argument("plain is not valid for encryption parameters"); // valcheck.cpp:236-281
                padded.assign(n, 0);
                std::copy(words.begin(), words.end(), padded.begin());
                src = padded.data();
                count = n;
            }
            block_.reserve(count);
            throw_on(sealhip_memcpy_h2d(ctx.get(), block_.ptr(), src, count * 8));
            words_ = count;
            k_ = k;
            ntt_ = ntt_form;
        }
        void download(std::vector<std::uint64_t> &out) const
        {
            out.resize(words_);
            if (words_)
                throw_on(sealhip_memcpy_d2h(block_.context()->get(), out.data(), block_.ptr(), words_ * 8));
        }
        const std::uint64_t *data() const { return block_.ptr(); } // a DEVICE pointer
        std::size_t words() const { return words_; }
        std::size_t coeff_modulus_size() const { return k_; } // NTT form: its level; coefficient form: 0
        bool is_ntt_form() const { return ntt_; }
        // Plaintext::scale() of a CKKS plaintext (the caller sets it next to upload; 1.0 otherwise): read by
        // Evaluator::apply_galois_dot_plain, kept by copies
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        // (Evaluator) the words in `block` replace these
        void adopt(void *block, std::size_t cap_words, std::size_t words, std::size_t k, bool ntt_form)
        {
            block_.adopt(block, cap_words);
            words_ = words;
            k_ = k;
            ntt_ = ntt_form;
        }

    private:
        PoolBlock block_;
        std::size_t words_ = 0, k_ = 0;
        bool ntt_ = false;
        double scale_ = 1.0;
    };

    class KSwitchKeys // one key of RelinKeys / GaloisKeys (kswitchkeys.h:92-130), resident on the device
    {
    public:
        KSwitchKeys(const Context &c, const std::uint64_t *host_key, std::uint32_t n_digits) : c_(c)
        {
            throw_on(sealhip_kswitch_key_load(c.get(), host_key, n_digits, 1, &key_));
        }
        ~KSwitchKeys()
        {
            if (key_)
                sealhip_kswitch_key_destroy(c_.get(), key_);
        }
        KSwitchKeys(const Context &c, sealhip_kswitch_key *adopt) : c_(c), key_(adopt) {} // a handle the ABI made
        KSwitchKeys(const KSwitchKeys &) = delete;
        const sealhip_kswitch_key *get() const { return key_; }

    private:
        const Context &c_;
        sealhip_kswitch_key *key_ = nullptr;
    };

    // One RGSW ciphertext, resident on the device: the key-switch keys K_b (new key m) and K_a (new
    // key m s) of a small polynomial m in one block. Made by KeyGenerator::rgsw, or from two key-switch keys (for example
    // loaded from a stream; a device copy -- digit counts or levels that differ -> std::invalid_argument).
    // Evaluator::external_product / cmux / select take it.
    class RgswCiphertext
    {
    public:
        RgswCiphertext(const Context &c, const KSwitchKeys &key_b, const KSwitchKeys &key_a) : c_(c)
        {
            throw_on(sealhip_rgsw_create(c.get(), key_b.get(), key_a.get(), &g_));
        }
        RgswCiphertext(const Context &c, sealhip_rgsw *adopt) : c_(c), g_(adopt) {} // a handle the ABI made
        ~RgswCiphertext()
        {
            if (g_)
                sealhip_rgsw_destroy(c_.get(), g_);
        }
        RgswCiphertext(const RgswCiphertext &) = delete;
        RgswCiphertext &operator=(const RgswCiphertext &) = delete;
        const sealhip_rgsw *get() const { return g_; }
        // (K_b, K_a) as two owned key-switch keys holding copies of the halves (sealhip_rgsw_export)
        std::pair<std::unique_ptr<KSwitchKeys>, std::unique_ptr<KSwitchKeys>> export_keys() const
        {
            sealhip_kswitch_key *raw[2] = { nullptr, nullptr };
            throw_on(sealhip_rgsw_export(c_.get(), g_, raw));
            return { std::make_unique<KSwitchKeys>(c_, raw[0]), std::make_unique<KSwitchKeys>(c_, raw[1]) };
        }

    private:
        const Context &c_;
        sealhip_rgsw *g_ = nullptr;
    };

    // The keys of a blind rotation, resident on the device: the RGSW encryptions of the indicators
    // [s_j = 1] (and, for a ternary secret, [s_j = -1] behind each) of an LWE secret, in step order. Made by
    // KeyGenerator::blind_rotation_keys; Evaluator::blind_rotate takes them.
    class BlindRotationKeys
    {
    public:
        BlindRotationKeys(std::vector<std::unique_ptr<RgswCiphertext>> keys, bool ternary) : keys_(std::move(keys)), ternary_(ternary)
        {
            for (const auto &g : keys_)
                raw_.push_back(g->get());
        }
        std::size_t n_steps() const { return keys_.size(); }
        bool ternary() const { return ternary_; }
        const sealhip_rgsw *const *get() const { return raw_.empty() ? nullptr : raw_.data(); }

    private:
        std::vector<std::unique_ptr<RgswCiphertext>> keys_;
        std::vector<const sealhip_rgsw *> raw_;
        bool ternary_;
    };

    // The test vector of a lookup table for Evaluator::blind_rotate: the plaintext coefficients tv[j] = f(floor(j t / 2N)),
    // j < N. Messages are restricted to [0, t/2); with b_offset = N / t in sealhip_lwe_mod_switch the windows are centred
    // and the constant coefficient of the rotation's result is f(m).
    inline std::vector<std::uint64_t> lut_test_vector(const std::function<std::uint64_t(std::uint64_t)> &f, std::uint64_t t,
                                                      std::size_t n)
    {
        std::vector<std::uint64_t> tv(n);
        for (std::size_t j = 0; j < n; j++)
            tv[j] = f((j * t) / (2 * n));
        return tv;
    }

    // What HomomorphicDFT and Bootstrapper share: the tables' handle (destroyed with the object, not copyable), the plan and
    // its key steps. plan_entry(plan, key_steps, capacity) is the ABI's plan entry over the owner's arguments, called
    // twice (the plan says how many steps there are); create(tables) its create entry. The plan comes first: its
    // refusals need no device.
    template <class Tables, class Plan, long (*Destroy)(Tables *)>
    class PlannedTables
    {
    public:
        ~PlannedTables()
        {
            if (tables_)
                Destroy(tables_);
        }
        PlannedTables(const PlannedTables &) = delete;
        PlannedTables &operator=(const PlannedTables &) = delete;
        const Tables *get() const { return tables_; }
        const Plan &plan() const { return plan_; }
        std::size_t out_level() const { return plan_.out_level; }
        const std::vector<std::uint32_t> &key_steps() const { return key_steps_; }

    protected:
        PlannedTables() = default;
        template <class PlanEntry, class Create>
        void make(PlanEntry plan_entry, Create create)
        {
            throw_on(plan_entry(&plan_, nullptr, 0));
            key_steps_.resize(plan_.n_key_steps);
            throw_on(plan_entry(&plan_, key_steps_.data(), plan_.n_key_steps));
            throw_on(create(&tables_));
        }
        Tables *tables_ = nullptr;
        Plan plan_{};
        std::vector<std::uint32_t> key_steps_;
    };

    // The plan and the device tables of one homomorphic DFT (sealhip_dft_tables_create): CoeffToSlot
    // (SEALHIP_DFT_COEFFS_TO_SLOTS) or SlotToCoeff (SEALHIP_DFT_SLOTS_TO_COEFFS) for ciphertexts at level k, as the stages
    // `stages` (layer counts in application order, summing to log2(N/2)). Evaluator::coeffs_to_slots / slots_to_coeffs take
    // it; the result is n_stages levels lower at the same scale. key_steps(): the rotation steps whose Galois keys the
    // client must make (CoeffToSlot also needs the key of element 2N - 1).
    class HomomorphicDFT : public PlannedTables<sealhip_dft_tables, sealhip_dft_plan, sealhip_dft_tables_destroy>
    {
    public:
        HomomorphicDFT(const Context &c, std::uint32_t direction, std::size_t k, const std::vector<std::uint32_t> &stages,
                       const std::vector<std::uint32_t> &n_baby = {}, double gain = 1.0)
        {
            if (!n_baby.empty() && n_baby.size() != stages.size())
                throw std::invalid_argument("n_baby and stages differ in length");
            const std::uint32_t *nb = n_baby.empty() ? nullptr : n_baby.data();
            const std::uint32_t n_stages = std::uint32_t(stages.size());
            const auto plan_entry = [&](sealhip_dft_plan *p, std::uint32_t *steps, std::uint32_t capacity) {
                return sealhip_evaluator_dft_plan(c.get(), direction, std::uint32_t(k), stages.data(), n_stages, nb, p, steps, capacity);
            };
            make(plan_entry, [&](sealhip_dft_tables **t) {
                return sealhip_dft_tables_create(c.get(), direction, std::uint32_t(k), stages.data(), n_stages, nb, gain, t);
            });
        }
        std::uint32_t direction() const { return plan_.direction; }
        std::size_t in_level() const { return plan_.in_level; }
    };

    // The plan and the device tables of one bootstrap shape (sealhip_bootstrap_tables_create):
    // ModRaise to level k_top, CoeffToSlot as `c2s_stages`, EvalMod (K, r, degree, n_baby), SlotToCoeff as `s2c_stages`.
    // K bounds ModRaise's integer polynomial, K >= max|I| + 1: it grows with the secret's Hamming weight, and the library
    // does not sample sparse secrets. Evaluator::bootstrap takes it; the result is at out_level() with the operand's scale,
    // its precision bounded by |m| / q_0 (the sine step's relative error is (2 pi m / q_0)^2 / 6). key_steps(): the rotation
    // steps whose Galois keys the client must make, next to the key of element 2N - 1.
    class Bootstrapper : public PlannedTables<sealhip_bootstrap_tables, sealhip_bootstrap_plan, sealhip_bootstrap_tables_destroy>
    {
    public:
        Bootstrapper(const Context &c, std::size_t k_top, const std::vector<std::uint32_t> &c2s_stages,
                     const std::vector<std::uint32_t> &s2c_stages, std::uint32_t K, std::uint32_t r, std::uint32_t degree,
                     std::uint32_t n_baby = 0)
        {
            const std::uint32_t n1 = std::uint32_t(c2s_stages.size()), n2 = std::uint32_t(s2c_stages.size());
            const auto plan_entry = [&](sealhip_bootstrap_plan *p, std::uint32_t *steps, std::uint32_t capacity) {
                return sealhip_evaluator_bootstrap_plan(c.get(), std::uint32_t(k_top), c2s_stages.data(), n1, nullptr,
                                                        s2c_stages.data(), n2, nullptr, K, r, degree, n_baby, p, steps, capacity);
            };
            make(plan_entry, [&](sealhip_bootstrap_tables **t) {
                return sealhip_bootstrap_tables_create(c.get(), std::uint32_t(k_top), c2s_stages.data(), n1, nullptr,
                                                       s2c_stages.data(), n2, nullptr, K, r, degree, n_baby, t);
            });
        }
    };

    // The device tables of one d x d complex matrix (sealhip_linear_transform_create): the diagonals
    // that hold a non-zero entry, found, pre-rotated and encoded at the key level on the device, at `scale`. The matrix is
    // row-major, d a power of two <= N/2; it is read from device memory (16-byte aligned: a torch tensor's data_ptr()), or
    // from a host vector that is staged through the pool for the making. Evaluator::linear_transform takes the object at
    // any level; for a ciphertext whose slots are z the result's slots are
    //     out[p] = sum_c u_c[p] z[(p + c) mod n],  u_c[p] = M[p mod d][(p + c) mod d]
    // -- M z, tiled, when z is a d-vector tiled N/2d times. n1: the baby stride (0: the default); key_steps(): the rotation
    // steps whose Galois keys the client must make.
    class LinearTransform
    {
    public:
        LinearTransform(const Context &c, const double *matrix_dev, std::size_t d, double scale, std::uint32_t n1 = 0,
                        double gain = 1.0)
        {
            make(c, matrix_dev, d, scale, n1, gain);
        }
        LinearTransform(const Context &c, const std::vector<std::complex<double>> &matrix, std::size_t d, double scale,
                        std::uint32_t n1 = 0, double gain = 1.0)
        {
            if (matrix.size() != d * d)
                throw std::invalid_argument("matrix must hold d x d entries");
            sealhip_lintrans_plan dense; // (d and n1 are refused before the staging needs a device)
            throw_on(sealhip_linear_transform_plan(c.get(), std::uint32_t(d), nullptr, n1, &dense, nullptr, nullptr, nullptr, 0));
            Staged m(c, 2 * d * d);
            m.up(reinterpret_cast<const std::uint64_t *>(matrix.data()), 2 * d * d);
            make(c, reinterpret_cast<const double *>(m.ptr()), d, scale, n1, gain);
        }
        ~LinearTransform()
        {
            if (tables_)
                sealhip_linear_transform_destroy(tables_);
        }
        LinearTransform(const LinearTransform &) = delete;
        LinearTransform &operator=(const LinearTransform &) = delete;
        const sealhip_linear_transform *get() const { return tables_; }
        const sealhip_lintrans_plan &plan() const { return plan_; }
        double scale() const { return scale_; }
        const std::vector<int> &baby_steps() const { return baby_; }
        const std::vector<int> &giant_steps() const { return giant_; }
        const std::vector<std::uint32_t> &key_steps() const { return key_steps_; }
        const std::uint64_t *plain_ntt() const // device: n_giant x n_baby x n_key x N words
        {
            const std::uint64_t *p = nullptr;
            throw_on(sealhip_linear_transform_tables_plain(tables_, &p));
            return p;
        }

    private:
        void make(const Context &c, const double *matrix_dev, std::size_t d, double scale, std::uint32_t n1, double gain)
        {
            throw_on(sealhip_linear_transform_create(c.get(), matrix_dev, std::uint32_t(d), n1, scale, gain, &tables_));
            throw_on(sealhip_linear_transform_tables_plan(tables_, &plan_, &scale_));
            std::vector<std::int32_t> b(plan_.n_baby), g(plan_.n_giant);
            throw_on(sealhip_linear_transform_tables_steps(tables_, b.data(), g.data()));
            baby_.assign(b.begin(), b.end());
            giant_.assign(g.begin(), g.end());
            for (int s : baby_)
                if (s)
                    key_steps_.push_back(std::uint32_t(s));
            for (int s : giant_)
                if (s)
                    key_steps_.push_back(std::uint32_t(s));
            std::sort(key_steps_.begin(), key_steps_.end());
            key_steps_.erase(std::unique(key_steps_.begin(), key_steps_.end()), key_steps_.end());
        }
        sealhip_linear_transform *tables_ = nullptr;
        sealhip_lintrans_plan plan_{};
        double scale_ = 0;
        std::vector<int> baby_, giant_;
        std::vector<std::uint32_t> key_steps_;
    };

    // LWE samples of coefficients of one resident ciphertext (Evaluator::extract_lwe / pack_lwes): a is
    // n x k x N words and b is n x k words, in two blocks of the context's pool, with the level and the scale of the
    // ciphertext they came from. Move-only.
    class LweSamples
    {
    public:
        explicit LweSamples(const Context &context) : ctx_(&context) {}
        LweSamples(LweSamples &&) = default;
        LweSamples &operator=(LweSamples &&) = default;
        std::size_t size() const { return n_; } // samples
        std::size_t coeff_modulus_size() const { return k_; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        const std::uint64_t *a() const { return a_ ? a_->ptr() : nullptr; } // DEVICE pointers
        const std::uint64_t *b() const { return b_ ? b_->ptr() : nullptr; }
        // (Evaluator) fresh blocks for n samples at level k
        void reset(std::size_t n, std::size_t k)
        {
            a_.reset(new Staged(*ctx_, n * k * ctx_->n()));
            b_.reset(new Staged(*ctx_, n * k));
            n_ = n;
            k_ = k;
        }
        std::uint64_t *a_out() { return a_->ptr(); }
        std::uint64_t *b_out() { return b_->ptr(); }

    private:
        const Context *ctx_;
        std::unique_ptr<Staged> a_, b_;
        std::size_t n_ = 0, k_ = 0;
        double scale_ = 1.0;
    };
} // namespace sealhip_host
