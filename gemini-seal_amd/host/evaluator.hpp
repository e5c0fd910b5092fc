// evaluator.hpp -- C++ host adapter with seal::Evaluator's method names over the sealhip C ABI.
//
// seal::Evaluator is non-virtual and non-copyable (native/src/seal/evaluator.h:1316-1322), so this is not a
// subclass: it is a class with the same method names and argument meaning for the hot-path operations
// (evaluator.h:246-298 multiply/square, :344-371 relinearize, :396-430 mod_switch_to_next, :479-502 mod_switch_to, :565-583
// rescale_to_next, :606-629 rescale_to, :183 add_many, :902-947 transform_to/from_ntt, :984-1021 apply_galois, :1057-1103
// rotate_rows, :1131-1173 rotate_columns, :1201-1239 rotate_vector, :1269-1308 complex_conjugate, :859-900 transform_to_ntt
// and :430-548 mod_switch_to(_next) of plaintexts, and every destination-taking variant), doing
// the same metadata checks on the host and forwarding raw pointers to the ABI. It is a template over the
// ciphertext type so that it compiles both against seal::Ciphertext (where the reference headers exist) and
// against the plain sealhip::HostCiphertext below (everywhere else, e.g. the GPU box).
//
// Required of CT: data() -> uint64_t*, size(), coeff_modulus_size(), poly_modulus_degree(), is_ntt_form()
// (assignable), resize_raw(size, coeff_modulus_size). For seal::Ciphertext the last one is
//   ct.resize(context, parms_id_of_level, size)  -- see INTEGRATION.md.
//
// Exceptions mirror the reference: std::invalid_argument / std::logic_error (evaluator.cpp:238-271).
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

    // device staging of one host object, in a block of the context's pool (sealhip_pool_alloc): released stream-ordered,
    // so the host path makes no allocator call once the pool is warm
    class Staged
    {
    public:
        Staged(const Context &c, std::size_t words) : c_(c), words_(words)
        {
            throw_on(sealhip_pool_alloc(c.get(), (words ? words : 1) * 8, &d_));
        }
        ~Staged()
        {
            if (d_)
                sealhip_pool_release(c_.get(), d_);
        }
        Staged(const Staged &) = delete;
        Staged &operator=(const Staged &) = delete;
        void up(const std::uint64_t *h, std::size_t words) { throw_on(sealhip_memcpy_h2d(c_.get(), d_, h, words * 8)); }
        void down(std::uint64_t *h, std::size_t words) { throw_on(sealhip_memcpy_d2h(c_.get(), h, d_, words * 8)); }
        std::uint64_t *ptr() { return static_cast<std::uint64_t *>(d_); }
        std::size_t words() const { return words_; }
        void *release() // the block changes owner (a DeviceCiphertext adopts it)
        {
            void *p = d_;
            d_ = nullptr;
            return p;
        }

    private:
        const Context &c_;
        void *d_ = nullptr;
        std::size_t words_;
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
        explicit DeviceCiphertext(const Context &context) : ctx_(&context), n_(context.n()) {}
        DeviceCiphertext(const DeviceCiphertext &o) : ctx_(o.ctx_), n_(o.n_) { *this = o; }
        DeviceCiphertext(DeviceCiphertext &&o) noexcept { swap(o); }
        ~DeviceCiphertext() { release(); }
        DeviceCiphertext &operator=(const DeviceCiphertext &o)
        {
            if (this == &o)
                return *this;
            if (ctx_ != o.ctx_)
            {
                release(); // (to the pool it came from)
                ctx_ = o.ctx_;
            }
            n_ = o.n_;
            reserve(o.words());
            if (o.words())
                throw_on(sealhip_memcpy_d2d(ctx_->get(), ptr_, o.ptr_, o.words() * 8));
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
            std::swap(ctx_, o.ctx_);
            std::swap(ptr_, o.ptr_);
            std::swap(cap_, o.cap_);
            std::swap(size_, o.size_);
            std::swap(k_, o.k_);
            std::swap(n_, o.n_);
            std::swap(ntt_, o.ntt_);
            std::swap(scale_, o.scale_);
        }

        std::uint64_t *data() { return ptr_; } // a DEVICE pointer
        const std::uint64_t *data() const { return ptr_; }
        std::size_t size() const { return size_; }
        std::size_t coeff_modulus_size() const { return k_; }
        std::size_t poly_modulus_degree() const { return n_; }
        bool &is_ntt_form() { return ntt_; }
        bool is_ntt_form() const { return ntt_; }
        double &scale() { return scale_; }
        double scale() const { return scale_; }
        const Context &context() const { return *ctx_; }

        // host ciphertext -> device (one synchronous copy)
        template <class H>
        void upload(const H &h)
        {
            if (h.poly_modulus_degree() != n_)
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            const std::size_t words = h.size() * h.coeff_modulus_size() * n_;
            reserve(words);
            if (words)
                throw_on(sealhip_memcpy_h2d(ctx_->get(), ptr_, h.data(), words * 8));
            size_ = h.size();
            k_ = h.coeff_modulus_size();
            ntt_ = h.is_ntt_form();
            scale_ = h.scale();
        }
        // device -> host ciphertext; a host-visible point of the calling thread's deferred transparency checks
        template <class H>
        void download(H &h) const
        {
            ctx_->check_transparency();
            detail::prepare_host(h, n_);
            h.resize_raw(size_, k_);
            if (words())
                throw_on(sealhip_memcpy_d2h(ctx_->get(), h.data(), ptr_, words() * 8));
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
            reserve(std::size_t(info.size) * info.coeff_modulus_size * n_);
            throw_on(sealhip_ciphertext_load(ctx_->get(), bytes, len, &info, ptr_, cap_));
            size_ = info.size;
            k_ = info.coeff_modulus_size;
            ntt_ = info.is_ntt_form != 0;
            scale_ = info.scale;
        }
        // Ciphertext::save (compr_mode_type::none) straight from the block (sealhip_ciphertext_save); the level's parms_id
        // comes from Context::set_parms_id. A host-visible point.
        void save(std::vector<std::uint8_t> &out) const
        {
            ctx_->check_transparency();
            sealhip_ciphertext_info info{};
            if (!ctx_->parms_id(k_, info.parms_id))
                throw std::logic_error("the level's parms_id is not registered (Context::set_parms_id)");
            info.is_ntt_form = ntt_ ? 1 : 0;
            info.size = std::uint32_t(size_);
            info.coeff_modulus_size = std::uint32_t(k_);
            info.poly_modulus_degree = n_;
            info.scale = scale_;
            std::size_t need = 0, written = 0;
            throw_on(sealhip_ciphertext_save_size(ctx_->get(), std::uint32_t(size_), std::uint32_t(k_), &need));
            out.resize(need);
            throw_on(sealhip_ciphertext_save(ctx_->get(), &info, ptr_, out.data(), need, &written));
            out.resize(written);
        }
        // Ciphertext::resize (ciphertext.cpp:84-133): polynomials it adds are zero (sealhip_ciphertext_resize)
        void resize(std::size_t size)
        {
            if (size == size_)
                return;
            if ((size < 2 && size != 0) || size > 16)
                throw std::invalid_argument("invalid size");
            Staged next(*ctx_, size * k_ * n_);
            throw_on(sealhip_ciphertext_resize(ctx_->get(), std::uint32_t(k_), ptr_ ? ptr_ : next.ptr(), std::uint32_t(size_),
                                               next.ptr(), std::uint32_t(size), 1));
            adopt(next.release(), next.words(), size, k_);
        }

        // (Evaluator) the result in `block` (a pool block of cap_words words) replaces the words; the old block is
        // released stream-ordered
        void adopt(void *block, std::size_t cap_words, std::size_t size, std::size_t k)
        {
            release();
            ptr_ = static_cast<std::uint64_t *>(block);
            cap_ = cap_words;
            size_ = size;
            k_ = k;
        }
        void set_size(std::size_t size) { size_ = size; } // (Evaluator) fewer polynomials, the leading words kept
        void copy_meta(const DeviceCiphertext &o) // (Evaluator) NTT form and scale, not the words
        {
            ntt_ = o.ntt_;
            scale_ = o.scale_;
        }

    private:
        std::size_t words() const { return size_ * k_ * n_; }
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
        void release()
        {
            if (ptr_ && ctx_)
                sealhip_pool_release(ctx_->get(), ptr_);
            ptr_ = nullptr;
            cap_ = 0;
        }

        const Context *ctx_ = nullptr;
        std::uint64_t *ptr_ = nullptr;
        std::size_t cap_ = 0, size_ = 0, k_ = 0, n_ = 0;
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
        explicit DevicePlaintext(const Context &context) : ctx_(&context) {}
        DevicePlaintext(const DevicePlaintext &o) : ctx_(o.ctx_) { *this = o; }
        DevicePlaintext(DevicePlaintext &&o) noexcept { swap(o); }
        ~DevicePlaintext() { release(); }
        DevicePlaintext &operator=(const DevicePlaintext &o)
        {
            if (this == &o)
                return *this;
            if (ctx_ != o.ctx_)
            {
                release();
                ctx_ = o.ctx_;
            }
            reserve(o.words_);
            if (o.words_)
                throw_on(sealhip_memcpy_d2d(ctx_->get(), ptr_, o.ptr_, o.words_ * 8));
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
            std::swap(ctx_, o.ctx_);
            std::swap(ptr_, o.ptr_);
            std::swap(cap_, o.cap_);
            std::swap(words_, o.words_);
            std::swap(k_, o.k_);
            std::swap(ntt_, o.ntt_);
            std::swap(scale_, o.scale_);
        }
        // coefficient form: up to N coefficients below t; NTT form: k x N words (k = words.size() / N)
        void upload(const std::vector<std::uint64_t> &words, bool ntt_form)
        {
            const std::size_t n = ctx_->n();
            std::vector<std::uint64_t> padded;
            const std::uint64_t *src = words.data();
            std::size_t count = words.size(), k = 0;
            if (ntt_form)
            {
                k = count / n;
                if (count % n != 0 || k < 1 || k > ctx_->n_key())
                    throw std::invalid_argument("plain is not valid for encryption parameters");
            }
            else
            {
                if (count > n || std::any_of(words.begin(), words.end(),
                                             [&](std::uint64_t v) { return v >= ctx_->plain_modulus(); }))
                    throw std::invalid_argument("plain is not valid for encryption parameters"); // valcheck.cpp:236-281
                padded.assign(n, 0);
                std::copy(words.begin(), words.end(), padded.begin());
                src = padded.data();
                count = n;
            }
            reserve(count);
            throw_on(sealhip_memcpy_h2d(ctx_->get(), ptr_, src, count * 8));
            words_ = count;
            k_ = k;
            ntt_ = ntt_form;
        }
        void download(std::vector<std::uint64_t> &out) const
        {
            out.resize(words_);
            if (words_)
                throw_on(sealhip_memcpy_d2h(ctx_->get(), out.data(), ptr_, words_ * 8));
        }
        const std::uint64_t *data() const { return ptr_; } // a DEVICE pointer
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
            release();
            ptr_ = static_cast<std::uint64_t *>(block);
            cap_ = cap_words;
            words_ = words;
            k_ = k;
            ntt_ = ntt_form;
        }

    private:
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
        void release()
        {
            if (ptr_ && ctx_)
                sealhip_pool_release(ctx_->get(), ptr_);
            ptr_ = nullptr;
            cap_ = 0;
        }

        const Context *ctx_ = nullptr;
        std::uint64_t *ptr_ = nullptr;
        std::size_t cap_ = 0, words_ = 0, k_ = 0;
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

    template <class CT>
    class Evaluator
    {
    public:
        explicit Evaluator(const Context &context) : ctx_(context) {}
        ~Evaluator() { ctx_.drop_transparency(this); }

        // Every method on CT has an overload on DeviceCiphertext (the same template): the same host checks and messages,
        // the same ABI entries, but the operands are used in place in their pool blocks. Once the pool is warm a resident
        // call makes no hipMalloc / hipFree, no host<->device copy and no synchronisation; a result that grows or moves to
        // another level gets a pool block and the old one is released stream-ordered. Resident results are also checked
        // for transparency as under SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT (after exactly the operations the reference
        // checks), but LATE: the std::logic_error("result ciphertext is transparent") arrives at the calling thread's next
        // host-visible point -- DeviceCiphertext::download / save, Evaluator::synchronize(), or a full ring of flags. The
        // host overloads do not check (as before). Plaintext operands are host words, staged through the pool per call.
        template <class C>
        using IfCt = typename std::enable_if<std::is_same<C, CT>::value || std::is_same<C, DeviceCiphertext>::value, int>::type;
        // a plaintext operand: host words (staged through the pool per call) or a DevicePlaintext (used in place)
        template <class P>
        using IfPlain = typename std::enable_if<std::is_convertible<P, const std::uint64_t *>::value ||
                                                    std::is_same<P, DevicePlaintext>::value,
                                                int>::type;

        // waits for this thread's work on the context; a host-visible point of the deferred transparency check
        void synchronize()
        {
            throw_on(sealhip_synchronize(ctx_.get()));
            ctx_.check_transparency();
        }

        // Evaluator::multiply_inplace (evaluator.cpp:235-272)
        template <class C, IfCt<C> = 0>
        void multiply_inplace(C &encrypted1, const C &encrypted2)
        {
            check_multiply(encrypted1, encrypted2);
            const std::size_t k = encrypted1.coeff_modulus_size(), n = ctx_.n();
            const std::size_t s1 = encrypted1.size(), s2 = encrypted2.size(), dest = s1 + s2 - 1;
            Dev a = dev_in(encrypted1, s1 * k * n), b = dev_in(encrypted2, s2 * k * n), o = dev_out(dest * k * n);
            Check chk = checked(encrypted1);
            throw_on(sealhip_evaluator_multiply(ctx_.get(), std::uint32_t(k), a.ptr(), std::uint32_t(s1), b.ptr(),
                                                std::uint32_t(s2), 1, o.ptr()));
            chk.done();
            commit(encrypted1, o, dest, k); // :324 / :484
        }

        // Evaluator::square_inplace (evaluator.cpp:529-558) on its own entry (bfv_square / ckks_square, :560-770): the same
        // canonical residues as multiply_inplace(encrypted, encrypted)
        template <class C, IfCt<C> = 0>
        void square_inplace(C &encrypted)
        {
            check_multiply(encrypted, encrypted);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), s = encrypted.size(), dest = 2 * s - 1;
            Dev a = dev_in(encrypted, s * k * n), o = dev_out(dest * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_square(ctx_.get(), std::uint32_t(k), a.ptr(), std::uint32_t(s), 1, o.ptr()));
            chk.done();
            commit(encrypted, o, dest, k);
        }

        // Evaluator::relinearize_inplace (evaluator.cpp:772-827); relin_keys[i] = key of get_index(i + 2)
        template <class C, IfCt<C> = 0>
        void relinearize_inplace(C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            if (size < 2)
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            if (relin_keys.size() + 2 < size)
                throw std::invalid_argument("not enough relinearization keys"); // :793-796
            if (size == 2)
                return;
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto *rk : relin_keys)
                raw.push_back(rk ? rk->get() : nullptr);
            Dev c = dev_in(encrypted, size * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_relinearize(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1,
                                                   raw.data(), std::uint32_t(raw.size())));
            chk.done();
            dev_back(encrypted, c, size * k * n);
            shrink(encrypted, 2); // :819
        }

        // Evaluator::mod_switch_to_next_inplace (evaluator.cpp:996-1036)
        template <class C, IfCt<C> = 0>
        void mod_switch_to_next_inplace(C &encrypted) { switch_level(encrypted, false); }
        // Evaluator::rescale_to_next_inplace (evaluator.cpp:1090-1126); the caller updates scale() /= q_last (:889-890)
        template <class C, IfCt<C> = 0>
        void rescale_to_next_inplace(C &encrypted) { switch_level(encrypted, true); }

        template <class C, IfCt<C> = 0>
        void transform_to_ntt_inplace(C &encrypted)
        {
            if (encrypted.is_ntt_form())
                throw std::invalid_argument("encrypted is already in NTT form"); // :1759-1762
            transform(encrypted, true);
            encrypted.is_ntt_form() = true;
        }
        template <class C, IfCt<C> = 0>
        void transform_from_ntt_inplace(C &encrypted_ntt)
        {
            if (!encrypted_ntt.is_ntt_form())
                throw std::invalid_argument("encrypted_ntt is not in NTT form"); // :1807-1810
            transform(encrypted_ntt, false);
            encrypted_ntt.is_ntt_form() = false;
        }

        // Evaluator::apply_galois_inplace (evaluator.cpp:1841-1943)
        template <class C, IfCt<C> = 0>
        void apply_galois_inplace(C &encrypted, std::uint32_t galois_elt, const KSwitchKeys &galois_key)
        {
            if (encrypted.size() > 2)
                throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n();
            Dev c = dev_in(encrypted, 2 * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_apply_galois(ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elt,
                                                    galois_key.get()));
            chk.done();
            dev_back(encrypted, c, 2 * k * n);
        }

        // Evaluator::rotate_vector_inplace (evaluator.h:1201-1211): CKKS only, then rotate_internal
        template <class C, IfCt<C> = 0>
        void rotate_vector_inplace(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // :1205-1208
            rotate_vector_like(encrypted, steps, galois_keys);
        }
        // rotate_internal (evaluator.cpp:1945-2000): one automorphism when its key is present, else the NAF of the step count
        template <class C, IfCt<C> = 0>
        void rotate_vector_like(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (steps == 0)
                return;
            std::uint32_t elt = 0;
            throw_on(sealhip_galois_elt_from_step(ctx_.get(), steps, &elt));
            auto it = galois_keys.find(elt);
            if (it != galois_keys.end())
                return apply_galois_inplace(encrypted, elt, *it->second);
            std::vector<int> naf; // util/numth.h:22-42
            bool neg = steps < 0;
            int v = neg ? -steps : steps;
            for (int i = 0; v; i++)
            {
                int zi = (v % 2) ? 2 - (v % 4) : 0;
                v = (v - zi) / 2;
                if (zi)
                    naf.push_back((neg ? -zi : zi) * (1 << i));
            }
            if (naf.size() == 1)
                throw std::invalid_argument("Galois key not present"); // :1985-1988
            for (int s : naf)
                if (std::size_t(s < 0 ? -s : s) != (ctx_.n() >> 1))
                    rotate_vector_like(encrypted, s, galois_keys);
        }

        // Evaluator::rotate_rows_inplace (evaluator.h:1057-1067): BFV only, then rotate_internal like rotate_vector
        template <class C, IfCt<C> = 0>
        void rotate_rows_inplace(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::logic_error("unsupported scheme"); // :1061-1064
            rotate_vector_like(encrypted, steps, galois_keys);
        }
        // Evaluator::rotate_columns_inplace (evaluator.h:1131-1139): BFV only; conjugate_internal = apply_galois with
        // get_elt_from_step(0) = 2N - 1 (:1343-1363)
        template <class C, IfCt<C> = 0>
        void rotate_columns_inplace(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::logic_error("unsupported scheme"); // :1134-1137
            conjugate_internal(encrypted, galois_keys);
        }
        // Evaluator::complex_conjugate_inplace (evaluator.h:1269-1277): CKKS only, the same automorphism
        template <class C, IfCt<C> = 0>
        void complex_conjugate_inplace(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // :1272-1275
            conjugate_internal(encrypted, galois_keys);
        }

        // Hoisted rotation (sealhip_evaluator_apply_galois_many): `encrypted` under every element of
        // galois_elts with one decomposition of its second polynomial; destinations[i] is the result of galois_elts[i], with
        // the operand's scale / NTT form (and, for a host type, its parms_id). The reference has no such method: each result
        // decrypts like apply_galois's, with noise of the same bound, but is not the same words. An element without its key
        // in galois_keys -> std::invalid_argument("Galois key not present"). BFV needs a STRICT context.
        // The ABI writes all results back to back into one block. A resident destination owns a pool block of its own, so
        // every result but a single one is copied once more on the device (2 k N words each, stream-ordered); and the
        // deferred transparency check takes one ring slot per result, so a resident call takes at most 256 elements
        // (std::invalid_argument("too many results for one checked operation")): split longer lists. Host destinations
        // have neither: they are downloaded straight from the one block, and not checked.
        template <class C, IfCt<C> = 0>
        void apply_galois_many(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                               const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, std::vector<C> &destinations)
        {
            check_galois_operand(encrypted);
            std::vector<const sealhip_kswitch_key *> raw;
            for (std::uint32_t elt : galois_elts)
            {
                auto it = galois_keys.find(elt);
                if (it == galois_keys.end() || !it->second)
                    throw std::invalid_argument("Galois key not present"); // evaluator.cpp:1871-1874
                raw.push_back(it->second->get());
            }
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), count = galois_elts.size(), words = 2 * k * n;
            if (count == 0)
                return destinations.clear();
            Dev c = dev_in(encrypted, words), o = dev_out(count * words);
            Check chk = checked(encrypted, count);
            throw_on(sealhip_evaluator_apply_galois_many(ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elts.data(), raw.data(),
                                                         std::uint32_t(count), o.ptr()));
            chk.done();
            scatter(encrypted, o, count, words, destinations);
        }
        // The same by rotation steps (sealhip_evaluator_rotate_vector_many): rotate_vector's steps for CKKS, rotate_rows'
        // for BFV; a step of 0 copies the operand; no non-adjacent-form fallback (a chain cannot share a decomposition)
        template <class C, IfCt<C> = 0>
        void rotate_vector_many(const C &encrypted, const std::vector<int> &steps,
                                const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, std::vector<C> &destinations)
        {
            check_galois_operand(encrypted);
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto &kv : galois_keys)
                if (kv.second)
                {
                    elts.push_back(kv.first);
                    raw.push_back(kv.second->get());
                }
            std::vector<std::int32_t> st(steps.begin(), steps.end());
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), count = st.size(), words = 2 * k * n;
            if (count == 0)
                return destinations.clear();
            Dev c = dev_in(encrypted, words), o = dev_out(count * words);
            Check chk = checked(encrypted, count);
            throw_on(sealhip_evaluator_rotate_vector_many(ctx_.get(), std::uint32_t(k), c.ptr(), 1, st.data(), std::uint32_t(count),
                                                          elts.data(), raw.data(), std::uint32_t(elts.size()), o.ptr()));
            chk.done();
            scatter(encrypted, o, count, words, destinations);
        }

        // Ring packing (sealhip_evaluator_extract_lwe / _pack_lwes), on resident ciphertexts. The
        // reference has no such methods. extract_lwe: the LWE samples of the coefficients `indices` (each below N, any
        // order, repeats allowed) of a size-2 ciphertext, which is not modified. pack_lwes: n = 2^l samples into one
        // ciphertext, sample j at coefficient (N / n) j, times n -- times N with `trace`, which also clears every other
        // coefficient, times 1 with `normalize`; galois_keys holds the elements of sealhip_pack_lwes_galois_elts (an absent
        // one -> std::invalid_argument("Galois key not present")); the destination gets the samples' level and scale and
        // the scheme's form, and one deferred transparency slot. BFV needs a STRICT context.
        void extract_lwe(const DeviceCiphertext &encrypted, const std::vector<std::uint32_t> &indices, LweSamples &destination)
        {
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2");
            const std::size_t k = encrypted.coeff_modulus_size();
            LweSamples next(ctx_);
            next.reset(indices.size(), k);
            throw_on(sealhip_evaluator_extract_lwe(ctx_.get(), std::uint32_t(k), encrypted.data(), 1, indices.data(), indices.size(),
                                                   next.a_out(), next.b_out()));
            next.scale() = encrypted.scale();
            destination = std::move(next);
        }
        void pack_lwes(const LweSamples &samples, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       DeviceCiphertext &destination, bool trace = false, bool normalize = false)
        {
            if (!samples.a())
                throw std::invalid_argument("samples are empty");
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto &kv : galois_keys)
                if (kv.second)
                {
                    elts.push_back(kv.first);
                    raw.push_back(kv.second->get());
                }
            const std::size_t k = samples.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev o = dev_out(words);
            Check chk = checked(destination);
            throw_on(sealhip_evaluator_pack_lwes(ctx_.get(), std::uint32_t(k), samples.a(), samples.b(), samples.size(), 1, elts.data(),
                                                 raw.data(), std::uint32_t(elts.size()), trace ? 1 : 0, normalize ? 1 : 0, o.ptr()));
            chk.done();
            destination.adopt(o.st->release(), words, 2, k);
            destination.is_ntt_form() = ctx_.scheme() == SEALHIP_SCHEME_CKKS;
            destination.scale() = samples.scale();
        }

        // Oblivious expansion (sealhip_evaluator_expand): `encrypted`, whose phase carries n = 2^l values
        // in its first n coefficients, into n ciphertexts; destinations[i] holds n times coefficient i of the phase as its
        // constant coefficient (1 times with `normalize`), with the operand's level, scale and form (and, for a host type,
        // its parms_id). galois_keys holds the elements of sealhip_expand_galois_elts (an absent one ->
        // std::invalid_argument("Galois key not present")). The reference has no such method. BFV needs a STRICT context.
        // One block from the ABI, then one pool block and one deferred transparency slot per result, as apply_galois_many's:
        // a resident call takes at most 256 results (std::invalid_argument("too many results for one checked operation")).
        template <class C, IfCt<C> = 0>
        void expand(const C &encrypted, std::size_t n, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                    std::vector<C> &destinations, bool normalize = false)
        {
            check_galois_operand(encrypted);
            if (n == 0)
                throw std::invalid_argument("n must be a power of two between 1 and N");
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto &kv : galois_keys)
                if (kv.second)
                {
                    elts.push_back(kv.first);
                    raw.push_back(kv.second->get());
                }
            const std::size_t k = encrypted.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev c = dev_in(encrypted, words), o = dev_out(n * words);
            Check chk = checked(encrypted, n);
            throw_on(sealhip_evaluator_expand(ctx_.get(), std::uint32_t(k), c.ptr(), 1, n, elts.data(), raw.data(),
                                              std::uint32_t(elts.size()), normalize ? 1 : 0, o.ptr()));
            chk.done();
            scatter(encrypted, o, n, words, destinations);
        }

        // Sums against plaintext rows (sealhip_evaluator_dot_plain) on resident operands:
        // destinations[s] = sum_i terms[i] (.) plains[s][i], everything in NTT form at one level: the ciphertexts of one size
        // and (CKKS) one scale, the plaintexts k x N words in NTT form and (CKKS) of one scale. Each result has the terms'
        // size, level and form and, for CKKS, the scale terms[0].scale() * plains[0][0].scale(). The ABI reads the terms and
        // the plaintexts from one block each: they are gathered on the device (stream-ordered copies). One pool block and
        // one deferred transparency slot per sum. std::invalid_argument: no terms or no sums, terms that differ in size,
        // level or scale or are not in NTT form, a ragged plaintext matrix, a plaintext of another level, form or scale.
        void dot_plain(const std::vector<DeviceCiphertext> &terms, const std::vector<std::vector<const DevicePlaintext *>> &plains,
                       std::vector<DeviceCiphertext> &destinations)
        {
            if (terms.empty() || plains.empty())
                throw std::invalid_argument("the term list and the sums must not be empty");
            const bool ckks = ctx_.scheme() == SEALHIP_SCHEME_CKKS;
            const std::size_t size = terms[0].size(), k = terms[0].coeff_modulus_size(), n = ctx_.n();
            const std::size_t pw = k * n, words = size * pw, n_terms = terms.size(), n_sums = plains.size();
            for (const DeviceCiphertext &t : terms)
            {
                if (!t.is_ntt_form())
                    throw std::invalid_argument("encrypted must be in NTT form");
                if (t.size() != size || t.coeff_modulus_size() != k || t.size() < 2)
                    throw std::invalid_argument("encrypted parameter mismatch");
                if (ckks && t.scale() != terms[0].scale())
                    throw std::invalid_argument("scale mismatch");
            }
            for (const auto &row : plains)
            {
                if (row.size() != n_terms)
                    throw std::invalid_argument("plains must hold one plaintext per term in every sum");
                for (const DevicePlaintext *p : row)
                {
                    if (!p || !p->is_ntt_form() || p->coeff_modulus_size() != k || p->words() != pw)
                        throw std::invalid_argument("plain must be in NTT form at the terms' level");
                    if (ckks && p->scale() != plains[0][0]->scale())
                        throw std::invalid_argument("scale mismatch");
                }
            }
            Staged x(ctx_, n_terms * words), w(ctx_, n_sums * n_terms * pw);
            for (std::size_t i = 0; i < n_terms; i++)
                throw_on(sealhip_memcpy_d2d(ctx_.get(), x.ptr() + i * words, terms[i].data(), words * 8));
            for (std::size_t s = 0; s < n_sums; s++)
                for (std::size_t i = 0; i < n_terms; i++)
                    plain_to(*plains[s][i], w.ptr() + (s * n_terms + i) * pw, pw);
            Dev o = dev_out(n_sums * words);
            Check chk = checked(terms[0], n_sums);
            throw_on(sealhip_evaluator_dot_plain(ctx_.get(), std::uint32_t(k), x.ptr(), std::uint32_t(n_terms), std::uint32_t(size), 1,
                                                 w.ptr(), std::uint32_t(n_sums), o.ptr()));
            chk.done();
            std::vector<DeviceCiphertext> next;
            next.reserve(n_sums);
            for (std::size_t s = 0; s < n_sums; s++)
            {
                next.emplace_back(ctx_);
                Staged one(ctx_, words); // (each destination owns a pool block of its own)
                throw_on(sealhip_memcpy_d2d(ctx_.get(), one.ptr(), o.ptr() + s * words, words * 8));
                next[s].adopt(one.release(), words, size, k);
                next[s].copy_meta(terms[0]);
                if (ckks)
                    next[s].scale() = terms[0].scale() * plains[0][0]->scale();
            }
            destinations.swap(next);
        }

        // Plaintext-weighted sums of rotations (sealhip_evaluator_apply_galois_dot_plain):
        // destinations[s] = sum_i plains[s][i] * sigma_{galois_elts[i]}(encrypted), with one decomposition of the operand's
        // second polynomial and one mod-down per sum. plains[s][i] is a plaintext in KEY-LEVEL NTT form (n_key x N words:
        // what CKKSEncoder::encode and transform_to_ntt give at the key level): a DevicePlaintext, or a host plaintext of
        // HostPlaintext's shape (words, k, ntt_form, scale). Element 1 needs no key. Each result has the operand's level
        // and NTT form and, for CKKS, the scale encrypted.scale() * plain.scale (all plaintexts must share one scale).
        // std::invalid_argument: a plaintext that is not key-level NTT form, a ragged plaintext matrix (a row whose length
        // is not galois_elts.size()), CKKS plaintexts of unequal scale, an element other than 1 without its key ("Galois
        // key not present"). The reference has no such method; the words are those of the ABI entry, not of the
        // composition. Resident destinations: one pool block and one deferred transparency slot per sum, as
        // apply_galois_many's.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_dot_plain(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                                    const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                    const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            dot_plain_internal(encrypted, galois_elts, galois_keys, plains, destinations, false);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_apply_galois_dot_plain_rescale,
        // DESIGN.md section 19): CKKS only; the unmerged method's checks, and "end of modulus switching chain reached" at the
        // last level. Each result is one level down with the scale encrypted.scale() * plain.scale / q_{k-1}.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_dot_plain_rescale(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                                            const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                            const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            dot_plain_internal(encrypted, galois_elts, galois_keys, plains, destinations, true);
        }
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_dot_plain_rescale(const C &encrypted, const std::vector<int> &steps,
                                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                             const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1205-1208
            dot_plain_internal(encrypted, elts_of_steps(steps), galois_keys, plains, destinations, true);
        }

    private:
        template <class C, class P>
        void dot_plain_internal(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                                const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                const std::vector<std::vector<P>> &plains, std::vector<C> &destinations, bool rescale)
        {
            check_galois_operand(encrypted);
            if (rescale)
                check_rescale_operand(encrypted);
            std::vector<const sealhip_kswitch_key *> raw;
            for (std::uint32_t elt : galois_elts)
            {
                auto it = galois_keys.find(elt);
                if (elt != 1 && (it == galois_keys.end() || !it->second))
                    throw std::invalid_argument("Galois key not present"); // evaluator.cpp:1871-1874
                raw.push_back(elt != 1 ? it->second->get() : nullptr);
            }
            const std::size_t n_elts = galois_elts.size(), n_sums = plains.size();
            const double scale = check_dot_plains(plains, n_elts);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n, pw = ctx_.n_key() * n;
            const std::size_t k_out = rescale ? k - 1 : k, out_words = 2 * k_out * n;
            Dev c = dev_in(encrypted, words), o = dev_out((n_sums ? n_sums : 1) * out_words);
            Staged w(ctx_, n_sums * n_elts ? n_sums * n_elts * pw : 1);
            for (std::size_t s = 0; s < n_sums; s++)
                for (std::size_t i = 0; i < n_elts; i++)
                    plain_to(plains[s][i], w.ptr() + (s * n_elts + i) * pw, pw);
            Check chk = checked(encrypted, n_sums ? n_sums : 1);
            throw_on((rescale ? sealhip_evaluator_apply_galois_dot_plain_rescale : sealhip_evaluator_apply_galois_dot_plain)(
                ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elts.data(), raw.data(), std::uint32_t(n_elts), w.ptr(),
                std::uint32_t(n_sums), o.ptr()));
            chk.done();
            scatter(encrypted, o, n_sums, out_words, destinations, k_out);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                for (C &d : destinations)
                    d.scale() = encrypted.scale() * scale / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
        }

    public:
        // The same by rotation steps (sealhip_evaluator_rotate_vector_dot_plain): CKKS rotate_vector's steps; step 0 is the
        // identity; no non-adjacent-form fallback
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_dot_plain(const C &encrypted, const std::vector<int> &steps,
                                     const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                     const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1205-1208
            apply_galois_dot_plain(encrypted, elts_of_steps(steps), galois_keys, plains, destinations);
        }
        // ... and BFV rotate_rows' steps
        template <class C, class P, IfCt<C> = 0>
        void rotate_rows_dot_plain(const C &encrypted, const std::vector<int> &steps,
                                   const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                   const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1061-1064
            apply_galois_dot_plain(encrypted, elts_of_steps(steps), galois_keys, plains, destinations);
        }

        // Baby-step/giant-step matrix-vector product (sealhip_evaluator_apply_galois_bsgs_plain):
        // destination = sum_j sigma_{giant_elts[j]}( sum_i plains[j][i] * sigma_{baby_elts[i]}(encrypted) ), the giant steps
        // accumulated in the extended basis and ONE full mod-down. plains[giant][baby]: key-level NTT form, DevicePlaintext
        // or host plaintexts, as apply_galois_dot_plain's; element 1 needs no key on either axis; one set of keys serves
        // both. The result has the operand's level and NTT form and, for CKKS, the scale encrypted.scale() * plain.scale.
        // std::invalid_argument as apply_galois_dot_plain (a row whose length is not baby_elts.size(), a matrix without
        // giant_elts.size() rows). The words are those of the ABI entry, not of the composition.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_bsgs_plain(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                     const std::vector<std::uint32_t> &giant_elts,
                                     const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                     const std::vector<std::vector<P>> &plains, C &destination)
        {
            bsgs_plain_internal(encrypted, baby_elts, giant_elts, galois_keys, plains, destination, false);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_apply_galois_bsgs_plain_rescale,
        // DESIGN.md section 19): CKKS only; the unmerged method's checks, and "end of modulus switching chain reached" at the
        // last level. The result is one level down with the scale encrypted.scale() * plain.scale / q_{k-1}.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_bsgs_plain_rescale(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                             const std::vector<std::uint32_t> &giant_elts,
                                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                             const std::vector<std::vector<P>> &plains, C &destination)
        {
            bsgs_plain_internal(encrypted, baby_elts, giant_elts, galois_keys, plains, destination, true);
        }
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_bsgs_plain_rescale(const C &encrypted, const std::vector<int> &baby_steps,
                                              const std::vector<int> &giant_steps,
                                              const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                              const std::vector<std::vector<P>> &plains, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1205-1208
            bsgs_plain_internal(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains, destination,
                                true);
        }

    private:
        template <class C, class P>
        void bsgs_plain_internal(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                 const std::vector<std::uint32_t> &giant_elts,
                                 const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                 const std::vector<std::vector<P>> &plains, C &destination, bool rescale)
        {
            check_galois_operand(encrypted);
            if (rescale)
                check_rescale_operand(encrypted);
            const auto raw_keys = [&](const std::vector<std::uint32_t> &elts) {
                std::vector<const sealhip_kswitch_key *> raw;
                for (std::uint32_t elt : elts)
                {
                    auto it = galois_keys.find(elt);
                    if (elt != 1 && (it == galois_keys.end() || !it->second))
                        throw std::invalid_argument("Galois key not present"); // evaluator.cpp:1871-1874
                    raw.push_back(elt != 1 ? it->second->get() : nullptr);
                }
                return raw;
            };
            const std::vector<const sealhip_kswitch_key *> bk = raw_keys(baby_elts), gk = raw_keys(giant_elts);
            const std::size_t n_baby = baby_elts.size(), n_giant = giant_elts.size();
            if (plains.size() != n_giant)
                throw std::invalid_argument("plains must hold one row of plaintexts per giant element");
            const double scale = check_dot_plains(plains, n_baby);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n, pw = ctx_.n_key() * n;
            const std::size_t k_out = rescale ? k - 1 : k, out_words = 2 * k_out * n;
            Dev c = dev_in(encrypted, words), o = dev_out(out_words);
            Staged w(ctx_, (n_giant && n_baby) ? n_giant * n_baby * pw : 1);
            for (std::size_t j = 0; j < n_giant; j++)
                for (std::size_t i = 0; i < n_baby; i++)
                    plain_to(plains[j][i], w.ptr() + (j * n_baby + i) * pw, pw);
            Check chk = checked(encrypted, 1);
            throw_on((rescale ? sealhip_evaluator_apply_galois_bsgs_plain_rescale : sealhip_evaluator_apply_galois_bsgs_plain)(
                ctx_.get(), std::uint32_t(k), c.ptr(), 1, baby_elts.data(), bk.data(), std::uint32_t(n_baby), giant_elts.data(),
                gk.data(), std::uint32_t(n_giant), w.ptr(), o.ptr()));
            chk.done();
            const double in_scale = encrypted.scale(); // (the destination may be the operand)
            std::vector<C> one;
            scatter(encrypted, o, 1, out_words, one, k_out);
            destination = std::move(one[0]);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                destination.scale() = in_scale * scale / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
        }

    public:
        // CoeffToSlot in one call (sealhip_evaluator_coeffs_to_slots): slot j of destination_re /
        // destination_im holds coefficient bitrev(j) / bitrev(j) + N/2 of the operand's message over its scale. The results
        // are dft.out_level() primes long at the operand's scale. galois_keys: element -> key, with the keys of
        // dft.key_steps() and of element 2N - 1.
        template <class C, IfCt<C> = 0>
        void coeffs_to_slots(const C &encrypted, const HomomorphicDFT &dft,
                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination_re,
                             C &destination_im)
        {
            check_dft_operand(encrypted, dft, SEALHIP_DFT_COEFFS_TO_SLOTS);
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            dft_keys(galois_keys, elts, raw);
            const std::size_t n = ctx_.n(), words = 2 * dft.in_level() * n, out_words = 2 * dft.out_level() * n;
            Dev c = dev_in(encrypted, words), o = dev_out(2 * out_words);
            Check chk = checked(encrypted, 2);
            throw_on(sealhip_evaluator_coeffs_to_slots(ctx_.get(), dft.get(), c.ptr(), 1, elts.data(), raw.data(),
                                                       std::uint32_t(elts.size()), o.ptr(), o.ptr() + out_words));
            chk.done();
            std::vector<C> two;
            scatter(encrypted, o, 2, out_words, two, dft.out_level());
            destination_re = std::move(two[0]);
            destination_im = std::move(two[1]);
        }
        // SlotToCoeff in one call (sealhip_evaluator_slots_to_coeffs): the inverse of coeffs_to_slots, from its slot order
        template <class C, IfCt<C> = 0>
        void slots_to_coeffs(const C &encrypted_re, const C &encrypted_im, const HomomorphicDFT &dft,
                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            check_dft_operand(encrypted_re, dft, SEALHIP_DFT_SLOTS_TO_COEFFS);
            check_dft_operand(encrypted_im, dft, SEALHIP_DFT_SLOTS_TO_COEFFS);
            if (encrypted_re.scale() != encrypted_im.scale())
                throw std::invalid_argument("scale mismatch");
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            dft_keys(galois_keys, elts, raw);
            const std::size_t n = ctx_.n(), words = 2 * dft.in_level() * n, out_words = 2 * dft.out_level() * n;
            Dev a = dev_in(encrypted_re, words), b = dev_in(encrypted_im, words), o = dev_out(out_words);
            Check chk = checked(encrypted_re, 1);
            throw_on(sealhip_evaluator_slots_to_coeffs(ctx_.get(), dft.get(), a.ptr(), b.ptr(), 1, elts.data(), raw.data(),
                                                       std::uint32_t(elts.size()), o.ptr()));
            chk.done();
            std::vector<C> one;
            scatter(encrypted_re, o, 1, out_words, one, dft.out_level());
            destination = std::move(one[0]);
        }

        // The matrix of `lt` applied to the slots of `encrypted` (sealhip_evaluator_linear_transform),
        // at the operand's level; with rescale the result is one level down. The result's scale is encrypted.scale() *
        // lt.scale(), divided by q_{k-1} with rescale. galois_keys: element -> key, with the keys of lt.key_steps(); a step
        // whose key is absent throws std::invalid_argument("Galois key not present").
        template <class C, IfCt<C> = 0>
        void linear_transform(const C &encrypted, const LinearTransform &lt,
                              const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination, bool rescale = false)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme");
            check_galois_operand(encrypted);
            if (rescale)
                check_rescale_operand(encrypted);
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            dft_keys(galois_keys, elts, raw);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n;
            const std::size_t k_out = rescale ? k - 1 : k, out_words = 2 * k_out * n;
            Dev c = dev_in(encrypted, words), o = dev_out(out_words);
            Check chk = checked(encrypted, 1);
            throw_on(sealhip_evaluator_linear_transform(ctx_.get(), lt.get(), std::uint32_t(k), c.ptr(), 1, elts.data(), raw.data(),
                                                        std::uint32_t(elts.size()), rescale ? 1 : 0, o.ptr()));
            chk.done();
            const double in_scale = encrypted.scale(); // (the destination may be the operand)
            std::vector<C> one;
            scatter(encrypted, o, 1, out_words, one, k_out);
            destination = std::move(one[0]);
            destination.scale() = in_scale * lt.scale() / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
        }

    private:
        template <class C>
        void check_dft_operand(const C &encrypted, const HomomorphicDFT &dft, std::uint32_t direction) const
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme");
            check_galois_operand(encrypted);
            if (dft.direction() != direction)
                throw std::invalid_argument("the DFT tables were made for the other direction");
            if (encrypted.coeff_modulus_size() != dft.in_level())
                throw std::invalid_argument("encrypted is not at the level of the DFT tables");
        }
        template <class C>
        void check_bootstrap_operand(const C &encrypted) const
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme");
            check_galois_operand(encrypted);
        }
        static void dft_keys(const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, std::vector<std::uint32_t> &elts,
                             std::vector<const sealhip_kswitch_key *> &raw)
        {
            for (const auto &kv : galois_keys)
                if (kv.second)
                {
                    elts.push_back(kv.first);
                    raw.push_back(kv.second->get());
                }
        }

    public:
        // The same by rotation steps (sealhip_evaluator_rotate_vector_bsgs_plain): CKKS rotate_vector's steps; step 0 is the
        // identity; no non-adjacent-form fallback
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_bsgs_plain(const C &encrypted, const std::vector<int> &baby_steps, const std::vector<int> &giant_steps,
                                      const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                      const std::vector<std::vector<P>> &plains, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1205-1208
            apply_galois_bsgs_plain(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains,
                                    destination);
        }
        // ... and BFV rotate_rows' steps
        template <class C, class P, IfCt<C> = 0>
        void rotate_rows_bsgs_plain(const C &encrypted, const std::vector<int> &baby_steps, const std::vector<int> &giant_steps,
                                    const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                    const std::vector<std::vector<P>> &plains, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::logic_error("unsupported scheme"); // evaluator.h:1061-1064
            apply_galois_bsgs_plain(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains,
                                    destination);
        }

        // Evaluator::mod_switch_to_inplace (evaluator.cpp:1038-1060) / rescale_to_inplace (:1128-1165). The ABI names a level by
        // its number of primes k (the chain drops one prime per level, context.cpp:423-431); for seal::Ciphertext the
        // binding maps the parms_id argument to it.
        template <class C, IfCt<C> = 0>
        void mod_switch_to_inplace(C &encrypted, std::size_t target_coeff_modulus_size)
        {
            if (target_coeff_modulus_size < 1)
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1047-1050
            if (encrypted.coeff_modulus_size() < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1051-1054
            while (encrypted.coeff_modulus_size() != target_coeff_modulus_size)
                mod_switch_to_next_inplace(encrypted); // :1056-1059
        }
        template <class C, IfCt<C> = 0>
        void rescale_to_inplace(C &encrypted, std::size_t target_coeff_modulus_size)
        {
            if (target_coeff_modulus_size < 1)
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1137-1140
            if (encrypted.coeff_modulus_size() < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1141-1144
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::invalid_argument("unsupported operation for scheme type"); // :1146-1162
            while (encrypted.coeff_modulus_size() != target_coeff_modulus_size)
                rescale_to_next_inplace(encrypted);
        }
        // Evaluator::add_many (evaluator.cpp:153-172)
        template <class C, IfCt<C> = 0>
        void add_many(const std::vector<C> &encrypteds, C &destination)
        {
            if (encrypteds.empty())
                throw std::invalid_argument("encrypteds cannot be empty"); // :155-158
            for (const C &c : encrypteds)
                if (&c == &destination)
                    throw std::invalid_argument("encrypteds must be different from destination"); // :159-165
            destination = encrypteds[0];
            for (std::size_t i = 1; i < encrypteds.size(); i++)
                add_inplace(destination, encrypteds[i]);
        }

        // ---- destination-taking variants (evaluator.h:121-126, :156-168, :214-226, :268-284, :317-322, :371-376, :396-430,
        // :565-583, :916-947, :1021-1027, :1097-1103, :1167-1173, :1239-1245, :1302-1308): copy, then the in-place form
        template <class C, IfCt<C> = 0>
        void negate(const C &encrypted, C &destination) { destination = encrypted; negate_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void add(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // (:160-163: addition commutes, the alias is kept valid)
                add_inplace(destination, encrypted1);
            else
            {
                destination = encrypted1;
                add_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void sub(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // :216-222: destination = -(encrypted2 - encrypted1)
            {
                sub_inplace(destination, encrypted1);
                negate_inplace(destination);
            }
            else
            {
                destination = encrypted1;
                sub_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void multiply(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // :272-275
                multiply_inplace(destination, encrypted1);
            else
            {
                destination = encrypted1;
                multiply_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void square(const C &encrypted, C &destination) { destination = encrypted; square_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void relinearize(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            destination = encrypted;
            relinearize_inplace(destination, relin_keys);
        }
        template <class C, IfCt<C> = 0>
        void mod_switch_to_next(const C &encrypted, C &destination) { destination = encrypted; mod_switch_to_next_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void rescale_to_next(const C &encrypted, C &destination) { destination = encrypted; rescale_to_next_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void mod_switch_to(const C &encrypted, std::size_t target_coeff_modulus_size, C &destination)
        {
            destination = encrypted;
            mod_switch_to_inplace(destination, target_coeff_modulus_size);
        }
        template <class C, IfCt<C> = 0>
        void rescale_to(const C &encrypted, std::size_t target_coeff_modulus_size, C &destination)
        {
            destination = encrypted;
            rescale_to_inplace(destination, target_coeff_modulus_size);
        }
        template <class C, IfCt<C> = 0>
        void transform_to_ntt(const C &encrypted, C &destination_ntt) { destination_ntt = encrypted; transform_to_ntt_inplace(destination_ntt); }
        template <class C, IfCt<C> = 0>
        void transform_from_ntt(const C &encrypted_ntt, C &destination) { destination = encrypted_ntt; transform_from_ntt_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void apply_galois(const C &encrypted, std::uint32_t galois_elt, const KSwitchKeys &galois_key, C &destination)
        {
            destination = encrypted;
            apply_galois_inplace(destination, galois_elt, galois_key);
        }
        template <class C, IfCt<C> = 0>
        void rotate_vector(const C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_vector_inplace(destination, steps, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void rotate_rows(const C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_rows_inplace(destination, steps, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void rotate_columns(const C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_columns_inplace(destination, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void complex_conjugate(const C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            complex_conjugate_inplace(destination, galois_keys);
        }
        template <class C, class P, IfCt<C> = 0>
        void multiply_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            multiply_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, class P, IfCt<C> = 0>
        void add_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            add_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, class P, IfCt<C> = 0>
        void sub_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            sub_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, IfCt<C> = 0>
        void exponentiate(const C &encrypted, std::uint64_t exponent, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            destination = encrypted; // :719-726
            exponentiate_inplace(destination, exponent, relin_keys);
        }

        // Ciphertext inner product (sealhip_evaluator_dot_product): destination = sum_i
        // encrypteds1[i] * encrypteds2[i] over size-2 ciphertexts, the tensor products summed in NTT form, ONE floor (BFV,
        // STRICT contexts only) and, in the overload with a relinearization key, ONE relinearization (size 2; size 3
        // without). Every term is checked like multiply's operands and against the first: same level, and for CKKS one
        // scale on each side (the products must be addable); the result has the terms' level and form and, for CKKS, the
        // scale encrypteds1[0].scale() * encrypteds2[0].scale(). An object may appear in several terms and on both sides.
        // The reference has no such method; for BFV the words are those of the ABI entry, not of the composition.
        template <class C, IfCt<C> = 0>
        void dot_product(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, nullptr, destination);
        }
        template <class C, IfCt<C> = 0>
        void dot_product(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, const KSwitchKeys &relin_key,
                         C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, &relin_key, destination);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_dot_product_rescale, DESIGN.md
        // section 19): CKKS only; dot_product's checks, and "end of modulus switching chain reached" at the last level. The
        // result has size 2, one level down, with the scale encrypteds1[0].scale() * encrypteds2[0].scale() / q_{k-1}. With
        // one term it is multiply + relinearize + rescale_to_next.
        template <class C, IfCt<C> = 0>
        void dot_product_rescale(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, const KSwitchKeys &relin_key,
                                 C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, &relin_key, destination, true);
        }
        // Linear combination with scalar weights (sealhip_evaluator_linear_combination): destination =
        // sum_i weights[i] * terms[i], one streaming pass over the terms -- no transforms, no plaintext objects. Every term is
        // checked like add's operands and against the first: same size (>= 2), same level, the scheme's form. An object may
        // appear in several terms. The reference has no such method; the words are those of multiply_plain with a constant
        // plaintext per term and add over the products.
        // BFV: weights are scalars mod t (a weight >= t is refused); the product uses the residue multiply_plain uses for a
        // one-coefficient plaintext, (c - t [c >= (t + 1) / 2]) mod q_r.
        template <class C, IfCt<C> = 0>
        void linear_combination(const std::vector<C> &terms, const std::vector<std::uint64_t> &weights, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::invalid_argument("integer weights are for BFV; CKKS takes doubles and a scale");
            check_lincomb_terms(terms, weights.size());
            const std::size_t k = terms[0].coeff_modulus_size();
            const std::uint64_t t = ctx_.plain_modulus(), half = (t + 1) >> 1;
            std::vector<std::uint64_t> w(weights.size() * k);
            for (std::size_t i = 0; i < weights.size(); i++)
            {
                if (weights[i] >= t)
                    throw std::invalid_argument("a weight is not below the plain modulus");
                for (std::size_t r = 0; r < k; r++)
                {
                    const std::uint64_t q = ctx_.key_modulus(r);
                    w[i * k + r] = weights[i] >= half ? (weights[i] % q + (q - t % q)) % q : weights[i] % q;
                }
            }
            linear_combination_internal(terms, w, destination, terms[0].scale());
        }
        // CKKS: weights are doubles with ONE scale; the residues are those of encode(double value, scale)'s constant,
        // round(weight * scale) reduced per prime (ckks.h:405-470), |weight * scale| >= 2^62 is refused. Terms are checked for
        // one scale; the result's scale is terms[0].scale() * scale.
        template <class C, IfCt<C> = 0>
        void linear_combination(const std::vector<C> &terms, const std::vector<double> &weights, double scale, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::invalid_argument("weights with a scale are for CKKS; BFV takes scalars mod t");
            check_lincomb_terms(terms, weights.size());
            if (!(scale > 0))
                throw std::invalid_argument("scale out of bounds"); // ckks.h:420-424
            const std::size_t k = terms[0].coeff_modulus_size();
            std::vector<std::uint64_t> w(weights.size() * k);
            for (std::size_t i = 0; i < weights.size(); i++)
            {
                const double v = std::round(weights[i] * scale);
                if (!(std::fabs(v) < 4611686018427387904.0)) // 2^62 (also refuses NaN)
                    throw std::invalid_argument("encoded value is too large");
                const std::uint64_t mag = static_cast<std::uint64_t>(std::fabs(v));
                for (std::size_t r = 0; r < k; r++)
                {
                    const std::uint64_t q = ctx_.key_modulus(r), res = mag % q;
                    w[i * k + r] = std::signbit(v) && res ? q - res : res;
                }
            }
            linear_combination_internal(terms, w, destination, terms[0].scale() * scale);
        }

        // Evaluator-style polynomial evaluation (sealhip_evaluator_evaluate_polynomial): destination =
        // sum_e coeffs[e] * encrypted^e by Paterson-Stockmeyer, BFV on STRICT contexts, a size-2 operand in coefficient form,
        // coefficients below t (lowest degree first), relin_keys as relinearize_inplace takes them (index 0 is read; none is
        // needed for degree one). The reference has no such method; the words are those of tests/poly_eval_ref.py.
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial(const C &encrypted, const std::vector<std::uint64_t> &coeffs,
                                 const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::logic_error("unsupported scheme");
            if (encrypted.is_ntt_form())
                throw std::invalid_argument("BFV encrypted cannot be in NTT form");
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2");
            if (coeffs.empty())
                throw std::invalid_argument("coeffs must not be empty");
            const std::size_t k = encrypted.coeff_modulus_size();
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_evaluate_polynomial(ctx_.get(), std::uint32_t(k), c, 1, coeffs.data(),
                                                             std::uint32_t(coeffs.size() - 1), 0, raw ? &raw : nullptr, raw ? 1u : 0u, o);
            });
        }
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial_inplace(C &encrypted, const std::vector<std::uint64_t> &coeffs,
                                         const std::vector<const KSwitchKeys *> &relin_keys)
        {
            evaluate_polynomial(encrypted, coeffs, relin_keys, encrypted);
        }

        // CKKS: destination = p(encrypted) with planned levels and scales (sealhip_evaluator_evaluate_polynomial_ckks, DESIGN.md
        // section 21). coeffs are doubles, lowest degree first, in the monomial basis (basis 0) or the Chebyshev basis of
        // the first kind (basis 1, for messages in [-1, 1]); a size-2 operand in NTT form; relin_keys as above. The
        // destination gets the plan's level (sealhip_evaluator_polynomial_plan_ckks: "end of modulus switching chain
        // reached" when the operand's level is too low for the degree) and the scale scale_out, or the operand's scale when
        // scale_out is 0 -- exactly, by construction. The words are those of tests/poly_eval_ckks_ref.py.
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial(const C &encrypted, const std::vector<double> &coeffs,
                                 const std::vector<const KSwitchKeys *> &relin_keys, C &destination, std::uint32_t basis = 0,
                                 double scale_out = 0.0)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme");
            if (!encrypted.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form");
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2");
            if (coeffs.empty())
                throw std::invalid_argument("coeffs must not be empty");
            const std::size_t k = encrypted.coeff_modulus_size();
            sealhip_poly_plan plan{};
            throw_on(sealhip_evaluator_polynomial_plan_ckks(ctx_.get(), std::uint32_t(k), encrypted.scale(), coeffs.data(),
                                                            std::uint32_t(coeffs.size() - 1), basis, 0, scale_out, &plan, nullptr,
                                                            nullptr));
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, plan.out_level, destination, &plan.out_scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_evaluate_polynomial_ckks(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), coeffs.data(),
                                                                  std::uint32_t(coeffs.size() - 1), basis, 0, scale_out,
                                                                  raw ? &raw : nullptr, raw ? 1u : 0u, o, nullptr, nullptr);
            });
        }
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial_inplace(C &encrypted, const std::vector<double> &coeffs,
                                         const std::vector<const KSwitchKeys *> &relin_keys, std::uint32_t basis = 0,
                                         double scale_out = 0.0)
        {
            evaluate_polynomial(encrypted, coeffs, relin_keys, encrypted, basis, scale_out);
        }

        // relinearize + rescale_to_next in one call and with one rounding (sealhip_evaluator_relinearize_rescale, DESIGN.md
        // section 19): CKKS only, a size-3 operand in NTT form, relin_keys as relinearize_inplace takes them (index 0 is
        // read); "end of modulus switching chain reached" at the last level. The result has size 2, one level down, with
        // the scale encrypted.scale() / q_{k-1}.
        template <class C, IfCt<C> = 0>
        void relinearize_rescale(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            if (encrypted.size() != 3)
                throw std::invalid_argument("encrypted size must be 3");
            check_rescale_operand(encrypted);
            const sealhip_kswitch_key *raw = first_relin_key(relin_keys);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n();
            const double scale = encrypted.scale() / double(ctx_.key_modulus(k - 1));
            to_size2(encrypted, 3, k - 1, destination, &scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_relinearize_rescale(ctx_.get(), std::uint32_t(k), c, 3, 3 * k * n, 1, &raw, 1, o);
            });
        }

        // ---- CKKS bootstrapping and its parts; size-2 operands in NTT form
        // ModRaise (sealhip_evaluator_mod_raise): the centred coefficients of the operand modulo q_0 re-read modulo the
        // first k_out primes. Only the operand's q_0 rows are read; the destination decrypts to m + q_0 I and keeps the
        // operand's scale (the caller re-declares it, e.g. as q_0 K ahead of coeffs_to_slots).
        template <class C, IfCt<C> = 0>
        void mod_raise(const C &encrypted, std::size_t k_out, C &destination)
        {
            check_bootstrap_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            if (k_out < 2)
                throw std::invalid_argument("k_out must be at least 2");
            to_size2(encrypted, 2, k_out, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_mod_raise(ctx_.get(), std::uint32_t(k), c, 1, std::uint32_t(k_out), o);
            });
        }
        // destination = 2 encrypted^2 - 1, one level down, at the scale scale^2 / q_(k-1) (sealhip_evaluator_double_angle)
        template <class C, IfCt<C> = 0>
        void double_angle(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            check_bootstrap_operand(encrypted);
            const sealhip_kswitch_key *raw = first_relin_key(relin_keys);
            const std::size_t k = encrypted.coeff_modulus_size();
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached");
            double scale = 0.0; // (the entry reports it)
            to_size2(encrypted, 2, k - 1, destination, &scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_double_angle(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), &raw, 1, o, &scale);
            });
        }
        // EvalMod (sealhip_evaluator_eval_mod): slots x = c / (q_0 K) in [-1, 1] become sin(2 pi K x); the destination gets
        // the plan's level and scale (sealhip_evaluator_evalmod_plan), scale_out or the operand's scale up to rounding
        template <class C, IfCt<C> = 0>
        void eval_mod(const C &encrypted, std::uint32_t K, std::uint32_t r, std::uint32_t degree,
                      const std::vector<const KSwitchKeys *> &relin_keys, C &destination, std::uint32_t n_baby = 0,
                      double scale_out = 0.0)
        {
            check_bootstrap_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            sealhip_evalmod_plan plan{};
            throw_on(sealhip_evaluator_evalmod_plan(ctx_.get(), std::uint32_t(k), encrypted.scale(), K, r, degree, n_baby, scale_out,
                                                    &plan));
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, plan.out_level, destination, &plan.scales[plan.r], [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_eval_mod(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), K, r, degree, n_baby,
                                                  scale_out, raw ? &raw : nullptr, raw ? 1u : 0u, o, nullptr, nullptr);
            });
        }
        // The bootstrap in one call (sealhip_evaluator_bootstrap): the destination is at boot.out_level() with the operand's
        // scale. galois_keys: element -> key, with the keys of boot.key_steps() and of element 2N - 1.
        template <class C, IfCt<C> = 0>
        void bootstrap(const C &encrypted, const Bootstrapper &boot, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            bootstrap_internal(encrypted, boot, galois_keys, relin_keys, nullptr, nullptr, destination);
        }
        // The same with ModRaise alone under a sparse secret (sealhip_evaluator_bootstrap_encapsulated):
        // to_sparse = KeyGenerator(sparse secret).switching_keys(dense secret, 1, 1)[0], to_dense =
        // KeyGenerator(dense secret).switching_keys(sparse secret, 1)[0]; the operand, the destination and every other key
        // are under the dense secret
        template <class C, IfCt<C> = 0>
        void bootstrap(const C &encrypted, const Bootstrapper &boot, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       const std::vector<const KSwitchKeys *> &relin_keys, const KSwitchKeys &to_sparse, const KSwitchKeys &to_dense,
                       C &destination)
        {
            bootstrap_internal(encrypted, boot, galois_keys, relin_keys, to_sparse.get(), to_dense.get(), destination);
        }
        // Re-encryption under another secret (sealhip_evaluator_switch_secret): destination = (c_0, 0) + switch_key(c_1), the
        // operand under the key's source secret, the destination under its target secret (KeyGenerator::switching_keys)
        template <class C, IfCt<C> = 0>
        void switch_secret(const C &encrypted, const KSwitchKeys &key, C &destination)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_switch_secret(ctx_.get(), std::uint32_t(k), c, 1, key.get(), o);
            });
        }

        // The external product (sealhip_evaluator_external_product): destination = base + encrypted (x)
        // rgsw, the phase of `encrypted` times the small polynomial the RGSW encrypts, with additive noise; base (optional)
        // has the operand's size, level and form. The destination (which may be an operand) takes the metadata of
        // `encrypted`. The reference has no such method. CKKS in NTT form; BFV in coefficient form on a STRICT context.
        template <class C, IfCt<C> = 0>
        void external_product(const C &encrypted, const RgswCiphertext &rgsw, C &destination, const C *base = nullptr)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev b;
            if (base)
            {
                check_rgsw_pair(encrypted, *base);
                b = dev_in(*base, words);
            }
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_external_product(ctx_.get(), std::uint32_t(k), c, 1, rgsw.get(), b.ptr(), o);
            });
        }
        // CMux (sealhip_evaluator_cmux): destination = encrypted0 + (encrypted1 - encrypted0) (x) rgsw, i.e. encrypted1 where
        // the RGSW encrypts 1 and encrypted0 where it encrypts 0; the metadata is encrypted0's
        template <class C, IfCt<C> = 0>
        void cmux(const C &encrypted0, const C &encrypted1, const RgswCiphertext &rgsw, C &destination)
        {
            check_galois_operand(encrypted0);
            check_rgsw_pair(encrypted0, encrypted1);
            const std::size_t k = encrypted0.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev c1 = dev_in(encrypted1, words);
            to_size2(encrypted0, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_cmux(ctx_.get(), std::uint32_t(k), c, c1.ptr(), 1, rgsw.get(), o);
            });
        }
        // Selection (sealhip_evaluator_select): destination = encrypteds[index] for the index whose bit t (least significant
        // first) rgsw_bits[t] encrypts: a CMux tree over 2^l ciphertexts of one size, level and form, l = rgsw_bits.size()
        // (another count -> std::invalid_argument). The metadata is encrypteds[0]'s. The operands are gathered into one
        // block for the call.
        template <class C, IfCt<C> = 0>
        void select(const std::vector<C> &encrypteds, const std::vector<const RgswCiphertext *> &rgsw_bits, C &destination)
        {
            if (rgsw_bits.size() > 16 || encrypteds.size() != (std::size_t(1) << rgsw_bits.size()))
                throw std::invalid_argument("select needs 2^l ciphertexts for l RGSW bits");
            check_galois_operand(encrypteds[0]);
            const std::size_t k = encrypteds[0].coeff_modulus_size(), words = 2 * k * ctx_.n();
            std::vector<const sealhip_rgsw *> raw;
            for (const RgswCiphertext *g : rgsw_bits)
            {
                if (!g)
                    throw std::invalid_argument("rgsw_bits holds a null entry");
                raw.push_back(g->get());
            }
            Dev all = dev_out(encrypteds.size() * words), o = dev_out(words);
            for (std::size_t i = 0; i < encrypteds.size(); i++)
            {
                check_rgsw_pair(encrypteds[0], encrypteds[i]);
                gather_words(encrypteds[i], all.ptr() + i * words, words);
            }
            Check chk = checked(encrypteds[0]);
            throw_on(sealhip_evaluator_select(ctx_.get(), std::uint32_t(k), all.ptr(), 1, std::uint32_t(raw.size()),
                                              raw.empty() ? nullptr : raw.data(), o.ptr()));
            chk.done();
            const C first = meta_of(encrypteds[0]); // (the destination may be one of the operands)
            take_meta(destination, first);
            commit(destination, o, 2, k);
        }

        // The monomial product (sealhip_evaluator_multiply_monomial): destination = X^exponent encrypted,
        // or (X^exponent - 1) encrypted with minus_one; the exponent is taken modulo 2N with X^N = -1. The destination (which
        // may be the operand) takes the operand's metadata. CKKS in NTT form; BFV in coefficient form on a STRICT context.
        template <class C, IfCt<C> = 0>
        void multiply_monomial(const C &encrypted, std::uint32_t exponent, C &destination, bool minus_one = false)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            Staged e(ctx_, 1);
            const std::uint64_t word = exponent;
            e.up(&word, 1);
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_multiply_monomial(ctx_.get(), std::uint32_t(k), c, 1, 1,
                                                           reinterpret_cast<const std::uint32_t *>(e.ptr()), 1, minus_one ? 1 : 0, o);
            });
        }
        // Blind rotation (sealhip_evaluator_blind_rotate): destination = X^(exponents[0]) test_vector, then for every step t
        // the accumulator plus ((X^(exponents[t]) - 1) accumulator) (x) keys[t - 1]. exponents holds 1 + keys.n_steps() words,
        // one row of what sealhip_lwe_mod_switch writes (another count -> std::invalid_argument). The metadata is the test
        // vector's.
        template <class C, IfCt<C> = 0>
        void blind_rotate(const C &test_vector, const std::vector<std::uint32_t> &exponents, const BlindRotationKeys &keys,
                          C &destination)
        {
            if (exponents.size() != 1 + keys.n_steps())
                throw std::invalid_argument("blind_rotate needs one exponent and one more per key");
            check_galois_operand(test_vector);
            const std::size_t k = test_vector.coeff_modulus_size();
            std::vector<std::uint64_t> packed((exponents.size() + 1) / 2, 0);
            std::memcpy(packed.data(), exponents.data(), exponents.size() * sizeof(std::uint32_t));
            Staged e(ctx_, packed.size());
            e.up(packed.data(), packed.size());
            to_size2(test_vector, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_blind_rotate(ctx_.get(), std::uint32_t(k), c, 1, 1,
                                                      reinterpret_cast<const std::uint32_t *>(e.ptr()),
                                                      std::uint32_t(keys.n_steps()), keys.get(), o);
            });
        }

        // Evaluator::multiply_many (evaluator.cpp:1180-1255): destination = product of all, relinearized after every step
        template <class C, IfCt<C> = 0>
        void multiply_many(const std::vector<C> &encrypteds, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            if (encrypteds.empty())
                throw std::invalid_argument("encrypteds vector must not be empty"); // :1185-1188
            for (const C &c : encrypteds)
                if (&c == &destination)
                    throw std::invalid_argument("encrypteds must be different from destination"); // :1193-1199
            const std::size_t k = encrypteds[0].coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n;
            std::vector<Dev> dev;
            std::vector<const std::uint64_t *> ptrs;
            for (const C &c : encrypteds)
            {
                if (c.size() != 2 || c.coeff_modulus_size() != k || c.poly_modulus_degree() != n)
                    throw std::invalid_argument("encrypteds is not valid for encryption parameters");
                dev.push_back(dev_in(c, words));
                ptrs.push_back(dev.back().ptr());
            }
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto *rk : relin_keys)
                raw.push_back(rk ? rk->get() : nullptr);
            Dev o = dev_out(words);
            Check chk = checked(destination); // the composite entry leaves the sink alone: the read pass notes the product
            throw_on(sealhip_evaluator_multiply_many(ctx_.get(), std::uint32_t(k), ptrs.data(), std::uint32_t(ptrs.size()), 1,
                                                     raw.data(), std::uint32_t(raw.size()), o.ptr()));
            chk.note(k, o.ptr(), 2);
            chk.done();
            take_meta(destination, encrypteds[0]);
            commit(destination, o, 2, k);
        }
        // Evaluator::exponentiate_inplace (evaluator.cpp:1257-1288)
        template <class C, IfCt<C> = 0>
        void exponentiate_inplace(C &encrypted, std::uint64_t exponent, const std::vector<const KSwitchKeys *> &relin_keys)
        {
            if (exponent == 0)
                throw std::invalid_argument("exponent cannot be 0"); // :1275-1278
            if (exponent == 1)
                return; // :1281-1284
            const std::vector<C> copies(static_cast<std::size_t>(exponent), encrypted);
            multiply_many(copies, relin_keys, encrypted);
        }

        // ---- batches: what `for (auto &ct : cts) evaluator.multiply_inplace(ct, other)` does in the reference, as one call
        // that pipelines the separately allocated ciphertexts through the device (sealhip_evaluator_multiply_host).
        // encrypted1[i] *= encrypted2[i]; with relin_keys the products come back relinearized (size 2).
        void multiply_inplace(std::vector<CT *> &encrypted1, const std::vector<const CT *> &encrypted2,
                              const std::vector<const KSwitchKeys *> *relin_keys = nullptr)
        {
            const std::size_t count = encrypted1.size();
            if (count != encrypted2.size())
                throw std::invalid_argument("encrypted1 and encrypted2 batch size mismatch");
            if (!count)
                return;
            const std::size_t k = encrypted1[0]->coeff_modulus_size(), s1 = encrypted1[0]->size(), s2 = encrypted2[0]->size();
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            for (std::size_t i = 0; i < count; i++)
            {
                check_pair(*encrypted1[i], *encrypted2[i]);
                if (encrypted1[i]->coeff_modulus_size() != k || encrypted1[i]->size() != s1 || encrypted2[i]->size() != s2)
                    throw std::invalid_argument("a batch must be uniform in level and size");
                if (bfv && (encrypted1[i]->is_ntt_form() || encrypted2[i]->is_ntt_form()))
                    throw std::invalid_argument("encrypted1 or encrypted2 cannot be in NTT form");
                if (!bfv && !(encrypted1[i]->is_ntt_form() && encrypted2[i]->is_ntt_form()))
                    throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
            }
            const std::size_t dest = s1 + s2 - 1, out_size = relin_keys && dest > 2 ? 2 : dest;
            std::vector<const sealhip_kswitch_key *> raw;
            if (relin_keys)
                for (auto *rk : *relin_keys)
                    raw.push_back(rk ? rk->get() : nullptr);
            // the results land in fresh buffers of the final size, then replace the operands' storage
            std::vector<std::vector<std::uint64_t>> res(count, std::vector<std::uint64_t>(out_size * k * ctx_.n()));
            std::vector<const std::uint64_t *> pa(count), pb(count);
            std::vector<std::uint64_t *> po(count);
            for (std::size_t i = 0; i < count; i++)
            {
                pa[i] = encrypted1[i]->data();
                pb[i] = encrypted2[i]->data();
                po[i] = res[i].data();
            }
            throw_on(sealhip_evaluator_multiply_host(ctx_.get(), std::uint32_t(k), pa.data(), std::uint32_t(s1), pb.data(),
                                                     std::uint32_t(s2), count, po.data(), relin_keys ? raw.data() : nullptr,
                                                     std::uint32_t(raw.size())));
            for (std::size_t i = 0; i < count; i++)
            {
                encrypted1[i]->resize_raw(out_size, k);
                std::copy(res[i].begin(), res[i].end(), encrypted1[i]->data());
            }
        }
        void rotate_vector_inplace(std::vector<CT *> &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (encrypted.empty() || steps == 0)
                return;
            const std::size_t k = encrypted[0]->coeff_modulus_size();
            std::vector<std::uint64_t *> p;
            for (CT *ct : encrypted)
            {
                if (ct->size() != 2 || ct->coeff_modulus_size() != k)
                    throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
                p.push_back(ct->data());
            }
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> keys;
            for (auto &kv : galois_keys)
            {
                elts.push_back(kv.first);
                keys.push_back(kv.second ? kv.second->get() : nullptr);
            }
            throw_on(sealhip_evaluator_rotate_vector_host(ctx_.get(), std::uint32_t(k), p.data(), p.size(), steps, elts.data(),
                                                          keys.data(), std::uint32_t(elts.size())));
        }

        // The vector entries above read / write the ciphertexts' own buffers; a pool block (mempool.cpp:45,145) pinned here
        // once lets the DMA engine do that in place (sealhip_host_register). Unregister before freeing.
        void register_pool_block(void *ptr, std::size_t bytes)
        {
            throw_on(sealhip_host_register(ctx_.get(), ptr, bytes));
        }
        void unregister_pool_block(void *ptr)
        {
            throw_on(sealhip_host_unregister(ctx_.get(), ptr));
        }

        // ---- the rest of the Evaluator surface
        // Evaluator::negate_inplace (evaluator.cpp:65-88)
        template <class C, IfCt<C> = 0>
        void negate_inplace(C &encrypted)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            Dev c = dev_in(encrypted, size * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_negate(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, c.ptr()));
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        // Evaluator::add_inplace (evaluator.cpp:90-151) / sub_inplace (:174-233)
        template <class C, IfCt<C> = 0>
        void add_inplace(C &encrypted1, const C &encrypted2) { add_sub(encrypted1, encrypted2, false); }
        template <class C, IfCt<C> = 0>
        void sub_inplace(C &encrypted1, const C &encrypted2) { add_sub(encrypted1, encrypted2, true); }
        // Evaluator::multiply_plain_inplace (evaluator.cpp:1438-1473). plain: NTT form -> k*N words (multiply_plain_ntt,
        // :1605-1646), coefficient form -> N coefficients below t (multiply_plain_normal, :1475-1603). Host words; the
        // resident overloads stage them through a pool block too.
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void multiply_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            if (encrypted.is_ntt_form() != plain_is_ntt_form)
                throw std::invalid_argument("NTT form mismatch"); // :1449-1452
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            const std::size_t pw = plain_is_ntt_form ? k * n : n;
            Dev c = dev_in(encrypted, size * k * n), p = dev_plain(plain, pw, plain_is_ntt_form);
            Check chk = checked(encrypted);
            throw_on((plain_is_ntt_form ? sealhip_evaluator_multiply_plain_ntt : sealhip_evaluator_multiply_plain)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, p.ptr(), 0));
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        // Evaluator::add_plain_inplace (evaluator.cpp:1290-1362) / sub_plain_inplace (:1364-1435). BFV: plain = N
        // coefficients below t, ciphertext in coefficient form; CKKS: plain = k*N words in NTT form, same level.
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void add_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            plain_linear(encrypted, plain, plain_is_ntt_form, false);
        }
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void sub_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            plain_linear(encrypted, plain, plain_is_ntt_form, true);
        }
        // the resident plaintext names its own form
        void multiply_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            multiply_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        void add_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            add_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        void sub_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            sub_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        // transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744) on a resident coefficient-form plaintext
        void transform_to_ntt(const DevicePlaintext &plain, std::size_t k, DevicePlaintext &destination_ntt)
        {
            if (plain.is_ntt_form())
                throw std::invalid_argument("plain is already in NTT form"); // :1662-1665
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context"); // :1657-1661
            const std::size_t n = ctx_.n();
            Staged o(ctx_, k * n);
            throw_on(sealhip_evaluator_transform_plain_to_ntt(ctx_.get(), std::uint32_t(k), plain.data(), plain.words(), 0, 1,
                                                              o.ptr()));
            destination_ntt.adopt(o.release(), k * n, k * n, k, true);
        }
        void transform_to_ntt_inplace(DevicePlaintext &plain, std::size_t k) { transform_to_ntt(plain, k, plain); }
        // mod_switch_to(Plaintext &, parms_id) (evaluator.cpp:1062-1088) / mod_switch_to_next (:959-994), resident
        void mod_switch_to_inplace(DevicePlaintext &plain, std::size_t target_coeff_modulus_size)
        {
            const std::size_t k = plain.coeff_modulus_size();
            if (target_coeff_modulus_size < 1 || target_coeff_modulus_size > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1071-1074
            if (!plain.is_ntt_form())
                throw std::invalid_argument("plain is not in NTT form"); // :1075-1078
            if (k < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1079-1082
            if (k == target_coeff_modulus_size)
                return;
            const std::size_t n = ctx_.n(), words = target_coeff_modulus_size * n;
            Staged o(ctx_, words);
            throw_on(sealhip_evaluator_mod_switch_plain_to(ctx_.get(), std::uint32_t(k), plain.data(), 1,
                                                           std::uint32_t(target_coeff_modulus_size), o.ptr()));
            plain.adopt(o.release(), words, words, target_coeff_modulus_size, true);
        }
        void mod_switch_to(const DevicePlaintext &plain, std::size_t target_coeff_modulus_size, DevicePlaintext &destination)
        {
            destination = plain;
            mod_switch_to_inplace(destination, target_coeff_modulus_size);
        }
        void mod_switch_to_next_inplace(DevicePlaintext &plain)
        {
            if (!plain.is_ntt_form())
                throw std::invalid_argument("plain is not in NTT form"); // :963-966
            if (plain.coeff_modulus_size() < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :967-970
            mod_switch_to_inplace(plain, plain.coeff_modulus_size() - 1);
        }
        // Evaluator::transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744), BFV, with or without fast plain lift.
        // plain: coeff_count coefficients in coefficient form (Plaintext::coeff_count()); destination_ntt: k*N words, the
        // plaintext at level k (k primes) in NTT form, ready for multiply_plain on an NTT-form ciphertext of that level.
        void transform_to_ntt(const std::uint64_t *plain, std::size_t coeff_count, std::size_t k, std::uint64_t *destination_ntt)
        {
            check_plain(plain, coeff_count);
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context"); // :1657-1661
            const std::size_t n = ctx_.n();
            Staged p(ctx_, coeff_count ? coeff_count : 1), o(ctx_, k * n);
            if (coeff_count)
                p.up(plain, coeff_count);
            throw_on(sealhip_evaluator_transform_plain_to_ntt(ctx_.get(), std::uint32_t(k), p.ptr(), coeff_count, 0, 1, o.ptr()));
            o.down(destination_ntt, k * n);
        }
        // transform_to_ntt_inplace(Plaintext &, parms_id): plain holds plain.size() coefficients and is resized to k*N words
        // like Plaintext::resize (:1682-1683); is_ntt_form plays Plaintext::is_ntt_form() and is set on success.
        void transform_to_ntt_inplace(std::vector<std::uint64_t> &plain, std::size_t k, bool &is_ntt_form)
        {
            check_plain(plain.data(), plain.size());
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context");
            if (is_ntt_form)
                throw std::invalid_argument("plain is already in NTT form"); // :1662-1665
            std::vector<std::uint64_t> out(k * ctx_.n());
            transform_to_ntt(plain.data(), plain.size(), k, out.data());
            plain.swap(out);
            is_ntt_form = true;
        }
        // Evaluator::mod_switch_to_inplace(Plaintext &, parms_id) (evaluator.cpp:1062-1088) on an NTT-form plaintext of
        // plain.size() / N primes: the leading target_coeff_modulus_size rows stay (mod_switch_drop_to_next, :959-994).
        void mod_switch_to_inplace(std::vector<std::uint64_t> &plain, bool is_ntt_form, std::size_t target_coeff_modulus_size)
        {
            const std::size_t k = plain_level(plain);
            if (target_coeff_modulus_size < 1 || target_coeff_modulus_size > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1071-1074
            if (!is_ntt_form)
                throw std::invalid_argument("plain is not in NTT form"); // :1075-1078
            if (k < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1079-1082
            if (k == target_coeff_modulus_size)
                return;
            const std::size_t n = ctx_.n();
            Staged in(ctx_, k * n), out(ctx_, target_coeff_modulus_size * n);
            in.up(plain.data(), k * n);
            throw_on(sealhip_evaluator_mod_switch_plain_to(ctx_.get(), std::uint32_t(k), in.ptr(), 1,
                                                           std::uint32_t(target_coeff_modulus_size), out.ptr()));
            plain.resize(target_coeff_modulus_size * n);
            out.down(plain.data(), target_coeff_modulus_size * n);
        }
        void mod_switch_to(const std::vector<std::uint64_t> &plain, bool is_ntt_form, std::size_t target_coeff_modulus_size,
                           std::vector<std::uint64_t> &destination)
        {
            destination = plain;
            mod_switch_to_inplace(destination, is_ntt_form, target_coeff_modulus_size);
        }
        // Evaluator::mod_switch_to_next_inplace(Plaintext &) (evaluator.h:430-438, evaluator.cpp:959-994)
        void mod_switch_to_next_inplace(std::vector<std::uint64_t> &plain, bool is_ntt_form)
        {
            const std::size_t k = plain_level(plain);
            if (!is_ntt_form)
                throw std::invalid_argument("plain is not in NTT form"); // :963-966
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :967-970
            mod_switch_to_inplace(plain, true, k - 1);
        }
        void mod_switch_to_next(const std::vector<std::uint64_t> &plain, bool is_ntt_form, std::vector<std::uint64_t> &destination)
        {
            destination = plain;
            mod_switch_to_next_inplace(destination, is_ntt_form);
        }
        // Ciphertext::is_transparent (ciphertext.h:471-476) evaluated on the device copy
        template <class C, IfCt<C> = 0>
        bool is_transparent(const C &encrypted)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            Dev c = dev_in(encrypted, size * k * n);
            std::uint8_t flag = 0;
            throw_on(sealhip_is_transparent(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, &flag));
            return flag != 0;
        }

    private:
        // The words of an operand on the device for one call: a host ciphertext is staged through a pool block (up, and
        // down again for an in-place result), a resident one is its own block.
        struct Dev
        {
            std::unique_ptr<Staged> st;
            std::uint64_t *p = nullptr;
            std::uint64_t *ptr() const { return p; }
        };
        Dev dev_in(const CT &c, std::size_t words)
        {
            Dev d;
            d.st.reset(new Staged(ctx_, words));
            d.st->up(c.data(), words);
            d.p = d.st->ptr();
            return d;
        }
        Dev dev_in(const DeviceCiphertext &c, std::size_t)
        {
            Dev d;
            d.p = const_cast<std::uint64_t *>(c.data());
            return d;
        }
        Dev dev_plain(const std::uint64_t *plain, std::size_t words, bool)
        {
            Dev d;
            d.st.reset(new Staged(ctx_, words));
            d.st->up(plain, words);
            d.p = d.st->ptr();
            return d;
        }
        Dev dev_plain(const DevicePlaintext &plain, std::size_t words, bool ntt_form)
        {
            if (plain.is_ntt_form() != ntt_form || plain.words() != words)
                throw std::invalid_argument("plain is not valid for encryption parameters");
            Dev d;
            d.p = const_cast<std::uint64_t *>(plain.data());
            return d;
        }
        Dev dev_out(std::size_t words)
        {
            Dev d;
            d.st.reset(new Staged(ctx_, words));
            d.p = d.st->ptr();
            return d;
        }
        void dev_back(CT &c, Dev &d, std::size_t words) { d.st->down(c.data(), words); }
        void dev_back(DeviceCiphertext &, Dev &, std::size_t) {}
        // the result of `size` polynomials at level k in `o` replaces the operand's words
        void commit(CT &c, Dev &o, std::size_t size, std::size_t k)
        {
            c.resize_raw(size, k);
            o.st->down(c.data(), size * k * ctx_.n());
        }
        void commit(DeviceCiphertext &c, Dev &o, std::size_t size, std::size_t k)
        {
            const std::size_t words = o.st->words();
            c.adopt(o.st->release(), words, size, k);
        }
        // the destination takes the metadata of `src` (host: as the whole object, like before)
        void take_meta(CT &dst, const CT &src) { dst = src; }
        void take_meta(DeviceCiphertext &dst, const DeviceCiphertext &src) { dst.copy_meta(src); }
        // fewer polynomials at the same level, the leading words kept (relinearize)
        void shrink(CT &c, std::size_t size) { c.resize_raw(size, c.coeff_modulus_size()); }
        void shrink(DeviceCiphertext &c, std::size_t size) { c.set_size(size); }

        // The deferred transparency check of one resident result (see the class comment): a slot of this Evaluator's ring
        // is the lane's sink while the operation runs; none is left installed afterwards. Inert for host operands.
        class Check
        {
        public:
            Check() = default;
            Check(const Context &c, const void *owner, std::size_t count = 1) : c_(&c), owner_(owner), count_(count)
            {
                std::uint32_t *slot = c.transparency_slot(owner, count);
                const long hr = sealhip_transparency_sink(c.get(), slot, count);
                if (hr != SEALHIP_S_OK)
                {
                    c.transparency_unslot(owner, count);
                    c_ = nullptr;
                    throw_on(hr);
                }
            }
            Check(const Check &) = delete;
            Check &operator=(const Check &) = delete;
            // entries that leave the sink alone: the read pass over their result
            void note(std::size_t k, const std::uint64_t *ct, std::size_t size)
            {
                if (c_)
                    throw_on(sealhip_transparency_note(c_->get(), std::uint32_t(k), ct, std::uint32_t(size), 1));
            }
            void done() { ok_ = true; }
            ~Check()
            {
                if (!c_)
                    return;
                (void)sealhip_transparency_sink(c_->get(), nullptr, 0);
                if (!ok_)
                    c_->transparency_unslot(owner_, count_);
            }

        private:
            const Context *c_ = nullptr;
            const void *owner_ = nullptr;
            std::size_t count_ = 1;
            bool ok_ = false;
        };
        Check checked(const CT &, std::size_t = 1) { return Check(); }
        Check checked(const DeviceCiphertext &, std::size_t count = 1) { return Check(ctx_, this, count); }

        // the second operand of an RGSW operation: the first one's size, level and form
        template <class C>
        void check_rgsw_pair(const C &first, const C &other) const
        {
            if (other.size() != 2 || other.coeff_modulus_size() != first.coeff_modulus_size() ||
                other.is_ntt_form() != first.is_ntt_form())
                throw std::invalid_argument("encrypted operands differ in size, level or form");
        }
        // an operand's words into a block that gathers several
        void gather_words(const CT &c, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_h2d(ctx_.get(), dst, c.data(), words * 8));
        }
        void gather_words(const DeviceCiphertext &c, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_d2d(ctx_.get(), dst, c.data(), words * 8));
        }
        // an operand's metadata, detached from its words (a host ciphertext is its own metadata)
        CT meta_of(const CT &c) { return c; }
        DeviceCiphertext meta_of(const DeviceCiphertext &c)
        {
            DeviceCiphertext m(ctx_);
            m.copy_meta(c);
            return m;
        }

        // One operand of in_size polynomials in, one size-2 result at level k_out out: call(in, out) is the ABI entry over
        // the two device blocks. The destination (which may be the operand) takes the operand's metadata, the result's
        // words and, where `scale` is not null, that scale, read after the call.
        template <class C, class Call>
        void to_size2(const C &encrypted, std::size_t in_size, std::size_t k_out, C &destination, const double *scale, Call call)
        {
            const std::size_t n = ctx_.n();
            Dev c = dev_in(encrypted, in_size * encrypted.coeff_modulus_size() * n), o = dev_out(2 * k_out * n);
            Check chk = checked(encrypted);
            throw_on(call(c.ptr(), o.ptr()));
            chk.done();
            take_meta(destination, encrypted);
            commit(destination, o, 2, k_out);
            if (scale)
                destination.scale() = *scale;
        }

        template <class C>
        void bootstrap_internal(const C &encrypted, const Bootstrapper &boot,
                                const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                const std::vector<const KSwitchKeys *> &relin_keys, const sealhip_kswitch_key *to_sparse,
                                const sealhip_kswitch_key *to_dense, C &destination)
        {
            check_bootstrap_operand(encrypted);
            const sealhip_kswitch_key *relin = first_relin_key(relin_keys);
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
            dft_keys(galois_keys, elts, raw);
            const std::size_t k = encrypted.coeff_modulus_size();
            to_size2(encrypted, 2, boot.out_level(), destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                if (to_sparse)
                    return sealhip_evaluator_bootstrap_encapsulated(ctx_.get(), boot.get(), std::uint32_t(k), c, 1, elts.data(),
                                                                    raw.data(), std::uint32_t(elts.size()), &relin, 1, to_sparse,
                                                                    to_dense, o);
                return sealhip_evaluator_bootstrap(ctx_.get(), boot.get(), std::uint32_t(k), c, 1, elts.data(), raw.data(),
                                                   std::uint32_t(elts.size()), &relin, 1, o);
            });
        }

        // relin_keys as relinearize_inplace takes them, of which index 0 is read: required (:793-796), or null without one
        static const sealhip_kswitch_key *first_relin_key(const std::vector<const KSwitchKeys *> &relin_keys)
        {
            if (relin_keys.empty() || !relin_keys[0])
                throw std::invalid_argument("not enough relinearization keys");
            return relin_keys[0]->get();
        }
        static const sealhip_kswitch_key *first_relin_key_or_null(const std::vector<const KSwitchKeys *> &relin_keys)
        {
            return !relin_keys.empty() && relin_keys[0] ? relin_keys[0]->get() : nullptr;
        }

        // the n results of a hoisted rotation, back to back in `o`, become the destinations (metadata of the operand)
        // (k: the level of the results when it is not the operand's -- the *_rescale methods)
        void scatter(const CT &src, Dev &o, std::size_t n, std::size_t words, std::vector<CT> &dst, std::size_t k = 0)
        {
            dst.assign(n, src);
            for (std::size_t i = 0; k && i < n; i++)
                dst[i].resize_raw(2, k);
            for (std::size_t i = 0; i < n; i++)
                throw_on(sealhip_memcpy_d2h(ctx_.get(), dst[i].data(), o.ptr() + i * words, words * 8));
        }
        void scatter(const DeviceCiphertext &src, Dev &o, std::size_t n, std::size_t words, std::vector<DeviceCiphertext> &dst,
                     std::size_t k = 0)
        {
            k = k ? k : src.coeff_modulus_size();
            std::vector<DeviceCiphertext> next;
            next.reserve(n);
            for (std::size_t i = 0; i < n; i++)
            {
                next.emplace_back(ctx_);
                if (n == 1)
                    next[i].adopt(o.st->release(), o.st->words(), 2, k);
                else
                {
                    Staged one(ctx_, words); // (each destination owns a pool block of its own)
                    throw_on(sealhip_memcpy_d2d(ctx_.get(), one.ptr(), o.ptr() + i * words, words * 8));
                    next[i].adopt(one.release(), words, 2, k);
                }
                next[i].copy_meta(src);
            }
            dst.swap(next);
        }
        // the plaintexts of apply_galois_dot_plain: a DevicePlaintext, or a host plaintext of HostPlaintext's shape
        static const std::uint64_t *plain_data(const DevicePlaintext &p) { return p.data(); }
        static std::size_t plain_words(const DevicePlaintext &p) { return p.words(); }
        static std::size_t plain_k(const DevicePlaintext &p) { return p.coeff_modulus_size(); }
        static bool plain_ntt(const DevicePlaintext &p) { return p.is_ntt_form(); }
        static double plain_scale(const DevicePlaintext &p) { return p.scale(); }
        template <class P>
        static const std::uint64_t *plain_data(const P &p) { return p.words.data(); }
        template <class P>
        static std::size_t plain_words(const P &p) { return p.words.size(); }
        template <class P>
        static std::size_t plain_k(const P &p) { return p.k; }
        template <class P>
        static bool plain_ntt(const P &p) { return p.ntt_form; }
        template <class P>
        static double plain_scale(const P &p) { return p.scale; }
        void plain_to(const DevicePlaintext &p, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_d2d(ctx_.get(), dst, p.data(), words * 8));
        }
        template <class P>
        void plain_to(const P &p, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_h2d(ctx_.get(), dst, p.words.data(), words * 8));
        }
        // every plains[s] has n_elts plaintexts in key-level NTT form; returns their common scale (CKKS; 1.0 if none)
        template <class P>
        double check_dot_plains(const std::vector<std::vector<P>> &plains, std::size_t n_elts) const
        {
            const std::size_t n_key = ctx_.n_key(), n = ctx_.n();
            bool first = true;
            double scale = 1.0;
            for (const auto &row : plains)
            {
                if (row.size() != n_elts)
                    throw std::invalid_argument("plains must hold one plaintext per Galois element in every sum");
                for (const P &p : row)
                {
                    if (!plain_ntt(p) || plain_k(p) != n_key || plain_words(p) != n_key * n)
                        throw std::invalid_argument("plain must be in NTT form at the key level");
                    if (ctx_.scheme() == SEALHIP_SCHEME_CKKS && !first && plain_scale(p) != scale)
                        throw std::invalid_argument("scale mismatch");
                    if (first)
                        scale = plain_scale(p);
                    first = false;
                }
            }
            return scale;
        }
        std::vector<std::uint32_t> elts_of_steps(const std::vector<int> &steps) const
        {
            std::vector<std::uint32_t> elts(steps.size(), 1);
            for (std::size_t i = 0; i < steps.size(); i++)
                if (steps[i] != 0)
                    throw_on(sealhip_galois_elt_from_step(ctx_.get(), steps[i], &elts[i]));
            return elts;
        }
        // apply_galois_inplace's checks on the operand (evaluator.cpp:1848-1887)
        template <class C>
        void check_galois_operand(const C &encrypted) const
        {
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            if (bfv && encrypted.is_ntt_form())
                throw std::invalid_argument("BFV encrypted cannot be in NTT form");
            if (!bfv && !encrypted.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form");
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
        }

        // what every *_rescale method adds to the unmerged method's checks
        template <class C>
        void check_rescale_operand(const C &encrypted) const
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::logic_error("unsupported scheme"); // (rescale_to_next: evaluator.cpp:1098-1101)
            if (!encrypted.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form");
            if (encrypted.coeff_modulus_size() < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :1005-1008
        }

        template <class C>
        void dot_product_internal(const std::vector<C> &a, const std::vector<C> &b, const KSwitchKeys *relin_key, C &destination,
                                  bool rescale = false)
        {
            if (a.empty() || a.size() != b.size())
                throw std::invalid_argument("encrypteds1 and encrypteds2 must hold the same, non-zero number of terms");
            for (std::size_t i = 0; i < a.size(); i++)
            {
                check_multiply(a[i], b[i]);
                if (a[i].size() != 2 || b[i].size() != 2)
                    throw std::invalid_argument("encrypted size must be 2");
                if (a[i].coeff_modulus_size() != a[0].coeff_modulus_size())
                    throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
                if (ctx_.scheme() == SEALHIP_SCHEME_CKKS && (a[i].scale() != a[0].scale() || b[i].scale() != b[0].scale()))
                    throw std::invalid_argument("scale mismatch");
            }
            if (rescale)
                check_rescale_operand(a[0]);
            const std::size_t k = a[0].coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n, size = relin_key ? 2 : 3;
            const std::size_t k_out = rescale ? k - 1 : k;
            const double scale = a[0].scale() * b[0].scale() / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
            std::vector<Dev> staged;
            std::vector<const std::uint64_t *> pa, pb;
            staged.reserve(2 * a.size());
            for (std::size_t i = 0; i < a.size(); i++)
            {
                staged.push_back(dev_in(a[i], words));
                pa.push_back(staged.back().ptr());
                staged.push_back(dev_in(b[i], words));
                pb.push_back(staged.back().ptr());
            }
            Dev o = dev_out(size * k_out * n);
            const sealhip_kswitch_key *raw = relin_key ? relin_key->get() : nullptr;
            Check chk = checked(a[0]);
            throw_on((rescale ? sealhip_evaluator_dot_product_rescale : sealhip_evaluator_dot_product)(
                ctx_.get(), std::uint32_t(k), pa.data(), pb.data(), std::uint32_t(a.size()), 1, relin_key ? &raw : nullptr,
                relin_key ? 1u : 0u, o.ptr()));
            chk.done();
            take_meta(destination, a[0]); // (every term is staged or enqueued by now: the destination may be one of them)
            commit(destination, o, size, k_out);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                destination.scale() = scale;
        }

        // linear_combination's checks on the term list: one size, one level, the scheme's form and, for CKKS, one scale
        template <class C>
        void check_lincomb_terms(const std::vector<C> &terms, std::size_t n_weights) const
        {
            if (terms.empty() || terms.size() != n_weights)
                throw std::invalid_argument("terms and weights must hold the same, non-zero number of entries");
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            for (const C &c : terms)
            {
                if (bfv && c.is_ntt_form())
                    throw std::invalid_argument("BFV encrypted cannot be in NTT form");
                if (!bfv && !c.is_ntt_form())
                    throw std::invalid_argument("CKKS encrypted must be in NTT form");
                if (c.size() < 2 || c.size() != terms[0].size())
                    throw std::invalid_argument("terms must have one size of at least 2");
                if (c.coeff_modulus_size() != terms[0].coeff_modulus_size() || c.poly_modulus_degree() != ctx_.n())
                    throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
                if (!bfv && c.scale() != terms[0].scale())
                    throw std::invalid_argument("scale mismatch");
            }
        }
        // w: terms.size() x k canonical residues (one sum, no constant)
        template <class C>
        void linear_combination_internal(const std::vector<C> &terms, const std::vector<std::uint64_t> &w, C &destination,
                                         double scale)
        {
            const std::size_t size = terms[0].size(), k = terms[0].coeff_modulus_size(), words = size * k * ctx_.n();
            std::vector<Dev> staged;
            std::vector<const std::uint64_t *> ptrs;
            staged.reserve(terms.size());
            for (const C &c : terms)
            {
                staged.push_back(dev_in(c, words));
                ptrs.push_back(staged.back().ptr());
            }
            Staged dw(ctx_, w.size());
            dw.up(w.data(), w.size());
            Dev o = dev_out(words);
            Check chk = checked(terms[0]);
            throw_on(sealhip_evaluator_linear_combination(ctx_.get(), std::uint32_t(k), ptrs.data(), std::uint32_t(ptrs.size()),
                                                          std::uint32_t(size), 1, dw.ptr(), nullptr, 1, o.ptr()));
            chk.done();
            take_meta(destination, terms[0]); // (every term is staged or enqueued by now: the destination may be one of them)
            commit(destination, o, size, k);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                destination.scale() = scale;
        }

        // the host checks of multiply / square (evaluator.cpp:238-249, :276-279, :449-452)
        template <class C>
        void check_multiply(const C &encrypted1, const C &encrypted2) const
        {
            check_pair(encrypted1, encrypted2);
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            if (bfv && (encrypted1.is_ntt_form() || encrypted2.is_ntt_form()))
                throw std::invalid_argument("encrypted1 or encrypted2 cannot be in NTT form"); // :276-279
            if (!bfv && !(encrypted1.is_ntt_form() && encrypted2.is_ntt_form()))
                throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form"); // :449-452
        }

        // conjugate_internal (evaluator.h:1343-1363): the automorphism x -> x^(2N-1), i.e. get_elt_from_step(0)
        template <class C>
        void conjugate_internal(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            std::uint32_t elt = 0;
            throw_on(sealhip_galois_elt_from_step(ctx_.get(), 0, &elt));
            auto it = galois_keys.find(elt);
            if (it == galois_keys.end() || !it->second)
                throw std::invalid_argument("Galois key not present"); // evaluator.cpp:1871-1874
            apply_galois_inplace(encrypted, elt, *it->second);
        }
        template <class C, class P>
        void plain_linear(C &encrypted, const P &plain, bool plain_is_ntt_form, bool sub)
        {
            if (ctx_.scheme() == SEALHIP_SCHEME_BFV && encrypted.is_ntt_form())
                throw std::invalid_argument("BFV encrypted cannot be in NTT form"); // :1304-1307
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS && !encrypted.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form"); // :1308-1311
            if (encrypted.is_ntt_form() != plain_is_ntt_form)
                throw std::invalid_argument("NTT form mismatch"); // :1312-1315
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            const std::size_t pw = plain_is_ntt_form ? k * n : n;
            Dev c = dev_in(encrypted, size * k * n), p = dev_plain(plain, pw, plain_is_ntt_form);
            Check chk = checked(encrypted); // (the entry has no sink: the read pass notes the result)
            throw_on(sealhip_evaluator_add_plain(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, p.ptr(), pw,
                                                 sub ? 1 : 0));
            chk.note(k, c.ptr(), size);
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        template <class C>
        void add_sub(C &a, const C &b, bool sub)
        {
            if (a.poly_modulus_degree() != ctx_.n() || b.poly_modulus_degree() != ctx_.n() || a.size() < 1 || b.size() < 1)
                throw std::invalid_argument("encrypted1 is not valid for encryption parameters"); // :93-100
            if (a.coeff_modulus_size() != b.coeff_modulus_size())
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch"); // :101-104
            if (a.is_ntt_form() != b.is_ntt_form())
                throw std::invalid_argument("NTT form mismatch"); // :105-108
            const std::size_t k = a.coeff_modulus_size(), n = ctx_.n(), sa = a.size(), sb = b.size();
            const std::size_t so = sa > sb ? sa : sb;
            Dev x = dev_in(a, sa * k * n), y = dev_in(b, sb * k * n), o = dev_out(so * k * n);
            Check chk = checked(a);
            throw_on((sub ? sealhip_evaluator_sub : sealhip_evaluator_add)(ctx_.get(), std::uint32_t(k), x.ptr(),
                                                                           std::uint32_t(sa), y.ptr(), std::uint32_t(sb), 1,
                                                                           o.ptr()));
            chk.done();
            commit(a, o, so, k); // :131-132
        }
        // is_valid_for(Plaintext) (valcheck.cpp:236-281) in coefficient form: at most N coefficients, each below t
        // (plain_modulus 0 under CKKS: no non-empty coefficient-form plaintext is valid)
        void check_plain(const std::uint64_t *plain, std::size_t coeff_count) const
        {
            if (coeff_count > ctx_.n())
                throw std::invalid_argument("plain is not valid for encryption parameters");
            for (std::size_t i = 0; i < coeff_count; i++)
                if (plain[i] >= ctx_.plain_modulus())
                    throw std::invalid_argument("plain is not valid for encryption parameters");
        }
        // level (number of primes) of an NTT-form plaintext: k*N words, 1 <= k <= n_key
        std::size_t plain_level(const std::vector<std::uint64_t> &plain) const
        {
            const std::size_t n = ctx_.n(), k = plain.size() / n;
            if (plain.size() % n != 0 || k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("plain is not valid for encryption parameters");
            return k;
        }
        template <class C>
        void check_pair(const C &a, const C &b) const
        {
            if (a.poly_modulus_degree() != ctx_.n() || b.poly_modulus_degree() != ctx_.n() || a.size() < 2 || b.size() < 2)
                throw std::invalid_argument("encrypted1 is not valid for encryption parameters"); // :238-245
            if (a.coeff_modulus_size() != b.coeff_modulus_size())
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch"); // :246-249
        }
        template <class C>
        void switch_level(C &ct, bool rescale)
        {
            const std::size_t k = ct.coeff_modulus_size(), n = ctx_.n(), size = ct.size();
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :1005-1008
            Dev c = dev_in(ct, size * k * n), o = dev_out(size * (k - 1) * n);
            Check chk = checked(ct);
            throw_on((rescale ? sealhip_evaluator_rescale_to_next : sealhip_evaluator_mod_switch_to_next)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, o.ptr()));
            chk.done();
            commit(ct, o, size, k - 1); // :879
        }
        template <class C>
        void transform(C &ct, bool to_ntt)
        {
            const std::size_t k = ct.coeff_modulus_size(), n = ctx_.n(), size = ct.size();
            Dev c = dev_in(ct, size * k * n);
            Check chk = checked(ct); // (the transforms have no sink: the read pass notes the result)
            throw_on((to_ntt ? sealhip_evaluator_transform_to_ntt : sealhip_evaluator_transform_from_ntt)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1));
            chk.note(k, c.ptr(), size);
            chk.done();
            dev_back(ct, c, size * k * n);
        }
        const Context &ctx_;
    };

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
        void decrypt(const CT &encrypted, std::vector<std::uint64_t> &destination)
        {
            std::vector<std::vector<std::uint64_t>> out;
            decrypt(std::vector<const CT *>{ &encrypted }, out);
            destination.swap(out[0]);
        }
        void decrypt(const std::vector<const CT *> &encrypted, std::vector<std::vector<std::uint64_t>> &destination)
        {
            decrypt_impl(encrypted, destination);
        }
        void decrypt(const DeviceCiphertext &encrypted, std::vector<std::uint64_t> &destination)
        {
            std::vector<std::vector<std::uint64_t>> out;
            decrypt_impl(std::vector<const DeviceCiphertext *>{ &encrypted }, out);
            destination.swap(out[0]);
        }
        void decrypt(const std::vector<const DeviceCiphertext *> &encrypted, std::vector<std::vector<std::uint64_t>> &destination)
        {
            decrypt_impl(encrypted, destination);
        }

        // invariant_noise_budget (:269-325)
        int invariant_noise_budget(const CT &encrypted)
        {
            return invariant_noise_budget(std::vector<const CT *>{ &encrypted })[0];
        }
        std::vector<int> invariant_noise_budget(const std::vector<const CT *> &encrypted) { return budget_impl(encrypted); }
        int invariant_noise_budget(const DeviceCiphertext &encrypted)
        {
            return budget_impl(std::vector<const DeviceCiphertext *>{ &encrypted })[0];
        }
        std::vector<int> invariant_noise_budget(const std::vector<const DeviceCiphertext *> &encrypted)
        {
            return budget_impl(encrypted);
        }

    private:
        template <class C>
        void decrypt_impl(const std::vector<const C *> &encrypted, std::vector<std::vector<std::uint64_t>> &destination)
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

        template <class C>
        std::vector<int> budget_impl(const std::vector<const C *> &encrypted)
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

        // the same into resident ciphertexts: the words stay on the device (the samples still come from the samplers)
        void encrypt(const HostPlaintext &plain, DeviceCiphertext &destination)
        {
            std::vector<DeviceCiphertext *> d{ &destination };
            run(true, std::vector<const HostPlaintext *>{ &plain }, d, 0, false);
        }
        void encrypt_zero(DeviceCiphertext &destination) { encrypt_zero(k_first_, destination); }
        void encrypt_zero(std::size_t k, DeviceCiphertext &destination)
        {
            std::vector<DeviceCiphertext *> d{ &destination };
            run(true, {}, d, k, false);
        }
        void encrypt_symmetric(const HostPlaintext &plain, DeviceCiphertext &destination)
        {
            std::vector<DeviceCiphertext *> d{ &destination };
            run(false, std::vector<const HostPlaintext *>{ &plain }, d, 0, false);
        }
        void encrypt_zero_symmetric(DeviceCiphertext &destination) { encrypt_zero_symmetric(k_first_, destination); }
        void encrypt_zero_symmetric(std::size_t k, DeviceCiphertext &destination)
        {
            std::vector<DeviceCiphertext *> d{ &destination };
            run(false, {}, d, k, false);
        }

        // encrypt (:205-253) / encrypt_zero() at the first level / encrypt_zero(parms_id) at level k
        void encrypt(const HostPlaintext &plain, CT &destination) { encrypt(std::vector<const HostPlaintext *>{ &plain }, one(destination)); }
        void encrypt(const std::vector<const HostPlaintext *> &plain, std::vector<CT *> destination)
        {
            run(true, plain, destination, 0, false);
        }
        void encrypt_zero(CT &destination) { encrypt_zero(k_first_, destination); }
        void encrypt_zero(std::size_t k, CT &destination) { encrypt_zero(k, one(destination)); }
        void encrypt_zero(std::size_t k, std::vector<CT *> destination) { run(true, {}, destination, k, false); }

        // encrypt_symmetric / encrypt_zero_symmetric (rlwe.cpp:204-300)
        void encrypt_symmetric(const HostPlaintext &plain, CT &destination)
        {
            encrypt_symmetric(std::vector<const HostPlaintext *>{ &plain }, one(destination));
        }
        void encrypt_symmetric(const std::vector<const HostPlaintext *> &plain, std::vector<CT *> destination)
        {
            run(false, plain, destination, 0, false);
        }
        void encrypt_zero_symmetric(CT &destination) { encrypt_zero_symmetric(k_first_, destination); }
        void encrypt_zero_symmetric(std::size_t k, CT &destination) { encrypt_zero_symmetric(k, one(destination)); }
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
        static std::vector<CT *> one(CT &c) { return std::vector<CT *>{ &c }; }

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
            if (count == 1) // the block itself changes owner
            {
                d.adopt(ct.release(), ct.words(), 2, k);
                return;
            }
            Staged one(ctx_, words);
            throw_on(sealhip_memcpy_d2d(ctx_.get(), one.ptr(), ct.ptr() + i * words, words * 8));
            d.adopt(one.release(), words, 2, k);
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
