// api.cpp -- the C ABI of include/sealhip.h. Conventions follow the reference's C export layer
// (native/src/seal/c/defines.h:34-58, c/evaluator.cpp:39-47): null checks -> E_POINTER, C++ exceptions
// mapped to HRESULTs (invalid_argument -> E_INVALIDARG, logic_error -> COR_E_INVALIDOPERATION,
// everything else -> E_UNEXPECTED), nothing thrown across the boundary.
#include "../../include/sealhip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>
#include <cstring>
#include <new>

#include "blake2xb.hpp"
#include "engine.hpp"
#include "evalmod_plan.hpp"
#include "homdft_plan.hpp"
#include "lintrans_plan.hpp"
#include "poly_plan.hpp"

using namespace sealhip;

namespace sealhip
{
    // wire.cpp
    void wire_set_parms_id(Engine &e, int k, const std::uint64_t *id);
    void wire_peek(const void *bytes, std::size_t len, sealhip_ciphertext_info *info);
    void wire_load(Engine &e, const void *bytes, std::size_t len, sealhip_ciphertext_info *info, u64 *dst,
                   std::size_t capacity_words);
    void wire_load_many(Engine &e, const void *const *streams, const std::size_t *lens, std::size_t count,
                        sealhip_ciphertext_info *infos, u64 *dst, std::size_t stride);
    std::size_t wire_save_size(std::uint32_t size, std::uint32_t k, std::size_t n);
    std::size_t wire_save(Engine &e, const sealhip_ciphertext_info &ci, const u64 *src, void *bytes, std::size_t capacity);
    std::size_t wire_save_seeded_size(const Engine &e, const sealhip_ciphertext_info &ci);
    std::size_t wire_save_seeded(Engine &e, const sealhip_ciphertext_info &ci, const u64 *src, const std::uint64_t *seed,
                                 void *bytes, std::size_t capacity);
    std::uint32_t wire_load_kswitch_key(Engine &e, const void *bytes, std::size_t len, std::uint32_t index, u64 **d_out,
                                        std::size_t *words_out, std::uint64_t *dim1_out);
    std::size_t wire_kswitch_save_size(const Engine &e, const KSwitchKey *const *keys, std::size_t n_slots, bool seeded);
    std::vector<u64> wire_expand_seed(const Engine &e, int rows, const unsigned char *seed_bytes);
    std::size_t wire_save_kswitch_keys(Engine &e, const KSwitchKey *const *keys, std::size_t n_slots, void *bytes,
                                       std::size_t capacity, bool seeded);
} // namespace sealhip

struct sealhip_context
{
    std::unique_ptr<Engine> engine;
};
struct sealhip_kswitch_key
{
    KSwitchKey key;
};
struct sealhip_rgsw
{
    RgswKey key;
};
struct sealhip_graph
{
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    Lane *lane = nullptr;                  // the lane it was captured on (its arena addresses are baked in)
    unsigned long long generation = 0;     // Lane::alloc_generation at capture
    unsigned long long key_generation = 0; // Engine::key_generation at capture (key addresses are baked in too)
    unsigned long long pool_id = 0;        // LanePool::id of the context it belongs to (checked at launch)
};

namespace
{
    thread_local std::string g_last_error;

    long fail(long code, const std::string &msg)
    {
        g_last_error = msg;
        return code;
    }

    // Entry points may be called concurrently from several host threads on one context (the reference's Evaluator is
    // re-entrant, evaluator.h:1375-1377): every thread works on its own lane (stream + arena, engine.hpp). An operation
    // holds its lane's lock until it returns; that lock is only ever contended when a graph captured on one thread is
    // launched from another.
    struct OpLock
    {
        Engine *engine;
        std::unique_lock<std::recursive_mutex> lock;
        explicit OpLock(Engine &e) : engine(&e), lock(e.lane().busy)
        {}
    };
    thread_local std::vector<std::unique_ptr<OpLock>> g_locks;
    struct LockScope
    {
        std::size_t depth = g_locks.size();
        ~LockScope()
        {
            while (g_locks.size() > depth)
                g_locks.pop_back();
        }
    };

    // An operation that fails while its lane is capturing a graph leaves the stream in capture mode and the graph
    // half-built: end the capture, drop the graph and say so (the caller must not call _capture_end for it).
    std::string abort_capture_if_any()
    {
        if (g_locks.empty())
            return "";
        Engine &e = *g_locks.back()->engine;
        Lane &l = e.lane();
        if (!l.capturing)
            return "";
        l.capturing = false;
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(l.stream, &g);
        if (g)
            (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return " (the graph capture in progress on this thread was aborted and discarded)";
    }

    template <class F>
    long guarded(F &&body)
    {
        LockScope scope;
        try
        {
            body();
            return SEALHIP_S_OK;
        }
        catch (const HipError &err)
        {
            const std::string note = abort_capture_if_any();
            return fail(err.code == hipErrorOutOfMemory ? SEALHIP_E_OUTOFMEMORY : SEALHIP_E_UNEXPECTED, err.what() + note);
        }
        catch (const std::invalid_argument &err)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_E_INVALIDARG, err.what() + note);
        }
        catch (const std::out_of_range &err)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_E_INVALIDARG, err.what() + note);
        }
        catch (const std::logic_error &err)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_COR_E_INVALIDOPERATION, err.what() + note);
        }
        catch (const std::bad_alloc &)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_E_OUTOFMEMORY, "out of host memory" + note);
        }
        catch (const std::exception &err)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_E_UNEXPECTED, err.what() + note);
        }
        catch (...)
        {
            const std::string note = abort_capture_if_any();
            return fail(SEALHIP_E_UNEXPECTED, "unknown error" + note);
        }
    }

#define REQUIRE_PTR(p)                                             \
    do                                                             \
    {                                                              \
        if (!(p))                                                  \
            return fail(SEALHIP_E_POINTER, #p " is null");         \
    } while (0)

// The pointer checks of the key lists, by the parameter names every entry uses. A Galois list of n entries (an empty one
// may be null): the two arrays alone (the rotate_vector entries look keys up by step); every key as well; every key but
// those of element 1, the identity, which needs none. The relinearization list: required, or optional (null = no key).
#define REQUIRE_GALOIS_LIST(n)        \
    do                                \
    {                                 \
        if (n)                        \
        {                             \
            REQUIRE_PTR(galois_elts); \
            REQUIRE_PTR(galois_keys); \
        }                             \
    } while (0)
#define REQUIRE_GALOIS_KEYS_WHERE(n, needed)  \
    do                                       \
    {                                        \
        REQUIRE_GALOIS_LIST(n);              \
        for (uint32_t i = 0; i < (n); i++)   \
            if (needed)                      \
                REQUIRE_PTR(galois_keys[i]); \
    } while (0)
#define REQUIRE_GALOIS_KEYS(n) REQUIRE_GALOIS_KEYS_WHERE(n, true)
#define REQUIRE_GALOIS_KEYS_BUT_IDENTITY(n) REQUIRE_GALOIS_KEYS_WHERE(n, galois_elts[i] != 1)
#define REQUIRE_RELIN_KEYS_IF_ANY()         \
    do                                      \
    {                                       \
        if (relin_keys && n_relin_keys)     \
            REQUIRE_PTR(relin_keys[0]);     \
    } while (0)
#define REQUIRE_RELIN_KEYS()         \
    do                               \
    {                                \
        REQUIRE_PTR(relin_keys);     \
        REQUIRE_RELIN_KEYS_IF_ANY(); \
    } while (0)

    Engine &device_engine(sealhip_context *ctx)
    {
        Engine &e = *ctx->engine;
        if (e.device < 0)
            throw std::logic_error("host-only context: there is no CPU fallback, create the context on a HIP device");
        (void)hipGetLastError(); // an error an earlier call already reported must not be attributed to this one's launches
        SEALHIP_CHECK(hipSetDevice(e.device));
        g_locks.push_back(std::make_unique<OpLock>(e));
        return e;
    }

    // The rules the entries share. A new entry calls these; it does not restate them.
    // any level up to the key level (k data primes or all n_key key primes): the low-level entries
    void check_level(const Engine &e, uint32_t k)
    {
        if (k < 1 || static_cast<int>(k) > e.n_key)
            throw std::invalid_argument("level k out of range");
    }

    // a ciphertext level, 1 .. first data level: the Evaluator entries that check before they need a device
    void check_data_level(const Engine &h, uint32_t k)
    {
        if (k < 1 || static_cast<int>(k) > h.k_first)
            throw std::invalid_argument("level k out of range");
    }

    // the first checks of every *_rescale entry, ahead of the unmerged entry's own: CKKS only, 2 <= k <= first level
    void check_rescale_level(const Engine &h, uint32_t k)
    {
        if (h.scheme != 2)
            throw std::invalid_argument("the merged rescale is CKKS only");
        check_data_level(h, k);
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached"); // evaluator.cpp:1005-1008
    }

    uint32_t kswitch_digits(const Engine &h, uint32_t k)
    {
        return (k + h.nsp - 1) / h.nsp; // decomposition digits of a key switch at level k, keygenerator.cpp:334-336
    }

    void check_key_digits(const Engine &h, uint32_t k, const sealhip_kswitch_key *key)
    {
        // (a switching key made for levels <= key.level has zero rows above it)
        if (key->key.n_digits < kswitch_digits(h, k) || (key->key.level && k > key->key.level))
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
    }

    // the key of sk^2, checked; the caller asks only when it needs one (a null list may mean "leave the result at size 3")
    const KSwitchKey *first_relin_key(const Engine &h, uint32_t k, const sealhip_kswitch_key *const *relin_keys,
                                      uint32_t n_relin_keys)
    {
        if (!relin_keys || n_relin_keys == 0)
            throw std::invalid_argument("not enough relinearization keys"); // evaluator.cpp:793-796
        check_key_digits(h, k, relin_keys[0]);
        return &relin_keys[0]->key;
    }

    void check_galois_elt(const Engine &h, uint32_t elt)
    {
        if (!(elt & 1) || elt >= 2 * h.n)
            throw std::invalid_argument("Galois element is not valid"); // evaluator.cpp:1880-1883
    }

    bool words_overlap(const u64 *a, std::size_t a_words, const u64 *b, std::size_t b_words)
    {
        return a < b + b_words && b < a + a_words;
    }

    void ntt_entry(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k, uint32_t base, bool inverse,
                   int flags)
    {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (base == SEALHIP_BASE_BSK || base == SEALHIP_BASE_KEY)
            (void)e.level(static_cast<int>(k));
        const RowMap map = e.map_for(static_cast<int>(k), base);
        check(launch_ntt(e, reinterpret_cast<u64 *>(data), count * map.rows, map, inverse, flags), "ntt");
    }

    void poly_entry(sealhip_context *ctx, PolyOp op, const uint64_t *a, const uint64_t *b, uint64_t scalar,
                    uint64_t *r, size_t count, uint32_t k, uint32_t base)
    {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        const RowMap map = e.map_for(static_cast<int>(k), base);
        check(launch_poly_op(e, op, reinterpret_cast<const u64 *>(a), reinterpret_cast<const u64 *>(b), scalar,
                             reinterpret_cast<u64 *>(r), count * map.rows, map),
              "poly op");
    }

    // GaloisTool::get_elt_from_step (galois.cpp:49-91), generator 5 (util/galois.h:169)
    std::uint32_t host_galois_elt_from_step(std::size_t n_, int step)
    {
        const uint32_t n = static_cast<uint32_t>(n_);
        const uint64_t m = static_cast<uint64_t>(n) * 2;
        if (step == 0)
            return static_cast<uint32_t>(m - 1);
        const bool negative = step < 0;
        const uint32_t pos = static_cast<uint32_t>(negative ? -static_cast<int64_t>(step) : step);
        if (pos >= (n >> 1))
            throw std::invalid_argument("step count too large");
        uint32_t s = negative ? (n >> 1) - pos : pos;
        uint64_t elt = 1;
        while (s--)
            elt = (elt * 5) & (m - 1);
        return static_cast<uint32_t>(elt);
    }

    // steps -> elements and their keys out of the caller's key list; step 0 gets `identity` (evaluator.cpp:1958-1962) and no key
    void keys_for_steps(const Engine &h, const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                        const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, uint32_t identity,
                        std::vector<uint32_t> &elts, std::vector<const sealhip_kswitch_key *> &keys)
    {
        elts.assign(n_steps, identity);
        keys.assign(n_steps, nullptr);
        for (uint32_t s = 0; s < n_steps; s++)
        {
            if (steps[s] == 0)
                continue;
            elts[s] = host_galois_elt_from_step(h.n, steps[s]);
            for (uint32_t i = 0; i < n_keys && !keys[s]; i++)
                if (galois_elts[i] == elts[s])
                    keys[s] = galois_keys[i];
            if (!keys[s])
                throw std::invalid_argument("Galois key not present");
        }
    }

    // the pipelines' key list: null where the element is the identity
    std::vector<const KSwitchKey *> run_keys(const std::vector<uint32_t> &elts, const std::vector<const sealhip_kswitch_key *> &keys,
                                             uint32_t identity)
    {
        std::vector<const KSwitchKey *> r(elts.size(), nullptr);
        for (size_t i = 0; i < elts.size(); i++)
            if (elts[i] != identity)
                r[i] = &keys[i]->key;
        return r;
    }

    LevelTools &bfv_level(Engine &e, uint32_t k)
    {
        check_level(e, k);
        if (e.scheme != 1)
            throw std::logic_error("unsupported operation for scheme type");
        return e.level(static_cast<int>(k));
    }
} // namespace

extern "C" {

const char *sealhip_last_error_string(void)
{
    return g_last_error.c_str();
}

long sealhip_num_devices(int32_t *count)
{
    REQUIRE_PTR(count);
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    *count = err == hipSuccess ? n : 0;
    return SEALHIP_S_OK;
}

long sealhip_context_create(const sealhip_params *params, sealhip_context **out)
{
    REQUIRE_PTR(params);
    REQUIRE_PTR(out);
    REQUIRE_PTR(params->key_moduli);
    *out = nullptr;
    return guarded([&] {
        if (params->mode != SEALHIP_MODE_PARITY && params->mode != SEALHIP_MODE_STRICT)
            throw std::invalid_argument("unknown mode");
        if (params->device >= 0)
        {
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess || params->device >= n)
                throw HipError(hipErrorNoDevice, "no such HIP device (the engine has no CPU fallback)");
        }
        auto ctx = std::make_unique<sealhip_context>();
        ctx->engine = make_engine(static_cast<int>(params->scheme), static_cast<int>(params->log_n),
                                  reinterpret_cast<const u64 *>(params->key_moduli),
                                  static_cast<int>(params->n_key_moduli), static_cast<int>(params->n_special_primes),
                                  params->plain_modulus, params->mode == SEALHIP_MODE_STRICT, params->device);
        *out = ctx.release();
    });
}

long sealhip_context_destroy(sealhip_context *ctx)
{
    REQUIRE_PTR(ctx);
    return guarded([&] { delete ctx; });
}

long sealhip_context_first_level(const sealhip_context *ctx, uint32_t *k_first)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(k_first);
    *k_first = static_cast<uint32_t>(ctx->engine->k_first);
    return SEALHIP_S_OK;
}

long sealhip_context_bsk_size(sealhip_context *ctx, uint32_t k, uint32_t *bsk_size)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(bsk_size);
    return guarded([&] {
        Engine &e = *ctx->engine;
        check_level(e, k);
        if (e.scheme != 1)
            throw std::logic_error("base Bsk exists only for BFV");
        *bsk_size = static_cast<uint32_t>(e.level_host(static_cast<int>(k)).map_bsk.rows);
    });
}

namespace
{
    void adopt_stream(Engine &e, hipStream_t stream, bool own)
    {
        Lane &l = e.lane();
        if (l.capturing)
            throw std::logic_error("a graph capture is in progress on this thread");
        SEALHIP_CHECK(hipStreamSynchronize(l.stream));
        if (l.own_stream)
            SEALHIP_CHECK(hipStreamDestroy(l.stream));
        l.stream = stream;
        l.own_stream = own;
    }
} // namespace

long sealhip_set_stream(sealhip_context *ctx, void *hip_stream)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (hip_stream)
            adopt_stream(e, static_cast<hipStream_t>(hip_stream), false);
        else if (!e.lane().own_stream)
        {
            hipStream_t s = nullptr;
            SEALHIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            adopt_stream(e, s, true);
        }
    });
}

long sealhip_use_default_stream(sealhip_context *ctx)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        adopt_stream(e, nullptr, false); // the legacy NULL stream: ordered against every blocking stream of the device
    });
}

long sealhip_synchronize(sealhip_context *ctx)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true);
    });
}

long sealhip_context_lane_count(sealhip_context *ctx, uint32_t *lanes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(lanes);
    return guarded([&] {
        Engine &e = *ctx->engine;
        *lanes = 0;
        if (e.lanes)
        {
            std::lock_guard<std::mutex> lock(e.lanes->mu);
            *lanes = static_cast<uint32_t>(e.lanes->all.size());
        }
    });
}

long sealhip_debug_ntt_handoff(sealhip_context *ctx, uint32_t spin_limit, int32_t suppress_signal)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true);
        e.ntt_spin_limit = spin_limit ? spin_limit : (1u << 24);
        e.ntt_suppress_signal = suppress_signal != 0;
    });
}

long sealhip_debug_chunk_log(sealhip_context *ctx, size_t *count_chunk_pairs, size_t capacity_pairs, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(count_chunk_pairs);
    REQUIRE_PTR(written);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        auto &log = e.lane().chunk_log;
        std::size_t n = 0;
        for (; n < log.size() && n < capacity_pairs; n++)
        {
            count_chunk_pairs[2 * n] = log[n].first;
            count_chunk_pairs[2 * n + 1] = log[n].second;
        }
        *written = n;
        log.clear();
    });
}

long sealhip_debug_butterfly_rate(sealhip_context *ctx, uint32_t kind, uint32_t prime_index, double *butterflies_per_s)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(butterflies_per_s);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true);
        const hipError_t err = ntt_butterfly_rate(e, static_cast<int>(kind), static_cast<int>(prime_index), butterflies_per_s);
        if (err == hipErrorInvalidValue)
            throw std::invalid_argument("butterfly_rate: kind 0..5, a prime of the context (kind 3: one below 2^50)");
        SEALHIP_CHECK(err);
    });
}

long sealhip_malloc(sealhip_context *ctx, size_t bytes, void **dptr)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dptr);
    return guarded([&] {
        device_engine(ctx);
        SEALHIP_CHECK(hipMalloc(dptr, bytes ? bytes : 1));
    });
}

long sealhip_free(sealhip_context *ctx, void *dptr)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
        SEALHIP_CHECK(hipFree(dptr));
    });
}

long sealhip_memcpy_h2d(sealhip_context *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dst_dev);
    REQUIRE_PTR(src_host);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SEALHIP_CHECK(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, e.lane().stream));
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
    });
}

long sealhip_memcpy_d2h(sealhip_context *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dst_host);
    REQUIRE_PTR(src_dev);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SEALHIP_CHECK(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, e.lane().stream));
        e.sync_and_check(); // results become host-visible here: a failed launch must not return S_OK
    });
}

long sealhip_pool_alloc(sealhip_context *ctx, size_t bytes, void **dptr)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dptr);
    *dptr = nullptr;
    return guarded([&] {
        if (bytes == 0 || bytes > kPoolMaxBytes)
            throw std::invalid_argument("pool block size out of range (1 byte .. 2^46 bytes)");
        *dptr = pool_alloc(device_engine(ctx), bytes);
    });
}

long sealhip_pool_release(sealhip_context *ctx, void *dptr)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dptr);
    return guarded([&] {
        pool_check_held(*ctx->engine, dptr); // (a host-only context never handed a block out)
        pool_release(device_engine(ctx), dptr);
    });
}

long sealhip_pool_trim(sealhip_context *ctx)
{
    REQUIRE_PTR(ctx);
    return guarded([&] { pool_trim(device_engine(ctx)); });
}

long sealhip_pool_stats(sealhip_context *ctx, struct sealhip_pool_stats *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    return guarded([&] {
        DevicePool &P = *ctx->engine->pool;
        std::lock_guard<std::mutex> lock(P.mu);
        out->bytes_in_use = P.in_use;
        out->bytes_cached = P.cached;
        out->device_mallocs = P.mallocs;
        out->device_frees = P.frees;
        out->hits = P.hits;
        out->misses = P.misses;
        out->cross_lane_hits = P.cross_lane_hits;
    });
}

long sealhip_memcpy_d2d(sealhip_context *ctx, void *dst_dev, const void *src_dev, size_t bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dst_dev);
    REQUIRE_PTR(src_dev);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (bytes && dst_dev != src_dev)
            SEALHIP_CHECK(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, e.lane().stream));
    });
}

long sealhip_profile_enable(sealhip_context *ctx, int32_t enable)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.lane().prof_on = enable != 0;
    });
}

long sealhip_profile_fetch(sealhip_context *ctx, char *json, size_t capacity)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(json);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check();
        struct Agg
        {
            std::size_t launches = 0;
            double ms = 0, units = 0;
        };
        std::map<std::string, Agg> agg;
        for (ProfRecord &r : e.lane().prof)
        {
            float ms = 0;
            if (r.start && r.stop && hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess)
            {
                Agg &a = agg[r.tag];
                a.launches++;
                a.ms += ms;
                a.units += r.units;
            }
            if (r.start)
                (void)hipEventDestroy(r.start);
            if (r.stop)
                (void)hipEventDestroy(r.stop);
        }
        e.lane().prof.clear();
        std::string out = "{";
        bool first = true;
        for (auto &kv : agg)
        {
            char buf[256];
            std::snprintf(buf, sizeof(buf), "%s\"%s\": {\"launches\": %zu, \"ms\": %.6f, \"units\": %.0f}",
                          first ? "" : ", ", kv.first.c_str(), kv.second.launches, kv.second.ms, kv.second.units);
            out += buf;
            first = false;
        }
        out += "}";
        if (out.size() + 1 > capacity)
            throw std::invalid_argument("capacity too small");
        std::memcpy(json, out.c_str(), out.size() + 1);
    });
}

long sealhip_debug_ntt_table(sealhip_context *ctx, uint32_t prime_index, uint32_t kind, uint64_t *out_host,
                             size_t capacity)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out_host);
    return guarded([&] {
        Engine &e = *ctx->engine;
        if (static_cast<int>(prime_index) >= e.n_primes() || kind > 3)
            throw std::invalid_argument("table index out of range");
        if (capacity < e.n)
            throw std::invalid_argument("capacity too small");
        const HostNttTables &tb = e.tables[prime_index];
        if (tb.fwd.empty())
            throw std::invalid_argument("this prime has no NTT tables");
        const std::vector<u64> v = tb.reference_table(static_cast<int>(kind));
        std::memcpy(out_host, v.data(), v.size() * sizeof(u64));
    });
}

long sealhip_debug_rns_constants(sealhip_context *ctx, uint32_t k, uint32_t which, uint64_t *out_host,
                                 size_t capacity, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out_host);
    REQUIRE_PTR(written);
    return guarded([&] {
        Engine &e = *ctx->engine;
        check_level(e, k);
        const HostRnsTool &r = *e.level_host(static_cast<int>(k)).host_rns;
        std::vector<u64> v;
        switch (which)
        {
        case 0: v = r.Bsk; break;
        case 1: v = r.inv_prod_q_mod_Bsk; break;
        case 2: v = r.prod_q_mod_Bsk; break;
        case 3: v = r.inv_m_tilde_mod_Bsk; break;
        case 4: v = r.prod_B_mod_q; break;
        case 5: v = r.inv_q_last_mod_q; break;
        case 6: v = { r.inv_prod_q_mod_m_tilde, r.inv_prod_B_mod_m_sk, r.m_sk, r.gamma }; break;
        case 7: v = r.q_to_Bsk.matrix; break;
        case 8: v = r.B_to_q.matrix; break;
        case 9: v = r.q_to_Bsk.inv_punct; break;
        case 10: v = r.B_to_q.inv_punct; break;
        case 11: v = r.q_to_m_tilde.matrix; break;
        case 12: v = r.B_to_m_sk.matrix; break;
        default: throw std::invalid_argument("unknown constant selector");
        }
        if (capacity < v.size())
            throw std::invalid_argument("capacity too small");
        std::memcpy(out_host, v.data(), v.size() * sizeof(u64));
        *written = v.size();
    });
}

long sealhip_debug_bfv_multiply_plan(sealhip_context *ctx, uint32_t k, uint32_t size_a, uint32_t size_b, int32_t square,
                                     int32_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = *ctx->engine;
        check_level(e, k);
        if (size_a < 2 || size_b < 2 || size_a + size_b - 1 > 16) // check_multiply_args
            throw std::invalid_argument("encrypted1 or encrypted2 is not valid for encryption parameters");
        const BfvMulPlan p = plan_bfv_multiply(e, static_cast<int>(k), static_cast<int>(size_a), static_cast<int>(size_b),
                                               square != 0);
        const int32_t v[13] = { p.k, p.B, p.nB, p.square, p.redc_small, p.gather, p.defer, p.fused_tensor, p.tensor_apx,
                                p.lift_top, p.lift_kernel, p.floor_kernel, p.deferred_top };
        std::memcpy(out, v, sizeof v);
    });
}

long sealhip_debug_ks_split_last(sealhip_context *ctx, uint32_t k, size_t count, int32_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        *out = ks_split_last_plan(e, static_cast<int>(k), count) ? 1 : 0;
    });
}

long sealhip_debug_ntt_split_last(sealhip_context *ctx, uint32_t prime_index, uint32_t treatment, int32_t exact,
                                  const uint64_t *src_device, uint64_t *dst_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(src_device);
    REQUIRE_PTR(dst_device);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (prime_index >= e.key_moduli.size() || treatment > 2 || src_device == dst_device)
            throw std::invalid_argument("ntt_split_last: a key prime, treatment 0..2, distinct buffers");
        RowMap map{};
        map.rows = 1;
        map.prime[0] = static_cast<unsigned short>(prime_index);
        NttSource ns{};
        ns.base[0] = reinterpret_cast<const u64 *>(src_device);
        ns.code[0] = 0;
        ns.reduce_mode = static_cast<int>(treatment);
        const int flags = exact ? 0 : (kNttAnyRep | kNttApprox);
        if (!ntt_can_split_last(e, map, ns, flags, 1))
            throw std::invalid_argument("ntt_split_last: no instance of this form for the ring and prime");
        SEALHIP_CHECK(launch_ntt_gather(e, reinterpret_cast<u64 *>(dst_device), 1, map, ns, flags | kNttSplitLast));
    });
}

long sealhip_debug_behz_dot_split(sealhip_context *ctx, uint32_t k, int32_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = *ctx->engine;
        check_level(e, k);
        if (e.scheme != 1)
            throw std::invalid_argument("BFV contexts only");
        // with a device: what the level's tables were packed with; host-only contexts: what they would be packed with
        if (e.device >= 0)
        {
            *out = e.level(static_cast<int>(k)).h_rns.dot_split;
            return;
        }
        const HostRnsTool &r = *e.level_host(static_cast<int>(k)).host_rns;
        const u64 max_q = *std::max_element(r.q.begin(), r.q.end()), max_b = *std::max_element(r.Bsk.begin(), r.Bsk.end());
        *out = bounds::behz_select_split(static_cast<int>(k), max_q, max_b);
    });
}

/* ---------------------------------------------------------------- NTT */
long sealhip_ntt_negacyclic_harvey_lazy(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k, uint32_t base)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] { ntt_entry(ctx, data, count, k, base, false, 0); });
}
long sealhip_ntt_negacyclic_harvey(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k, uint32_t base)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] { ntt_entry(ctx, data, count, k, base, false, kNttCanonical); });
}
long sealhip_inverse_ntt_negacyclic_harvey_lazy(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k,
                                                uint32_t base)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] { ntt_entry(ctx, data, count, k, base, true, 0); });
}
long sealhip_inverse_ntt_negacyclic_harvey(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k,
                                           uint32_t base)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] { ntt_entry(ctx, data, count, k, base, true, kNttCanonical); });
}

/* ---------------------------------------------------------------- coefficient-wise */
long sealhip_dyadic_product_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count,
                                     uint32_t k, uint32_t base, uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(b);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Dyadic, a, b, 0, result, count, k, base); });
}
long sealhip_multiply_poly_scalar_coeffmod(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k,
                                           uint32_t base, uint64_t scalar, uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Scalar, a, a, scalar, result, count, k, base); });
}
long sealhip_add_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint32_t k,
                               uint32_t base, uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(b);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Add, a, b, 0, result, count, k, base); });
}
long sealhip_sub_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint32_t k,
                               uint32_t base, uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(b);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Sub, a, b, 0, result, count, k, base); });
}
long sealhip_negate_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k, uint32_t base,
                                  uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Negate, a, a, 0, result, count, k, base); });
}

/* ---------------------------------------------------------------- RNSTool */
long sealhip_fastbconv_m_tilde(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        LevelTools &lt = bfv_level(e, k);
        check(launch_fastbconv_m_tilde(e, lt.d_rns, lt.h_rns, reinterpret_cast<const u64 *>(in), k * e.n,
                                       reinterpret_cast<u64 *>(out), (lt.h_rns.nB + 1) * e.n, count),
              "fastbconv_m_tilde");
    });
}
long sealhip_sm_mrq(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        LevelTools &lt = bfv_level(e, k);
        check(launch_sm_mrq(e, lt.d_rns, lt.h_rns, reinterpret_cast<const u64 *>(in), (lt.h_rns.nB + 1) * e.n,
                            reinterpret_cast<u64 *>(out), lt.h_rns.nB * e.n, count),
              "sm_mrq");
    });
}
long sealhip_fast_floor(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        LevelTools &lt = bfv_level(e, k);
        check(launch_fast_floor(e, lt.d_rns, lt.h_rns, reinterpret_cast<const u64 *>(in),
                                (k + lt.h_rns.nB) * e.n, reinterpret_cast<u64 *>(out), lt.h_rns.nB * e.n, count,
                                0),
              "fast_floor");
    });
}
long sealhip_fastbconv_sk(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        LevelTools &lt = bfv_level(e, k);
        check(launch_fastbconv_sk(e, lt.d_rns, lt.h_rns, reinterpret_cast<const u64 *>(in), lt.h_rns.nB * e.n,
                                  reinterpret_cast<u64 *>(out), k * e.n, count),
              "fastbconv_sk");
    });
}
long sealhip_divide_and_round_q_last_inplace(sealhip_context *ctx, uint32_t k, uint64_t *data, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (k < 2)
            throw std::invalid_argument("divide_and_round_q_last needs at least two primes");
        LevelTools &lt = e.level(static_cast<int>(k));
        u64 *p = reinterpret_cast<u64 *>(data);
        check(launch_divround_bfv(e, lt.d_rns, lt.h_rns, p, k * e.n, p, k * e.n, count, static_cast<int>(k)),
              "divide_and_round_q_last");
    });
}
long sealhip_divide_and_round_q_last_ntt_inplace(sealhip_context *ctx, uint32_t k, uint64_t *data, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(data);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        op_divround_ntt_inplace(e, static_cast<int>(k), reinterpret_cast<u64 *>(data), count);
    });
}

/* ---------------------------------------------------------------- Galois */
long sealhip_galois_elt_from_step(const sealhip_context *ctx, int32_t step, uint32_t *galois_elt)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(galois_elt);
    return guarded([&] {
        *galois_elt = host_galois_elt_from_step(ctx->engine->n, step);
    });
}

static long galois_entry(sealhip_context *ctx, const uint64_t *in, size_t count, uint32_t k, uint32_t galois_elt,
                         uint64_t *out, bool ntt_form)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (in == out)
            throw std::invalid_argument("result cannot point to the same value as operand"); // galois.cpp:156-159
        check_galois_elt(e, galois_elt);
        const RowMap map = e.map_for(static_cast<int>(k), SEALHIP_BASE_Q);
        const uint32_t *table = ntt_form ? e.galois_table(galois_elt) : nullptr;
        check(launch_galois(e, reinterpret_cast<const u64 *>(in), reinterpret_cast<u64 *>(out), count * k, map,
                            galois_elt, table),
              "apply_galois");
    });
}
long sealhip_apply_galois(sealhip_context *ctx, const uint64_t *in, size_t count, uint32_t k, uint32_t galois_elt,
                          uint64_t *out)
{
    return galois_entry(ctx, in, count, k, galois_elt, out, false);
}
long sealhip_apply_galois_ntt(sealhip_context *ctx, const uint64_t *in, size_t count, uint32_t k, uint32_t galois_elt,
                              uint64_t *out)
{
    return galois_entry(ctx, in, count, k, galois_elt, out, true);
}

/* ---------------------------------------------------------------- key switch */
long sealhip_kswitch_key_load(sealhip_context *ctx, const uint64_t *key, uint32_t n_digits, int32_t from_host,
                              sealhip_kswitch_key **out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(key);
    REQUIRE_PTR(out);
    *out = nullptr;
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (n_digits == 0 || n_digits > kswitch_digits(e, static_cast<uint32_t>(e.k_first)))
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
        auto k = std::make_unique<sealhip_kswitch_key>();
        k->key.n_digits = n_digits;
        k->key.words = static_cast<std::size_t>(n_digits) * 2 * e.n_key * e.n;
        SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&k->key.d_data), k->key.words * sizeof(u64)));
        hipError_t err = hipMemcpyAsync(k->key.d_data, key, k->key.words * sizeof(u64),
                                        from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, e.lane().stream);
        if (err == hipSuccess)
            err = hipStreamSynchronize(e.lane().stream);
        if (err != hipSuccess)
        {
            (void)hipFree(k->key.d_data);
            throw HipError(err, hipGetErrorString(err));
        }
        *out = k.release();
    });
}
long sealhip_kswitch_key_destroy(sealhip_context *ctx, sealhip_kswitch_key *key)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(key);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true); // any thread's lane may still be reading the key
        e.key_generation++;     // graphs captured earlier may embed this key's address: they are stale now
        SEALHIP_CHECK(hipFree(key->key.d_data));
        delete key;
    });
}
long sealhip_modup_rns(sealhip_context *ctx, uint32_t k, uint32_t src_bundle_index, uint64_t *ext, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ext);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        op_modup(e, static_cast<int>(k), static_cast<int>(src_bundle_index), reinterpret_cast<u64 *>(ext), count);
    });
}
long sealhip_rescale_special_rns_inplace(sealhip_context *ctx, uint32_t k, uint64_t *poly, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(poly);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        op_rescale_special_inplace(e, static_cast<int>(k), reinterpret_cast<u64 *>(poly), count);
    });
}
long sealhip_switch_key_inplace(sealhip_context *ctx, uint32_t k, uint64_t *ct, const uint64_t *target, size_t count,
                                const sealhip_kswitch_key *key)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(target);
    REQUIRE_PTR(key);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        op_switch_key(e, static_cast<int>(k), reinterpret_cast<u64 *>(ct), 2 * poly,
                      reinterpret_cast<const u64 *>(target), poly, count, key->key);
    });
}

/* SURVEY 8(e) "latency mode": the decomposition digits of ONE key switch split across devices (one process per GPU; the
   caller sums the partials with an all-reduce -- RCCL over xGMI -- between the two calls). */
long sealhip_switch_key_partial(sealhip_context *ctx, uint32_t k, const uint64_t *target, size_t count,
                                const sealhip_kswitch_key *key, uint32_t digit_begin, uint32_t digit_end, uint64_t *partial)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(target);
    REQUIRE_PTR(key);
    REQUIRE_PTR(partial);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        KsSplit split;
        split.j0 = static_cast<int>(digit_begin);
        split.j1 = static_cast<int>(digit_end);
        split.partial_out = reinterpret_cast<u64 *>(partial);
        op_switch_key(e, static_cast<int>(k), nullptr, 2 * poly, reinterpret_cast<const u64 *>(target), poly, count, key->key,
                      nullptr, 0, &split);
    });
}

long sealhip_switch_key_finish(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint64_t *partial_sum, size_t count,
                               uint32_t n_partials)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(partial_sum);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        // the sum of n_partials canonical residues is reduced with barrett_reduce_63 (words below 2^63): refuse a world
        // size that could pass it (61-bit key primes: more than 4 partials) instead of wrapping silently
        if (n_partials < 1)
            throw std::invalid_argument("n_partials: at least one partial was summed");
        for (u64 p : e.key_moduli)
            if (static_cast<unsigned __int128>(n_partials) * (p - 1) >= (static_cast<unsigned __int128>(1) << 63))
                throw std::invalid_argument("n_partials * max(key prime) reaches 2^63: reduce the partials before summing more of them");
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        KsSplit split;
        split.partial_sum = reinterpret_cast<u64 *>(partial_sum);
        op_switch_key(e, static_cast<int>(k), reinterpret_cast<u64 *>(ct), 2 * poly, nullptr, poly, count, KSwitchKey{}, nullptr, 0,
                      &split);
    });
}

long sealhip_kswitch_digits(sealhip_context *ctx, uint32_t k, uint32_t *digits)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(digits);
    return guarded([&] {
        Engine &e = *ctx->engine;
        check_level(e, k);
        if (static_cast<int>(k) > e.k_first)
            throw std::invalid_argument("key switching needs a ciphertext level");
        *digits = kswitch_digits(e, k);
    });
}

namespace
{
    // SEAL_CIPHERTEXT_SIZE_MIN/MAX (util/defines.h:56-57) and the aliasing rule of the raw-buffer form
    void check_multiply_args(Engine &e, uint32_t k, const u64 *a, uint32_t size_a, const u64 *b, uint32_t size_b, const u64 *out)
    {
        check_level(e, k);
        if (size_a < 2 || size_b < 2 || size_a + size_b - 1 > 16)
            throw std::invalid_argument("encrypted1 or encrypted2 is not valid for encryption parameters");
        if (out == a || out == b)
            throw std::invalid_argument("out must not alias an operand");
    }

    // Evaluator::multiply (evaluator.cpp:235-527) on device batches
    void do_multiply(Engine &e, uint32_t k, const u64 *a, uint32_t size_a, const u64 *b, uint32_t size_b, size_t count, u64 *out)
    {
        check_multiply_args(e, k, a, size_a, b, size_b, out);
        if (e.scheme == 1)
            op_bfv_multiply(e, static_cast<int>(k), a, static_cast<int>(size_a), b, static_cast<int>(size_b), count, out);
        else
            op_ckks_multiply(e, static_cast<int>(k), a, static_cast<int>(size_a), b, static_cast<int>(size_b), count, out);
    }

    // relinearize_internal (evaluator.cpp:772-827) on a device batch
    void do_relinearize(Engine &e, uint32_t k, u64 *p, uint32_t size, size_t count, const sealhip_kswitch_key *const *relin_keys,
                        uint32_t n_relin_keys, SinkScope *sink = nullptr)
    {
        check_level(e, k);
        if (size < 2 || size > 16)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (size == 2)
            return; // evaluator.cpp:798-802
        if (!relin_keys || n_relin_keys < size - 2)
            throw std::invalid_argument("not enough relinearization keys"); // :793-796
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        // :811-815 -- the target stays the LAST polynomial for every step, exactly like the reference
        for (uint32_t I = 0; I + 2 < size; I++)
        {
            const uint32_t key_power = size - 1 - I;
            const sealhip_kswitch_key *key = relin_keys[key_power - 2];
            if (!key)
                throw std::invalid_argument("not enough relinearization keys");
            if (sink && I + 3 == size)
                sink->arm(); // the last key switch stores the final polynomial 1
            op_switch_key(e, static_cast<int>(k), p, size * poly, p + (size - 1) * poly, size * poly, count, key->key);
        }
    }

    // rotate_internal (evaluator.cpp:1945-2000) on a device batch of size-2 ciphertexts
    void do_rotate(Engine &e, uint32_t k, u64 *ct, size_t count, int32_t steps, const uint32_t *galois_elts,
                   const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys)
    {
        check_level(e, k);
        std::function<void(int)> rotate = [&](int st) {
            if (st == 0)
                return;
            const std::uint32_t elt = host_galois_elt_from_step(e.n, st);
            for (uint32_t i = 0; i < n_keys; i++)
                if (galois_elts[i] == elt)
                {
                    if (!galois_keys[i])
                        throw std::invalid_argument("Galois key not present");
                    op_apply_galois(e, static_cast<int>(k), ct, count, elt, galois_keys[i]->key);
                    return;
                }
            // non-adjacent form, util/numth.h:22-42
            std::vector<int> naf;
            {
                const bool sign = st < 0;
                int value = std::abs(st);
                for (int i = 0; value; i++)
                {
                    const int zi = (value % 2) ? 2 - (value % 4) : 0;
                    value = (value - zi) / 2;
                    if (zi)
                        naf.push_back((sign ? -zi : zi) * (1 << i));
                }
            }
            if (naf.size() == 1)
                throw std::invalid_argument("Galois key not present");
            for (int s : naf)
                if (static_cast<std::size_t>(std::abs(s)) != (e.n >> 1))
                    rotate(s);
        };
        rotate(steps);
    }

    // mod_switch_to_next (evaluator.cpp:996-1036) / rescale_to_next (:1090-1126) on a device batch
    // item_stride (words, 0 = back to back): distance between consecutive ciphertexts of `in` (the *_strided entries)
    void do_level_down(Engine &e, uint32_t k, const u64 *in, uint32_t size, size_t count, u64 *o, bool rescale,
                       size_t item_stride = 0)
    {
        check_level(e, k);
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached");
        if (rescale && e.scheme != 2)
            throw std::invalid_argument("unsupported operation for scheme type"); // evaluator.cpp:1108-1109
        const std::size_t in_poly = static_cast<std::size_t>(k) * e.n, out_poly = static_cast<std::size_t>(k - 1) * e.n;
        if (item_stride != 0 && item_stride < size * in_poly)
            throw std::invalid_argument("item stride smaller than one ciphertext");
        if (rescale || e.scheme == 1)
            op_mod_switch_scale(e, static_cast<int>(k), in, static_cast<int>(size), count, o, item_stride);
        else if (item_stride == 0 || item_stride == size * in_poly)
            // mod_switch_drop_to_next (evaluator.cpp:894-957): keep the first k-1 rows of every polynomial
            check(launch_copy_rows(e, in, in_poly, o, out_poly, count * size, static_cast<int>(k - 1)), "mod_switch_drop");
        else
            for (uint32_t comp = 0; comp < size; comp++)
                check(launch_copy_rows(e, in + comp * in_poly, item_stride, o + comp * out_poly, size * out_poly, count,
                                       static_cast<int>(k - 1)),
                      "mod_switch_drop");
    }
} // namespace

// engine.hpp: one relinearized product of multiply_many and evaluate_polynomial, the callers' buffers
extern "C++" const u64 *sealhip::relin_product(Engine &e, uint32_t k, const u64 *a, const u64 *b, std::size_t count,
                                               const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, u64 *wide,
                                               u64 *narrow)
{
    const std::size_t poly = static_cast<std::size_t>(k) * e.n;
    // (multiply(x, x) and square(x) give the same canonical residues, evaluator.cpp:1228-1235)
    do_multiply(e, k, a, 2, b, 2, count, wide);
    do_relinearize(e, k, wide, 3, count, relin_keys, n_relin_keys);
    check(launch_copy_rows(e, wide, 3 * poly, narrow, 2 * poly, count, static_cast<int>(2 * k)), "resize");
    return narrow;
}

/* ---------------------------------------------------------------- Evaluator level */
long sealhip_evaluator_multiply(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a,
                                const uint64_t *b, uint32_t size_b, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(b);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_multiply_args(e, k, reinterpret_cast<const u64 *>(a), size_a, reinterpret_cast<const u64 *>(b), size_b,
                            reinterpret_cast<const u64 *>(out));
        SinkScope sink(e, count);
        sink.begin();
        do_multiply(e, k, reinterpret_cast<const u64 *>(a), size_a, reinterpret_cast<const u64 *>(b), size_b, count,
                    reinterpret_cast<u64 *>(out));
    });
}

long sealhip_evaluator_square(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, size_t count,
                              uint64_t *out)
{
    // bfv_square / ckks_square (evaluator.cpp:560-770) as their own path: a size-2 operand is lifted / transformed once and
    // c_1 = x_0 x_1 is formed once and added to itself; any other size goes through multiply(a, a) like the reference
    // (:579-583, :720-724). The canonical residues equal multiply(a, a)'s: 2 c0 c1 mod p == c0 c1 + c1 c0 mod p.
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size_a < 2 || 2 * size_a - 1 > 16)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (out == a)
            throw std::invalid_argument("out must not alias the operand");
        const u64 *pa = reinterpret_cast<const u64 *>(a);
        SinkScope sink(e, count);
        sink.begin();
        if (e.scheme == 1)
            op_bfv_square(e, static_cast<int>(k), pa, static_cast<int>(size_a), count, reinterpret_cast<u64 *>(out));
        else
            op_ckks_square(e, static_cast<int>(k), pa, static_cast<int>(size_a), count, reinterpret_cast<u64 *>(out));
    });
}

long sealhip_evaluator_relinearize(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                   const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        do_relinearize(e, k, reinterpret_cast<u64 *>(ct), size, count, relin_keys, n_relin_keys, &sink);
        if (size == 2) // nothing was done (evaluator.cpp:798-802): the flags describe the input
            sink.read_pass(reinterpret_cast<const u64 *>(ct), 2, static_cast<std::size_t>(k) * e.n, count);
    });
}

/* Evaluator::multiply_many (evaluator.cpp:1180-1255) and exponentiate_inplace (:1257-1288) on device batches of size-2
   ciphertexts: the reference's queue order -- neighbours multiplied left to right, an odd last operand appended, then
   products of products appended until one is left -- every product relinearized. Temporaries come from the stream-ordered
   allocator of the calling thread's lane: nothing here synchronises. */
namespace
{
    void do_multiply_many(Engine &e, uint32_t k, const u64 *const *enc, std::size_t n_enc, size_t count,
                          const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, u64 *out)
    {
        check_level(e, k);
        if (n_enc == 0)
            throw std::invalid_argument("encrypteds vector must not be empty"); // :1185-1188
        if (e.scheme != 1)
            throw std::logic_error("unsupported scheme"); // :1212-1215
        for (std::size_t i = 0; i < n_enc; i++)
        {
            if (!enc[i])
                throw std::invalid_argument("encrypteds is not valid for encryption parameters");
            if (enc[i] == out)
                throw std::invalid_argument("encrypteds must be different from destination"); // :1193-1199
        }
        const std::size_t poly = static_cast<std::size_t>(k) * e.n, two = count * 2 * poly * sizeof(u64);
        hipStream_t stream = e.lane().stream;
        if (n_enc == 1 || count == 0)
        {
            if (count)
                SEALHIP_CHECK(hipMemcpyAsync(out, enc[0], two, hipMemcpyDeviceToDevice, stream)); // :1218-1222
            return;
        }
        std::vector<void *> owned;
        struct Cleanup
        {
            std::vector<void *> &v;
            hipStream_t s;
            ~Cleanup()
            {
                for (void *p : v)
                    (void)hipFreeAsync(p, s);
            }
        } cleanup{ owned, stream };
        auto product = [&](const u64 *a, const u64 *b) {
            void *wide = nullptr, *narrow = nullptr;
            SEALHIP_CHECK(hipMallocAsync(&wide, count * 3 * poly * sizeof(u64), stream));
            owned.push_back(wide);
            SEALHIP_CHECK(hipMallocAsync(&narrow, two, stream));
            owned.push_back(narrow);
            return relin_product(e, k, a, b, count, relin_keys, n_relin_keys, static_cast<u64 *>(wide), static_cast<u64 *>(narrow));
        };
        std::vector<const u64 *> queue;
        for (std::size_t i = 0; i + 1 < n_enc; i += 2)
            queue.push_back(product(enc[i], enc[i + 1]));
        if (n_enc & 1)
            queue.push_back(enc[n_enc - 1]);
        for (std::size_t i = 0; i + 1 < queue.size(); i += 2)
            queue.push_back(product(queue[i], queue[i + 1]));
        SEALHIP_CHECK(hipMemcpyAsync(out, queue.back(), two, hipMemcpyDeviceToDevice, stream));
    }
} // namespace

long sealhip_evaluator_multiply_many(sealhip_context *ctx, uint32_t k, const uint64_t *const *encrypteds, uint32_t n_encrypteds,
                                     size_t count, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                     uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    if (n_encrypteds)
        REQUIRE_PTR(encrypteds);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        do_multiply_many(e, k, reinterpret_cast<const u64 *const *>(encrypteds), n_encrypteds, count, relin_keys, n_relin_keys,
                         reinterpret_cast<u64 *>(out));
    });
}

long sealhip_evaluator_exponentiate(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint64_t exponent, size_t count,
                                    const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (exponent == 0)
            throw std::invalid_argument("exponent cannot be 0"); // :1275-1278
        if (exponent > (1u << 16))
            throw std::invalid_argument("exponent is too large"); // (the reference would copy the ciphertext `exponent` times)
        if (ct == out && exponent > 1)
            throw std::invalid_argument("out must not alias the operand");
        // :1286-1287 -- multiply_many over `exponent` copies of the ciphertext
        const std::vector<const u64 *> copies(static_cast<std::size_t>(exponent), reinterpret_cast<const u64 *>(ct));
        if (exponent == 1 && ct == out)
            return;
        do_multiply_many(e, k, copies.data(), copies.size(), count, relin_keys, n_relin_keys, reinterpret_cast<u64 *>(out));
    });
}

/* ---------------------------------------------------------------- batches of separately allocated HOST ciphertexts */
long sealhip_evaluator_multiply_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *a, uint32_t size_a,
                                     const uint64_t *const *b, uint32_t size_b, size_t count, uint64_t *const *out,
                                     const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys)
{
    REQUIRE_PTR(ctx);
    if (count)
    {
        REQUIRE_PTR(a);
        REQUIRE_PTR(b);
        REQUIRE_PTR(out);
    }
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size_a < 2 || size_b < 2 || size_a + size_b - 1 > 16)
            throw std::invalid_argument("encrypted1 or encrypted2 is not valid for encryption parameters");
        const uint32_t dest = size_a + size_b - 1;
        const bool relin = relin_keys != nullptr && dest > 2;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        HostBatchIO io;
        io.in.push_back({ reinterpret_cast<const u64 *const *>(a), size_a * poly });
        io.in.push_back({ reinterpret_cast<const u64 *const *>(b), size_b * poly });
        io.out.push_back({ reinterpret_cast<u64 *const *>(out), (relin ? 2 : dest) * poly });
        io.tmp_words = relin ? dest * poly : 0;
        run_host_batch(e, io, count, [&](Engine &en, const std::vector<u64 *> &d_in, const std::vector<u64 *> &d_out, u64 *tmp,
                                         std::size_t m) {
            if (!relin)
                return do_multiply(en, k, d_in[0], size_a, d_in[1], size_b, m, d_out[0]);
            do_multiply(en, k, d_in[0], size_a, d_in[1], size_b, m, tmp);
            do_relinearize(en, k, tmp, dest, m, relin_keys, n_relin_keys);
            check(launch_copy_rows(en, tmp, dest * poly, d_out[0], 2 * poly, m, static_cast<int>(2 * k)), "resize"); // :819
        });
    });
}

long sealhip_evaluator_relinearize_host(sealhip_context *ctx, uint32_t k, uint64_t *const *ct, uint32_t size, size_t count,
                                        const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys)
{
    REQUIRE_PTR(ctx);
    if (count)
        REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 2 || size > 16)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (size == 2)
            return;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        HostBatchIO io;
        io.in.push_back({ reinterpret_cast<const u64 *const *>(ct), size * poly });
        io.out.push_back({ reinterpret_cast<u64 *const *>(ct), 2 * poly });
        run_host_batch(e, io, count, [&](Engine &en, const std::vector<u64 *> &d_in, const std::vector<u64 *> &d_out, u64 *,
                                         std::size_t m) {
            do_relinearize(en, k, d_in[0], size, m, relin_keys, n_relin_keys);
            check(launch_copy_rows(en, d_in[0], size * poly, d_out[0], 2 * poly, m, static_cast<int>(2 * k)), "resize");
        });
    });
}

long sealhip_evaluator_rotate_vector_host(sealhip_context *ctx, uint32_t k, uint64_t *const *ct, size_t count, int32_t steps,
                                          const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                          uint32_t n_keys)
{
    REQUIRE_PTR(ctx);
    if (count)
        REQUIRE_PTR(ct);
    REQUIRE_GALOIS_LIST(n_keys);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        const std::size_t item = 2 * static_cast<std::size_t>(k) * e.n;
        HostBatchIO io;
        io.in.push_back({ reinterpret_cast<const u64 *const *>(ct), item });
        io.out.push_back({ reinterpret_cast<u64 *const *>(ct), item });
        run_host_batch(e, io, count, [&](Engine &en, const std::vector<u64 *> &d_in, const std::vector<u64 *> &d_out, u64 *,
                                         std::size_t m) {
            do_rotate(en, k, d_in[0], m, steps, galois_elts, galois_keys, n_keys);
            SEALHIP_CHECK(hipMemcpyAsync(d_out[0], d_in[0], m * item * sizeof(u64), hipMemcpyDeviceToDevice, en.lane().stream));
        });
    });
}

static long level_down_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *ct, uint32_t size, size_t count,
                            uint64_t *const *out, bool rescale)
{
    REQUIRE_PTR(ctx);
    if (count)
    {
        REQUIRE_PTR(ct);
        REQUIRE_PTR(out);
    }
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached");
        if (size < 1 || size > 16)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        HostBatchIO io;
        io.in.push_back({ reinterpret_cast<const u64 *const *>(ct), static_cast<std::size_t>(size) * k * e.n });
        io.out.push_back({ reinterpret_cast<u64 *const *>(out), static_cast<std::size_t>(size) * (k - 1) * e.n });
        run_host_batch(e, io, count, [&](Engine &en, const std::vector<u64 *> &d_in, const std::vector<u64 *> &d_out, u64 *,
                                         std::size_t m) { do_level_down(en, k, d_in[0], size, m, d_out[0], rescale); });
    });
}

long sealhip_evaluator_mod_switch_to_next_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *ct, uint32_t size,
                                               size_t count, uint64_t *const *out)
{
    return level_down_host(ctx, k, ct, size, count, out, false);
}

long sealhip_evaluator_rescale_to_next_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *ct, uint32_t size,
                                            size_t count, uint64_t *const *out)
{
    return level_down_host(ctx, k, ct, size, count, out, true);
}

long sealhip_host_register(sealhip_context *ctx, void *ptr, size_t bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ptr);
    return guarded([&] { host_register(device_engine(ctx), ptr, bytes); });
}

long sealhip_host_unregister(sealhip_context *ctx, void *ptr)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ptr);
    return guarded([&] { host_unregister(device_engine(ctx), ptr); });
}

long sealhip_evaluator_mod_switch_to_next(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                          size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        do_level_down(e, k, reinterpret_cast<const u64 *>(ct), size, count, reinterpret_cast<u64 *>(out), false);
        sink.read_pass(reinterpret_cast<const u64 *>(out), size, static_cast<std::size_t>(k - 1) * e.n, count);
    });
}

long sealhip_evaluator_mod_switch_to_next_strided(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                                  size_t ct_item_stride, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        do_level_down(e, k, reinterpret_cast<const u64 *>(ct), size, count, reinterpret_cast<u64 *>(out), false, ct_item_stride);
        sink.read_pass(reinterpret_cast<const u64 *>(out), size, static_cast<std::size_t>(k - 1) * e.n, count);
    });
}

long sealhip_evaluator_rescale_to_next_strided(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                               size_t ct_item_stride, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        do_level_down(e, k, reinterpret_cast<const u64 *>(ct), size, count, reinterpret_cast<u64 *>(out), true, ct_item_stride);
        sink.read_pass(reinterpret_cast<const u64 *>(out), size, static_cast<std::size_t>(k - 1) * e.n, count);
    });
}

long sealhip_evaluator_rescale_to_next(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                       size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        do_level_down(e, k, reinterpret_cast<const u64 *>(ct), size, count, reinterpret_cast<u64 *>(out), true);
        sink.read_pass(reinterpret_cast<const u64 *>(out), size, static_cast<std::size_t>(k - 1) * e.n, count);
    });
}

long sealhip_evaluator_apply_galois(sealhip_context *ctx, uint32_t k, uint64_t *ct, size_t count,
                                    uint32_t galois_elt, const sealhip_kswitch_key *galois_key)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(galois_key);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        SinkScope sink(e, count);
        sink.begin();
        op_apply_galois(e, static_cast<int>(k), reinterpret_cast<u64 *>(ct), count, galois_elt, galois_key->key);
    });
}

long sealhip_evaluator_transform_to_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    return guarded([&] { ntt_entry(ctx, ct, count * size, k, SEALHIP_BASE_Q, false, kNttCanonical); });
}

long sealhip_evaluator_transform_from_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    return guarded([&] { ntt_entry(ctx, ct, count * size, k, SEALHIP_BASE_Q, true, kNttCanonical); });
}

/* ------------------------------------------------------------------ Evaluator surface beyond the hot path */

long sealhip_evaluator_negate(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                              uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        SinkScope sink(e, count);
        check(launch_ct_linear(e, CtLinearOp::Negate, reinterpret_cast<const u64 *>(ct), static_cast<int>(size),
                               nullptr, 0, 0, reinterpret_cast<u64 *>(out), count,
                               e.map_for(static_cast<int>(k), SEALHIP_BASE_Q)),
              "negate");
        sink.read_pass(reinterpret_cast<const u64 *>(out), size, static_cast<std::size_t>(k) * e.n, count);
    });
}

static long add_sub_entry(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                          uint32_t size_b, size_t count, uint64_t *out, bool sub)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(b);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size_a < 1 || size_b < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        // in place (out == a) is only well defined when the result is not larger than a (the reference resizes
        // encrypted1 first, evaluator.cpp:131-132; a raw buffer cannot grow)
        if (out == a && size_b > size_a)
            throw std::invalid_argument("in-place result needs a destination of max(size_a, size_b) polynomials");
        SinkScope sink(e, count);
        check(launch_ct_linear(e, sub ? CtLinearOp::Sub : CtLinearOp::Add, reinterpret_cast<const u64 *>(a),
                               static_cast<int>(size_a), reinterpret_cast<const u64 *>(b), static_cast<int>(size_b), 0,
                               reinterpret_cast<u64 *>(out), count, e.map_for(static_cast<int>(k), SEALHIP_BASE_Q)),
              sub ? "sub" : "add");
        sink.read_pass(reinterpret_cast<const u64 *>(out), std::max(size_a, size_b), static_cast<std::size_t>(k) * e.n, count);
    });
}

long sealhip_evaluator_add(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                           uint32_t size_b, size_t count, uint64_t *out)
{
    return add_sub_entry(ctx, k, a, size_a, b, size_b, count, out, false);
}

long sealhip_evaluator_sub(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                           uint32_t size_b, size_t count, uint64_t *out)
{
    return add_sub_entry(ctx, k, a, size_a, b, size_b, count, out, true);
}

long sealhip_evaluator_multiply_plain_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                          const uint64_t *plain_ntt, size_t plain_stride)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(plain_ntt);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (plain_stride != 0 && plain_stride < static_cast<size_t>(k) * e.n)
            throw std::invalid_argument("plain_stride is smaller than one plaintext");
        SinkScope sink(e, count); // (capacity checked before ct is overwritten)
        check(launch_ct_linear(e, CtLinearOp::MulPlain, reinterpret_cast<const u64 *>(ct), static_cast<int>(size),
                               reinterpret_cast<const u64 *>(plain_ntt), 0, plain_stride, reinterpret_cast<u64 *>(ct),
                               count, e.map_for(static_cast<int>(k), SEALHIP_BASE_Q)),
              "multiply_plain_ntt");
        sink.read_pass(reinterpret_cast<const u64 *>(ct), size, static_cast<std::size_t>(k) * e.n, count);
    });
}

long sealhip_evaluator_multiply_plain(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                      const uint64_t *plain, size_t plain_stride)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(plain);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if (plain_stride != 0 && plain_stride < e.n)
            throw std::invalid_argument("plain_stride is smaller than one plaintext");
        SinkScope sink(e, count); // (capacity checked before ct is overwritten)
        op_multiply_plain(e, static_cast<int>(k), reinterpret_cast<u64 *>(ct), static_cast<int>(size), count,
                          reinterpret_cast<const u64 *>(plain), plain_stride);
        sink.read_pass(reinterpret_cast<const u64 *>(ct), size, static_cast<std::size_t>(k) * e.n, count);
    });
}

long sealhip_evaluator_transform_plain_to_ntt(sealhip_context *ctx, uint32_t k, const uint64_t *plain, size_t plain_coeff_count,
                                              size_t plain_stride, size_t count, uint64_t *plain_ntt)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(plain_ntt);
    return guarded([&] {
        // (the argument checks need no device: they come before the host-only context's refusal)
        const Engine &h = *ctx->engine;
        check_level(h, k);
        if (plain_coeff_count > h.n)
            throw std::invalid_argument("plain is not valid for encryption parameters"); // valcheck.cpp:236-281
        if (plain_stride != 0 && plain_stride < plain_coeff_count)
            throw std::invalid_argument("plain_stride is smaller than one plaintext");
        if (h.scheme != 1 && plain_coeff_count > 0)
            throw std::invalid_argument("plain is not valid for encryption parameters"); // plain_modulus 0 (valcheck.cpp:266-279)
        const std::size_t out_words = count * k * h.n;
        const std::size_t in_words = count ? (count - 1) * (plain_stride ? plain_stride : plain_coeff_count) + plain_coeff_count : 0;
        if (in_words && out_words && plain < plain_ntt + out_words && plain_ntt < plain + in_words)
            throw std::invalid_argument("plain and plain_ntt overlap");
        Engine &e = device_engine(ctx);
        op_transform_plain_to_ntt(e, static_cast<int>(k), reinterpret_cast<const u64 *>(plain), plain_coeff_count, plain_stride,
                                  count, reinterpret_cast<u64 *>(plain_ntt));
    });
}

long sealhip_evaluator_mod_switch_plain_to(sealhip_context *ctx, uint32_t k_from, const uint64_t *plain, size_t count,
                                          uint32_t k_to, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(out);
    return guarded([&] {
        const Engine &h = *ctx->engine;
        check_level(h, k_from);
        if (k_to > k_from)
            throw std::invalid_argument("cannot switch to higher level modulus"); // evaluator.cpp:1079-1082
        if (k_to < 1)
            throw std::invalid_argument("end of modulus switching chain reached"); // :967-970
        const std::size_t in_words = count * k_from * h.n, out_words = count * k_to * h.n;
        const bool in_place_ok = plain == out && (k_to == k_from || count <= 1); // (every word goes back where it was read)
        if (count && !in_place_ok && plain < out + out_words && out < plain + in_words)
            throw std::invalid_argument("plain and out overlap");
        Engine &e = device_engine(ctx);
        // mod_switch_drop_to_next (evaluator.cpp:959-994) per level: Plaintext::resize keeps the leading rows
        check(launch_copy_rows(e, reinterpret_cast<const u64 *>(plain), static_cast<std::size_t>(k_from) * e.n,
                               reinterpret_cast<u64 *>(out), static_cast<std::size_t>(k_to) * e.n, count,
                               static_cast<int>(k_to)),
              "mod_switch_plain");
    });
}

long sealhip_transparency_sink(sealhip_context *ctx, uint32_t *nonzero_flags, size_t capacity)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        Lane &l = e.lane();
        if (nonzero_flags && capacity == 0)
            throw std::invalid_argument("a transparency sink needs room for at least one ciphertext");
        static_assert(sizeof(unsigned) == sizeof(uint32_t), "flag words");
        l.tsink = reinterpret_cast<unsigned *>(nonzero_flags);
        l.tsink_cap = nonzero_flags ? capacity : 0;
        l.tsink_cur = l.tsink_arm = nullptr;
    });
}

long sealhip_transparency_note(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    return guarded([&] {
        check_level(*ctx->engine, k);
        if (size < 1 || size > 16)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        sink.read_pass(reinterpret_cast<const u64 *>(ct), size, static_cast<std::size_t>(k) * e.n, count);
    });
}

long sealhip_is_transparent(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                            uint8_t *transparent)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(transparent);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (count == 0)
            return;
        if (size < 2) // ciphertext.h:474: fewer than SEAL_CIPHERTEXT_SIZE_MIN polynomials
        {
            std::fill(transparent, transparent + count, static_cast<uint8_t>(1));
            return;
        }
        const std::size_t poly_words = static_cast<std::size_t>(k) * e.n;
        e.ws_reserve(e.lane().ws_floor + count * sizeof(unsigned) + 512);
        e.ws_reset();
        unsigned *flags = reinterpret_cast<unsigned *>(e.ws_alloc((count * sizeof(unsigned) + 7) / 8));
        SEALHIP_CHECK(hipMemsetAsync(flags, 0, count * sizeof(unsigned), e.lane().stream));
        check(launch_nonzero_tail(e, reinterpret_cast<const u64 *>(ct), poly_words * size, poly_words, count, flags),
              "is_transparent");
        std::vector<unsigned> host(count);
        SEALHIP_CHECK(hipMemcpyAsync(host.data(), flags, count * sizeof(unsigned), hipMemcpyDeviceToHost, e.lane().stream));
        e.sync_and_check();
        for (size_t i = 0; i < count; i++)
            transparent[i] = host[i] ? 0 : 1;
    });
}

long sealhip_modulo_poly_coeffs_63(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k, uint32_t base,
                                   uint64_t *result)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a);
    REQUIRE_PTR(result);
    return guarded([&] { poly_entry(ctx, PolyOp::Mod63, a, nullptr, 0, result, count, k, base); });
}

long sealhip_evaluator_rotate_vector(sealhip_context *ctx, uint32_t k, uint64_t *ct, size_t count, int32_t steps,
                                     const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                     uint32_t n_keys)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_GALOIS_LIST(n_keys);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        // (the NAF fallback applies several automorphisms: the flags are read off the final ciphertext)
        SinkScope sink(e, count);
        do_rotate(e, k, reinterpret_cast<u64 *>(ct), count, steps, galois_elts, galois_keys, n_keys);
        sink.read_pass(reinterpret_cast<const u64 *>(ct), 2, static_cast<std::size_t>(k) * e.n, count);
    });
}

/* ------------------------------------------------------------------ hoisted rotation */
namespace
{
    // elts / keys: the elements to apply (zero = a copy of the input, rotate_vector_many's step 0) and their keys. The checks
    // that need no device come first and run on host-only contexts too (the order the header documents).
    void do_apply_galois_many(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                              const std::vector<uint32_t> &elts, const std::vector<const sealhip_kswitch_key *> &keys,
                              uint64_t *out)
    {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        for (size_t i = 0; i < elts.size(); i++)
        {
            if (!elts[i])
                continue;
            check_galois_elt(h, elts[i]);
            check_key_digits(h, k, keys[i]);
        }
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("hoisted rotation of BFV ciphertexts needs a STRICT context");
        if (elts.empty() || count == 0)
            return;
        Engine &e = device_engine(ctx);
        const std::size_t item = 2 * static_cast<std::size_t>(k) * e.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, elts.size() * count * item, in, count * item))
            throw std::invalid_argument("out must not overlap ct");
        SinkScope sink(e, elts.size() * count);
        sink.begin();
        // every non-zero element goes through ONE hoisted call, each into its own output slot; a zero is a copy
        std::vector<uint32_t> run_elts, run_slots;
        std::vector<const KSwitchKey *> slot_keys; // (compacted, so not run_keys()'s list)
        for (size_t i = 0; i < elts.size(); i++)
            if (elts[i])
            {
                run_elts.push_back(elts[i]);
                run_slots.push_back(static_cast<uint32_t>(i));
                slot_keys.push_back(&keys[i]->key);
            }
        op_apply_galois_many(e, static_cast<int>(k), in, count, run_elts.data(), slot_keys.data(), run_elts.size(), o,
                             run_slots.data());
        for (size_t i = 0; i < elts.size(); i++)
            if (!elts[i])
            {
                SEALHIP_CHECK(hipMemcpyAsync(o + i * count * item, in, count * item * sizeof(u64), hipMemcpyDeviceToDevice,
                                             e.lane().stream));
                if (sink.on)
                    check(launch_nonzero_tail(e, o + i * count * item, item, item / 2, count, e.lane().tsink + i * count),
                          "transparency");
            }
    }
} // namespace

long sealhip_evaluator_apply_galois_many(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                         const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                         uint32_t n_elts, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_KEYS(n_elts);
    return guarded([&] {
        const std::vector<uint32_t> elts(galois_elts, galois_elts + n_elts);
        for (uint32_t elt : elts)
            if (!elt)
                throw std::invalid_argument("Galois element is not valid");
        do_apply_galois_many(ctx, k, ct, count, elts,
                             std::vector<const sealhip_kswitch_key *>(galois_keys, galois_keys + n_elts), out);
    });
}

long sealhip_evaluator_rotate_vector_many(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                          const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                          const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    if (n_steps)
        REQUIRE_PTR(steps);
    REQUIRE_GALOIS_LIST(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        std::vector<uint32_t> elts;
        std::vector<const sealhip_kswitch_key *> keys;
        keys_for_steps(h, steps, n_steps, galois_elts, galois_keys, n_keys, 0, elts, keys);
        do_apply_galois_many(ctx, k, ct, count, elts, keys, out);
    });
}

/* ------------------------------------------------------------------ ring packing */
namespace
{
    // n = 2^l samples, 0 <= l <= log N: l, or the refusal
    int pack_log_n(const Engine &h, size_t n)
    {
        if (n < 1 || n > h.n || (n & (n - 1)))
            throw std::invalid_argument("n must be a power of two between 1 and N");
        int l = 0;
        while ((static_cast<size_t>(1) << l) < n)
            l++;
        return l;
    }
} // namespace

long sealhip_pack_lwes_galois_elts(sealhip_context *ctx, size_t n, int32_t trace, uint32_t *elts, uint32_t capacity,
                                   uint32_t *n_elts)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(n_elts);
    return guarded([&] {
        const Engine &h = *ctx->engine;
        const int l = pack_log_n(h, n), last = trace ? h.logn : l; // the steps t = 1 .. last run
        *n_elts = static_cast<uint32_t>(last);
        if (!elts)
            return;
        if (capacity < static_cast<uint32_t>(last))
            throw std::invalid_argument("capacity is smaller than the number of Galois elements");
        for (int t = 1; t <= last; t++)
            elts[t - 1] = (1u << t) + 1;
    });
}

long sealhip_evaluator_extract_lwe(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                   const uint32_t *indices_host, size_t n_idx, uint64_t *lwe_a, uint64_t *lwe_b)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(lwe_a);
    REQUIRE_PTR(lwe_b);
    if (n_idx)
        REQUIRE_PTR(indices_host);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        for (size_t i = 0; i < n_idx; i++)
            if (indices_host[i] >= h.n)
                throw std::invalid_argument("coefficient index out of range");
        if (reinterpret_cast<uintptr_t>(lwe_a) % 16)
            throw std::invalid_argument("lwe_a must be 16-byte aligned");
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        const u64 *a = reinterpret_cast<const u64 *>(lwe_a), *b = reinterpret_cast<const u64 *>(lwe_b);
        const std::size_t a_words = count * n_idx * poly, b_words = count * n_idx * k;
        if (words_overlap(a, a_words, in, count * 2 * poly) || words_overlap(b, b_words, in, count * 2 * poly) ||
            words_overlap(a, a_words, b, b_words))
            throw std::invalid_argument("lwe_a and lwe_b must not overlap ct or each other");
        if (count == 0 || n_idx == 0)
            return;
        Engine &e = device_engine(ctx);
        if (e.lane().capturing)
            throw std::logic_error("extract_lwe stages its indices: it cannot be captured");
        Scratch scratch(e);
        std::uint32_t *idx = reinterpret_cast<std::uint32_t *>(scratch.take(n_idx * sizeof(std::uint32_t)));
        SEALHIP_CHECK(hipMemcpyAsync(idx, indices_host, n_idx * sizeof(std::uint32_t), hipMemcpyHostToDevice, e.lane().stream));
        op_extract_lwe(e, static_cast<int>(k), in, count, idx, n_idx, reinterpret_cast<u64 *>(lwe_a), reinterpret_cast<u64 *>(lwe_b));
    });
}

long sealhip_evaluator_pack_lwes(sealhip_context *ctx, uint32_t k, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t n,
                                 size_t count, const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                 uint32_t n_keys, int32_t trace, int32_t normalize, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(lwe_a);
    REQUIRE_PTR(lwe_b);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_KEYS(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        const int l = pack_log_n(h, n), last = trace ? h.logn : l;
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("ring packing of BFV ciphertexts needs a STRICT context");
        for (uint32_t i = 0; i < n_keys; i++)
            check_galois_elt(h, galois_elts[i]);
        std::vector<const KSwitchKey *> keys(static_cast<size_t>(h.logn) + 1, nullptr);
        for (int t = 1; t <= last; t++)
        {
            const uint32_t g = (1u << t) + 1;
            for (uint32_t i = 0; i < n_keys && !keys[t]; i++)
                if (galois_elts[i] == g)
                {
                    check_key_digits(h, k, galois_keys[i]);
                    keys[t] = &galois_keys[i]->key;
                }
            if (!keys[t])
                throw std::invalid_argument("Galois key not present");
        }
        if (reinterpret_cast<uintptr_t>(lwe_a) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
            throw std::invalid_argument("lwe_a and out must be 16-byte aligned");
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *a = reinterpret_cast<const u64 *>(lwe_a), *b = reinterpret_cast<const u64 *>(lwe_b);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * poly, a, count * n * poly) || words_overlap(o, count * 2 * poly, b, count * n * k))
            throw std::invalid_argument("out must not overlap lwe_a or lwe_b");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op_pack_lwes(e, static_cast<int>(k), a, b, l, count, keys.data(), trace != 0, normalize != 0, o, sink);
    });
}

/* ------------------------------------------------------------------ oblivious expansion */
long sealhip_expand_galois_elts(sealhip_context *ctx, size_t n, uint32_t *elts, uint32_t capacity, uint32_t *n_elts)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(n_elts);
    return guarded([&] {
        const Engine &h = *ctx->engine;
        const int l = pack_log_n(h, n); // the steps t = 1 .. l run, with the elements N / 2^(t-1) + 1
        *n_elts = static_cast<uint32_t>(l);
        if (!elts)
            return;
        if (capacity < static_cast<uint32_t>(l))
            throw std::invalid_argument("capacity is smaller than the number of Galois elements");
        for (int t = l; t >= 1; t--) // ascending
            elts[l - t] = static_cast<uint32_t>(h.n >> (t - 1)) + 1;
    });
}

long sealhip_evaluator_expand(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, size_t n,
                              const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                              int32_t normalize, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_KEYS(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        const int l = pack_log_n(h, n);
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("oblivious expansion of BFV ciphertexts needs a STRICT context");
        for (uint32_t i = 0; i < n_keys; i++)
            check_galois_elt(h, galois_elts[i]);
        std::vector<const KSwitchKey *> keys(static_cast<size_t>(h.logn) + 1, nullptr);
        for (int t = 1; t <= l; t++)
        {
            const uint32_t g = static_cast<uint32_t>(h.n >> (t - 1)) + 1;
            for (uint32_t i = 0; i < n_keys && !keys[t]; i++)
                if (galois_elts[i] == g)
                {
                    check_key_digits(h, k, galois_keys[i]);
                    keys[t] = &galois_keys[i]->key;
                }
            if (!keys[t])
                throw std::invalid_argument("Galois key not present");
        }
        if (reinterpret_cast<uintptr_t>(ct) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
            throw std::invalid_argument("ct and out must be 16-byte aligned");
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * n * 2 * poly, in, count * 2 * poly))
            throw std::invalid_argument("out must not overlap ct");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count * n);
        op_expand(e, static_cast<int>(k), in, l, count, keys.data(), normalize != 0, o, sink);
    });
}

long sealhip_evaluator_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *cts, uint32_t n_terms, uint32_t size,
                                 size_t count, const uint64_t *plain, uint32_t n_sums, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(cts);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(out);
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (size < 2 || size > 16) // SEAL_CIPHERTEXT_SIZE_MIN / _MAX (util/defines.h:56-57), as linear_combination checks
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if ((n_terms == 0 || n_sums == 0) && count > 0)
            throw std::invalid_argument("the term list and the sums must not be empty");
        if (reinterpret_cast<uintptr_t>(cts) % 16 || reinterpret_cast<uintptr_t>(plain) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
            throw std::invalid_argument("cts, plain and out must be 16-byte aligned");
        const std::size_t poly = static_cast<std::size_t>(k) * h.n, item = static_cast<std::size_t>(size) * poly;
        const u64 *o = reinterpret_cast<const u64 *>(out), *x = reinterpret_cast<const u64 *>(cts),
                  *p = reinterpret_cast<const u64 *>(plain);
        const std::size_t out_words = n_sums * count * item;
        if (words_overlap(o, out_words, x, count * n_terms * item))
            throw std::invalid_argument("out must not overlap cts");
        if (words_overlap(o, out_words, p, static_cast<std::size_t>(n_sums) * n_terms * poly))
            throw std::invalid_argument("out must not overlap plain");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, static_cast<size_t>(n_sums) * count);
        sink.begin();
        op_dot_plain(e, static_cast<int>(k), x, n_terms, static_cast<int>(size), count, p, n_sums, reinterpret_cast<u64 *>(out));
    });
}

/* ------------------------------------------------------------------ mod-down merged with the rescale */
long sealhip_evaluator_relinearize_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                           size_t ct_item_stride, size_t count, const sealhip_kswitch_key *const *relin_keys,
                                           uint32_t n_relin_keys, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_RELIN_KEYS();
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        check_rescale_level(h, k);
        if (size != 3)
            throw std::invalid_argument("encrypted must have size 3");
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        if (ct_item_stride < 3 * poly)
            throw std::invalid_argument("item stride smaller than one ciphertext");
        const KSwitchKey *key = first_relin_key(h, k, relin_keys, n_relin_keys);
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (count && words_overlap(o, count * 2 * (poly - h.n), in, (count - 1) * ct_item_stride + 3 * poly))
            throw std::invalid_argument("out must not overlap ct");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        sink.begin();
        op_switch_key_rescale(e, static_cast<int>(k), in, ct_item_stride, in + 2 * poly, ct_item_stride, count, *key, o);
    });
}

/* ------------------------------------------------------------------ weighted sums of rotations */
namespace
{
    // every element valid, every key but the identity's with the level's digits (the sums of rotations and both BSGS axes)
    void check_elts_and_keys(const Engine &h, uint32_t k, const std::vector<uint32_t> &elts,
                             const std::vector<const sealhip_kswitch_key *> &keys)
    {
        for (size_t i = 0; i < elts.size(); i++)
        {
            check_galois_elt(h, elts[i]);
            if (elts[i] != 1)
                check_key_digits(h, k, keys[i]);
        }
    }

    // The end of the checks of the sums of rotations and of BSGS: out against ct and plain_ntt, the empty batch (null), the
    // device. The overlap check runs before device_engine() in the merged form and after it otherwise: the merged entries
    // report it on host-only contexts too, the unmerged ones keep the order they always had.
    Engine *rotation_sum_device(sealhip_context *ctx, bool rescale, size_t count, const u64 *o, std::size_t out_words,
                                const u64 *in, std::size_t in_words, const u64 *w, std::size_t w_words)
    {
        const auto check_overlap = [&] {
            if (words_overlap(o, out_words, in, in_words))
                throw std::invalid_argument("out must not overlap ct");
            if (words_overlap(o, out_words, w, w_words))
                throw std::invalid_argument("out must not overlap plain_ntt");
        };
        if (rescale)
            check_overlap();
        if (count == 0)
            return nullptr;
        Engine &e = device_engine(ctx);
        if (!rescale)
            check_overlap();
        return &e;
    }

    // elts: the elements (1 = the identity, which needs no key). The checks that need no device come first and run on
    // host-only contexts too (the order the header documents).
    void do_apply_galois_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                   const std::vector<uint32_t> &elts, const std::vector<const sealhip_kswitch_key *> &keys,
                                   const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out, bool rescale = false)
    {
        Engine &h = *ctx->engine;
        rescale ? check_rescale_level(h, k) : check_data_level(h, k);
        check_elts_and_keys(h, k, elts, keys);
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("hoisted rotation of BFV ciphertexts needs a STRICT context");
        if (count && (elts.empty() || !n_sums))
            throw std::invalid_argument("an empty sum of rotations is a transparent ciphertext");
        const std::size_t item = 2 * static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct), *w = reinterpret_cast<const u64 *>(plain_ntt);
        u64 *o = reinterpret_cast<u64 *>(out);
        Engine *dev = rotation_sum_device(ctx, rescale, count, o, n_sums * count * (rescale ? item - 2 * h.n : item), in,
                                          count * item, w, n_sums * elts.size() * h.key_moduli.size() * h.n);
        if (!dev)
            return;
        SinkScope sink(*dev, static_cast<size_t>(n_sums) * count);
        sink.begin();
        op_apply_galois_dot_plain(*dev, static_cast<int>(k), in, count, elts.data(), run_keys(elts, keys, 1).data(), elts.size(), w,
                                  n_sums, o, rescale);
    }

    long apply_galois_dot_plain_entry(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                      const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys, uint32_t n_elts,
                                      const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out, bool rescale)
    {
        REQUIRE_PTR(ctx);
        REQUIRE_PTR(ct);
        REQUIRE_PTR(plain_ntt);
        REQUIRE_PTR(out);
        REQUIRE_GALOIS_KEYS_BUT_IDENTITY(n_elts);
        return guarded([&] {
            do_apply_galois_dot_plain(ctx, k, ct, count, std::vector<uint32_t>(galois_elts, galois_elts + n_elts),
                                      std::vector<const sealhip_kswitch_key *>(galois_keys, galois_keys + n_elts), plain_ntt,
                                      n_sums, out, rescale);
        });
    }

    long rotate_vector_dot_plain_entry(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, const int32_t *steps,
                                       uint32_t n_steps, const uint32_t *galois_elts,
                                       const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, const uint64_t *plain_ntt,
                                       uint32_t n_sums, uint64_t *out, bool rescale)
    {
        REQUIRE_PTR(ctx);
        REQUIRE_PTR(ct);
        REQUIRE_PTR(plain_ntt);
        REQUIRE_PTR(out);
        if (n_steps)
            REQUIRE_PTR(steps);
        REQUIRE_GALOIS_LIST(n_keys);
        return guarded([&] {
            Engine &h = *ctx->engine;
            rescale ? check_rescale_level(h, k) : check_data_level(h, k);
            std::vector<uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> keys;
            keys_for_steps(h, steps, n_steps, galois_elts, galois_keys, n_keys, 1, elts, keys);
            do_apply_galois_dot_plain(ctx, k, ct, count, elts, keys, plain_ntt, n_sums, out, rescale);
        });
    }
} // namespace

long sealhip_evaluator_apply_galois_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                              const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                              uint32_t n_elts, const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out)
{
    return apply_galois_dot_plain_entry(ctx, k, ct, count, galois_elts, galois_keys, n_elts, plain_ntt, n_sums, out, false);
}

long sealhip_evaluator_apply_galois_dot_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                      const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                                      uint32_t n_elts, const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out)
{
    return apply_galois_dot_plain_entry(ctx, k, ct, count, galois_elts, galois_keys, n_elts, plain_ntt, n_sums, out, true);
}

long sealhip_evaluator_rotate_vector_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                               const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                               const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                               const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out)
{
    return rotate_vector_dot_plain_entry(ctx, k, ct, count, steps, n_steps, galois_elts, galois_keys, n_keys, plain_ntt, n_sums,
                                         out, false);
}

long sealhip_evaluator_rotate_vector_dot_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                       const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                                       const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                       const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out)
{
    return rotate_vector_dot_plain_entry(ctx, k, ct, count, steps, n_steps, galois_elts, galois_keys, n_keys, plain_ntt, n_sums,
                                         out, true);
}

/* ------------------------------------------------------------------ BSGS matrix-vector product */
namespace
{
    // The checks that need no device come first and run on host-only contexts too (the order the header documents).
    void do_apply_galois_bsgs_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                    const std::vector<uint32_t> &baby, const std::vector<const sealhip_kswitch_key *> &bkeys,
                                    const std::vector<uint32_t> &giant, const std::vector<const sealhip_kswitch_key *> &gkeys,
                                    const uint64_t *plain_ntt, uint64_t *out, bool rescale = false)
    {
        Engine &h = *ctx->engine;
        rescale ? check_rescale_level(h, k) : check_data_level(h, k);
        check_elts_and_keys(h, k, baby, bkeys);
        check_elts_and_keys(h, k, giant, gkeys);
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("hoisted rotation of BFV ciphertexts needs a STRICT context");
        if (count && (baby.empty() || giant.empty()))
            throw std::invalid_argument("an empty sum of rotations is a transparent ciphertext");
        const std::size_t item = 2 * static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct), *w = reinterpret_cast<const u64 *>(plain_ntt);
        u64 *o = reinterpret_cast<u64 *>(out);
        Engine *dev = rotation_sum_device(ctx, rescale, count, o, count * (rescale ? item - 2 * h.n : item), in, count * item, w,
                                          giant.size() * baby.size() * h.key_moduli.size() * h.n);
        if (!dev)
            return;
        SinkScope sink(*dev, count);
        sink.begin();
        const std::vector<const KSwitchKey *> bk = run_keys(baby, bkeys, 1), gk = run_keys(giant, gkeys, 1);
        op_apply_galois_bsgs_plain(*dev, static_cast<int>(k), in, count, baby.data(), bk.data(), baby.size(), giant.data(),
                                   gk.data(), giant.size(), w, o, rescale);
    }

long apply_galois_bsgs_plain_entry(sealhip_context *ctx, bool rescale, uint32_t k, const uint64_t *ct, size_t count,
                                               const uint32_t *baby_elts, const sealhip_kswitch_key *const *baby_keys,
                                               uint32_t n_baby, const uint32_t *giant_elts,
                                               const sealhip_kswitch_key *const *giant_keys, uint32_t n_giant,
                                               const uint64_t *plain_ntt, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(plain_ntt);
    REQUIRE_PTR(out);
    if (n_baby)
    {
        REQUIRE_PTR(baby_elts);
        REQUIRE_PTR(baby_keys);
        for (uint32_t i = 0; i < n_baby; i++)
            if (baby_elts[i] != 1)
                REQUIRE_PTR(baby_keys[i]);
    }
    if (n_giant)
    {
        REQUIRE_PTR(giant_elts);
        REQUIRE_PTR(giant_keys);
        for (uint32_t i = 0; i < n_giant; i++)
            if (giant_elts[i] != 1)
                REQUIRE_PTR(giant_keys[i]);
    }
    return guarded([&] {
        do_apply_galois_bsgs_plain(ctx, k, ct, count, std::vector<uint32_t>(baby_elts, baby_elts + n_baby),
                                   std::vector<const sealhip_kswitch_key *>(baby_keys, baby_keys + n_baby),
                                   std::vector<uint32_t>(giant_elts, giant_elts + n_giant),
                                   std::vector<const sealhip_kswitch_key *>(giant_keys, giant_keys + n_giant), plain_ntt, out,
                                   rescale);
    });
}

long rotate_vector_bsgs_plain_entry(sealhip_context *ctx, bool rescale, uint32_t k, const uint64_t *ct, size_t count,
                                                const int32_t *baby_steps, uint32_t n_baby, const int32_t *giant_steps,
                                                uint32_t n_giant, const uint32_t *galois_elts,
                                                const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                const uint64_t *plain_ntt, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(plain_ntt);
    REQUIRE_PTR(out);
    if (n_baby)
        REQUIRE_PTR(baby_steps);
    if (n_giant)
        REQUIRE_PTR(giant_steps);
    REQUIRE_GALOIS_LIST(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        rescale ? check_rescale_level(h, k) : check_data_level(h, k);
        std::vector<uint32_t> baby, giant;
        std::vector<const sealhip_kswitch_key *> bkeys, gkeys;
        keys_for_steps(h, baby_steps, n_baby, galois_elts, galois_keys, n_keys, 1, baby, bkeys);
        keys_for_steps(h, giant_steps, n_giant, galois_elts, galois_keys, n_keys, 1, giant, gkeys);
        do_apply_galois_bsgs_plain(ctx, k, ct, count, baby, bkeys, giant, gkeys, plain_ntt, out, rescale);
    });
}
} // namespace

long sealhip_evaluator_apply_galois_bsgs_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                               const uint32_t *baby_elts, const sealhip_kswitch_key *const *baby_keys,
                                               uint32_t n_baby, const uint32_t *giant_elts,
                                               const sealhip_kswitch_key *const *giant_keys, uint32_t n_giant,
                                               const uint64_t *plain_ntt, uint64_t *out)
{
    return apply_galois_bsgs_plain_entry(ctx, false, k, ct, count, baby_elts, baby_keys, n_baby, giant_elts, giant_keys, n_giant,
                                         plain_ntt, out);
}

long sealhip_evaluator_apply_galois_bsgs_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                       const uint32_t *baby_elts, const sealhip_kswitch_key *const *baby_keys,
                                                       uint32_t n_baby, const uint32_t *giant_elts,
                                                       const sealhip_kswitch_key *const *giant_keys, uint32_t n_giant,
                                                       const uint64_t *plain_ntt, uint64_t *out)
{
    return apply_galois_bsgs_plain_entry(ctx, true, k, ct, count, baby_elts, baby_keys, n_baby, giant_elts, giant_keys, n_giant,
                                         plain_ntt, out);
}

long sealhip_evaluator_rotate_vector_bsgs_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                const int32_t *baby_steps, uint32_t n_baby, const int32_t *giant_steps,
                                                uint32_t n_giant, const uint32_t *galois_elts,
                                                const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                const uint64_t *plain_ntt, uint64_t *out)
{
    return rotate_vector_bsgs_plain_entry(ctx, false, k, ct, count, baby_steps, n_baby, giant_steps, n_giant, galois_elts,
                                          galois_keys, n_keys, plain_ntt, out);
}

long sealhip_evaluator_rotate_vector_bsgs_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                        const int32_t *baby_steps, uint32_t n_baby, const int32_t *giant_steps,
                                                        uint32_t n_giant, const uint32_t *galois_elts,
                                                        const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                        const uint64_t *plain_ntt, uint64_t *out)
{
    return rotate_vector_bsgs_plain_entry(ctx, true, k, ct, count, baby_steps, n_baby, giant_steps, n_giant, galois_elts,
                                          galois_keys, n_keys, plain_ntt, out);
}

/* ------------------------------------------------------------------ homomorphic DFT */
extern "C++" {
struct sealhip_dft_tables
{
    DftTables *tables = nullptr;
};

namespace
{
    dftplan::Plan dft_make_plan(const Engine &h, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                                const uint32_t *n_baby)
    {
        dftplan::Ring ring;
        ring.scheme = h.scheme;
        ring.logn = static_cast<uint32_t>(h.logn);
        ring.n_key = static_cast<uint32_t>(h.n_key);
        ring.k_first = static_cast<uint32_t>(h.k_first);
        ring.key_moduli = h.key_moduli.data();
        if (n_stages > SEALHIP_DFT_MAX_STAGES)
            throw std::invalid_argument("the stages' layer counts must sum to log2(N/2)");
        return dftplan::make_plan(ring, direction, k, stages, n_stages, n_baby);
    }

    void dft_plan_to_abi(const dftplan::Plan &p, sealhip_dft_plan *out)
    {
        std::memset(out, 0, sizeof(*out));
        out->direction = p.direction;
        out->n_stages = static_cast<uint32_t>(p.stages.size());
        out->in_level = p.in_level;
        out->out_level = p.out_level;
        out->needs_conjugation = p.needs_conjugation ? 1 : 0;
        out->n_key_steps = static_cast<uint32_t>(p.key_steps.size());
        out->table_words = p.table_words;
        out->temp_bytes_per_item = p.temp_bytes_per_item;
        for (size_t t = 0; t < p.stages.size(); t++)
        {
            const dftplan::Stage &s = p.stages[t];
            sealhip_dft_stage &o = out->stages[t];
            o.s0 = s.s0;
            o.r = s.r;
            o.h0 = s.h0;
            o.level = s.level;
            o.n_baby = s.n_baby;
            o.n_giant = s.n_giant;
            o.folded = s.folded ? 1 : 0;
            o.scale = s.scale;
        }
    }

    // the tables' context is the caller's: another ring's tables would be read with the wrong strides. kind: "DFT", "bootstrap"
    void check_tables_context(const sealhip_context *ctx, const Engine *made_on, const char *kind)
    {
        if (made_on != ctx->engine.get())
            throw std::invalid_argument(std::string("the ") + kind + " tables were made on another context");
    }

    // "<entry> synchronises": refused during a graph capture; else a handle that `fill` completes, freed if it throws
    template <class Handle, class Fill>
    Handle *create_tables_outside_capture(Engine &e, const char *entry, Fill fill)
    {
        if (e.lane().capturing)
            throw std::logic_error(std::string(entry) + " synchronises: it cannot be captured");
        std::unique_ptr<Handle> t(new Handle);
        fill(*t);
        return t.release();
    }

    // a plan entry's two calls: key_steps null = the plan alone, which says how many steps there are; else the steps too
    template <class WritePlan>
    void plan_with_key_steps(const std::vector<uint32_t> &steps, uint32_t *key_steps, uint32_t key_steps_capacity,
                             WritePlan write_plan)
    {
        if (key_steps && key_steps_capacity < steps.size())
            throw std::invalid_argument("key_steps is too small");
        write_plan();
        if (key_steps)
            std::copy(steps.begin(), steps.end(), key_steps);
    }

    // what a kernel loads or stores 16 bytes at a time (the DFT's split and merge, ModRaise, the double angle's square)
    void check_aligned16(const void *p, const char *name)
    {
        if (reinterpret_cast<std::uintptr_t>(p) & 15)
            throw std::invalid_argument(std::string(name) + " must be 16-byte aligned");
    }

    void check_dft_gain(double gain)
    {
        if (!std::isfinite(gain) || gain == 0)
            throw std::invalid_argument("gain must be finite and non-zero");
    }

    // every stage's elements and keys out of the caller's key list, checked against the stage's level
    std::vector<DftStageKeys> dft_stage_keys(const Engine &h, const dftplan::Plan &p, const uint32_t *galois_elts,
                                             const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys)
    {
        std::vector<DftStageKeys> all;
        for (const dftplan::Stage &s : p.stages)
        {
            DftStageKeys sk;
            std::vector<const sealhip_kswitch_key *> bk, gk;
            keys_for_steps(h, s.baby.data(), s.n_baby, galois_elts, galois_keys, n_keys, 1, sk.baby, bk);
            keys_for_steps(h, s.giant.data(), s.n_giant, galois_elts, galois_keys, n_keys, 1, sk.giant, gk);
            check_elts_and_keys(h, s.level, sk.baby, bk);
            check_elts_and_keys(h, s.level, sk.giant, gk);
            sk.baby_keys = run_keys(sk.baby, bk, 1);
            sk.giant_keys = run_keys(sk.giant, gk, 1);
            all.push_back(std::move(sk));
        }
        return all;
    }

    // the key of element 2N - 1 out of the caller's key list, checked for a key switch at `level`
    const KSwitchKey &conjugation_key(const Engine &h, uint32_t level, const uint32_t *galois_elts,
                                      const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys)
    {
        const uint32_t conj_elt = static_cast<uint32_t>(2 * h.n - 1);
        const sealhip_kswitch_key *conj = nullptr;
        for (uint32_t i = 0; i < n_keys && !conj; i++)
            if (galois_elts[i] == conj_elt)
                conj = galois_keys[i];
        if (!conj)
            throw std::invalid_argument("Galois key not present");
        check_key_digits(h, level, conj);
        return conj->key;
    }
} // namespace
} // extern "C++"

long sealhip_evaluator_dft_plan(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                      const uint32_t *n_baby, sealhip_dft_plan *plan, uint32_t *key_steps, uint32_t key_steps_capacity)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plan);
    return guarded([&] {
        const dftplan::Plan p = dft_make_plan(*ctx->engine, direction, k, stages, n_stages, n_baby);
        plan_with_key_steps(p.key_steps, key_steps, key_steps_capacity, [&] { dft_plan_to_abi(p, plan); });
    });
}

long sealhip_dft_stage_steps(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages,
                             uint32_t n_stages, const uint32_t *n_baby, uint32_t stage, int32_t *baby_steps,
                             int32_t *giant_steps)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(baby_steps);
    REQUIRE_PTR(giant_steps);
    return guarded([&] {
        const dftplan::Plan p = dft_make_plan(*ctx->engine, direction, k, stages, n_stages, n_baby);
        if (stage >= p.stages.size())
            throw std::invalid_argument("stage out of range");
        std::copy(p.stages[stage].baby.begin(), p.stages[stage].baby.end(), baby_steps);
        std::copy(p.stages[stage].giant.begin(), p.stages[stage].giant.end(), giant_steps);
    });
}

long sealhip_dft_stage_values(sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                              const uint32_t *n_baby, double gain, uint32_t stage, double *values)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(values);
    return guarded([&] {
        const dftplan::Plan p = dft_make_plan(*ctx->engine, direction, k, stages, n_stages, n_baby);
        if (stage >= p.stages.size())
            throw std::invalid_argument("stage out of range");
        check_dft_gain(gain);
        Engine &e = device_engine(ctx);
        op_dft_stage_values(e, p, stage, gain, values);
    });
}

long sealhip_dft_stage_values_host(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages,
                                   uint32_t n_stages, const uint32_t *n_baby, double gain, uint32_t stage, double *values)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(values);
    return guarded([&] {
        const dftplan::Plan p = dft_make_plan(*ctx->engine, direction, k, stages, n_stages, n_baby);
        if (stage >= p.stages.size())
            throw std::invalid_argument("stage out of range");
        check_dft_gain(gain);
        dft_stage_values_host(*ctx->engine, p, stage, gain, values);
    });
}

long sealhip_dft_tables_create(sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                               const uint32_t *n_baby, double gain, sealhip_dft_tables **tables)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    return guarded([&] {
        const dftplan::Plan p = dft_make_plan(*ctx->engine, direction, k, stages, n_stages, n_baby);
        check_dft_gain(gain);
        Engine &e = device_engine(ctx);
        *tables = create_tables_outside_capture<sealhip_dft_tables>(
            e, "sealhip_dft_tables_create", [&](sealhip_dft_tables &t) { t.tables = dft_tables_create(e, p, gain); });
    });
}

long sealhip_dft_tables_destroy(sealhip_dft_tables *tables)
{
    REQUIRE_PTR(tables);
    return guarded([&] {
        dft_tables_destroy(tables->tables); // (throws, and leaves the tables alone, during a graph capture)
        delete tables;
    });
}

long sealhip_dft_tables_plan(const sealhip_dft_tables *tables, sealhip_dft_plan *plan)
{
    REQUIRE_PTR(tables);
    REQUIRE_PTR(plan);
    return guarded([&] { dft_plan_to_abi(dft_tables_plan(*tables->tables), plan); });
}

long sealhip_dft_tables_stage(const sealhip_dft_tables *tables, uint32_t stage, const uint64_t **plain_ntt)
{
    REQUIRE_PTR(tables);
    REQUIRE_PTR(plain_ntt);
    return guarded([&] {
        if (stage >= dft_tables_plan(*tables->tables).stages.size())
            throw std::invalid_argument("stage out of range");
        *plain_ntt = reinterpret_cast<const uint64_t *>(dft_tables_stage(*tables->tables, stage));
    });
}

long sealhip_evaluator_coeffs_to_slots(sealhip_context *ctx, const sealhip_dft_tables *tables, const uint64_t *ct, size_t count,
                                       const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                       uint32_t n_keys, uint64_t *out_re, uint64_t *out_im)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out_re);
    REQUIRE_PTR(out_im);
    REQUIRE_GALOIS_KEYS(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const dftplan::Plan &p = dft_tables_plan(*tables->tables);
        check_tables_context(ctx, dft_tables_engine(*tables->tables), "DFT");
        check_aligned16(out_re, "out_re");
        check_aligned16(out_im, "out_im");
        if (p.direction != dftplan::kCoeffsToSlots)
            throw std::invalid_argument("the tables were made for slots_to_coeffs");
        const std::vector<DftStageKeys> keys = dft_stage_keys(h, p, galois_elts, galois_keys, n_keys);
        const KSwitchKey &conj = conjugation_key(h, p.out_level, galois_elts, galois_keys, n_keys);
        const std::size_t in_words = count * 2 * p.in_level * h.n, out_words = count * 2 * p.out_level * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *re = reinterpret_cast<u64 *>(out_re), *im = reinterpret_cast<u64 *>(out_im);
        if (words_overlap(re, out_words, in, in_words) || words_overlap(im, out_words, in, in_words))
            throw std::invalid_argument("out must not overlap ct");
        if (words_overlap(re, out_words, im, out_words))
            throw std::invalid_argument("out_re must not overlap out_im");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, 2 * count);
        op_coeffs_to_slots(e, *tables->tables, in, count, keys, conj, re, im);
        const std::size_t poly = static_cast<std::size_t>(p.out_level) * h.n;
        sink.read_pass(re, 2, poly, count);
        if (sink.on)
            check(launch_nonzero_tail(e, im, 2 * poly, poly, count, e.lane().tsink + count), "transparency");
    });
}

long sealhip_evaluator_slots_to_coeffs(sealhip_context *ctx, const sealhip_dft_tables *tables, const uint64_t *ct_re,
                                       const uint64_t *ct_im, size_t count, const uint32_t *galois_elts,
                                       const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    REQUIRE_PTR(ct_re);
    REQUIRE_PTR(ct_im);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_KEYS(n_keys);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const dftplan::Plan &p = dft_tables_plan(*tables->tables);
        check_tables_context(ctx, dft_tables_engine(*tables->tables), "DFT");
        check_aligned16(ct_re, "ct_re");
        check_aligned16(ct_im, "ct_im");
        if (p.direction != dftplan::kSlotsToCoeffs)
            throw std::invalid_argument("the tables were made for coeffs_to_slots");
        const std::vector<DftStageKeys> keys = dft_stage_keys(h, p, galois_elts, galois_keys, n_keys);
        const std::size_t in_words = count * 2 * p.in_level * h.n, out_words = count * 2 * p.out_level * h.n;
        const u64 *re = reinterpret_cast<const u64 *>(ct_re), *im = reinterpret_cast<const u64 *>(ct_im);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, out_words, re, in_words) || words_overlap(o, out_words, im, in_words))
            throw std::invalid_argument("out must not overlap ct");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op_slots_to_coeffs(e, *tables->tables, re, im, count, keys, o);
        sink.read_pass(o, 2, static_cast<std::size_t>(p.out_level) * h.n, count);
    });
}

/* ------------------------------------------------------------------ matrix-vector products from a caller's matrix */
extern "C++" {
struct sealhip_linear_transform
{
    LinearTransform *tables = nullptr;
};

namespace
{
    // The checks that need no device, in the order the header documents; mask null = every diagonal
    ltplan::Plan lintrans_make_plan(const Engine &h, uint32_t d, const uint8_t *mask, uint32_t n1)
    {
        if (h.scheme != 2)
            throw std::invalid_argument("linear transforms are CKKS only");
        return ltplan::make_plan(static_cast<uint32_t>(h.logn - 1), d, mask, n1);
    }

    // d alone, for the entries that have no mask yet
    void check_lintrans_size(const Engine &h, uint32_t d)
    {
        if (h.scheme != 2)
            throw std::invalid_argument("linear transforms are CKKS only");
        if (!ltplan::is_pow2(d) || d > h.n / 2)
            throw std::invalid_argument("d must be a power of two between 1 and N/2");
    }

    void lintrans_plan_to_abi(const Engine &h, const ltplan::Plan &p, sealhip_lintrans_plan *out)
    {
        std::memset(out, 0, sizeof(*out));
        out->d = p.d;
        out->n_diagonals = p.n_diagonals;
        out->n1 = p.n1;
        out->n_baby = static_cast<uint32_t>(p.baby.size());
        out->n_giant = static_cast<uint32_t>(p.giant.size());
        out->n_key_steps = static_cast<uint32_t>(p.key_steps.size());
        out->table_words = static_cast<uint64_t>(p.cells()) * h.key_moduli.size() * h.n;
        out->temp_bytes_per_item = 0;
    }
} // namespace
} // extern "C++"

long sealhip_linear_transform_plan(const sealhip_context *ctx, uint32_t d, const uint8_t *diag_mask_host, uint32_t n1,
                                   sealhip_lintrans_plan *plan, int32_t *baby_steps, int32_t *giant_steps, uint32_t *key_steps,
                                   uint32_t capacity)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plan);
    return guarded([&] {
        const Engine &h = *ctx->engine;
        const ltplan::Plan p = lintrans_make_plan(h, d, diag_mask_host, n1);
        if ((baby_steps && capacity < p.baby.size()) || (giant_steps && capacity < p.giant.size()) ||
            (key_steps && capacity < p.key_steps.size()))
            throw std::invalid_argument("capacity is too small");
        lintrans_plan_to_abi(h, p, plan);
        if (baby_steps)
            std::copy(p.baby.begin(), p.baby.end(), baby_steps);
        if (giant_steps)
            std::copy(p.giant.begin(), p.giant.end(), giant_steps);
        if (key_steps)
            std::copy(p.key_steps.begin(), p.key_steps.end(), key_steps);
    });
}

long sealhip_linear_transform_diagonals(sealhip_context *ctx, const double *matrix_dev, uint32_t d, uint8_t *diag_mask_host)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(matrix_dev);
    REQUIRE_PTR(diag_mask_host);
    return guarded([&] {
        check_lintrans_size(*ctx->engine, d);
        check_aligned16(matrix_dev, "matrix_dev");
        Engine &e = device_engine(ctx);
        if (e.lane().capturing)
            throw std::logic_error("sealhip_linear_transform_diagonals synchronises: it cannot be captured");
        if (!op_lintrans_occupancy(e, matrix_dev, d, diag_mask_host))
            throw std::invalid_argument("the matrix has an entry that is not finite");
    });
}

long sealhip_linear_transform_values(sealhip_context *ctx, const double *matrix_dev, uint32_t d, const uint8_t *diag_mask_host,
                                     uint32_t n1, double gain, double *values_dev)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(matrix_dev);
    REQUIRE_PTR(values_dev);
    return guarded([&] {
        const ltplan::Plan p = lintrans_make_plan(*ctx->engine, d, diag_mask_host, n1);
        check_dft_gain(gain);
        check_aligned16(matrix_dev, "matrix_dev");
        check_aligned16(values_dev, "values_dev");
        Engine &e = device_engine(ctx);
        if (e.lane().capturing)
            throw std::logic_error("sealhip_linear_transform_values synchronises: it cannot be captured");
        op_lintrans_values(e, p, matrix_dev, gain, values_dev);
    });
}

long sealhip_linear_transform_values_host(const sealhip_context *ctx, const double *matrix_host, uint32_t d,
                                          const uint8_t *diag_mask_host, uint32_t n1, double gain, double *values_host)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(matrix_host);
    REQUIRE_PTR(values_host);
    return guarded([&] {
        const ltplan::Plan p = lintrans_make_plan(*ctx->engine, d, diag_mask_host, n1);
        check_dft_gain(gain);
        ltplan::values_host(p, matrix_host, gain, values_host);
    });
}

long sealhip_linear_transform_create(sealhip_context *ctx, const double *matrix_dev, uint32_t d, uint32_t n1, double scale,
                                     double gain, sealhip_linear_transform **tables)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(matrix_dev);
    REQUIRE_PTR(tables);
    return guarded([&] {
        (void)lintrans_make_plan(*ctx->engine, d, nullptr, n1); // (d and n1, before the device is needed)
        check_dft_gain(gain);
        check_aligned16(matrix_dev, "matrix_dev");
        Engine &e = device_engine(ctx);
        *tables = create_tables_outside_capture<sealhip_linear_transform>(
            e, "sealhip_linear_transform_create",
            [&](sealhip_linear_transform &t) { t.tables = lintrans_create(e, matrix_dev, d, n1, scale, gain); });
    });
}

long sealhip_linear_transform_destroy(sealhip_linear_transform *tables)
{
    REQUIRE_PTR(tables);
    return guarded([&] {
        lintrans_destroy(tables->tables); // (throws, and leaves the tables alone, during a graph capture)
        delete tables;
    });
}

long sealhip_linear_transform_tables_plan(const sealhip_linear_transform *tables, sealhip_lintrans_plan *plan, double *scale)
{
    REQUIRE_PTR(tables);
    REQUIRE_PTR(plan);
    return guarded([&] {
        lintrans_plan_to_abi(*lintrans_engine(*tables->tables), lintrans_plan(*tables->tables), plan);
        if (scale)
            *scale = lintrans_scale(*tables->tables);
    });
}

long sealhip_linear_transform_tables_steps(const sealhip_linear_transform *tables, int32_t *baby_steps, int32_t *giant_steps)
{
    REQUIRE_PTR(tables);
    return guarded([&] {
        const ltplan::Plan &p = lintrans_plan(*tables->tables);
        if (baby_steps)
            std::copy(p.baby.begin(), p.baby.end(), baby_steps);
        if (giant_steps)
            std::copy(p.giant.begin(), p.giant.end(), giant_steps);
    });
}

long sealhip_linear_transform_tables_plain(const sealhip_linear_transform *tables, const uint64_t **plain_ntt)
{
    REQUIRE_PTR(tables);
    REQUIRE_PTR(plain_ntt);
    return guarded([&] { *plain_ntt = reinterpret_cast<const uint64_t *>(lintrans_plain(*tables->tables)); });
}

long sealhip_evaluator_linear_transform(sealhip_context *ctx, const sealhip_linear_transform *tables, uint32_t k,
                                        const uint64_t *ct, size_t count, const uint32_t *galois_elts,
                                        const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, int32_t rescale,
                                        uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_LIST(n_keys);
    const long same = guarded([&] { check_tables_context(ctx, lintrans_engine(*tables->tables), "linear-transform"); });
    if (same != SEALHIP_S_OK)
        return same;
    // the BSGS entry with the tables' steps and plaintexts: its checks, its pipeline, its transparency flags
    const ltplan::Plan &p = lintrans_plan(*tables->tables);
    return rotate_vector_bsgs_plain_entry(ctx, rescale != 0, k, ct, count, p.baby.data(), static_cast<uint32_t>(p.baby.size()),
                                          p.giant.data(), static_cast<uint32_t>(p.giant.size()), galois_elts, galois_keys, n_keys,
                                          reinterpret_cast<const uint64_t *>(lintrans_plain(*tables->tables)), out);
}

/* ------------------------------------------------------------------ ModRaise and the double-angle step */
long sealhip_evaluator_mod_raise(sealhip_context *ctx, uint32_t k_in, const uint64_t *ct, size_t count, uint32_t k_out,
                                 uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        if (h.scheme != 2)
            throw std::invalid_argument("ModRaise is CKKS only");
        check_data_level(h, k_in);
        check_data_level(h, k_out);
        if (k_out < 2)
            throw std::invalid_argument("k_out must be at least 2");
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * k_out * h.n, in, count * 2 * k_in * h.n))
            throw std::invalid_argument("out must not overlap ct");
        check_aligned16(ct, "ct");
        check_aligned16(out, "out");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op_mod_raise(e, static_cast<int>(k_in), in, count, static_cast<int>(k_out), o);
        sink.read_pass(o, 2, static_cast<std::size_t>(k_out) * h.n, count);
    });
}

long sealhip_evaluator_double_angle(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale,
                                    const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out,
                                    double *out_scale)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_PTR(out_scale);
    REQUIRE_RELIN_KEYS();
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        check_rescale_level(h, k);
        const double square = scale * scale;
        if (!std::isfinite(scale) || scale <= 0 || !std::isfinite(square))
            throw std::invalid_argument("scale out of bounds");
        const KSwitchKey *key = first_relin_key(h, k, relin_keys, n_relin_keys);
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * (poly - h.n), in, count * 2 * poly))
            throw std::invalid_argument("out must not overlap an operand");
        check_aligned16(ct, "ct"); // (square_affine_kernel loads it two words at a time)
        std::vector<u64> constant(k);
        for (uint32_t r = 0; r < k; r++)
            constant[r] = polyplan::rint_residue(-std::nearbyint(square), h.key_moduli[r]);
        *out_scale = square / static_cast<double>(h.key_moduli[k - 1]);
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        sink.begin();
        op_double_angle(e, static_cast<int>(k), in, count, constant.data(), *key, o);
    });
}

/* ------------------------------------------------------------------ ciphertext inner product */
long sealhip_evaluator_dot_product_max_terms(sealhip_context *ctx, uint32_t k, uint64_t *max_terms)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(max_terms);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        *max_terms = dot_product_max_terms(h, static_cast<int>(k));
    });
}

namespace
{
long dot_product_entry(sealhip_context *ctx, uint32_t k, const uint64_t *const *a_terms, const uint64_t *const *b_terms,
                       uint32_t n_terms, size_t count, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                       uint64_t *out, bool rescale)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    if (rescale)
        REQUIRE_PTR(relin_keys); // (the merged finish is the key switch's: there is no size-3 form)
    if (n_terms)
    {
        REQUIRE_PTR(a_terms);
        REQUIRE_PTR(b_terms);
        for (uint32_t i = 0; i < n_terms; i++)
        {
            REQUIRE_PTR(a_terms[i]);
            REQUIRE_PTR(b_terms[i]);
        }
    }
    REQUIRE_RELIN_KEYS_IF_ANY();
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        rescale ? check_rescale_level(h, k) : check_data_level(h, k);
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument("the inner product of BFV ciphertexts needs a STRICT context");
        if (n_terms == 0 && count > 0)
            throw std::invalid_argument("the term lists must not be empty");
        if (n_terms > dot_product_max_terms(h, static_cast<int>(k)))
            throw std::invalid_argument("too many terms for one floor at this level (sealhip_evaluator_dot_product_max_terms)");
        const KSwitchKey *key = relin_keys ? first_relin_key(h, k, relin_keys, n_relin_keys) : nullptr;
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *o = reinterpret_cast<const u64 *>(out);
        const std::size_t out_words = count * (rescale ? 2 * (poly - h.n) : (key ? 2 : 3) * poly);
        for (uint32_t i = 0; i < n_terms; i++)
            for (const uint64_t *term : { a_terms[i], b_terms[i] })
                if (words_overlap(o, out_words, reinterpret_cast<const u64 *>(term), count * 2 * poly))
                    throw std::invalid_argument("out must not overlap an operand");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        sink.begin();
        op_dot_product(e, static_cast<int>(k), reinterpret_cast<const u64 *const *>(a_terms),
                       reinterpret_cast<const u64 *const *>(b_terms), n_terms, count, key, reinterpret_cast<u64 *>(out), rescale);
    });
}
} // namespace

long sealhip_evaluator_dot_product(sealhip_context *ctx, uint32_t k, const uint64_t *const *a_terms, const uint64_t *const *b_terms,
                                   uint32_t n_terms, size_t count, const sealhip_kswitch_key *const *relin_keys,
                                   uint32_t n_relin_keys, uint64_t *out)
{
    return dot_product_entry(ctx, k, a_terms, b_terms, n_terms, count, relin_keys, n_relin_keys, out, false);
}

long sealhip_evaluator_dot_product_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *const *a_terms,
                                           const uint64_t *const *b_terms, uint32_t n_terms, size_t count,
                                           const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out)
{
    return dot_product_entry(ctx, k, a_terms, b_terms, n_terms, count, relin_keys, n_relin_keys, out, true);
}

/* ------------------------------------------------------------------ polynomial evaluation */
long sealhip_evaluator_linear_combination(sealhip_context *ctx, uint32_t k, const uint64_t *const *terms, uint32_t n_terms,
                                          uint32_t size, size_t count, const uint64_t *weights, const uint64_t *constant,
                                          uint32_t n_sums, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(weights);
    REQUIRE_PTR(out);
    if (n_terms)
    {
        REQUIRE_PTR(terms);
        for (uint32_t i = 0; i < n_terms; i++)
            REQUIRE_PTR(terms[i]);
    }
    return guarded([&] {
        // The checks that need no device come first and run on host-only contexts too (the order the header documents).
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (size < 2 || size > 16) // SEAL_CIPHERTEXT_SIZE_MIN / _MAX (util/defines.h:56-57), as multiply and relinearize check
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        if ((n_terms == 0 || n_sums == 0) && count > 0)
            throw std::invalid_argument("the term list and the sums must not be empty");
        const std::size_t item = static_cast<std::size_t>(size) * k * h.n;
        const u64 *o = reinterpret_cast<const u64 *>(out), *w = reinterpret_cast<const u64 *>(weights),
                  *kc = reinterpret_cast<const u64 *>(constant);
        const std::size_t out_words = n_sums * count * item;
        for (uint32_t i = 0; i < n_terms; i++)
            if (words_overlap(o, out_words, reinterpret_cast<const u64 *>(terms[i]), count * item))
                throw std::invalid_argument("out must not overlap a term");
        if (words_overlap(o, out_words, w, static_cast<std::size_t>(n_sums) * n_terms * k))
            throw std::invalid_argument("out must not overlap weights");
        if (kc && words_overlap(o, out_words, kc, static_cast<std::size_t>(n_sums) * k))
            throw std::invalid_argument("out must not overlap constant");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, static_cast<size_t>(n_sums) * count);
        sink.begin();
        op_linear_combination(e, static_cast<int>(k), reinterpret_cast<const u64 *const *>(terms), n_terms, static_cast<int>(size),
                              count, w, kc, n_sums, reinterpret_cast<u64 *>(out));
    });
}

/* The same sums over CKKS terms that keep their own level and size: lincomb_levels_kernel reads rows
   r < k of every term at that term's row stride, so nothing is dropped to level k by a copy first. */
long sealhip_evaluator_linear_combination_levels(sealhip_context *ctx, uint32_t k, const uint64_t *const *terms,
                                                 const uint32_t *term_levels, const uint32_t *term_sizes, uint32_t n_terms,
                                                 uint32_t size, size_t count, const uint64_t *weights, const uint64_t *constant,
                                                 uint32_t n_sums, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(weights);
    REQUIRE_PTR(out);
    if (n_terms)
    {
        REQUIRE_PTR(terms);
        for (uint32_t i = 0; i < n_terms; i++)
            REQUIRE_PTR(terms[i]);
        REQUIRE_PTR(term_levels);
        REQUIRE_PTR(term_sizes);
    }
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (h.scheme != 2) // (a BFV mod_switch_to_next rounds every row: a higher level does not hold the lower one's words)
            throw std::invalid_argument("terms at their own level are CKKS only");
        for (uint32_t i = 0; i < n_terms; i++)
            if (term_levels[i] < k || static_cast<int>(term_levels[i]) > h.k_first)
                throw std::invalid_argument("a term's level is below k or out of range");
        if (size < 2 || size > 16) // SEAL_CIPHERTEXT_SIZE_MIN / _MAX (util/defines.h:56-57)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        for (uint32_t i = 0; i < n_terms; i++)
            if (term_sizes[i] < 2 || term_sizes[i] > size)
                throw std::invalid_argument("a term's size is below 2 or above the sum's");
        if ((n_terms == 0 || n_sums == 0) && count > 0)
            throw std::invalid_argument("the term list and the sums must not be empty");
        const std::size_t item = static_cast<std::size_t>(size) * k * h.n;
        const u64 *o = reinterpret_cast<const u64 *>(out), *w = reinterpret_cast<const u64 *>(weights),
                  *kc = reinterpret_cast<const u64 *>(constant);
        const std::size_t out_words = n_sums * count * item;
        for (uint32_t i = 0; i < n_terms; i++)
            if (words_overlap(o, out_words, reinterpret_cast<const u64 *>(terms[i]),
                              count * term_sizes[i] * term_levels[i] * h.n))
                throw std::invalid_argument("out must not overlap a term");
        if (words_overlap(o, out_words, w, static_cast<std::size_t>(n_sums) * n_terms * k))
            throw std::invalid_argument("out must not overlap weights");
        if (kc && words_overlap(o, out_words, kc, static_cast<std::size_t>(n_sums) * k))
            throw std::invalid_argument("out must not overlap constant");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, static_cast<size_t>(n_sums) * count);
        sink.begin();
        op_linear_combination_levels(e, static_cast<int>(k), reinterpret_cast<const u64 *const *>(terms), term_levels, term_sizes,
                                     n_terms, static_cast<int>(size), count, w, kc, n_sums, reinterpret_cast<u64 *>(out));
    });
}

/* Paterson-Stockmeyer over the two entries above: the checks, then bfv_poly_plan and op_evaluate_polynomial (poly_eval.cpp). */
long sealhip_evaluator_evaluate_polynomial(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                           const uint64_t *coeffs, uint32_t degree, uint32_t n_baby,
                                           const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(coeffs);
    REQUIRE_PTR(out);
    REQUIRE_RELIN_KEYS_IF_ANY();
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (h.scheme != 1)
            throw std::invalid_argument("polynomial evaluation is BFV only (CKKS: sealhip_evaluator_linear_combination)");
        if (!h.mode_strict)
            throw std::invalid_argument("polynomial evaluation of BFV ciphertexts needs a STRICT context");
        const BfvPolyPlan plan = bfv_poly_plan(h, k, reinterpret_cast<const u64 *>(coeffs), degree, n_baby);
        const KSwitchKey *key = plan.d >= 2 ? first_relin_key(h, k, relin_keys, n_relin_keys) : nullptr; // (d = 1: no product)
        const std::size_t two_words = count * 2 * k * h.n;
        const u64 *x = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, two_words, x, two_words))
            throw std::invalid_argument("out must not overlap ct");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op_evaluate_polynomial(e, plan, k, x, count, key, relin_keys, n_relin_keys, o, sink);
    });
}

/* ------------------------------------------------------------------ CKKS polynomial evaluation */
extern "C++"
{
namespace
{
    // The checks both entries share, in the header's order, and the plan (poly_plan.hpp). tables: also the inner tables.
    polyplan::Plan ckks_poly_plan(Engine &h, uint32_t k, double scale, const double *coeffs, uint32_t degree, uint32_t basis,
                                  uint32_t n_baby, double scale_out, bool tables)
    {
        check_data_level(h, k);
        if (h.scheme != 2)
            throw std::invalid_argument("planned polynomial evaluation is CKKS only (BFV: sealhip_evaluator_evaluate_polynomial)");
        return polyplan::make_plan(h.key_moduli.data(), static_cast<int>(k), scale, coeffs, degree, basis, n_baby, scale_out,
                                   tables);
    }

    void fill_plan(const polyplan::Plan &p, std::size_t N, sealhip_poly_plan *plan)
    {
        plan->d = static_cast<uint32_t>(p.d), plan->m = static_cast<uint32_t>(p.m), plan->g = static_cast<uint32_t>(p.g);
        plan->inner_level = static_cast<uint32_t>(p.inner_level), plan->out_level = static_cast<uint32_t>(p.out_level);
        plan->n_products = static_cast<uint32_t>(p.n_products);
        plan->out_scale = p.scale_out;
        plan->temp_bytes_per_item = ckks_poly_temp_words(p, N) * sizeof(u64);
    }

    // What evaluate_polynomial_ckks and eval_mod do once they have their plan: the relinearization key if the plan has a
    // product, `out` at the plan's level against `ct` at k, the plan's level and scale reported, and op(e, x, key, o, sink).
    template <class Op>
    void planned_ckks_run(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, bool needs_key,
                          const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out,
                          uint32_t plan_level, double plan_scale, uint32_t *out_level, double *out_scale, Op op)
    {
        Engine &h = *ctx->engine;
        const KSwitchKey *key = needs_key ? first_relin_key(h, k, relin_keys, n_relin_keys) : nullptr;
        const u64 *x = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * plan_level * h.n, x, count * 2 * k * h.n))
            throw std::invalid_argument("out must not overlap ct");
        if (out_level)
            *out_level = plan_level;
        if (out_scale)
            *out_scale = plan_scale;
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op(e, x, key, o, sink);
    }
} // namespace
} // extern "C++"

long sealhip_evaluator_polynomial_plan_ckks(sealhip_context *ctx, uint32_t k, double scale, const double *coeffs, uint32_t degree,
                                            uint32_t basis, uint32_t n_baby, double scale_out, sealhip_poly_plan *plan,
                                            uint64_t *inner_weights, uint64_t *inner_constants)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(coeffs);
    REQUIRE_PTR(plan);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const bool tables = inner_weights || inner_constants;
        const polyplan::Plan p = ckks_poly_plan(h, k, scale, coeffs, degree, basis, n_baby, scale_out, tables);
        fill_plan(p, h.n, plan);
        if (inner_weights)
            std::copy(p.W.begin(), p.W.end(), inner_weights);
        if (inner_constants)
            std::copy(p.K.begin(), p.K.end(), inner_constants);
    });
}

long sealhip_evaluator_evaluate_polynomial_ckks(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale,
                                                const double *coeffs, uint32_t degree, uint32_t basis, uint32_t n_baby,
                                                double scale_out, const sealhip_kswitch_key *const *relin_keys,
                                                uint32_t n_relin_keys, uint64_t *out, uint32_t *out_level, double *out_scale)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(coeffs);
    REQUIRE_PTR(out);
    REQUIRE_RELIN_KEYS_IF_ANY();
    return guarded([&] {
        Engine &h = *ctx->engine;
        const polyplan::Plan p = ckks_poly_plan(h, k, scale, coeffs, degree, basis, n_baby, scale_out, true);
        planned_ckks_run(ctx, k, ct, count, p.d >= 2 /* (d = 1: no product) */, relin_keys, n_relin_keys, out,
                         static_cast<uint32_t>(p.out_level), p.scale_out, out_level, out_scale,
                         [&](Engine &e, const u64 *x, const KSwitchKey *key, u64 *o, SinkScope &sink) {
                             op_evaluate_polynomial_ckks(e, p, k, x, count, key, o, sink);
                         });
    });
}

/* ------------------------------------------------------------------ EvalMod */
extern "C++"
{
namespace
{
    evalmod::Plan evalmod_make_plan(Engine &h, uint32_t k, double scale, uint32_t K, uint32_t r, uint32_t degree, uint32_t n_baby,
                                    double scale_out, bool tables)
    {
        check_data_level(h, k);
        if (h.scheme != 2)
            throw std::invalid_argument("EvalMod is CKKS only");
        return evalmod::make_plan(h.key_moduli.data(), static_cast<int>(k), scale, K, r, degree, n_baby, scale_out, tables);
    }

    void evalmod_plan_to_abi(const evalmod::Plan &p, std::size_t N, sealhip_evalmod_plan *plan)
    {
        std::memset(plan, 0, sizeof(*plan));
        plan->K = p.K, plan->r = p.r, plan->degree = p.d, plan->n_baby = static_cast<uint32_t>(p.poly.m);
        plan->poly_level = static_cast<uint32_t>(p.poly_level), plan->out_level = static_cast<uint32_t>(p.out_level);
        plan->n_products = static_cast<uint32_t>(p.n_products);
        plan->poly_scale_out = p.t0;
        std::copy(p.scales.begin(), p.scales.end(), plan->scales);
        plan->temp_bytes_per_item = evalmod_temp_words(p, N) * sizeof(u64);
    }
} // namespace
} // extern "C++"

long sealhip_evalmod_coeffs(uint32_t K, uint32_t r, uint32_t degree, double *coeffs)
{
    REQUIRE_PTR(coeffs);
    return guarded([&] {
        const std::vector<double> c = evalmod::coeffs(K, r, degree);
        std::copy(c.begin(), c.end(), coeffs);
    });
}

long sealhip_evaluator_evalmod_plan(const sealhip_context *ctx, uint32_t k, double scale, uint32_t K, uint32_t r, uint32_t degree,
                                    uint32_t n_baby, double scale_out, sealhip_evalmod_plan *plan)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plan);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const evalmod::Plan p = evalmod_make_plan(h, k, scale, K, r, degree, n_baby, scale_out, false);
        evalmod_plan_to_abi(p, h.n, plan);
    });
}

long sealhip_evaluator_eval_mod(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale, uint32_t K,
                                uint32_t r, uint32_t degree, uint32_t n_baby, double scale_out,
                                const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out,
                                uint32_t *out_level, double *out_scale)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_RELIN_KEYS_IF_ANY();
    return guarded([&] {
        Engine &h = *ctx->engine;
        const evalmod::Plan p = evalmod_make_plan(h, k, scale, K, r, degree, n_baby, scale_out, true);
        planned_ckks_run(ctx, k, ct, count, p.poly.d >= 2 || r > 0, relin_keys, n_relin_keys, out,
                         static_cast<uint32_t>(p.out_level), p.scales.back(), out_level, out_scale,
                         [&](Engine &e, const u64 *x, const KSwitchKey *key, u64 *o, SinkScope &sink) {
                             op_eval_mod(e, p, k, x, count, key, o, sink);
                         });
    });
}

/* ------------------------------------------------------------------ the bootstrap */
extern "C++"
{
struct sealhip_bootstrap_tables
{
    BootstrapTables *tables = nullptr;
    sealhip_bootstrap_plan plan{};
};

namespace
{
    struct BootPlan
    {
        dftplan::Plan c2s, s2c;
        evalmod::Plan em;
        double raise_scale = 0, s2c_gain = 0;
        std::vector<uint32_t> key_steps;
    };

    BootPlan boot_make_plan(Engine &h, uint32_t k_top, const uint32_t *c2s_stages, uint32_t n_c2s, const uint32_t *c2s_n_baby,
                            const uint32_t *s2c_stages, uint32_t n_s2c, const uint32_t *s2c_n_baby, uint32_t K, uint32_t r,
                            uint32_t degree, uint32_t n_baby, bool tables)
    {
        BootPlan b;
        b.c2s = dft_make_plan(h, dftplan::kCoeffsToSlots, k_top, c2s_stages, n_c2s, c2s_n_baby);
        if (K < 1)
            throw std::invalid_argument("K must be at least 1");
        b.raise_scale = static_cast<double>(h.key_moduli[0]) * static_cast<double>(K);
        b.em = evalmod_make_plan(h, b.c2s.out_level, b.raise_scale, K, r, degree, n_baby, 0.0, tables);
        if (b.em.out_level < 2)
            throw std::invalid_argument("end of modulus switching chain reached");
        b.s2c = dft_make_plan(h, dftplan::kSlotsToCoeffs, static_cast<uint32_t>(b.em.out_level), s2c_stages, n_s2c, s2c_n_baby);
        const double two_pi_s = 6.283185307179586476925286766559 * b.em.scales.back();
        b.s2c_gain = static_cast<double>(h.key_moduli[0]) / two_pi_s;
        b.key_steps = b.c2s.key_steps;
        b.key_steps.insert(b.key_steps.end(), b.s2c.key_steps.begin(), b.s2c.key_steps.end());
        std::sort(b.key_steps.begin(), b.key_steps.end());
        b.key_steps.erase(std::unique(b.key_steps.begin(), b.key_steps.end()), b.key_steps.end());
        return b;
    }

    void boot_plan_to_abi(const Engine &h, const BootPlan &b, sealhip_bootstrap_plan *out)
    {
        std::memset(out, 0, sizeof(*out));
        out->k_top = b.c2s.in_level, out->c2s_out_level = b.c2s.out_level;
        out->evalmod_out_level = static_cast<uint32_t>(b.em.out_level), out->out_level = b.s2c.out_level;
        out->needs_conjugation = 1;
        out->n_key_steps = static_cast<uint32_t>(b.key_steps.size());
        out->raise_scale = b.raise_scale, out->s2c_gain = b.s2c_gain;
        out->table_words = b.c2s.table_words + b.s2c.table_words;
        out->temp_bytes_per_item = bootstrap_temp_words(b.c2s.in_level, b.c2s, b.em, h.n) * sizeof(u64);
        evalmod_plan_to_abi(b.em, h.n, &out->evalmod);
    }
} // namespace
} // extern "C++"

long sealhip_evaluator_bootstrap_plan(const sealhip_context *ctx, uint32_t k_top, const uint32_t *c2s_stages, uint32_t n_c2s,
                                      const uint32_t *c2s_n_baby, const uint32_t *s2c_stages, uint32_t n_s2c,
                                      const uint32_t *s2c_n_baby, uint32_t K, uint32_t r, uint32_t degree, uint32_t n_baby,
                                      sealhip_bootstrap_plan *plan, uint32_t *key_steps, uint32_t key_steps_capacity)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plan);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const BootPlan b = boot_make_plan(h, k_top, c2s_stages, n_c2s, c2s_n_baby, s2c_stages, n_s2c, s2c_n_baby, K, r, degree,
                                          n_baby, false);
        plan_with_key_steps(b.key_steps, key_steps, key_steps_capacity, [&] { boot_plan_to_abi(h, b, plan); });
    });
}

long sealhip_bootstrap_tables_create(sealhip_context *ctx, uint32_t k_top, const uint32_t *c2s_stages, uint32_t n_c2s,
                                     const uint32_t *c2s_n_baby, const uint32_t *s2c_stages, uint32_t n_s2c,
                                     const uint32_t *s2c_n_baby, uint32_t K, uint32_t r, uint32_t degree, uint32_t n_baby,
                                     sealhip_bootstrap_tables **tables)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    return guarded([&] {
        Engine &h = *ctx->engine;
        const BootPlan b = boot_make_plan(h, k_top, c2s_stages, n_c2s, c2s_n_baby, s2c_stages, n_s2c, s2c_n_baby, K, r, degree,
                                          n_baby, true);
        check_dft_gain(b.s2c_gain);
        Engine &e = device_engine(ctx);
        *tables = create_tables_outside_capture<sealhip_bootstrap_tables>(
            e, "sealhip_bootstrap_tables_create", [&](sealhip_bootstrap_tables &t) {
                boot_plan_to_abi(h, b, &t.plan);
                t.tables = bootstrap_tables_create(e, k_top, b.c2s, b.em, b.s2c, b.s2c_gain);
            });
    });
}

long sealhip_bootstrap_tables_destroy(sealhip_bootstrap_tables *tables)
{
    REQUIRE_PTR(tables);
    return guarded([&] {
        bootstrap_tables_destroy(tables->tables); // (throws, and leaves the tables alone, during a graph capture)
        delete tables;
    });
}

long sealhip_bootstrap_tables_plan(const sealhip_bootstrap_tables *tables, sealhip_bootstrap_plan *plan)
{
    REQUIRE_PTR(tables);
    REQUIRE_PTR(plan);
    return guarded([&] { *plan = tables->plan; });
}

// sealhip_evaluator_bootstrap (to_sparse = to_dense = NULL) and sealhip_evaluator_bootstrap_encapsulated: the same checks, then
// the two keys' (to_sparse serves level 1, to_dense level k_top)
static long bootstrap_entry(sealhip_context *ctx, const sealhip_bootstrap_tables *tables, uint32_t k_in, const uint64_t *ct,
                            size_t count, const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                            uint32_t n_keys, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                            const sealhip_kswitch_key *to_sparse, const sealhip_kswitch_key *to_dense, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tables);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    REQUIRE_GALOIS_KEYS(n_keys);
    REQUIRE_RELIN_KEYS_IF_ANY();
    return guarded([&] {
        Engine &h = *ctx->engine;
        const BootstrapTables &t = *tables->tables;
        check_tables_context(ctx, bootstrap_tables_engine(t), "bootstrap");
        check_data_level(h, k_in);
        check_aligned16(ct, "ct");
        check_aligned16(out, "out");
        const dftplan::Plan &c2s = dft_tables_plan(bootstrap_tables_c2s(t)), &s2c = dft_tables_plan(bootstrap_tables_s2c(t));
        const std::vector<DftStageKeys> c2s_keys = dft_stage_keys(h, c2s, galois_elts, galois_keys, n_keys);
        const std::vector<DftStageKeys> s2c_keys = dft_stage_keys(h, s2c, galois_elts, galois_keys, n_keys);
        const KSwitchKey &conj = conjugation_key(h, c2s.out_level, galois_elts, galois_keys, n_keys);
        const KSwitchKey *relin = first_relin_key(h, c2s.out_level, relin_keys, n_relin_keys);
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * s2c.out_level * h.n, in, count * 2 * k_in * h.n))
            throw std::invalid_argument("out must not overlap ct");
        if (to_sparse)
        {
            check_key_digits(h, 1, to_sparse);
            check_key_digits(h, c2s.in_level, to_dense);
        }
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        op_bootstrap(e, t, static_cast<int>(k_in), in, count, c2s_keys, conj, s2c_keys, *relin, o,
                     to_sparse ? &to_sparse->key : nullptr, to_dense ? &to_dense->key : nullptr);
        sink.read_pass(o, 2, static_cast<std::size_t>(s2c.out_level) * h.n, count);
    });
}

long sealhip_evaluator_bootstrap(sealhip_context *ctx, const sealhip_bootstrap_tables *tables, uint32_t k_in, const uint64_t *ct,
                                 size_t count, const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                 uint32_t n_keys, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                 uint64_t *out)
{
    return bootstrap_entry(ctx, tables, k_in, ct, count, galois_elts, galois_keys, n_keys, relin_keys, n_relin_keys, nullptr,
                           nullptr, out);
}

/* ------------------------------------------------------------------ sparse-secret encapsulation */
long sealhip_evaluator_switch_secret(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                     const sealhip_kswitch_key *key, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(key);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        check_key_digits(h, k, key);
        const std::size_t poly = static_cast<std::size_t>(k) * h.n;
        const u64 *in = reinterpret_cast<const u64 *>(ct);
        u64 *o = reinterpret_cast<u64 *>(out);
        if (words_overlap(o, count * 2 * poly, in, count * 2 * poly))
            throw std::invalid_argument("out must not overlap ct");
        if (count == 0)
            return;
        Engine &e = device_engine(ctx);
        SinkScope sink(e, count);
        sink.begin(); // (fused, as apply_galois: the key switch's last kernel writes the flags)
        op_switch_secret(e, static_cast<int>(k), in, in + poly, 2 * poly, count, key->key, o);
    });
}

long sealhip_evaluator_bootstrap_encapsulated(sealhip_context *ctx, const sealhip_bootstrap_tables *tables, uint32_t k_in,
                                              const uint64_t *ct, size_t count, const uint32_t *galois_elts,
                                              const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                              const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                              const sealhip_kswitch_key *to_sparse, const sealhip_kswitch_key *to_dense,
                                              uint64_t *out)
{
    REQUIRE_PTR(to_sparse);
    REQUIRE_PTR(to_dense);
    return bootstrap_entry(ctx, tables, k_in, ct, count, galois_elts, galois_keys, n_keys, relin_keys, n_relin_keys, to_sparse,
                           to_dense, out);
}

/* ------------------------------------------------------------------ decrypt-side arithmetic */

long sealhip_decryptor_dot_product_ct_sk(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                                         const uint64_t *sk_powers_ntt, int32_t is_ntt_form, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(out);
    if (size > 1)
        REQUIRE_PTR(sk_powers_ntt);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        op_dot_product_ct_sk(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct), static_cast<int>(size), count,
                             reinterpret_cast<const u64 *>(sk_powers_ntt), is_ntt_form != 0, reinterpret_cast<u64 *>(out));
    });
}

long sealhip_decrypt_scale_and_round(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(in);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        LevelTools &lt = bfv_level(e, k);
        check(launch_decrypt_scale_and_round(e, lt.d_rns, lt.h_rns, reinterpret_cast<const u64 *>(in),
                                             reinterpret_cast<u64 *>(out), count),
              "decrypt_scale_and_round");
    });
}

namespace
{
    // Decryptor's checks (decryptor.cpp:53-57, :271-285) before any device work, also on host-only contexts
    void check_decrypt_args(const Engine &e, uint32_t k, uint32_t size)
    {
        check_level(e, k);
        if (size < 2 || size > 16) // SEAL_CIPHERTEXT_SIZE_MIN / _MAX (ciphertext.h:474)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
    }
} // namespace

long sealhip_decryptor_invariant_noise_budget(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                              size_t count, const uint64_t *sk_powers_ntt, int32_t *budgets)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(sk_powers_ntt);
    REQUIRE_PTR(budgets);
    return guarded([&] {
        check_decrypt_args(*ctx->engine, k, size);
        if (ctx->engine->scheme != SEALHIP_SCHEME_BFV)
            throw std::logic_error("unsupported scheme"); // :276-279
        Engine &e = device_engine(ctx);
        if (count == 0)
            return;
        op_invariant_noise_budget(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct), static_cast<int>(size), count,
                                  reinterpret_cast<const u64 *>(sk_powers_ntt), budgets);
    });
}

long sealhip_decryptor_decrypt(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                               const uint64_t *sk_powers_ntt, int32_t is_ntt_form, uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(sk_powers_ntt);
    REQUIRE_PTR(plain);
    return guarded([&] {
        check_decrypt_args(*ctx->engine, k, size);
        if (ctx->engine->scheme == SEALHIP_SCHEME_BFV && is_ntt_form)
            throw std::invalid_argument("encrypted cannot be in NTT form"); // :79-82
        if (ctx->engine->scheme == SEALHIP_SCHEME_CKKS && !is_ntt_form)
            throw std::invalid_argument("encrypted must be in NTT form"); // :124-127
        Engine &e = device_engine(ctx);
        if (count == 0)
            return;
        op_decrypt(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct), static_cast<int>(size), count,
                   reinterpret_cast<const u64 *>(sk_powers_ntt), reinterpret_cast<u64 *>(plain));
    });
}

/* ------------------------------------------------------------------ HIP graphs */

long sealhip_graph_capture_begin(sealhip_context *ctx)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (e.lane().capturing)
            throw std::logic_error("a capture is already in progress on this context");
        if (e.lane().prof_on)
            throw std::logic_error("disable the launch profiler before capturing");
        SEALHIP_CHECK(hipStreamBeginCapture(e.lane().stream, hipStreamCaptureModeRelaxed));
        e.lane().capturing = true;
    });
}

long sealhip_graph_capture_end(sealhip_context *ctx, sealhip_graph **graph)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(graph);
    *graph = nullptr;
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (!e.lane().capturing)
            throw std::logic_error("no capture in progress");
        e.lane().capturing = false;
        auto g = std::make_unique<sealhip_graph>();
        SEALHIP_CHECK(hipStreamEndCapture(e.lane().stream, &g->graph));
        if (!g->graph)
            throw std::logic_error("the capture was invalidated (an operation allocated or synchronised): run the sequence "
                                   "once before capturing");
        const hipError_t err = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
        if (err != hipSuccess)
        {
            (void)hipGraphDestroy(g->graph);
            throw HipError(err, hipGetErrorString(err));
        }
        g->lane = &e.lane();
        g->generation = e.lane().alloc_generation;
        g->key_generation = e.key_generation.load();
        g->pool_id = e.lanes->id;
        *graph = g.release();
    });
}

long sealhip_graph_launch(sealhip_context *ctx, sealhip_graph *graph)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(graph);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (graph->pool_id != e.lanes->id)
            throw std::invalid_argument("the graph was captured on another context");
        // replay on the lane the graph was captured on (its arena is part of the graph), whichever thread asks. The caller's
        // own lane is released first: two threads that launch graphs captured on each other's lanes would otherwise take
        // the two lane locks in opposite order
        Lane &l = *graph->lane;
        if (&l != &e.lane() && !g_locks.empty())
            g_locks.pop_back();
        std::lock_guard<std::recursive_mutex> busy(l.busy);
        if (graph->generation != l.alloc_generation)
            throw std::logic_error("the graph is stale: the workspace was re-allocated by a larger operation after the capture");
        if (graph->key_generation != e.key_generation.load())
            throw std::logic_error("the graph is stale: a key-switch key was destroyed after the capture");
        SEALHIP_CHECK(hipGraphLaunch(graph->exec, l.stream));
    });
}

long sealhip_graph_destroy(sealhip_context *ctx, sealhip_graph *graph)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(graph);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true);
        (void)hipGraphExecDestroy(graph->exec);
        (void)hipGraphDestroy(graph->graph);
        delete graph;
    });
}

/* ------------------------------------------------------------------ encrypt-side arithmetic */

long sealhip_encrypt_zero_symmetric(sealhip_context *ctx, uint32_t rows, int32_t is_ntt_form, const uint64_t *a_ntt,
                                    const int32_t *noise, const uint64_t *sk_ntt, size_t count, uint64_t *ct)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(a_ntt);
    REQUIRE_PTR(noise);
    REQUIRE_PTR(sk_ntt);
    REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, rows);
        op_encrypt_zero_symmetric(e, static_cast<int>(rows), is_ntt_form != 0, reinterpret_cast<const u64 *>(a_ntt), noise,
                                  reinterpret_cast<const u64 *>(sk_ntt), count, reinterpret_cast<u64 *>(ct));
    });
}

long sealhip_encrypt_zero_asymmetric(sealhip_context *ctx, uint32_t rows, int32_t is_ntt_form, const uint64_t *pk_ntt,
                                     const int32_t *u, const int32_t *noise, size_t count, uint64_t *ct)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(pk_ntt);
    REQUIRE_PTR(u);
    REQUIRE_PTR(noise);
    REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, rows);
        op_encrypt_zero_asymmetric(e, static_cast<int>(rows), is_ntt_form != 0, reinterpret_cast<const u64 *>(pk_ntt), u,
                                   noise, count, reinterpret_cast<u64 *>(ct));
    });
}

long sealhip_multiply_add_plain_with_scaling_variant(sealhip_context *ctx, uint32_t k, const uint64_t *plain,
                                                     size_t plain_item_stride, uint64_t *ct, uint32_t size, size_t count,
                                                     int32_t subtract)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (e.scheme != 1)
            throw std::logic_error("unsupported operation for scheme type");
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        op_scaling_variant(e, static_cast<int>(k), reinterpret_cast<const u64 *>(plain), plain_item_stride,
                           reinterpret_cast<u64 *>(ct), static_cast<std::size_t>(size) * k * e.n, count, subtract != 0);
    });
}

namespace
{
    // Encryptor's checks (encryptor.cpp:117-121, :185-208, :227-238) before any device work, also on host-only contexts
    void check_encrypt_args(const Engine &e, uint32_t k, bool has_plain)
    {
        if (e.scheme != SEALHIP_SCHEME_BFV && e.scheme != SEALHIP_SCHEME_CKKS)
            throw std::invalid_argument("unsupported scheme");
        if (k < 1 || static_cast<int>(k) > e.n_key)
            throw std::invalid_argument("parms_id is not valid for encryption parameters");
        // BFV encrypts at the first level; a CKKS plaintext lives at a data level (is_metadata_valid_for, no key levels)
        if (has_plain && (e.scheme == SEALHIP_SCHEME_BFV ? static_cast<int>(k) != e.k_first : static_cast<int>(k) > e.k_first))
            throw std::invalid_argument("plain is not valid for encryption parameters");
    }
} // namespace

long sealhip_encryptor_encrypt(sealhip_context *ctx, uint32_t k, const uint64_t *pk_ntt, const uint64_t *plain,
                               size_t plain_item_stride, const int32_t *u, const int32_t *noise, size_t count,
                               uint64_t *ct)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(pk_ntt);
    REQUIRE_PTR(u);
    REQUIRE_PTR(noise);
    REQUIRE_PTR(ct);
    return guarded([&] {
        check_encrypt_args(*ctx->engine, k, plain != nullptr);
        Engine &e = device_engine(ctx);
        if (count == 0)
            return;
        op_encrypt(e, static_cast<int>(k), reinterpret_cast<const u64 *>(pk_ntt), reinterpret_cast<const u64 *>(plain),
                   plain_item_stride, u, noise, count, reinterpret_cast<u64 *>(ct));
    });
}

long sealhip_encryptor_encrypt_symmetric(sealhip_context *ctx, uint32_t k, const uint64_t *sk_ntt,
                                         const uint64_t *plain, size_t plain_item_stride, const uint64_t *seeds_host,
                                         const int32_t *noise, int32_t save_seed, size_t count, uint64_t *ct)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(sk_ntt);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(noise);
    REQUIRE_PTR(ct);
    return guarded([&] {
        check_encrypt_args(*ctx->engine, k, plain != nullptr);
        Engine &e = device_engine(ctx);
        if (count == 0)
            return;
        // the seeded branch only changes BFV (CKKS samples NTT form either way), and is dropped below 9 words (:225-230)
        const bool seeded = save_seed && e.scheme == SEALHIP_SCHEME_BFV && static_cast<std::size_t>(k) * e.n >= 9;
        op_encrypt_symmetric(e, static_cast<int>(k), reinterpret_cast<const u64 *>(sk_ntt),
                             reinterpret_cast<const u64 *>(plain), plain_item_stride, seeds_host, noise, seeded, count,
                             reinterpret_cast<u64 *>(ct));
    });
}

long sealhip_evaluator_add_plain(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                 const uint64_t *plain, size_t plain_item_stride, int32_t subtract)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(ct);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (size < 1)
            throw std::invalid_argument("encrypted is not valid for encryption parameters");
        const std::size_t item = static_cast<std::size_t>(size) * k * e.n;
        if (e.scheme == 1) // evaluator.cpp:1338-1342 / :1412-1416
        {
            op_scaling_variant(e, static_cast<int>(k), reinterpret_cast<const u64 *>(plain), plain_item_stride,
                               reinterpret_cast<u64 *>(ct), item, count, subtract != 0);
            return;
        }
        // CKKS: c_0 +-= plain, both in NTT form (evaluator.cpp:1344-1350 / :1418-1424)
        const RowMap map = e.map_for(static_cast<int>(k), SEALHIP_BASE_Q);
        u64 *c = reinterpret_cast<u64 *>(ct);
        const u64 *p = reinterpret_cast<const u64 *>(plain);
        if (plain_item_stride == static_cast<std::size_t>(k) * e.n)
        {
            // a batch of plaintexts laid out back to back is a batch of size-1 operands of add/sub (evaluator.cpp:131-143)
            check(launch_ct_linear(e, subtract ? CtLinearOp::Sub : CtLinearOp::Add, c, static_cast<int>(size), p, 1, 0, c,
                                   count, map),
                  "add_plain");
            return;
        }
        for (std::size_t i = 0; i < count; i++)
            check(launch_poly_op(e, subtract ? PolyOp::Sub : PolyOp::Add, c + i * item, p + i * plain_item_stride, 0,
                                 c + i * item, k, map),
                  "add_plain");
    });
}

/* ------------------------------------------------------------------ BatchEncoder */

long sealhip_context_using_batching(const sealhip_context *ctx, int32_t *using_batching)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(using_batching);
    *using_batching = ctx->engine->plain_prime >= 0 ? 1 : 0;
    return SEALHIP_S_OK;
}

long sealhip_batch_encode(sealhip_context *ctx, const uint64_t *values, size_t n_values, size_t count, uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(values);
    REQUIRE_PTR(plain);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        op_batch_encode(e, reinterpret_cast<const u64 *>(values), n_values, count, reinterpret_cast<u64 *>(plain));
    });
}

long sealhip_batch_decode(sealhip_context *ctx, const uint64_t *plain, size_t count, uint64_t *values)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(values);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        op_batch_decode(e, reinterpret_cast<const u64 *>(plain), count, reinterpret_cast<u64 *>(values));
    });
}

long sealhip_batch_encode_int64(sealhip_context *ctx, const int64_t *values, size_t n_values, size_t count, uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(values);
    REQUIRE_PTR(plain);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        op_batch_encode(e, reinterpret_cast<const u64 *>(values), n_values, count, reinterpret_cast<u64 *>(plain), true);
    });
}

long sealhip_batch_decode_int64(sealhip_context *ctx, const uint64_t *plain, size_t count, int64_t *values)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(values);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        op_batch_decode(e, reinterpret_cast<const u64 *>(plain), count, reinterpret_cast<u64 *>(values), true);
    });
}

long sealhip_ckks_encode(sealhip_context *ctx, uint32_t k, const double *values, size_t n_values, size_t count, double scale,
                         uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    if (n_values)
        REQUIRE_PTR(values);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        op_ckks_encode(e, static_cast<int>(k), values, n_values, count, scale, reinterpret_cast<u64 *>(plain));
    });
}

// CKKSEncoder::encode_internal(double value, ...) (ckks.cpp:80-216): every slot holds `value`, i.e. the plaintext is the
// constant polynomial round(value * scale), whose NTT form is that constant in every position of every row. The three
// decomposition branches of the reference (<= 64 bits, <= 128 bits, multi-precision) are exact decompositions of one
// integer -- a 53-bit mantissa times a power of two -- so one exact path gives their residues.
long sealhip_ckks_encode_value(sealhip_context *ctx, uint32_t k, double value, double scale, size_t count, uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (e.scheme != 2)
            throw std::invalid_argument("unsupported scheme"); // ckks.cpp:27-30
        const int total_bits = e.total_coeff_modulus_bit_count(static_cast<int>(k));
        if (scale <= 0 || (static_cast<int>(std::log2(scale)) >= total_bits))
            throw std::invalid_argument("scale out of bounds"); // :105-109
        value *= scale; // :112
        const int coeff_bit_count = static_cast<int>(std::log2(std::fabs(value))) + 2;
        if (coeff_bit_count >= total_bits)
            throw std::invalid_argument("encoded value is too large"); // :114-118
        double coeffd = std::round(value);
        const bool is_negative = std::signbit(coeffd);
        coeffd = std::fabs(coeffd);
        int exp2 = 0;
        const double frac = std::frexp(coeffd, &exp2);                      // coeffd = frac * 2^exp2, frac in [0.5, 1)
        const u64 mant = static_cast<u64>(std::ldexp(frac, 53));             // exact: 53-bit mantissa
        const int shift = exp2 - 53;                                          // coeffd = mant * 2^shift (shift may be < 0)
        u64 rows[kMaxModuli];
        for (uint32_t j = 0; j < k; j++)
        {
            const u64 q = e.key_moduli[j];
            u64 r;
            if (coeffd == 0)
                r = 0;
            else if (shift <= 0)
                r = (mant >> (-shift)) % q; // an integer: the low -shift bits of the mantissa are zero
            else
            {
                u64 pw = 1 % q, base = 2 % q; // 2^shift mod q
                for (int s2 = shift; s2; s2 >>= 1)
                {
                    if (s2 & 1)
                        pw = static_cast<u64>(static_cast<unsigned __int128>(pw) * base % q);
                    base = static_cast<u64>(static_cast<unsigned __int128>(base) * base % q);
                }
                r = static_cast<u64>(static_cast<unsigned __int128>(mant % q) * pw % q);
            }
            rows[j] = is_negative ? (r ? q - r : 0) : r; // negate_uint_mod, :137-140
        }
        check(launch_fill_rows(e, reinterpret_cast<u64 *>(plain), rows, static_cast<int>(k), count), "ckks encode value");
    });
}

// CKKSEncoder::encode_internal(int64_t value, ...) (ckks.cpp:218-275): scale 1.0, residues exactly as the reference forms them
long sealhip_ckks_encode_int64(sealhip_context *ctx, uint32_t k, int64_t value, size_t count, uint64_t *plain)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (e.scheme != 2)
            throw std::invalid_argument("unsupported scheme");
        const u64 mag = static_cast<u64>(value < 0 ? -(value + 1) : value) + (value < 0 ? 1u : 0u); // llabs without overflow
        const int bits = mag ? 64 - __builtin_clzll(mag) : 0;
        if (bits + 2 >= e.total_coeff_modulus_bit_count(static_cast<int>(k)))
            throw std::invalid_argument("encoded value is too large"); // :240-244
        u64 rows[kMaxModuli];
        for (uint32_t j = 0; j < k; j++)
        {
            const u64 q = e.key_moduli[j];
            u64 tmp = static_cast<u64>(value);
            if (value < 0)
                tmp += q; // :254-257 (wrapping, as written there)
            rows[j] = tmp % q;
        }
        check(launch_fill_rows(e, reinterpret_cast<u64 *>(plain), rows, static_cast<int>(k), count), "ckks encode int64");
    });
}

long sealhip_ckks_decode(sealhip_context *ctx, uint32_t k, const uint64_t *plain, size_t count, double scale, double *values)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(plain);
    REQUIRE_PTR(values);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        op_ckks_decode(e, static_cast<int>(k), reinterpret_cast<const u64 *>(plain), count, scale, values);
    });
}

long sealhip_ciphertext_resize(sealhip_context *ctx, uint32_t k, const uint64_t *src, uint32_t src_size, uint64_t *dst,
                               uint32_t dst_size, size_t count)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(src);
    REQUIRE_PTR(dst);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if ((dst_size < 2 && dst_size != 0) || dst_size > 16 || src_size > 16)
            throw std::invalid_argument("invalid size"); // ciphertext.cpp:111-114
        if (count == 0 || dst_size == 0)
            return;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        const uint32_t keep = std::min(src_size, dst_size);
        u64 *d = reinterpret_cast<u64 *>(dst);
        if (dst_size > keep)
            SEALHIP_CHECK(hipMemsetAsync(d, 0, count * dst_size * poly * sizeof(u64), e.lane().stream));
        if (keep)
            check(launch_copy_rows(e, reinterpret_cast<const u64 *>(src), src_size * poly, d, dst_size * poly, count,
                                   static_cast<int>(keep * k)),
                  "resize");
    });
}

/* ------------------------------------------------------------------ ciphertext wire format */

long sealhip_context_set_parms_id(sealhip_context *ctx, uint32_t k, const uint64_t parms_id[4])
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(parms_id);
    return guarded([&] { wire_set_parms_id(*ctx->engine, static_cast<int>(k), parms_id); });
}

long sealhip_ciphertext_peek(const void *bytes, size_t len, sealhip_ciphertext_info *info)
{
    REQUIRE_PTR(bytes);
    REQUIRE_PTR(info);
    return guarded([&] { wire_peek(bytes, len, info); });
}

long sealhip_ciphertext_load(sealhip_context *ctx, const void *bytes, size_t len, sealhip_ciphertext_info *info,
                             uint64_t *dst_device, size_t capacity_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(bytes);
    REQUIRE_PTR(info);
    REQUIRE_PTR(dst_device);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        wire_load(e, bytes, len, info, reinterpret_cast<u64 *>(dst_device), capacity_words);
    });
}

long sealhip_ciphertext_load_many(sealhip_context *ctx, const void *const *streams, const size_t *lens, size_t count,
                                  sealhip_ciphertext_info *infos, uint64_t *dst_device, size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(streams);
    REQUIRE_PTR(lens);
    REQUIRE_PTR(infos);
    REQUIRE_PTR(dst_device);
    for (size_t i = 0; i < count; i++)
        if (!streams[i])
            return fail(SEALHIP_E_POINTER, "streams[" + std::to_string(i) + "] is null");
    return guarded([&] {
        Engine &e = device_engine(ctx);
        wire_load_many(e, streams, lens, count, infos, reinterpret_cast<u64 *>(dst_device), item_stride_words);
    });
}

long sealhip_ciphertext_save_size(const sealhip_context *ctx, uint32_t size, uint32_t k, size_t *bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(bytes);
    *bytes = wire_save_size(size, k, ctx->engine->n);
    return SEALHIP_S_OK;
}

long sealhip_ciphertext_save(sealhip_context *ctx, const sealhip_ciphertext_info *info, const uint64_t *src_device,
                             void *bytes, size_t capacity, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(info);
    REQUIRE_PTR(src_device);
    REQUIRE_PTR(bytes);
    REQUIRE_PTR(written);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        *written = wire_save(e, *info, reinterpret_cast<const u64 *>(src_device), bytes, capacity);
    });
}

long sealhip_ciphertext_save_seeded(sealhip_context *ctx, const sealhip_ciphertext_info *info,
                                    const uint64_t *src_device, const uint64_t seed[8], void *bytes,
                                    size_t capacity, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(info);
    REQUIRE_PTR(src_device);
    REQUIRE_PTR(seed);
    REQUIRE_PTR(written);
    return guarded([&] {
        if (!bytes) // size query
        {
            *written = wire_save_seeded_size(*ctx->engine, *info);
            return;
        }
        Engine &e = device_engine(ctx);
        *written = wire_save_seeded(e, *info, reinterpret_cast<const u64 *>(src_device), seed, bytes, capacity);
    });
}

long sealhip_kswitch_key_load_stream(sealhip_context *ctx, const void *bytes, size_t len, uint32_t index,
                                     sealhip_kswitch_key **key, uint64_t *n_slots)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(bytes);
    REQUIRE_PTR(key);
    *key = nullptr;
    return guarded([&] {
        Engine &e = device_engine(ctx);
        u64 *dev = nullptr;
        std::size_t words = 0;
        std::uint64_t dim1 = 0;
        const std::uint32_t digits = wire_load_kswitch_key(e, bytes, len, index, &dev, &words, &dim1);
        if (n_slots)
            *n_slots = dim1;
        if (!digits)
            return;
        auto k = std::make_unique<sealhip_kswitch_key>();
        k->key.n_digits = digits;
        k->key.words = words;
        k->key.d_data = dev;
        *key = k.release();
    });
}

long sealhip_debug_blake2xb(void *out, size_t outlen, const void *in, size_t inlen, const void *key, size_t keylen)
{
    REQUIRE_PTR(out);
    return guarded([&] {
        if (!blake2xb(out, outlen, in, inlen, key, keylen))
            throw std::invalid_argument("blake2xb: bad arguments");
    });
}

long sealhip_expand_seed_host(sealhip_context *ctx, uint32_t rows, const uint64_t seed[8], uint64_t *out_host)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seed);
    REQUIRE_PTR(out_host);
    return guarded([&] {
        Engine &e = *ctx->engine; // host work: also on host-only contexts
        check_level(e, rows);
        const std::vector<u64> c1 = wire_expand_seed(e, static_cast<int>(rows), reinterpret_cast<const unsigned char *>(seed));
        std::memcpy(out_host, c1.data(), c1.size() * sizeof(u64));
    });
}

long sealhip_expand_seed(sealhip_context *ctx, uint32_t rows, const uint64_t *seeds_host, size_t count, uint64_t *out_device,
                         size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(out_device);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, rows);
        const std::size_t words = static_cast<std::size_t>(rows) * e.n;
        if (item_stride_words && item_stride_words < words)
            throw std::invalid_argument("item stride is below rows x N");
        const std::size_t stride = item_stride_words ? item_stride_words : words;
        std::vector<SeedJob> jobs(count);
        for (std::size_t i = 0; i < count; i++)
            jobs[i] = SeedJob{ seeds_host + 8 * i, reinterpret_cast<u64 *>(out_device) + i * stride };
        op_expand_seeds(e, static_cast<int>(rows), jobs.data(), count);
    });
}

long sealhip_debug_seed_slack(sealhip_context *ctx, int64_t extra_candidates_per_seed)
{
    REQUIRE_PTR(ctx);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.lane().seed_slack = extra_candidates_per_seed < 0 ? -1 : extra_candidates_per_seed;
    });
}

long sealhip_kswitch_keys_save(sealhip_context *ctx, const sealhip_kswitch_key *const *keys, uint32_t n_slots, void *bytes,
                               size_t capacity, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(written);
    if (n_slots)
        REQUIRE_PTR(keys);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        std::vector<const KSwitchKey *> raw(n_slots, nullptr);
        for (uint32_t i = 0; i < n_slots; i++)
            raw[i] = keys[i] ? &keys[i]->key : nullptr;
        if (!bytes) // size query
        {
            *written = wire_kswitch_save_size(e, raw.data(), n_slots, false);
            return;
        }
        *written = wire_save_kswitch_keys(e, raw.data(), n_slots, bytes, capacity, false);
    });
}

/* ---------------------------------------------------------------- KeyGenerator (keygenerator.cpp:146-240, :325-369) */
// elts == nullptr: relin keys sk^2 .. sk^(n_keys+1); otherwise the Galois keys of elts. Every check runs on the host before
// any device work (so host-only contexts report them too); on any failure every keys[i] stays NULL. switching: the new keys
// are handed in (s_from: n_keys x n_key x N) and `level` limits what the keys publish (sealhip_generate_switching_keys).
static long generate_keys(sealhip_context *ctx, const uint64_t *sk_ntt, const uint32_t *elts, bool galois, size_t n_keys,
                          const uint64_t *seeds_host, const int32_t *noise, int32_t keep_seeds, sealhip_kswitch_key **keys,
                          bool switching = false, const uint64_t *s_from = nullptr, uint32_t level = 0)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(sk_ntt);
    if (switching && n_keys)
        REQUIRE_PTR(s_from);
    if (n_keys)
    {
        if (galois)
            REQUIRE_PTR(elts);
        REQUIRE_PTR(seeds_host);
        REQUIRE_PTR(noise);
        REQUIRE_PTR(keys);
        std::fill(keys, keys + n_keys, nullptr);
    }
    return guarded([&] {
        Engine &h = *ctx->engine;
        if (galois)
        {
            std::vector<uint32_t> seen(elts, elts + n_keys);
            for (uint32_t elt : seen)
                check_galois_elt(h, elt); // keygenerator.cpp:213-216
            std::sort(seen.begin(), seen.end());
            if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
                throw std::invalid_argument("Galois elements must be distinct (one key per element)");
            if (h.scheme == 1 && h.plain_prime < 0) // CKKS always batches (context.cpp:351-352)
                throw std::logic_error("encryption parameters do not support batching"); // :198-201
        }
        else if (n_keys > 14) // SEAL_CIPHERTEXT_SIZE_MAX - 2, :152-155
            throw std::invalid_argument("invalid count");
        if (switching)
        {
            check_data_level(h, level);
            if (keep_seeds && static_cast<int>(level) < h.k_first)
                throw std::invalid_argument("a key limited to a level keeps no seeds: a seed gives back the rows it leaves out");
        }
        // (using_keyswitching, :327-330, holds for every context: sealhip_context_create refuses a single prime)
        Engine &e = device_engine(ctx);
        if (n_keys == 0)
            return;
        if (e.lane().capturing)
            throw std::logic_error("key generation allocates and synchronises: it cannot be captured in a graph");
        const uint32_t digits = kswitch_digits(e, static_cast<uint32_t>(e.k_first));
        const std::size_t words = static_cast<std::size_t>(digits) * 2 * e.n_key * e.n;
        std::vector<std::unique_ptr<sealhip_kswitch_key>> made(n_keys);
        std::vector<u64 *> data(n_keys, nullptr);
        auto release = [&] {
            for (auto &k : made)
                if (k && k->key.d_data)
                    (void)hipFree(k->key.d_data);
        };
        try
        {
            for (size_t i = 0; i < n_keys; i++)
            {
                made[i] = std::make_unique<sealhip_kswitch_key>();
                made[i]->key.n_digits = digits;
                made[i]->key.words = words;
                made[i]->key.level = switching && static_cast<int>(level) < e.k_first ? level : 0;
                SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&made[i]->key.d_data), words * sizeof(u64)));
                data[i] = made[i]->key.d_data;
                // (save_seed is dropped below n_key x N = 9 words, rlwe.cpp:225-230: every context has at least 2 x 8)
                if (keep_seeds)
                    made[i]->key.seeds.assign(seeds_host + i * digits * 8, seeds_host + (i + 1) * digits * 8);
            }
            op_generate_kswitch_keys(e, reinterpret_cast<const u64 *>(sk_ntt), galois ? elts : nullptr, n_keys, seeds_host,
                                     noise, data.data(), reinterpret_cast<const u64 *>(s_from), static_cast<int>(level));
            e.sync_and_check();
        }
        catch (...)
        {
            (void)hipStreamSynchronize(e.lane().stream); // nothing may still write into a buffer that is freed
            release();
            throw;
        }
        for (size_t i = 0; i < n_keys; i++)
            keys[i] = made[i].release();
    });
}

long sealhip_generate_relin_keys(sealhip_context *ctx, const uint64_t *sk_ntt, uint32_t count, const uint64_t *seeds_host,
                                 const int32_t *noise, int32_t keep_seeds, sealhip_kswitch_key **keys)
{
    return generate_keys(ctx, sk_ntt, nullptr, false, count, seeds_host, noise, keep_seeds, keys);
}

long sealhip_generate_galois_keys(sealhip_context *ctx, const uint64_t *sk_ntt, const uint32_t *galois_elts, uint32_t n_elts,
                                  const uint64_t *seeds_host, const int32_t *noise, int32_t keep_seeds,
                                  sealhip_kswitch_key **keys)
{
    return generate_keys(ctx, sk_ntt, galois_elts, true, n_elts, seeds_host, noise, keep_seeds, keys);
}

long sealhip_generate_switching_keys(sealhip_context *ctx, const uint64_t *sk_to_ntt, const uint64_t *sk_from_ntt,
                                     uint32_t n_keys, uint32_t level, const uint64_t *seeds_host, const int32_t *noise,
                                     int32_t keep_seeds, sealhip_kswitch_key **keys)
{
    return generate_keys(ctx, sk_to_ntt, nullptr, false, n_keys, seeds_host, noise, keep_seeds, keys, true, sk_from_ntt, level);
}

/* ---------------------------------------------------------------- RGSW */
extern "C++" {
namespace
{
    // an empty block for a context's digit count; the caller fills it on its lane and synchronises before it hands it out
    std::unique_ptr<sealhip_rgsw> rgsw_alloc(const Engine &e, uint32_t n_digits, uint32_t level)
    {
        auto g = std::make_unique<sealhip_rgsw>();
        g->key.n_digits = n_digits;
        g->key.half_words = static_cast<std::size_t>(n_digits) * 2 * e.n_key * e.n;
        g->key.level = level;
        SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&g->key.d_data), 2 * g->key.half_words * sizeof(u64)));
        return g;
    }
    // a stream-ordered device copy that is complete (or has thrown) on return
    void copy_words_sync(Engine &e, u64 *dst, const u64 *src, std::size_t words)
    {
        hipError_t err = hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToDevice, e.lane().stream);
        if (err == hipSuccess)
            err = hipStreamSynchronize(e.lane().stream);
        if (err != hipSuccess)
            throw HipError(err, hipGetErrorString(err));
    }

    // The checks the three evaluator entries share, in the header's order, up to the handle. ins: the operands the result
    // must not overlap, each of in_words words (NULL entries are skipped). Returns the engine once a device is known.
    Engine &rgsw_entry_checks(sealhip_context *ctx, uint32_t k, const char *what, std::initializer_list<const uint64_t *> ins,
                              std::size_t in_words, const uint64_t *out, std::size_t out_words)
    {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument(std::string(what) + " of BFV ciphertexts needs a STRICT context");
        for (const uint64_t *p : ins)
            if (reinterpret_cast<uintptr_t>(p) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
                throw std::invalid_argument("the operands and out must be 16-byte aligned");
        for (const uint64_t *p : ins)
            if (p && words_overlap(reinterpret_cast<const u64 *>(out), out_words, reinterpret_cast<const u64 *>(p), in_words))
                throw std::invalid_argument("out must not overlap an operand");
        return device_engine(ctx);
    }
    void check_rgsw_level(const Engine &e, uint32_t k, const sealhip_rgsw *g)
    {
        if (g->key.n_digits < kswitch_digits(e, k) || (g->key.level && k > g->key.level))
            throw std::invalid_argument("rgsw is not valid for encryption parameters");
    }
    void make_rgsw_objects(Engine &e, const uint64_t *sk_ntt, const int32_t *m_coeff, uint32_t n, uint32_t level,
                           const uint64_t *seeds_host, const int32_t *noise, sealhip_rgsw **out);
} // namespace
} // extern "C++"

long sealhip_generate_rgsw(sealhip_context *ctx, const uint64_t *sk_ntt, const int32_t *m_coeff, uint32_t n, uint32_t level,
                           const uint64_t *seeds_host, const int32_t *noise, sealhip_rgsw **out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(sk_ntt);
    if (n)
    {
        REQUIRE_PTR(m_coeff);
        REQUIRE_PTR(seeds_host);
        REQUIRE_PTR(noise);
        REQUIRE_PTR(out);
        std::fill(out, out + n, nullptr);
    }
    return guarded([&] {
        check_data_level(*ctx->engine, level);
        Engine &e = device_engine(ctx);
        if (n == 0)
            return;
        make_rgsw_objects(e, sk_ntt, m_coeff, n, level, seeds_host, noise, out);
    });
}

extern "C++" {
namespace
{
    // n owned objects from m_coeff (device) on a device context, n > 0: the body of sealhip_generate_rgsw, which
    // sealhip_generate_blind_rotation_keys shares. out is filled only on success.
    void make_rgsw_objects(Engine &e, const uint64_t *sk_ntt, const int32_t *m_coeff, uint32_t n, uint32_t level,
                           const uint64_t *seeds_host, const int32_t *noise, sealhip_rgsw **out)
    {
        if (e.lane().capturing)
            throw std::logic_error("key generation allocates and synchronises: it cannot be captured in a graph");
        const uint32_t digits = kswitch_digits(e, static_cast<uint32_t>(e.k_first));
        std::vector<std::unique_ptr<sealhip_rgsw>> made(n);
        std::vector<u64 *> data(n, nullptr);
        u64 *scratch = nullptr;
        const std::size_t scratch_bytes = static_cast<std::size_t>(n) * 2 * e.n_key * e.n * sizeof(u64);
        auto release = [&] {
            (void)hipStreamSynchronize(e.lane().stream); // nothing may still write into a buffer that is freed
            for (auto &g : made)
                if (g && g->key.d_data)
                    (void)hipFree(g->key.d_data);
            if (scratch) // (it may hold the lifted m and m s: erased before it goes back to the allocator, as on success)
            {
                (void)hipMemsetAsync(scratch, 0, scratch_bytes, e.lane().stream);
                (void)hipStreamSynchronize(e.lane().stream);
                (void)hipFree(scratch);
            }
        };
        try
        {
            for (uint32_t i = 0; i < n; i++)
            {
                made[i] = rgsw_alloc(e, digits, static_cast<int>(level) < e.k_first ? level : 0);
                data[i] = made[i]->key.d_data;
            }
            SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&scratch), scratch_bytes));
            op_generate_rgsw(e, reinterpret_cast<const u64 *>(sk_ntt), m_coeff, n, static_cast<int>(level), seeds_host, noise,
                             scratch, data.data());
            e.sync_and_check();
        }
        catch (...)
        {
            release();
            throw;
        }
        SEALHIP_CHECK(hipFree(scratch)); // (erased in stream order, and the lane is idle)
        for (uint32_t i = 0; i < n; i++)
            out[i] = made[i].release();
    }
} // namespace
} // extern "C++"

long sealhip_rgsw_create(sealhip_context *ctx, const sealhip_kswitch_key *key_b, const sealhip_kswitch_key *key_a,
                         sealhip_rgsw **out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(key_b);
    REQUIRE_PTR(key_a);
    REQUIRE_PTR(out);
    *out = nullptr;
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (key_b->key.n_digits != key_a->key.n_digits || key_b->key.level != key_a->key.level)
            throw std::invalid_argument("the two halves of an rgsw must have the same digit count and level");
        if (e.lane().capturing)
            throw std::logic_error("rgsw_create allocates and synchronises: it cannot be captured in a graph");
        auto g = rgsw_alloc(e, key_b->key.n_digits, key_b->key.level);
        try
        {
            SEALHIP_CHECK(hipMemcpyAsync(g->key.d_data, key_b->key.d_data, g->key.half_words * sizeof(u64), hipMemcpyDeviceToDevice,
                                         e.lane().stream));
            copy_words_sync(e, g->key.d_data + g->key.half_words, key_a->key.d_data, g->key.half_words);
        }
        catch (...)
        {
            (void)hipStreamSynchronize(e.lane().stream);
            (void)hipFree(g->key.d_data);
            throw;
        }
        *out = g.release();
    });
}

long sealhip_rgsw_export(sealhip_context *ctx, const sealhip_rgsw *rgsw, sealhip_kswitch_key **keys)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(rgsw);
    REQUIRE_PTR(keys);
    keys[0] = keys[1] = nullptr;
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (e.lane().capturing)
            throw std::logic_error("rgsw_export allocates and synchronises: it cannot be captured in a graph");
        std::unique_ptr<sealhip_kswitch_key> made[2];
        try
        {
            for (int h = 0; h < 2; h++)
            {
                made[h] = std::make_unique<sealhip_kswitch_key>();
                made[h]->key.n_digits = rgsw->key.n_digits;
                made[h]->key.words = rgsw->key.half_words;
                made[h]->key.level = rgsw->key.level;
                SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&made[h]->key.d_data), rgsw->key.half_words * sizeof(u64)));
                copy_words_sync(e, made[h]->key.d_data, rgsw->key.half(h), rgsw->key.half_words);
            }
        }
        catch (...)
        {
            (void)hipStreamSynchronize(e.lane().stream);
            for (auto &k : made)
                if (k && k->key.d_data)
                    (void)hipFree(k->key.d_data);
            throw;
        }
        keys[0] = made[0].release();
        keys[1] = made[1].release();
    });
}

long sealhip_rgsw_destroy(sealhip_context *ctx, sealhip_rgsw *rgsw)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(rgsw);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        e.sync_and_check(true); // any thread's lane may still be reading the block
        e.key_generation++;     // graphs captured earlier may embed its address: they are stale now
        SEALHIP_CHECK(hipFree(rgsw->key.d_data));
        delete rgsw;
    });
}

long sealhip_evaluator_external_product(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                        const sealhip_rgsw *rgsw, const uint64_t *base, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(rgsw);
    REQUIRE_PTR(out);
    return guarded([&] {
        const std::size_t poly = static_cast<std::size_t>(k) * ctx->engine->n, words = count * 2 * poly;
        Engine &e = rgsw_entry_checks(ctx, k, "the external product", { ct, base }, words, out, words);
        check_rgsw_level(e, k, rgsw);
        if (count == 0)
            return;
        u64 *o = reinterpret_cast<u64 *>(out);
        SinkScope sink(e, count);
        sink.begin();
        if (base)
            check(launch_copy_rows(e, reinterpret_cast<const u64 *>(base), poly, o, poly, 2 * count, static_cast<int>(k)), "copy(base)");
        else
            SEALHIP_CHECK(hipMemsetAsync(o, 0, words * sizeof(u64), e.lane().stream));
        op_external_product(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct), 2 * poly, count, rgsw->key, o);
    });
}

long sealhip_evaluator_cmux(sealhip_context *ctx, uint32_t k, const uint64_t *ct0, const uint64_t *ct1, size_t count,
                            const sealhip_rgsw *rgsw, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct0);
    REQUIRE_PTR(ct1);
    REQUIRE_PTR(rgsw);
    REQUIRE_PTR(out);
    return guarded([&] {
        const std::size_t poly = static_cast<std::size_t>(k) * ctx->engine->n, words = count * 2 * poly;
        Engine &e = rgsw_entry_checks(ctx, k, "CMux", { ct0, ct1 }, words, out, words);
        check_rgsw_level(e, k, rgsw);
        if (count == 0)
            return;
        SinkScope sink(e, count);
        sink.begin();
        op_cmux(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct0), 2 * poly, reinterpret_cast<const u64 *>(ct1), 2 * poly,
                count, rgsw->key, reinterpret_cast<u64 *>(out));
    });
}

long sealhip_evaluator_select(sealhip_context *ctx, uint32_t k, const uint64_t *cts, size_t count, uint32_t l,
                              const sealhip_rgsw *const *rgsw_bits, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(cts);
    REQUIRE_PTR(out);
    if (l)
    {
        REQUIRE_PTR(rgsw_bits);
        for (uint32_t t = 0; t < l && l <= 16; t++) // (a longer list is refused below, unread)
            REQUIRE_PTR(rgsw_bits[t]);
    }
    return guarded([&] {
        check_data_level(*ctx->engine, k);
        if (l > 16)
            throw std::invalid_argument("l out of range: a selection among at most 2^16 ciphertexts");
        const std::size_t poly = static_cast<std::size_t>(k) * ctx->engine->n, words = count * 2 * poly;
        Engine &e = rgsw_entry_checks(ctx, k, "selection", { cts }, words << l, out, words);
        std::vector<const RgswKey *> bits(l);
        for (uint32_t t = 0; t < l; t++)
        {
            check_rgsw_level(e, k, rgsw_bits[t]);
            bits[t] = &rgsw_bits[t]->key;
        }
        if (count == 0)
            return;
        SinkScope sink(e, count);
        op_select(e, static_cast<int>(k), reinterpret_cast<const u64 *>(cts), count, static_cast<int>(l), bits.data(),
                  reinterpret_cast<u64 *>(out), sink);
    });
}

long sealhip_debug_ext_mac_plan(sealhip_context *ctx, uint32_t k, size_t count, int32_t out[4])
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(out);
    return guarded([&] {
        check_data_level(*ctx->engine, k);
        Engine &e = device_engine(ctx);
        const ExtMacPlan plan = ext_mac_plan(e, e.level(static_cast<int>(k)).h_ks, count);
        out[0] = plan.choice.family == kMacItems ? 2 : (plan.choice.family == kMacLoop ? 1 : 0);
        out[1] = plan.choice.nd;
        out[2] = plan.split ? 1 : 0;
        out[3] = static_cast<int32_t>(plan.choice.group);
    });
}

/* ---------------------------------------------------------------- blind rotation */
extern "C++" {
namespace
{
    bool bytes_overlap(const void *a, std::size_t a_bytes, const void *b, std::size_t b_bytes)
    {
        const char *x = static_cast<const char *>(a), *y = static_cast<const char *>(b);
        return x < y + b_bytes && y < x + a_bytes;
    }
    // The checks multiply_monomial and blind_rotate share, in the header's order, up to the device. ct: n_ct size-2
    // ciphertexts; exps: count rows of exps_stride words, of which exps_row are read.
    Engine &monomial_entry_checks(sealhip_context *ctx, uint32_t k, const char *what, const uint64_t *ct, size_t n_ct, size_t count,
                                  const uint32_t *exps, size_t exps_stride, size_t exps_row, const uint64_t *out)
    {
        Engine &h = *ctx->engine;
        check_data_level(h, k);
        if (n_ct != 1 && n_ct != count)
            throw std::invalid_argument("n_ct must be 1 (one operand shared by the batch) or count");
        if (h.scheme == 1 && !h.mode_strict)
            throw std::invalid_argument(std::string(what) + " of BFV ciphertexts needs a STRICT context");
        if (reinterpret_cast<uintptr_t>(ct) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
            throw std::invalid_argument("the operands and out must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(exps) % 4)
            throw std::invalid_argument("exps must be 4-byte aligned");
        const std::size_t ct_bytes = 2 * static_cast<std::size_t>(k) * h.n * sizeof(u64);
        const std::size_t exps_bytes = count ? ((count - 1) * exps_stride + exps_row) * sizeof(uint32_t) : 0;
        if (bytes_overlap(out, count * ct_bytes, ct, n_ct * ct_bytes) || bytes_overlap(out, count * ct_bytes, exps, exps_bytes))
            throw std::invalid_argument("out must not overlap an operand or exps");
        return device_engine(ctx);
    }
} // namespace
} // extern "C++"

long sealhip_evaluator_multiply_monomial(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t n_ct, size_t count,
                                         const uint32_t *exps_dev, size_t exps_stride, int32_t minus_one, uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(exps_dev);
    REQUIRE_PTR(out);
    return guarded([&] {
        Engine &e = monomial_entry_checks(ctx, k, "the monomial product", ct, n_ct, count, exps_dev, exps_stride, 1, out);
        if (count == 0)
            return;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        SinkScope sink(e, count);
        op_multiply_monomial(e, static_cast<int>(k), reinterpret_cast<const u64 *>(ct), n_ct == count ? 2 * poly : 0, count, exps_dev,
                             exps_stride, minus_one != 0, reinterpret_cast<u64 *>(out));
        sink.read_pass(reinterpret_cast<const u64 *>(out), 2, poly, count);
    });
}

long sealhip_lwe_mod_switch(sealhip_context *ctx, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t n_samples,
                            int32_t ternary, uint32_t b_offset, uint32_t *exps_out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(lwe_a);
    REQUIRE_PTR(lwe_b);
    REQUIRE_PTR(exps_out);
    return guarded([&] {
        Engine &h = *ctx->engine;
        check_data_level(h, 1);
        if (reinterpret_cast<uintptr_t>(lwe_a) % 16 || reinterpret_cast<uintptr_t>(lwe_b) % 8)
            throw std::invalid_argument("lwe_a must be 16-byte aligned and lwe_b 8-byte aligned");
        if (reinterpret_cast<uintptr_t>(exps_out) % 4)
            throw std::invalid_argument("exps_out must be 4-byte aligned");
        const std::size_t out_bytes = n_samples * (1 + (ternary ? 2 : 1) * h.n) * sizeof(uint32_t);
        if (bytes_overlap(exps_out, out_bytes, lwe_a, n_samples * h.n * sizeof(u64)) ||
            bytes_overlap(exps_out, out_bytes, lwe_b, n_samples * sizeof(u64)))
            throw std::invalid_argument("exps_out must not overlap lwe_a or lwe_b");
        Engine &e = device_engine(ctx);
        if (n_samples == 0)
            return;
        op_lwe_mod_switch(e, reinterpret_cast<const u64 *>(lwe_a), reinterpret_cast<const u64 *>(lwe_b), n_samples, ternary != 0,
                          b_offset, exps_out);
    });
}

long sealhip_generate_blind_rotation_keys(sealhip_context *ctx, const uint64_t *sk_ntt, const int32_t *lwe_secret_dev,
                                          uint32_t n_lwe, int32_t ternary, uint32_t level, const uint64_t *seeds_host,
                                          const int32_t *noise, sealhip_rgsw **out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(sk_ntt);
    const uint32_t per = ternary ? 2 : 1;
    if (n_lwe)
    {
        REQUIRE_PTR(lwe_secret_dev);
        REQUIRE_PTR(seeds_host);
        REQUIRE_PTR(noise);
        REQUIRE_PTR(out);
        if (n_lwe <= UINT32_MAX / per)
            std::fill(out, out + static_cast<std::size_t>(n_lwe) * per, nullptr);
    }
    return guarded([&] {
        check_data_level(*ctx->engine, level);
        if (n_lwe > UINT32_MAX / per)
            throw std::invalid_argument("n_lwe out of range");
        Engine &e = device_engine(ctx);
        if (n_lwe == 0)
            return;
        if (e.lane().capturing)
            throw std::logic_error("key generation allocates and synchronises: it cannot be captured in a graph");
        const uint32_t n = n_lwe * per;
        const std::size_t m_bytes = static_cast<std::size_t>(n) * e.n * sizeof(int32_t);
        Scratch scratch(e);
        int32_t *m_coeff = reinterpret_cast<int32_t *>(scratch.take(m_bytes));
        // the indicators tell the secret: erased in stream order before the block goes back, on the failure paths too
        struct Erase
        {
            Engine &e;
            void *p;
            std::size_t bytes;
            ~Erase()
            {
                (void)hipMemsetAsync(p, 0, bytes, e.lane().stream);
            }
        } erase{ e, m_coeff, m_bytes };
        check(launch_lwe_indicators(e, lwe_secret_dev, n_lwe, ternary != 0, m_coeff), "lwe_indicators");
        make_rgsw_objects(e, sk_ntt, m_coeff, n, level, seeds_host, noise, out);
    });
}

long sealhip_evaluator_blind_rotate(sealhip_context *ctx, uint32_t k, const uint64_t *tv, size_t n_tv, size_t count,
                                    const uint32_t *exps_dev, uint32_t n_steps, const sealhip_rgsw *const *rgsw_list,
                                    uint64_t *out)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(tv);
    REQUIRE_PTR(exps_dev);
    REQUIRE_PTR(out);
    if (n_steps)
    {
        REQUIRE_PTR(rgsw_list);
        for (uint32_t t = 0; t < n_steps; t++)
            REQUIRE_PTR(rgsw_list[t]);
    }
    return guarded([&] {
        const std::size_t row = static_cast<std::size_t>(n_steps) + 1;
        Engine &e = monomial_entry_checks(ctx, k, "blind rotation", tv, n_tv, count, exps_dev, row, row, out);
        std::vector<const RgswKey *> keys(n_steps);
        for (uint32_t t = 0; t < n_steps; t++)
        {
            check_rgsw_level(e, k, rgsw_list[t]);
            keys[t] = &rgsw_list[t]->key;
        }
        if (count == 0)
            return;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        SinkScope sink(e, count);
        op_blind_rotate(e, static_cast<int>(k), reinterpret_cast<const u64 *>(tv), n_tv == count ? 2 * poly : 0, count, exps_dev,
                        n_steps, keys.data(), reinterpret_cast<u64 *>(out), sink);
    });
}

long sealhip_kswitch_keys_save_seeded(sealhip_context *ctx, const sealhip_kswitch_key *const *keys, uint32_t n_slots,
                                      void *bytes, size_t capacity, size_t *written)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(written);
    if (n_slots)
        REQUIRE_PTR(keys);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        std::vector<const KSwitchKey *> raw(n_slots, nullptr);
        for (uint32_t i = 0; i < n_slots; i++)
            raw[i] = keys[i] ? &keys[i]->key : nullptr;
        if (!bytes) // size query
        {
            *written = wire_kswitch_save_size(e, raw.data(), n_slots, true);
            return;
        }
        *written = wire_save_kswitch_keys(e, raw.data(), n_slots, bytes, capacity, true);
    });
}

/* ---------------------------------------------------------------- RLWE samples from seeds */
// the argument rules sealhip_sample_polys and its host form share; returns the item stride
static std::size_t check_sample_args(const Engine &h, uint32_t n_ternary, uint32_t n_noise, size_t item_stride_words)
{
    const uint64_t polys = static_cast<uint64_t>(n_ternary) + n_noise;
    if (polys == 0 || polys > kSampleMaxPolys)
        throw std::invalid_argument("n_ternary + n_noise must be 1 .. 16");
    const std::size_t words = static_cast<std::size_t>(polys) * h.n;
    if (item_stride_words && item_stride_words < words)
        throw std::invalid_argument("item stride is below (n_ternary + n_noise) x N");
    return item_stride_words ? item_stride_words : words;
}

long sealhip_sample_polys(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary, uint32_t n_noise,
                          int32_t *out_device, size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(out_device);
    return guarded([&] {
        const std::size_t stride = check_sample_args(*ctx->engine, n_ternary, n_noise, item_stride_words);
        if ((stride & 3) || (reinterpret_cast<std::uintptr_t>(out_device) & 15))
            throw std::invalid_argument("out_device must be 16-byte aligned and the item stride a multiple of 4");
        Engine &e = device_engine(ctx);
        op_sample_polys(e, seeds_host, count, n_ternary, n_noise, out_device, stride,
                        out_device + static_cast<std::size_t>(n_ternary) * e.n, stride);
    });
}

long sealhip_sample_polys_split(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary,
                                uint32_t n_noise, int32_t *ternary_device, int32_t *noise_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    if (n_ternary)
        REQUIRE_PTR(ternary_device);
    if (n_noise)
        REQUIRE_PTR(noise_device);
    return guarded([&] {
        (void)check_sample_args(*ctx->engine, n_ternary, n_noise, 0);
        if ((reinterpret_cast<std::uintptr_t>(ternary_device) | reinterpret_cast<std::uintptr_t>(noise_device)) & 15)
            throw std::invalid_argument("ternary_device and noise_device must be 16-byte aligned");
        Engine &e = device_engine(ctx);
        op_sample_polys(e, seeds_host, count, n_ternary, n_noise, ternary_device, static_cast<std::size_t>(n_ternary) * e.n,
                        noise_device, static_cast<std::size_t>(n_noise) * e.n);
    });
}

long sealhip_sample_polys_host(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary,
                               uint32_t n_noise, int32_t *out_host, size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(out_host);
    return guarded([&] {
        Engine &e = *ctx->engine; // host work: also on host-only contexts
        const std::size_t stride = check_sample_args(e, n_ternary, n_noise, item_stride_words);
        for (size_t i = 0; i < count; i++)
        {
            uint64_t seed[8];
            std::memcpy(seed, seeds_host + 8 * i, sizeof(seed));
            sample_polys_host(seed, e.n, n_ternary, n_noise, out_host + i * stride);
        }
    });
}

long sealhip_debug_sample_map(sealhip_context *ctx, const uint64_t *words_device, size_t n, int32_t kind, int32_t *out_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(words_device);
    REQUIRE_PTR(out_device);
    return guarded([&] {
        if (kind != 0 && kind != 1)
            throw std::invalid_argument("kind must be 0 (ternary) or 1 (noise)");
        Engine &e = device_engine(ctx);
        op_debug_sample_map(e, reinterpret_cast<const u64 *>(words_device), n, kind == 1, out_device);
    });
}

long sealhip_generate_secret_key(sealhip_context *ctx, const uint64_t seed_host[8], uint64_t *sk_ntt_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seed_host);
    REQUIRE_PTR(sk_ntt_device);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        op_generate_secret_key(e, seed_host, 0, reinterpret_cast<u64 *>(sk_ntt_device));
    });
}

/* ---------------------------------------------------------------- fixed-weight secrets */
// the argument rules the fixed-weight entries share; returns the item stride
static std::size_t check_fixed_weight_args(const Engine &h, uint32_t weight, size_t item_stride_words)
{
    if (weight < 1 || weight > h.n)
        throw std::invalid_argument("h must be 1 .. N");
    return check_sample_args(h, 1, 0, item_stride_words);
}

long sealhip_sample_fixed_weight(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t h, int32_t *out_device,
                                 size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(out_device);
    return guarded([&] {
        const std::size_t stride = check_fixed_weight_args(*ctx->engine, h, item_stride_words);
        if ((stride & 3) || (reinterpret_cast<std::uintptr_t>(out_device) & 15))
            throw std::invalid_argument("out_device must be 16-byte aligned and the item stride a multiple of 4");
        Engine &e = device_engine(ctx);
        op_sample_fixed_weight(e, seeds_host, count, h, out_device, stride);
    });
}

long sealhip_sample_fixed_weight_host(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t h,
                                      int32_t *out_host, size_t item_stride_words)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seeds_host);
    REQUIRE_PTR(out_host);
    return guarded([&] {
        Engine &e = *ctx->engine; // host work: also on host-only contexts
        const std::size_t stride = check_fixed_weight_args(e, h, item_stride_words);
        for (size_t i = 0; i < count; i++)
        {
            uint64_t seed[8];
            std::memcpy(seed, seeds_host + 8 * i, sizeof(seed));
            sample_fixed_weight_host(seed, e.n, h, out_host + i * stride);
        }
    });
}

long sealhip_debug_fixed_weight_map(sealhip_context *ctx, const uint64_t *words_device, size_t n_polys, uint32_t h,
                                    int32_t *out_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(words_device);
    REQUIRE_PTR(out_device);
    return guarded([&] {
        (void)check_fixed_weight_args(*ctx->engine, h, 0);
        if ((reinterpret_cast<std::uintptr_t>(words_device) | reinterpret_cast<std::uintptr_t>(out_device)) & 15)
            throw std::invalid_argument("words_device and out_device must be 16-byte aligned");
        Engine &e = device_engine(ctx);
        op_debug_fixed_weight_map(e, reinterpret_cast<const u64 *>(words_device), n_polys, h, out_device);
    });
}

long sealhip_generate_sparse_secret_key(sealhip_context *ctx, const uint64_t seed_host[8], uint32_t h, uint64_t *sk_ntt_device)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(seed_host);
    REQUIRE_PTR(sk_ntt_device);
    return guarded([&] {
        (void)check_fixed_weight_args(*ctx->engine, h, 0);
        Engine &e = device_engine(ctx);
        op_generate_secret_key(e, seed_host, h, reinterpret_cast<u64 *>(sk_ntt_device));
    });
}

long sealhip_memset_zero(sealhip_context *ctx, void *dptr, size_t bytes)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(dptr);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        if (bytes)
            SEALHIP_CHECK(hipMemsetAsync(dptr, 0, bytes, e.lane().stream));
    });
}

long sealhip_is_data_valid_for(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                               uint8_t *valid)
{
    REQUIRE_PTR(ctx);
    REQUIRE_PTR(ct);
    REQUIRE_PTR(valid);
    return guarded([&] {
        Engine &e = device_engine(ctx);
        check_level(e, k);
        if (count == 0)
            return;
        const RowMap map = ct_row_map(static_cast<int>(k), 1, -1);
        e.ws_reserve(e.lane().ws_floor + count * sizeof(unsigned) + 512);
        e.ws_reset();
        unsigned *flags = reinterpret_cast<unsigned *>(e.ws_alloc((count * sizeof(unsigned) + 7) / 8));
        SEALHIP_CHECK(hipMemsetAsync(flags, 0, count * sizeof(unsigned), e.lane().stream));
        check(launch_out_of_range(e, reinterpret_cast<const u64 *>(ct), static_cast<std::size_t>(size) * k * e.n, count,
                                  map, flags),
              "is_data_valid_for");
        std::vector<unsigned> host(count);
        SEALHIP_CHECK(hipMemcpyAsync(host.data(), flags, count * sizeof(unsigned), hipMemcpyDeviceToHost, e.lane().stream));
        e.sync_and_check();
        for (size_t i = 0; i < count; i++)
            valid[i] = host[i] ? 0 : 1;
    });
}

} // extern "C"
