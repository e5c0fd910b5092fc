/*
 * sealhip.h -- C ABI of the MI355X-native RNS-NTT polynomial engine that replaces the hot path
 * behind seal::Evaluator (Gemini-SEAL, a Microsoft SEAL 3.5.3 fork).
 *
 * Conventions (modelled on the reference's own C export layer, native/src/seal/c/defines.h:34-58):
 *   - every function returns an HRESULT-compatible `long`: S_OK (0) or one of the SEALHIP_E_* codes;
 *     nothing throws across the ABI; sealhip_last_error_string() returns the thread's last message;
 *   - plain pointers and sizes only, no C++/torch types;
 *   - all polynomial data are `uint64_t` matrices in the reference layout: a ciphertext is `size`
 *     polynomials, each a row-major (k x N) matrix, RNS row i of polynomial j at
 *     data + (j*k + i)*N   (native/src/seal/ciphertext.h:359-368, util/iterator.h:746-766);
 *   - a *batch* is `count` such objects stored back to back (the data-parallel axis);
 *   - unless a function name ends in `_host`, every data pointer is a DEVICE pointer (hipMalloc'd,
 *     or a torch CUDA tensor's data_ptr()); work is enqueued on a HIP stream and is asynchronous
 *     until sealhip_synchronize();
 *   - threading: like seal::Evaluator (native/src/seal/evaluator.h:1375-1377) a context is re-entrant.
 *     Every host thread that calls into a context works on its own LANE (HIP stream + temporaries
 *     arena), so operations issued by different threads overlap on the device; operations issued by
 *     one thread run in order. Work of different threads is NOT ordered against each other: hand a
 *     buffer from one thread to another only after sealhip_synchronize() (which waits for every lane);
 *   - a device-side failure (the forward NTT's bounded hand-off wait timing out) is sticky: the next
 *     entry point that makes results host-visible (sealhip_synchronize, sealhip_memcpy_d2h,
 *     sealhip_ciphertext_save, sealhip_is_transparent, sealhip_is_data_valid_for,
 *     sealhip_profile_fetch, the *_host batch entries) returns SEALHIP_E_UNEXPECTED;
 *   - a ciphertext level is addressed by `k` = number of leading coefficient-modulus primes
 *     (the chain drops the last prime per level: native/src/seal/context.cpp:423-431).
 *
 * There is no CPU fallback: without a HIP device every compute entry point fails with
 * SEALHIP_E_UNEXPECTED.
 */
#ifndef SEALHIP_H
#define SEALHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* HRESULT values of native/src/seal/c/defines.h:34-49 */
#define SEALHIP_S_OK 0L
#define SEALHIP_E_POINTER ((long)0x80004003L)
#define SEALHIP_E_INVALIDARG ((long)0x80070057L)
#define SEALHIP_E_OUTOFMEMORY ((long)0x8007000EL)
#define SEALHIP_E_UNEXPECTED ((long)0x8000FFFFL)
#define SEALHIP_COR_E_INVALIDOPERATION ((long)0x80131509L)

/* scheme_type values (native/src/seal/encryptionparams.h:24-34) */
#define SEALHIP_SCHEME_BFV 1u
#define SEALHIP_SCHEME_CKKS 2u

/* PARITY reproduces the reference bit for bit (including SURVEY F2/F3); STRICT is the
   mathematically correct variant (Harvey-corrected butterflies, NTT'd in-bundle rows for BFV). */
#define SEALHIP_MODE_PARITY 0u
#define SEALHIP_MODE_STRICT 1u

/* which RNS base the rows of a polynomial belong to */
#define SEALHIP_BASE_Q 0u   /* the first k coefficient-modulus primes                     */
#define SEALHIP_BASE_BSK 1u /* BEHZ auxiliary base Bsk of level k (B..., m_sk last)       */
#define SEALHIP_BASE_KEY 2u /* k ciphertext primes followed by the nsp special primes     */

typedef struct sealhip_context sealhip_context;
typedef struct sealhip_kswitch_key sealhip_kswitch_key;

/* Plain mirror of what the path needs from EncryptionParameters / SEALContext
   (native/src/seal/encryptionparams.h:205-214,319-322; native/src/seal/context.cpp:455-540). */
typedef struct sealhip_params
{
    uint32_t scheme;           /* SEALHIP_SCHEME_*                                                   */
    uint32_t log_n;            /* log2(poly_modulus_degree), 3..16                                   */
    uint32_t n_key_moduli;     /* |coeff_modulus| at key level (special primes last)                 */
    uint32_t n_special_primes; /* EncryptionParameters::n_special_primes(), >= 1                     */
    const uint64_t *key_moduli;
    uint64_t plain_modulus;    /* BFV only; 0 for CKKS                                               */
    uint32_t mode;             /* SEALHIP_MODE_*                                                     */
    int32_t device;            /* HIP device ordinal; -1 = host-only context (tables, no compute)    */
} sealhip_params;

/* ---------------------------------------------------------------- library / context */
const char *sealhip_last_error_string(void);
long sealhip_num_devices(int32_t *count);
long sealhip_context_create(const sealhip_params *params, sealhip_context **out);
long sealhip_context_destroy(sealhip_context *ctx);
long sealhip_context_first_level(const sealhip_context *ctx, uint32_t *k_first); /* = n_key - nsp */
long sealhip_context_bsk_size(sealhip_context *ctx, uint32_t k, uint32_t *bsk_size); /* |Bsk| of level k */
/* Stream of the CALLING THREAD's lane: a caller-owned hipStream_t (e.g. torch.cuda.Stream().cuda_stream), or NULL to go
   back to a private non-blocking stream. The legacy default stream cannot be named by its handle (it is NULL too): use
   sealhip_use_default_stream for it. */
long sealhip_set_stream(sealhip_context *ctx, void *hip_stream);
long sealhip_use_default_stream(sealhip_context *ctx);
/* waits for the work of every lane of the context (all host threads) and reports a pending device-side failure */
long sealhip_synchronize(sealhip_context *ctx);
/* introspection: lanes (per-thread stream + arena) the context has created so far */
long sealhip_context_lane_count(sealhip_context *ctx, uint32_t *lanes);

/* device memory helpers for hosts that do not bring their own allocator */
long sealhip_malloc(sealhip_context *ctx, size_t bytes, void **dptr);
long sealhip_free(sealhip_context *ctx, void *dptr);
long sealhip_memcpy_h2d(sealhip_context *ctx, void *dst_dev, const void *src_host, size_t bytes);
long sealhip_memcpy_d2h(sealhip_context *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* Pooled, stream-ordered device memory. Blocks come from slabs the pool allocates with hipMalloc (never from
   hipMallocAsync / hipMemPool) and are cached after release instead of being freed.
   - Size classes: a request is rounded up to a multiple of 256 bytes, then to the next m * 2^e with m in {4, 5, 6, 7}
     (four classes per doubling), so a block is less than 25 % larger than the rounded request. 1 byte .. 2^46 bytes.
   - Every lane (calling thread) keeps its own free lists, one per size class. sealhip_pool_release is stream-ordered on
     the calling thread's lane: it never synchronises and never calls hipFree. A later sealhip_pool_alloc on the same
     lane reuses the block with no wait; one on another lane makes its stream wait (hipStreamWaitEvent, no host block) on
     an event recorded at the release. The threading rule above still holds for the words of a block: hand them to
     another thread only after sealhip_synchronize().
   - A miss calls hipMalloc; when the device is out of memory the lane's cached blocks are freed once and the allocation
     retried, then SEALHIP_E_OUTOFMEMORY. A miss during a graph capture is COR_E_INVALIDOPERATION (run the sequence once
     before capturing); the capture is discarded. So is a release during a capture (the graph would keep using the block).
   - Releasing a pointer the pool did not hand out, or releasing it twice, is E_INVALIDARG and frees nothing.
   - sealhip_pool_trim synchronises the context and hipFree's every cached block; sealhip_context_destroy frees every
     block, held ones included. sealhip_pool_stats reports the counters (zeros on a host-only context). */
struct sealhip_pool_stats
{
    uint64_t bytes_in_use;    /* size classes of the blocks handed out and not released            */
    uint64_t bytes_cached;    /* size classes of the blocks on the free lists                        */
    uint64_t device_mallocs;  /* hipMalloc calls the pool made                                        */
    uint64_t device_frees;    /* hipFree calls the pool made (trim, out-of-memory retry)             */
    uint64_t hits;            /* allocations served from a free list (either lane)                   */
    uint64_t misses;          /* allocations that called hipMalloc                                   */
    uint64_t cross_lane_hits; /* hits on a block another lane released (the ones that wait an event)  */
};
long sealhip_pool_alloc(sealhip_context *ctx, size_t bytes, void **dptr);
long sealhip_pool_release(sealhip_context *ctx, void *dptr);
long sealhip_pool_trim(sealhip_context *ctx);
long sealhip_pool_stats(sealhip_context *ctx, struct sealhip_pool_stats *out);
/* stream-ordered device-to-device copy on the calling thread's lane; does not synchronise */
long sealhip_memcpy_d2d(sealhip_context *ctx, void *dst_dev, const void *src_dev, size_t bytes);
/* The transparency read pass of the sink-capable entries (sealhip_transparency_sink) on `count` ciphertexts of `size`
   polynomials at level k, into the installed sink, stream-ordered. The composite entries (multiply_many, exponentiate) and
   the entries without a sink (add_plain, transform_to_ntt / _from_ntt) leave the flags alone; a caller that wants their
   results' flags calls this after them. No sink installed: nothing is done. */
long sealhip_transparency_note(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count);

/* Per-kernel timing with HIP events recorded on the launch stream. While enabled every kernel launch of
   the engine is bracketed by two events; sealhip_profile_fetch synchronises the stream, writes a JSON
   object {"<kernel tag>": {"launches": n, "ms": total, "units": u}, ...} (NUL-terminated) into `json`,
   and clears the records. `units` counts RNS rows for the NTT passes (0 for other kernels). */
long sealhip_profile_enable(sealhip_context *ctx, int32_t enable);
long sealhip_profile_fetch(sealhip_context *ctx, char *json, size_t capacity);

/* Test hook of the forward NTT's sibling hand-off (csrc/ntt.hip): spin_limit = polls before a waiting wave gives up
   (0 restores the default 2^24), suppress_signal != 0 withholds the "finished reading" signal so that every wait times
   out. Used by the tests to prove that the failure surfaces at every host-visible synchronisation point. */
long sealhip_debug_ntt_handoff(sealhip_context *ctx, uint32_t spin_limit, int32_t suppress_signal);

/* How the calling thread's last operations walked their batches: operations whose temporaries do not fit the lane's arena for
   the whole batch process it in chunks of items. Writes up to capacity_pairs (batch size, items per
   chunk) pairs, oldest first, and clears the log (at most the last 64 operations are kept). bench.py uses it to verify the
   first and last item of every chunk of the timed batch against the oracle. One operation logs a second kind of pair:
   sealhip_evaluator_apply_galois_many / _rotate_vector_many, when not even one ciphertext fits the arena with all its Galois
   elements, walk the element list in passes and log (elements, elements per pass) immediately ahead of their
   (batch size, items per chunk) pair -- which is then (count, 1). */
long sealhip_debug_chunk_log(sealhip_context *ctx, size_t *count_chunk_pairs, size_t capacity_pairs, size_t *written);

/* Measurement hook (bench.py roofline.valu_ceiling): the rate at which this device executes nothing but the butterflies of
   the single-pass NTT kernels (same instruction sequences, values and twiddles in registers, same launch bounds) on the
   prime `prime_index` (numbering of sealhip_debug_ntt_table). kind: 0 the reference's lazy forward butterfly
   (ntt.cpp:245-252, exact Shoup quotient), 1 / 2 the approximate-quotient forms (csrc/ntt_bounds.hpp section 2), 3 the
   FP64 butterfly (primes below 2^50), 4 / 5 the inverse butterfly (lazy sums with the level-2 quotient / ntt.cpp:265-272).
   A row of N coefficients is N/2 log2 N butterflies: rate / that = the transform's arithmetic ceiling in rows per second. */
long sealhip_debug_butterfly_rate(sealhip_context *ctx, uint32_t kind, uint32_t prime_index, double *butterflies_per_s);

/* Introspection of the precomputed tables (works on host-only contexts; used by the CPU tests).
   kind: 0 root_powers, 1 scaled_root_powers, 2 inv_root_powers (reference order, n^-1 merged),
   3 scaled_inv_root_powers; prime_index: 0..n_key-1 key primes, n_key.. = 60-bit auxiliary primes
   in get_primes order (m_sk, gamma, B_0, B_1, ...). */
long sealhip_debug_ntt_table(sealhip_context *ctx, uint32_t prime_index, uint32_t kind, uint64_t *out_host,
                             size_t capacity);
/* which: 0 Bsk primes, 1 inv_prod_q_mod_Bsk, 2 prod_q_mod_Bsk, 3 inv_m_tilde_mod_Bsk, 4 prod_B_mod_q,
   5 inv_q_last_mod_q, 6 {inv_prod_q_mod_m_tilde, inv_prod_B_mod_m_sk, m_sk, gamma},
   7 q->Bsk matrix (row-major [Bsk][q]), 8 B->q matrix ([q][B]), 9 q inv_punctured, 10 B inv_punctured,
   11 q->m_tilde row, 12 B->m_sk row */
long sealhip_debug_rns_constants(sealhip_context *ctx, uint32_t k, uint32_t which, uint64_t *out_host,
                                 size_t capacity, size_t *written);
/* The dispatch of a BFV multiply (square != 0: the square of one size-2 operand) at level k with operands of sizes size_a
   and size_b (works on host-only contexts). out[0..12]: k, |B|, |Bsk|, square, redc_small, gather, defer, fused_tensor,
   tensor_apx, lift_top, lift instance, floor instance, deferred_top; instance 1..15 is the exact-k kernel, 32 the run-time-k
   kernel, 64 the step-by-step kernels. */
long sealhip_debug_bfv_multiply_plan(sealhip_context *ctx, uint32_t k, uint32_t size_a, uint32_t size_b, int32_t square,
                                     int32_t *out);
/* The split position (30 or 31) of the carry-free dot products of the exact-k BEHZ kernels at level k of a BFV context:
   what the level's constant tables are packed with (host-only contexts: would be packed with). 31 at k above 15. */
long sealhip_debug_behz_dot_split(sealhip_context *ctx, uint32_t k, int32_t *out);
/* Does a key switch whose inner product consumes the digit rows directly (relinearize, apply_galois, switch_key) store the
   digit rows of a chunk of `count` items at level k without the forward transform's last layer, which the inner product's
   pair form then applies? *out = 1 or 0. Device contexts. */
long sealhip_debug_ks_split_last(sealhip_context *ctx, uint32_t k, size_t count, int32_t *out);
/* One forward transform without its last layer, as the key switch launches it: the N words at src_device, taken as a row
   on key prime `prime_index` (load treatment 0 none, 1 Barrett-63, 2 one conditional subtraction; exact != 0: the exact
   Shoup quotient instead of the approximate one), go to dst_device (another buffer of N words) as E[0..N/2) | O[0..N/2): the
   transforms, as rings of N/2, of the even- and the odd-indexed words, any representative below
   (2 + 4 (log2 N - 1)) p. E_INVALIDARG where the form does not exist (rings other than 2^14..2^16, a prime outside its bound
   or one that the floating-point instances take). */
long sealhip_debug_ntt_split_last(sealhip_context *ctx, uint32_t prime_index, uint32_t treatment, int32_t exact,
                                  const uint64_t *src_device, uint64_t *dst_device);

/* ---------------------------------------------------------------- L2: NTT (util/ntt.h:189-368)
   data: count polynomials x rows x N, in place. `base` selects the primes of the `rows` rows of one
   polynomial: BASE_Q -> rows = k; BASE_BSK -> rows = |Bsk|(k); BASE_KEY -> rows = k + nsp.
   Operand ranges are what the reference's butterflies are written for (ntt.cpp:245-281, :341): forward inputs below 4p, inverse inputs below 2p.
   The `_lazy` entries reproduce the reference's representatives word for word (including the wrapped words of the
   60-bit Bsk rows). The canonicalising entries return the residues those words reduce to; on rows whose prime
   is below 2^50 they are computed with exact double-precision butterflies, which for operands
   inside the ranges above is the same function -- for words outside them (>= 2^52) both the reference's output and this
   one are meaningless, and they differ. Likewise the canonicalising forward entry on primes below 2^58 runs a cheaper
   exact schedule (approximate Shoup quotients, one reduction in the store) that is proved for inputs below 4p
   (csrc/ntt_bounds.hpp: fwd_canon_admits); SEALHIP_NTT_CANON_EXACT=1 runs the reference's own sequence instead, whose
   deterministic wrap-around on larger words is then reproduced as well. */
long sealhip_ntt_negacyclic_harvey_lazy(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k,
                                        uint32_t base);
long sealhip_ntt_negacyclic_harvey(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k, uint32_t base);
long sealhip_inverse_ntt_negacyclic_harvey_lazy(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k,
                                                uint32_t base);
long sealhip_inverse_ntt_negacyclic_harvey(sealhip_context *ctx, uint64_t *data, size_t count, uint32_t k,
                                           uint32_t base);

/* ---------------------------------------------------------------- L2: coefficient-wise (util/polyarithsmallmod.{h,cpp})
   operands: count polynomials x rows x N of the given base/level; result may alias an operand.
   Operand ranges (p = the row's prime; results are canonical, below p; tests/test_gpu_linear_layer.py covers exactly these):
     dyadic_product: a any 64-bit word (lazy NTT outputs), b below p;
     multiply_poly_scalar: a and scalar any 64-bit word (the reference reduces the 128-bit product, polyarithsmallmod.cpp:35-60);
     add, sub, negate: operands below p (one conditional correction, polyarithsmallmod.h:176-205, :261-299, :366-404). */
long sealhip_dyadic_product_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count,
                                     uint32_t k, uint32_t base, uint64_t *result);
long sealhip_multiply_poly_scalar_coeffmod(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k,
                                           uint32_t base, uint64_t scalar, uint64_t *result);
long sealhip_add_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint32_t k,
                               uint32_t base, uint64_t *result);
long sealhip_sub_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, const uint64_t *b, size_t count, uint32_t k,
                               uint32_t base, uint64_t *result);
long sealhip_negate_poly_coeffmod(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k, uint32_t base,
                                  uint64_t *result);

/* ---------------------------------------------------------------- L2: RNSTool (util/rns.cpp:731-1068), level k, batched
   shapes per item:  fastbconv_m_tilde k x N -> (|Bsk|+1) x N;  sm_mrq (|Bsk|+1) x N -> |Bsk| x N;
   fast_floor (k+|Bsk|) x N -> |Bsk| x N;  fastbconv_sk |Bsk| x N -> k x N;
   divide_and_round_q_last[_ntt]_inplace: k x N in place (last row clobbered). */
long sealhip_fastbconv_m_tilde(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out);
long sealhip_sm_mrq(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out);
long sealhip_fast_floor(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out);
long sealhip_fastbconv_sk(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out);
long sealhip_divide_and_round_q_last_inplace(sealhip_context *ctx, uint32_t k, uint64_t *data, size_t count);
long sealhip_divide_and_round_q_last_ntt_inplace(sealhip_context *ctx, uint32_t k, uint64_t *data, size_t count);

/* ---------------------------------------------------------------- L2: Galois (util/galois.cpp) */
long sealhip_galois_elt_from_step(const sealhip_context *ctx, int32_t step, uint32_t *galois_elt);
/* coefficient form (galois.cpp:144-186) / NTT form (:188-214); in and out must not alias. galois_elt: any odd element of
   [1, 2N), the identity 1 included; anything else is E_INVALIDARG. Coefficient form: words below the row's prime (the sign
   flip is p - v, and 0 stays 0); NTT form: a permutation of whatever words it is given. */
long sealhip_apply_galois(sealhip_context *ctx, const uint64_t *in, size_t count, uint32_t k, uint32_t galois_elt,
                          uint64_t *out);
long sealhip_apply_galois_ntt(sealhip_context *ctx, const uint64_t *in, size_t count, uint32_t k,
                              uint32_t galois_elt, uint64_t *out);

/* ---------------------------------------------------------------- hybrid key switch (multi_special_primes.cpp, evaluator.cpp:2259-2368) */
/* Key in the K1 layout of KeyGenerator::generate_one_kswitch_key (keygenerator.cpp:325-369):
   n_digits x 2 x n_key x N uint64 (digit, component, key-level row, coefficient). The key is copied
   to the device (from host memory if from_host != 0) and stays resident until destroyed. */
long sealhip_kswitch_key_load(sealhip_context *ctx, const uint64_t *key, uint32_t n_digits, int32_t from_host,
                              sealhip_kswitch_key **out);
long sealhip_kswitch_key_destroy(sealhip_context *ctx, sealhip_kswitch_key *key);
/* modup_rns (multi_special_primes.cpp:151-185): ext is count x (k+nsp) x N; the rows of bundle
   `src_bundle_index` are the input, every other row is overwritten. */
long sealhip_modup_rns(sealhip_context *ctx, uint32_t k, uint32_t src_bundle_index, uint64_t *ext, size_t count);
/* rescale_special_rns_inplace (multi_special_primes.cpp:237-304): poly is count x (k+nsp) x N */
long sealhip_rescale_special_rns_inplace(sealhip_context *ctx, uint32_t k, uint64_t *poly, size_t count);
/* switch_key_inplace: ct is count x 2 x k x N (updated in place), target count x k x N */
long sealhip_switch_key_inplace(sealhip_context *ctx, uint32_t k, uint64_t *ct, const uint64_t *target, size_t count,
                                const sealhip_kswitch_key *key);
/* switch_key_inplace in "latency mode" (SURVEY 8e): the d = ceil(k / nsp) decomposition digits (keygenerator.cpp:334-336;
   sealhip_kswitch_digits) of ONE key switch shared out over several devices, the key replicated on each. Every device calls
   _partial for its digits [digit_begin, digit_end): mod-up, forward transforms and the 128-bit inner product of
   evaluator.cpp:2302-2349 over those digits only, reduced to canonical residues -> partial = count x 2 x (k + nsp) x N words.
   The caller adds the partials of all devices element-wise (an all-reduce with SUM on 64-bit words: ranks * p < 2^63 cannot
   wrap) and hands the sum to _finish on the device(s) that need the result: one more reduction, then :2351-2366 as in the
   unsplit operation (partial_sum is clobbered). Modular sums are associative, so the result is word for word the unsplit one.
   n_partials = how many partials were summed (the world size of the all-reduce): _finish reduces with barrett_reduce_63 and
   returns E_INVALIDARG when n_partials * max(key prime) could reach 2^63 (61-bit primes: more than 4). Measured with one
   device only; the multi-device run is tools/latency_mode.py under torch.distributed. */
long sealhip_switch_key_partial(sealhip_context *ctx, uint32_t k, const uint64_t *target, size_t count,
                                const sealhip_kswitch_key *key, uint32_t digit_begin, uint32_t digit_end, uint64_t *partial);
long sealhip_switch_key_finish(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint64_t *partial_sum, size_t count,
                               uint32_t n_partials);
long sealhip_kswitch_digits(sealhip_context *ctx, uint32_t k, uint32_t *digits);

/* ---------------------------------------------------------------- L4: Evaluator operations (native/src/seal/evaluator.h)
   All are batched over `count` independent ciphertexts at level k. */
/* Evaluator::multiply (evaluator.cpp:235-527): a (size_a polys), b (size_b polys) -> out (size_a+size_b-1).
   BFV: coefficient form in/out (bfv_multiply); CKKS: NTT form (ckks_multiply). out must not alias a or b. */
long sealhip_evaluator_multiply(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a,
                                const uint64_t *b, uint32_t size_b, size_t count, uint64_t *out);
/* Evaluator::square (evaluator.cpp:529-770) */
long sealhip_evaluator_square(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, size_t count,
                              uint64_t *out);
/* Evaluator::relinearize (evaluator.cpp:772-827): ct has `size` polys and is reduced in place to 2;
   relin_keys[i] is the key at RelinKeys::get_index(i + 2) (relinkeys.h:61-68). The batch stride stays
   size x k x N. */
long sealhip_evaluator_relinearize(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                   const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys);
/* Evaluator::mod_switch_to_next (evaluator.cpp:996-1036): BFV divide-and-round, CKKS drop.
   out: count x size x (k-1) x N */
long sealhip_evaluator_mod_switch_to_next(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                          size_t count, uint64_t *out);
/* Evaluator::rescale_to_next (evaluator.cpp:1090-1126), CKKS only */
long sealhip_evaluator_rescale_to_next(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                       size_t count, uint64_t *out);
/* The same two operations on ciphertexts that sit `ct_item_stride` words apart (>= size * k * N): the size-2 result of
   relinearize inside its size-3 product, so that multiply -> relinearize -> mod_switch_to_next over a contiguous device batch
   needs no compaction pass in between. The reference's ciphertexts are separate objects (ciphertext.h:709-721); a contiguous
   batch takes the stride instead ("a contiguous batch with stride"). `out` is compact (size * (k-1) * N per item). */
long sealhip_evaluator_mod_switch_to_next_strided(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                                  size_t ct_item_stride, size_t count, uint64_t *out);
long sealhip_evaluator_rescale_to_next_strided(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                               size_t ct_item_stride, size_t count, uint64_t *out);
/* Evaluator::apply_galois_inplace (evaluator.cpp:1841-1943): ct is count x 2 x k x N */
long sealhip_evaluator_apply_galois(sealhip_context *ctx, uint32_t k, uint64_t *ct, size_t count,
                                    uint32_t galois_elt, const sealhip_kswitch_key *galois_key);
/* Evaluator::transform_to_ntt_inplace / transform_from_ntt_inplace (evaluator.cpp:1746-1839) */
long sealhip_evaluator_transform_to_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count);
long sealhip_evaluator_transform_from_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size,
                                          size_t count);

/* Evaluator::multiply_many (evaluator.cpp:1180-1255), BFV: encrypteds[0..n) are device batches of count size-2 ciphertexts
   ([count][2][k][N]); out receives their product, relinearized after every multiplication, in the reference's queue order
   (neighbours left to right, an odd last operand appended, products of products until one is left). relin_keys as in
   sealhip_evaluator_relinearize. out must not be one of the operands. Asynchronous (stream-ordered temporaries). */
long sealhip_evaluator_multiply_many(sealhip_context *ctx, uint32_t k, const uint64_t *const *encrypteds, uint32_t n_encrypteds,
                                     size_t count, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                     uint64_t *out);
/* Evaluator::exponentiate_inplace (evaluator.cpp:1257-1288): multiply_many over `exponent` copies; E_INVALIDARG for 0. */
long sealhip_evaluator_exponentiate(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint64_t exponent, size_t count,
                                    const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out);

/* ---------------------------------------------------------------- batches of separately allocated HOST ciphertexts
   What the reference's objects look like from C: a std::vector<seal::Ciphertext> is one separately allocated buffer per
   ciphertext (Ciphertext::data() of each element; native/src/seal/ciphertext.h:327-392,709-721). These entries take arrays of
   HOST pointers, one per ciphertext, and pipeline the batch through the device in chunks (SEALHIP_HOST_CHUNK, default 64):
   host threads gather the caller's buffers into pinned staging memory, host->device copy, the operation and device->host
   copy run on three HIP streams with two staging slots, host threads scatter the results -- so PCIe traffic in both
   directions overlaps the kernels. The calls return when every result is in the caller's buffers (they synchronise and
   report device-side failures). The library never frees or reallocates caller memory: every out[i] must already have room.

   Evaluator::multiply (evaluator.cpp:235-527) per pair (a[i], b[i]) -> out[i]. With relin_keys != NULL the product is
   relinearized before it leaves the device (Evaluator::relinearize_inplace, :772-827; relin_keys as in
   sealhip_evaluator_relinearize) and out[i] receives 2 polynomials; otherwise size_a + size_b - 1. */
long sealhip_evaluator_multiply_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *a, uint32_t size_a,
                                     const uint64_t *const *b, uint32_t size_b, size_t count, uint64_t *const *out,
                                     const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys);
/* Evaluator::relinearize_inplace: ct[i] holds `size` polynomials on entry; its first 2 polynomials are the result (the
   caller shrinks its object, evaluator.cpp:819). */
long sealhip_evaluator_relinearize_host(sealhip_context *ctx, uint32_t k, uint64_t *const *ct, uint32_t size, size_t count,
                                        const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys);
/* Evaluator::rotate_vector_inplace / rotate_rows_inplace (evaluator.h:1201-1239) on size-2 ciphertexts, in place; keys as in
   sealhip_evaluator_rotate_vector. */
long sealhip_evaluator_rotate_vector_host(sealhip_context *ctx, uint32_t k, uint64_t *const *ct, size_t count, int32_t steps,
                                          const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                          uint32_t n_keys);
/* Evaluator::mod_switch_to_next / rescale_to_next: ct[i] (size x k x N) -> out[i] (size x (k-1) x N) */
long sealhip_evaluator_mod_switch_to_next_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *ct, uint32_t size,
                                               size_t count, uint64_t *const *out);
long sealhip_evaluator_rescale_to_next_host(sealhip_context *ctx, uint32_t k, const uint64_t *const *ct, uint32_t size,
                                            size_t count, uint64_t *const *out);

/* Pins the caller's range [ptr, ptr + bytes) in place (hipHostRegister, visible to every device) and remembers it. A *_host
   entry whose item buffers of an array all lie inside registered ranges skips that array's staging copy: the DMA engine reads /
   writes the caller's buffers themselves, which takes the host threads (the bound of the pageable path) out of the transfer.
   Meant for memory the caller keeps -- the reference's ciphertexts come from a MemoryPool whose blocks are allocated at
   native/src/seal/util/mempool.cpp:45 and :145 and reused for the life of the pool: register a block once where it is
   allocated, unregister it where the pool frees it. Pinning costs far more than one copy, so registering a buffer for a single
   call does not pay. E_INVALIDARG: empty range, a range that overlaps a registered one, (unregister) a pointer that is not the
   start of a registered range; HIP's refusal (e.g. a locked-memory limit) -> E_UNEXPECTED with its message. The caller must not
   unregister or free a range while a *_host call that uses it is running. */
long sealhip_host_register(sealhip_context *ctx, void *ptr, size_t bytes);
long sealhip_host_unregister(sealhip_context *ctx, void *ptr);

/* ---------------------------------------------------------------- Evaluator surface beyond the hot path */
/* Ciphertext batches [count][size][k][N], words below their row's prime; sizes from 1 on, 0 is E_INVALIDARG.
   Evaluator::negate_inplace (evaluator.cpp:65-88); out may alias ct. */
long sealhip_evaluator_negate(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                              uint64_t *out);
/* Evaluator::add_inplace (evaluator.cpp:90-151) / sub_inplace (:174-233): out has max(size_a, size_b) polynomials per
   ciphertext; the tail of the longer operand is copied (add) or, when it is b's, negated (sub, :216-220).
   out may alias a when size_a >= size_b. */
long sealhip_evaluator_add(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                           uint32_t size_b, size_t count, uint64_t *out);
long sealhip_evaluator_sub(sealhip_context *ctx, uint32_t k, const uint64_t *a, uint32_t size_a, const uint64_t *b,
                           uint32_t size_b, size_t count, uint64_t *out);
/* Evaluator::multiply_plain_ntt (evaluator.cpp:1605-1646): every polynomial of every ciphertext times a plaintext in
   NTT form (k x N), in place. plain_stride = words between the plaintexts of consecutive ciphertexts, 0 = one
   plaintext for the whole batch. Ciphertext and plaintext words below their row's prime. */
long sealhip_evaluator_multiply_plain_ntt(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                          const uint64_t *plain_ntt, size_t plain_stride);
/* Evaluator::multiply_plain_normal (evaluator.cpp:1475-1603), BFV, coefficient form, in place. plain = N coefficients
   in [0, t) per plaintext (plain_stride as above). Requires every q_i > t ("fast plain lift", context.cpp:297-301);
   otherwise COR_E_INVALIDOPERATION. */
long sealhip_evaluator_multiply_plain(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                      const uint64_t *plain, size_t plain_stride);
/* Evaluator::transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744), BFV: plaintext i = plain_coeff_count
   coefficients < t at plain + i * plain_stride (0 = plain_coeff_count); plain_ntt[count][k][N] receives it lifted to
   level k and in NTT form. Coefficients >= t: unspecified words (as multiply_plain). Device memory. Every parameter set,
   with or without fast plain lift: (v - t [v >= (t+1)/2]) mod q_i, the residue both reference branches compute. CKKS:
   E_INVALIDARG for plain_coeff_count > 0 (plain_modulus 0, valcheck.cpp:266-279); an empty plaintext gives zero rows.
   E_INVALIDARG also for plain_coeff_count > N, a nonzero stride below it, and plain overlapping plain_ntt. count 0 does
   nothing. Runs on the calling thread's lane and synchronises nothing (capturable). */
long sealhip_evaluator_transform_plain_to_ntt(sealhip_context *ctx, uint32_t k, const uint64_t *plain,
                                              size_t plain_coeff_count, size_t plain_stride, size_t count,
                                              uint64_t *plain_ntt);
/* Evaluator::mod_switch_to(_inplace)(Plaintext, parms_id) / mod_switch_to_next (evaluator.cpp:959-994, 1062-1088):
   NTT-form plain[count][k_from][N] -> out[count][k_to][N], the leading k_to rows of each (Plaintext::resize). E_INVALIDARG
   "cannot switch to higher level modulus" for k_to > k_from, "end of modulus switching chain reached" for k_to < 1. */
long sealhip_evaluator_mod_switch_plain_to(sealhip_context *ctx, uint32_t k_from, const uint64_t *plain, size_t count,
                                           uint32_t k_to, uint64_t *out);
/* Ciphertext::is_transparent (ciphertext.h:471-476) per ciphertext of the batch: transparent[i] = 1 when polynomials
   1.. are identically zero (or size < 2). `transparent` is HOST memory (count bytes); the call synchronises.
   The reference throws logic_error("result ciphertext is transparent") after every operation when built with
   SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT (evaluator.cpp:265-271); the adapter does the same with this flag. */
long sealhip_is_transparent(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                            uint8_t *transparent);
/* The same test as a FLAG OUTPUT of the operations ("provide it as a flag output of the kernels"; replaces the
   read pass of Ciphertext::is_transparent that evaluator.cpp:265-271 runs after every operation). `nonzero_flags` is DEVICE
   memory, `capacity` 32-bit words; it belongs to the calling thread's lane of the context until it is replaced or removed
   (nullptr). While a sink is set, every sealhip_evaluator_* entry that produces ciphertexts first clears flags[0 .. count) and
   then makes flags[i] non-zero iff polynomials 1.. of result i hold a non-zero word: multiply, square, relinearize and
   apply_galois note it in the kernel that stores those polynomials anyway (no pass over the result); mod_switch_to_next,
   rescale_to_next, rotate_vector, add, sub, negate and multiply_plain(_ntt) run the read pass on their result, on the stream.
   A batch larger than `capacity` is E_INVALIDARG. Nothing synchronises: read the flags after sealhip_synchronize (or on the
   lane's stream). Composite entries (multiply_many, exponentiate, the *_host batches) leave the flags alone. */
long sealhip_transparency_sink(sealhip_context *ctx, uint32_t *nonzero_flags, size_t capacity);
/* modulo_poly_coeffs_63 (polyarithsmallmod.h:98-120): Barrett-63 reduction of rows with values < 2^63 */
long sealhip_modulo_poly_coeffs_63(sealhip_context *ctx, const uint64_t *a, size_t count, uint32_t k, uint32_t base,
                                   uint64_t *result);
/* Evaluator::rotate_vector_inplace / rotate_rows_inplace -> rotate_internal (evaluator.cpp:1945-2000): the key for
   the step's Galois element if the caller holds it, else the non-adjacent-form decomposition (util/numth.h:22-42).
   galois_elts[i] is the Galois element of galois_keys[i]. */
long sealhip_evaluator_rotate_vector(sealhip_context *ctx, uint32_t k, uint64_t *ct, size_t count, int32_t steps,
                                     const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                     uint32_t n_keys);

/* Hoisted rotation (Halevi-Shoup): every ciphertext of the batch under n_elts Galois elements with ONE
   decomposition of c_1. Of apply_galois_inplace + switch_key_inplace (evaluator.cpp:1841-1943, 2259-2368) the inverse
   transform, the mod-up and the forward transforms of the digits do not depend on the element and run once; per element
   remain the inner product with the key, sigma_g(c_0) and the mod-down. The fork has no such method, and the result is NOT
   the words of n_elts calls of sealhip_evaluator_apply_galois (the automorphism does not commute with the mod-up): it
   decrypts to the same plaintext with noise of the same bound. What defines it, word for word in the context's mode, is the
   restatement over the oracle in tests/hoist_ref.py: with D_j the rows switch_key_inplace multiplies with digit j of the key
   for target c_1 (:2302-2322) and T_g the NTT-form table of the element (galois.cpp:18-47),
       prod_g[l][r][c] = ( sum_j D_j[r][T_g[c]] * K_g[j][l][row_prime r][c] ) mod p_r   (canonical),
       out_g = the key switch's finish (:2351-2366) of prod_g added into (sigma_g(c_0), 0).
   CKKS in both modes and BFV in STRICT mode; BFV in PARITY mode is E_INVALIDARG (that key switch, SURVEY F3, does not
   decrypt, and there is no reference behaviour to reproduce for an operation the fork does not have).
   ct: count x 2 x k x N, not modified; out: n_elts x count x 2 x k x N, ELEMENT-major (each rotation is a contiguous batch);
   out must not overlap ct. galois_keys[i] is the key of galois_elts[i].
   Checks: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, an even element or
   one >= 2N, a key with fewer digits than the level, BFV in PARITY mode -> E_INVALIDARG; then n_elts == 0 or count == 0 ->
   S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION. With a transparency sink: one flag per output
   ciphertext, in output order (n_elts * count flags). Nothing synchronises; capturable once the Galois tables of the
   elements are resident (after one call with them), as sealhip_evaluator_apply_galois. */
long sealhip_evaluator_apply_galois_many(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                         const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                         uint32_t n_elts, uint64_t *out);
/* The same by rotation steps (galois_elt_from_step, galois.cpp:49-91): out: n_steps x count x 2 x k x N. A step of 0 is a
   copy of the input, wherever it stands in the list: all other steps still share one decomposition. galois_elts[i] is the Galois element of galois_keys[i] (n_keys of them); a step whose key is absent
   -> E_INVALIDARG ("Galois key not present"): there is no non-adjacent-form fallback here, a chain of dependent rotations
   cannot share a decomposition. Otherwise as sealhip_evaluator_apply_galois_many (S_OK without work when n_steps == 0). */
long sealhip_evaluator_rotate_vector_many(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                          const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                          const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, uint64_t *out);

/* Ring packing: one coefficient of a ciphertext as an LWE sample, and n = 2^l such samples packed into
   one ciphertext -- PackLWEs and the field trace of Chen, Dai, Kim, Song, "Efficient Homomorphic Conversion Between (Ring)
   LWE Ciphertexts" (Alg. 2 and 3) in iterative, batched order. The fork has no such method: what defines the words is the
   restatement over the oracle in tests/ring_pack_ref.py. Every word in and out is a canonical residue; -v is q_r - v, -0 = 0.
     sample of coefficient j of (c_0, c_1) in coefficient form:  b = c_0[j];  a[i] = c_1[j - i] for i <= j, -c_1[N + j - i]
       for i > j;  then b + <a, s> = (c_0 + c_1 s)[j] modulo every q_r.  lwe_a[count][n][k][N], lwe_b[count][n][k].
     embedding of a sample, scaled by w_r:  c_0 = w_r b at coefficient 0;  c_1[0] = w_r a[0], c_1[N - i] = -w_r a[i].
     pack of n = 2^l samples, W the n embeddings:  for t = 1 .. l, half = 2^(l - t), g = 2^t + 1, and for j < half:
       E = W[j], O = X^(N / 2^t) W[j + half], W'[j] = (E + O) + apply_galois(E - O, g) (sealhip_evaluator_apply_galois).
       Coefficient (N / n) j of the result's phase is n w phase_j.
     trace (optional):  for t = l + 1 .. log N:  W = W + apply_galois(W, 2^t + 1). Then coefficient (N / n) j holds
       N w phase_j and every other coefficient of the phase is the key switches' noise alone.
     normalize (optional):  w_r = n^{-1} mod q_r, or N^{-1} mod q_r with the trace; otherwise w_r = 1.
   Every step is ONE streaming kernel, which forms (E + O) + (sigma_g(E_0 - O_0), 0) and the key switch's target
   sigma_g(E_1 - O_1) in one pass over the operands, and ONE key switch batched over count * half ciphertexts: n - 1 key
   switches per item, plus log N - l with the trace. The sums are exact and only reordered: the words are those of the
   composition above. BFV works in coefficient form and needs a STRICT context (BFV in PARITY mode is E_INVALIDARG, as for
   apply_galois_many); CKKS works in NTT form: extract transforms a temporary copy back (ct is not modified), pack transforms
   the embedded c_1 rows forward and merges in NTT form.

   sealhip_pack_lwes_galois_elts: the elements 2^t + 1 the pack of n samples needs, ascending (t = 1 .. l, or 1 .. log N with
   trace), for sealhip_generate_galois_keys. *n_elts gets their number; elts (HOST, may be NULL to ask for the number alone)
   gets them when capacity suffices. Works on host-only contexts. Checks: NULL ctx or n_elts -> E_POINTER; n not a power of
   two in [1, N], elts given with capacity < *n_elts -> E_INVALIDARG.

   sealhip_evaluator_extract_lwe: ct: count x 2 x k x N in the scheme's form, not modified; indices_host: n_idx HOST words,
   each < N, in any order, repeats allowed; every item yields n_idx samples. Checks, in this order: NULL pointers
   (indices_host only when n_idx > 0) -> E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, an
   index >= N, lwe_a not 16-byte aligned, lwe_a or lwe_b overlapping ct or each other -> E_INVALIDARG; then count == 0 or
   n_idx == 0 -> S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION. The indices are staged into a
   pool block: the entry may allocate and is NOT capturable. No transparency flags (the outputs are not ciphertexts).

   sealhip_evaluator_pack_lwes: lwe_a: count x n x k x N, lwe_b: count x n x k, only read; out: count x 2 x k x N in the
   scheme's form. galois_elts[i] is the element of galois_keys[i] (n_keys of them; keys the pack does not need are ignored).
   Checks, in this order: NULL pointers (every key of the list) -> E_POINTER; then, also on host-only contexts, k outside the
   ciphertext levels, n not a power of two in [1, N], BFV in PARITY mode, an even listed element or one >= 2N, a needed
   element without its key ("Galois key not present"), a needed key with fewer digits than the level, lwe_a or out not
   16-byte aligned, out overlapping lwe_a or lwe_b -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a
   host-only context -> COR_E_INVALIDOPERATION. The working set (1.5 n + n / 4 ciphertexts per item) is parked in the lane's
   arena next to the key switch's and takes at most half of the arena's cap (the key switch plans with the whole cap, so
   the arena can reach 1.5 times the cap during a pack). A batch that does not fit is walked in chunks of items; one item
   that does not fit is walked over its samples (the first step embeds and merges {j, j + n/2} for a group of j at a
   time: the same words); sealhip_debug_chunk_log shows both. When even the first two steps' results of one item
   (0.875 n ciphertexts) do not fit -> E_OUTOFMEMORY with a message that names both sizes (raise SEALHIP_WORKSPACE_MB or
   pack fewer samples). With a transparency sink: one flag per output ciphertext, from the last key switch, or from a read pass over
   out when there is none (n == 1 without trace, the embedding alone). Nothing synchronises; capturable once the Galois
   tables and the monomial rows are resident (after one call of the same shape). */
long sealhip_pack_lwes_galois_elts(sealhip_context *ctx, size_t n, int32_t trace, uint32_t *elts, uint32_t capacity,
                                   uint32_t *n_elts);
long sealhip_evaluator_extract_lwe(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                   const uint32_t *indices_host, size_t n_idx, uint64_t *lwe_a, uint64_t *lwe_b);
long sealhip_evaluator_pack_lwes(sealhip_context *ctx, uint32_t k, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t n,
                                 size_t count, const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                 uint32_t n_keys, int32_t trace, int32_t normalize, uint64_t *out);

/* Oblivious expansion: one ciphertext whose phase carries n = 2^l values in its first n coefficients
   into n ciphertexts, one per coefficient -- the Expand of Angel, Chen, Laine, Setty, "PIR with compressed queries and
   amortized query processing" (Fig. 3), which is the coefficient extraction tree of Chen, Dai, Kim, Song; the other
   direction of the ring packing above. The fork has no such method: what defines the words is the restatement over the
   oracle in tests/expand_ref.py. The ring is Z_q[X]/(X^N + 1), rows are the level's primes q_r, r < k; every word in and
   out is a canonical residue; -v is q_r - v, -0 = 0.
     W_0[0] = the input (a size-2 ciphertext), times w_r.  For t = 1 .. l with cur = 2^(t-1), s = cur and
     g = N / 2^(t-1) + 1 (the elements N + 1, N / 2 + 1, ...), and for j < cur, E = W[j], O = X^(-s) E:
       W'[j]       = E + apply_galois(E, g)          (sealhip_evaluator_apply_galois)
       W'[j + cur] = O + apply_galois(O, g).
     After l steps the phase of output i is n w sum_u m[i + n u] X^(n u), m the input's phase: when the phase lives in the
     coefficients below n, output i holds the constant n w m[i]. Outputs are in natural order.
     normalize:  w_r = n^{-1} mod q_r (multiply_poly_scalar_coeffmod on both input polynomials), so that the factor n cancels
       exactly modulo q, the input's noise is not amplified and BFV decrypts to m[i] itself; otherwise w_r = 1. n = 1 is a copy.
   Key-switch noise of step t is multiplied by at most n / 2^t by the steps after it. Every step is ONE streaming kernel,
   which for every source E writes (E_0 + sigma_g(E_0), E_1), (O_0 + sigma_g(O_0), O_1) and the key switch's targets
   sigma_g(E_1), sigma_g(O_1) in one pass, and ONE key switch batched over all count * 2^t results: the sums are exact and
   only reordered, so the words are those of the composition above. BFV works in coefficient form and needs a STRICT
   context; CKKS works in NTT form in both modes (X^(-s) . is a dyadic product with NTT_r(X^(-s)), rows built once per
   context).

   sealhip_expand_galois_elts: the elements the expansion into n needs, ascending (N / 2^(l-1) + 1 .. N + 1), for
   sealhip_generate_galois_keys. *n_elts gets their number; elts (HOST, may be NULL to ask for the number alone) gets them
   when capacity suffices. Works on host-only contexts. Checks: NULL ctx or n_elts -> E_POINTER; n not a power of two in
   [1, N], elts given with capacity < *n_elts -> E_INVALIDARG.

   sealhip_evaluator_expand: ct: count x 2 x k x N in the scheme's form, only read; out: count x n x 2 x k x N.
   galois_elts[i] is the element of galois_keys[i] (n_keys of them; keys the expansion does not need are ignored). Checks,
   in this order: NULL pointers (every key of the list) -> E_POINTER; then, also on host-only contexts, k outside the
   ciphertext levels, n not a power of two in [1, N], BFV in PARITY mode, an even listed element or one >= 2N, a needed
   element without its key ("Galois key not present"), a needed key with fewer digits than the level, ct or out not 16-byte
   aligned, out overlapping ct -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only context ->
   COR_E_INVALIDOPERATION. The working set (3 n / 4 ciphertexts and n target polynomials per item) is parked in the lane's
   arena next to the key switch's and takes at most half of the arena's cap, as the pack's does. A batch that does not fit
   is walked in chunks of items; one item that does not fit has its last step walked in groups of c sources, c the largest
   power of two that fits (subtrees are independent: the same words); sealhip_debug_chunk_log ends with (count, items per
   chunk), preceded by (n / 2, c) when the last step was walked. When the results of the two steps before the last and the
   targets of the step before the last (n ciphertexts in all) do not fit -> E_OUTOFMEMORY with a message that names both
   sizes. With a transparency sink: one flag per output ciphertext, count * n in output order, from the last key switch, or
   from a read pass over out when there is none (n == 1). Nothing synchronises; capturable once the Galois tables and the
   monomial rows are resident (after one call of the same shape).

   sealhip_evaluator_dot_plain: what follows an expansion -- sums of ciphertexts against rows of plaintexts,
       out[s] = sum_{i < n_terms} ct_i (.) P[s][i]        s < n_sums,
   everything in NTT form at level k (CKKS: the ciphertexts' form; BFV callers bracket the call with transform_to_ntt and
   transform_from_ntt). cts: count x n_terms x size x k x N in DEVICE memory (the layout the expansion writes); plain:
   n_sums x n_terms x k x N in DEVICE memory, shared across the batch; out: n_sums x count x size x k x N, sum-major as for
   sealhip_evaluator_linear_combination. One streaming kernel in the shape of the linear combination's: every operand word
   is loaded once per tile of up to 4 sums, accumulated in plain 128-bit integers and reduced once; terms go in groups of 16
   per launch. Every output word is the canonical residue of the integer sum: word for word multiply_plain_ntt per term and
   add left to right. Checks, in this order: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside the
   ciphertext levels, size outside [2, 16], n_terms == 0 or n_sums == 0 with count > 0, cts, plain or out not 16-byte
   aligned, out overlapping cts or plain -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only
   context -> COR_E_INVALIDOPERATION. Nothing comes from the arena; nothing synchronises; capturable. With a transparency
   sink: n_sums * count flags, sum-major, from the kernel that stores the result. */
long sealhip_expand_galois_elts(sealhip_context *ctx, size_t n, uint32_t *elts, uint32_t capacity, uint32_t *n_elts);
long sealhip_evaluator_expand(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, size_t n,
                              const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                              int32_t normalize, uint64_t *out);
long sealhip_evaluator_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *cts, uint32_t n_terms, uint32_t size,
                                 size_t count, const uint64_t *plain, uint32_t n_sums, uint64_t *out);

/* Plaintext-weighted sums of rotations ("double hoisting", Bossuat et al.):
       out_s = sum_i W[s][i] * sigma_{g_i}(ct)   for s < n_sums,
   with ONE decomposition of c_1 per ciphertext and ONE mod-down per sum -- what a baby-step/giant-step matrix-vector product
   or an inner sum wants of the hoisted rotation above. The plaintexts multiply the key-switch inner products while these are
   still in the extended basis Q * P; the weighted products are summed there and the sum is brought down once, so the result
   carries one rounding error of the mod-down, which no plaintext amplifies. The fork has no such method, and the words are
   NOT those of apply_galois_many + multiply_plain_ntt + add; what defines them, word for word in the context's mode, is the
   restatement over the oracle in tests/hoist_dot_ref.py. With nsp special primes, rows = k + nsp, rp(r) the key prime of
   extended row r (r below k, n_key - nsp + (r - k) above), D_j and T_g as for sealhip_evaluator_apply_galois_many:
       prod_g[l][r][c]   = ( sum_j D_j[r][T_g[c]] * K_g[j][l][rp(r)][c] ) mod p_r            for every element g != 1,
       acc_s[l][r][c]    = ( sum_{i : g_i != 1} W[s][i][rp(r)][c] * prod_{g_i}[l][r][c] ) mod p_r,   l < 2, r < rows,
       base_s[0][r][c]   = ( sum_i W[s][i][r][c] * C[0][r][T_{g_i}[c]] ) mod q_r             over ALL elements, r < k,
       base_s[1][r][c]   = ( sum_{i : g_i = 1} W[s][i][r][c] * C[1][r][c] ) mod q_r,
       out_s             = the key switch's finish (:2351-2366) of acc_s added into (base_s[0], base_s[1]),
   every sum canonical. C is the NTT form of both input components: the components themselves for CKKS, their canonical
   forward transform for BFV, where the canonical inverse transform is applied to base_s. If no element differs from 1 no
   acc is formed and out_s = base_s. Element 1 (rotation step 0) needs no key: its key pointer may be NULL. Repeated
   elements add.
   plain_ntt: n_sums x n_elts x n_key x N words, each plaintext in KEY-LEVEL NTT form -- one integer polynomial reduced
   modulo every key prime, special primes included, row j modulo key prime j: what sealhip_ckks_encode and
   sealhip_evaluator_transform_plain_to_ntt write at k = n_key. The plaintexts are shared by the ciphertexts of the batch;
   words at or above their prime give unspecified words. ct: count x 2 x k x N, not modified. out: n_sums x count x 2 x k x N,
   SUM-major (each sum is a contiguous batch); out must overlap neither ct nor plain_ntt. Everything is device memory.
   CKKS in both modes and BFV in STRICT mode; BFV in PARITY mode is E_INVALIDARG, as for apply_galois_many.
   Checks: NULL pointers -> E_POINTER (a NULL key only for element 1); then, also on host-only contexts, k outside the
   ciphertext levels, an even element or one >= 2N, a key with fewer digits than the level, BFV in PARITY mode, n_elts == 0
   or n_sums == 0 when count > 0 (an empty sum would be a transparent zero ciphertext) -> E_INVALIDARG; then count == 0 ->
   S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION. With a transparency sink: one flag per output
   ciphertext, in output order (n_sums * count flags). Nothing synchronises; capturable once the Galois tables of the
   elements are resident (after one call with them). */
long sealhip_evaluator_apply_galois_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                              const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                              uint32_t n_elts, const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out);
/* The same by rotation steps (galois_elt_from_step): plain_ntt: n_sums x n_steps x n_key x N. Step 0 is element 1 and needs
   no key; a step whose key is absent -> E_INVALIDARG ("Galois key not present"), there is no non-adjacent-form fallback. */
long sealhip_evaluator_rotate_vector_dot_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                               const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                               const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                               const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out);

/* Baby-step/giant-step matrix-vector product with the giant steps in the extended basis:
       out = sum_j sigma_{h_j}( sum_i W[j][i] * sigma_{g_i}(ct) )   for j < n_giant, i < n_baby,
   the core of an encrypted linear layer. Composed from sealhip_evaluator_apply_galois_dot_plain, _apply_galois and an add
   per giant step, every inner sum is brought down to Q, goes through a full key switch with a second mod-down and is added
   in a pass of its own. Here only component 1 of an inner sum comes down (the giant step's decomposition needs it); its
   component 0 is permuted and accumulated in Q * P next to the giant steps' inner products, and the whole product is brought
   down once: n_giant half mod-downs and one full one (Lattigo's linear transforms; Bossuat et al.). The fork has no such
   method, and the words are NOT those of the composition; what defines them, word for word in the context's mode, is the
   restatement over the oracle in tests/hoist_bsgs_ref.py. Symbols as for sealhip_evaluator_apply_galois_dot_plain; D_t(x)
   are the rows switch_key_inplace multiplies with digit t for the target x:
     1. base_j (on the k rows, NTT form -- for BFV it stays in NTT form here) and acc_j (on the k + nsp rows) are base_s and
        acc_s of sealhip_evaluator_apply_galois_dot_plain for sum j with the elements g_i.
     2. d_j, for h_j != 1: component 1 of the key switch's finish of acc_j[1] added into base_j[1] (for BFV base_j[1] first
        goes through the canonical inverse transform). When no g_i differs from 1 there is no acc_j and d_j = base_j[1].
     3. Over j, every sum canonical modulo the row's prime:
          h_j  = 1:  ACC[l] += acc_j[l], BASE[l] += base_j[l], both l;
          h_j != 1:  ACC[l][r][c] += ( sum_t D_t(d_j)[r][T_h[c]] * K_h[t][l][rp(r)][c] ) mod p_r, both l,
                     ACC[0][r][c] += acc_j[0][r][T_h[c]], r < k + nsp;   BASE[0][r][c] += base_j[0][r][T_h[c]], r < k.
     4. For BFV the canonical inverse transform of BASE; out = the key switch's finish of ACC added into BASE. If no ACC
        term was ever formed (every g_i and every h_j is 1), out = BASE.
   Repeated elements add; element 1 needs no key on either axis (its key pointer may be NULL).
   plain_ntt: n_giant x n_baby x n_key x N words in KEY-LEVEL NTT form, exactly sealhip_evaluator_apply_galois_dot_plain's
   plain_ntt with n_sums = n_giant. ct: count x 2 x k x N, not modified. out: count x 2 x k x N; out must overlap neither ct
   nor plain_ntt. Everything is device memory. CKKS in both modes and BFV in STRICT mode; BFV in PARITY mode is E_INVALIDARG.
   Checks: NULL pointers -> E_POINTER (a NULL key only for element 1); then, also on host-only contexts, k outside the
   ciphertext levels, an even element or one >= 2N, a key with fewer digits than the level, BFV in PARITY mode, n_baby == 0
   or n_giant == 0 when count > 0 -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only context ->
   COR_E_INVALIDOPERATION. With a transparency sink: one flag per output ciphertext (count flags). Nothing synchronises;
   capturable once the Galois tables of the elements are resident (after one call with them). */
long sealhip_evaluator_apply_galois_bsgs_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                               const uint32_t *baby_elts, const sealhip_kswitch_key *const *baby_keys,
                                               uint32_t n_baby, const uint32_t *giant_elts,
                                               const sealhip_kswitch_key *const *giant_keys, uint32_t n_giant,
                                               const uint64_t *plain_ntt, uint64_t *out);
/* The same by rotation steps (galois_elt_from_step): baby and giant steps with ONE set of keys for both axes;
   plain_ntt: n_giant x n_baby x n_key x N. Step 0 is element 1 and needs no key; a step whose key is absent ->
   E_INVALIDARG ("Galois key not present"), there is no non-adjacent-form fallback. */
long sealhip_evaluator_rotate_vector_bsgs_plain(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                const int32_t *baby_steps, uint32_t n_baby, const int32_t *giant_steps,
                                                uint32_t n_giant, const uint32_t *galois_elts,
                                                const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                const uint64_t *plain_ntt, uint64_t *out);

/* Ciphertext inner product: out = sum_{i < n_terms} a_terms[i] * b_terms[i], the tensor products
   summed in NTT form by one streaming kernel, ONE floor for the whole sum (BFV) and, with relin_keys, ONE relinearization.
   a_terms / b_terms: host arrays of device pointers, as sealhip_evaluator_multiply_many takes them; each points at a batch
   count x 2 x k x N of size-2 ciphertexts at level k (BFV in coefficient form, CKKS in NTT form). Pointers may repeat, and
   a_terms[i] == b_terms[i] gives a sum of squares. The operands are never modified; operand words at or above their prime
   give unspecified words. relin_keys == NULL: out is count x 3 x k x N, the size-3 sum. Otherwise the sum is relinearized
   once (keys as for sealhip_evaluator_relinearize; only index 0 is read) and out is count x 2 x k x N, compact. out must
   overlap no operand.
   CKKS, both modes: the sum of canonical residues -- word for word ckks_multiply per term, add over the products left to
   right, then relinearize. BFV, STRICT mode only (PARITY is E_INVALIDARG, as for the hoisted entries): steps 1-3 of
   bfv_multiply (evaluator.cpp:335-353) per term, the tensor products summed canonically over the rows of q and Bsk, then
   bfv_multiply's tail (:423-444) ONCE. These are not the words of the composition (its floors round per term); what defines
   them is the restatement over the oracle in tests/dot_ct_ref.py. With n_terms == 1 they are sealhip_evaluator_multiply's.
   The floor's base conversion stays exact for at most sealhip_evaluator_dot_product_max_terms terms:
       room = bits(prod Bsk) - (bits(t) + log2 N + bits(q_1 ... q_k) + 4),  max_terms = max(1, 2^room - 1)
   saturating at 2^64 - 1; CKKS reports 2^32 - 1.
   Checks: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, BFV in PARITY mode,
   n_terms == 0 with count > 0, n_terms above max_terms, relin_keys given with n_relin_keys == 0 or a key with fewer digits
   than the level, out overlapping an operand -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only
   context -> COR_E_INVALIDOPERATION. Runs on the calling thread's lane and synchronises nothing; the term pointers travel
   in kernel arguments, so the call is capturable after one warm-up call. With a transparency sink: one flag per output
   ciphertext, written by the kernel that stores polynomials 1.. anyway. */
long sealhip_evaluator_dot_product_max_terms(sealhip_context *ctx, uint32_t k, uint64_t *max_terms);
long sealhip_evaluator_dot_product(sealhip_context *ctx, uint32_t k, const uint64_t *const *a_terms,
                                   const uint64_t *const *b_terms, uint32_t n_terms, size_t count,
                                   const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out);

/* The key switch's mod-down merged with rescale_to_next. CKKS only, both modes. Each *_rescale entry
   is its unmerged sibling followed by sealhip_evaluator_rescale_to_next in ONE call and with ONE rounding: where the sibling
   finishes with floor((acc + P/2) / P) added to base and the rescale divides that by q_{k-1}, the merged finish computes
       out = floor( (P * base + acc + floor(D / 2)) / D ),   D = P * q_{k-1},
   row by row over the k - 1 remaining primes, dropping {q_{k-1}, p_0 .. p_{nsp-1}} in one step with an exact integer
   quotient: 2 (nsp + k) row transforms per ciphertext instead of 2 (nsp + 2 k), and the level-k result is never formed.
   These are not the words of the composition (it rounds twice); what defines them is the restatement over the oracle in
   tests/ks_rescale_ref.py (finish_rescale and the per-operation functions named below). They decrypt with the error of the
   composition. When an operation forms no key-switch term (every Galois element is 1) the words are those of
   rescale_to_next of the sibling's result.
   k is the level of the operands, 2 <= k <= first level; every output is at level k - 1, compact, device memory, and must
   overlap no input. The result's scale is the sibling's divided by q_{k-1}.
   Checks, in this order: NULL pointers -> E_POINTER; then, also on host-only contexts, a BFV context ("CKKS only"), k < 2
   or above the first level, (relinearize_rescale) size != 3 or ct_item_stride < 3 k N, the sibling's own argument errors,
   out overlapping an input -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only context ->
   COR_E_INVALIDOPERATION. Every entry runs on the calling thread's lane, stages nothing from the host, synchronises
   nothing and is capturable under its sibling's conditions. With a transparency sink: one flag per output ciphertext, in
   output order, written by the kernel that stores the result.

   relinearize_rescale (ks_rescale_ref.relinearize_rescale): ct holds count size-3 ciphertexts, ct_item_stride >= 3 k N words
   apart, and is not modified; relin_keys as for sealhip_evaluator_relinearize (required; only index 0 is read);
   out is count x 2 x (k-1) x N.
   dot_product_rescale (ks_rescale_ref.dot_product_rescale): the arguments of sealhip_evaluator_dot_product with relin_keys
   required; out is count x 2 x (k-1) x N. With one term it is multiply + relinearize + rescale_to_next in one call.
   apply_galois_dot_plain_rescale / rotate_vector_dot_plain_rescale (ks_rescale_ref.dot_plain_rescale): the arguments of the
   unmerged entries; out is n_sums x count x 2 x (k-1) x N.
   apply_galois_bsgs_plain_rescale / rotate_vector_bsgs_plain_rescale (ks_rescale_ref.bsgs_plain_rescale): the arguments of
   the unmerged entries; only the final finish is merged, the giant steps' half mod-downs stay; out is count x 2 x (k-1) x N. */
long sealhip_evaluator_relinearize_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                           size_t ct_item_stride, size_t count, const sealhip_kswitch_key *const *relin_keys,
                                           uint32_t n_relin_keys, uint64_t *out);
long sealhip_evaluator_dot_product_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *const *a_terms,
                                           const uint64_t *const *b_terms, uint32_t n_terms, size_t count,
                                           const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out);
long sealhip_evaluator_apply_galois_dot_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                      const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                                      uint32_t n_elts, const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out);
long sealhip_evaluator_rotate_vector_dot_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                       const int32_t *steps, uint32_t n_steps, const uint32_t *galois_elts,
                                                       const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                       const uint64_t *plain_ntt, uint32_t n_sums, uint64_t *out);
long sealhip_evaluator_apply_galois_bsgs_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                       const uint32_t *baby_elts, const sealhip_kswitch_key *const *baby_keys,
                                                       uint32_t n_baby, const uint32_t *giant_elts,
                                                       const sealhip_kswitch_key *const *giant_keys, uint32_t n_giant,
                                                       const uint64_t *plain_ntt, uint64_t *out);
long sealhip_evaluator_rotate_vector_bsgs_plain_rescale(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                                        const int32_t *baby_steps, uint32_t n_baby, const int32_t *giant_steps,
                                                        uint32_t n_giant, const uint32_t *galois_elts,
                                                        const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                                        const uint64_t *plain_ntt, uint64_t *out);

/* Homomorphic DFT of CKKS bootstrapping: CoeffToSlot and SlotToCoeff, each one call over
   sealhip_evaluator_rotate_vector_bsgs_plain_rescale's pipeline, with the diagonals generated on the device. CKKS only, both
   modes. The fork has no such method; the plan and the values are restated from the layer matrices in tests/homdft_ref.py.
   Notation: n = N/2 slots, L = log2 n, zeta = exp(i pi / N); slot j of m(X) is z_j = m(zeta^(5^j mod 2N)); w_t = m_t + i m_(t+n).
   z = U w with U = F_L ... F_1 R, R the bit reversal on L bits and F_s the butterfly layer of span 2^s with twiddles
   omega_(s,j) = exp(2 pi i (5^j mod 4 2^s) / (4 2^s)) (csrc/homdft_plan.hpp). The bit reversal is dropped:
     CoeffToSlot  applies G = F_1^-1 ... F_L^-1, (G z)_j = w_(bitrev j), then splits real and imaginary parts:
                  slot j of out_re holds m_(bitrev j) / scale, slot j of out_im holds m_(bitrev j + n) / scale;
     SlotToCoeff  merges re + i im and applies F_L ... F_1 to a vector in that bit-reversed order.
   `stages` lists layer counts in application order, summing to L: a stage is that many consecutive layers as ONE
   baby-step/giant-step product (CoeffToSlot starts with the top layers, SlotToCoeff with the bottom ones). n_baby: per stage,
   a power of two at most 2^r, or NULL / 0 for 2^ceil((r+1)/2). The stage at level k_s encodes its diagonals at scale
   (double) q_(k_s - 1), the prime its merged rescale drops, so the ciphertext's scale is exactly unchanged; a transform of
   n_stages stages takes level k to k - n_stages.
   sealhip_evaluator_dft_plan: works on host-only contexts. key_steps == NULL: plan alone (n_key_steps says how many); else the sorted
   distinct non-zero rotation steps of all stages (the Galois keys the client must make; CoeffToSlot needs element 2N - 1
   too: needs_conjugation), key_steps_capacity < n_key_steps -> E_INVALIDARG. sealhip_dft_stage_steps: one stage's steps,
   n_baby and n_giant values in [0, n), 0 the identity.
   E_INVALIDARG: a BFV context, layer counts not summing to L, a zero count, n_stages >= k (more stages than levels below
   k), k outside the ciphertext levels, an n_baby that is no power of two or exceeds 2^r. */
#define SEALHIP_DFT_COEFFS_TO_SLOTS 0u
#define SEALHIP_DFT_SLOTS_TO_COEFFS 1u
#define SEALHIP_DFT_MAX_STAGES 16
typedef struct sealhip_dft_stage
{
    uint32_t s0, r, h0;       /* layers s0 .. s0 + r - 1, h0 = 2^(s0 - 1) */
    uint32_t level;           /* of the stage's input */
    uint32_t n_baby, n_giant; /* the table is n_giant x n_baby x n_key x N words */
    uint32_t folded;          /* 1: the stage holds the top layer, 2^r diagonals and no empty cell */
    uint32_t reserved;
    double scale;             /* of its plaintexts */
} sealhip_dft_stage;
typedef struct sealhip_dft_plan
{
    uint32_t direction, n_stages, in_level, out_level;
    uint32_t needs_conjugation, n_key_steps;
    uint64_t table_words;         /* device words of all stages' tables */
    uint64_t temp_bytes_per_item; /* a transform's workspace per ciphertext of the batch: a pool block the tables hold */
    sealhip_dft_stage stages[SEALHIP_DFT_MAX_STAGES];
} sealhip_dft_plan;
typedef struct sealhip_dft_tables sealhip_dft_tables;
long sealhip_evaluator_dft_plan(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                      const uint32_t *n_baby, sealhip_dft_plan *plan, uint32_t *key_steps, uint32_t key_steps_capacity);
long sealhip_dft_stage_steps(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages,
                             uint32_t n_stages, const uint32_t *n_baby, uint32_t stage, int32_t *baby_steps,
                             int32_t *giant_steps);
/* The generator alone: values = n_giant x n_baby x n complex doubles {re, im} of stage `stage`, cell [g][b] the diagonal
   c = c_g n_baby + b rotated by minus its giant step: values[g][b][p] = f M[i][i + c h0], i = (p - giant step) mod n, zero
   outside the stage's blocks. f is real: 1/2 on the last CoeffToSlot stage (the split adds a value to its conjugate), times
   `gain` on the last CoeffToSlot or the first SlotToCoeff stage. sealhip_dft_stage_values writes DEVICE memory (stream-ordered,
   one gather kernel over the encoder's resident root table); _host writes HOST memory with the same function over the same
   tables, also on host-only contexts, and gives the same bits. */
long sealhip_dft_stage_values(sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                              const uint32_t *n_baby, double gain, uint32_t stage, double *values);
long sealhip_dft_stage_values_host(const sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages,
                                   uint32_t n_stages, const uint32_t *n_baby, double gain, uint32_t stage, double *values);
/* The tables of one transform: every stage's values through sealhip_ckks_encode at k = n_key and the stage's scale, kept in
   device memory (plan.table_words words; the values are a temporary). Synchronises; not capturable. gain must be finite and
   non-zero. _stage: the device pointer of a stage's n_giant x n_baby x n_key x N words, the plain_ntt argument of
   sealhip_evaluator_rotate_vector_bsgs_plain_rescale; _plan: the plan they were made for. Destroy the tables before their
   context, not while a call that reads them is in flight, and not during a graph capture (COR_E_INVALIDOPERATION, the
   tables stay): _destroy gives the transforms' workspace blocks back to the context's pool. */
long sealhip_dft_tables_create(sealhip_context *ctx, uint32_t direction, uint32_t k, const uint32_t *stages, uint32_t n_stages,
                               const uint32_t *n_baby, double gain, sealhip_dft_tables **tables);
long sealhip_dft_tables_destroy(sealhip_dft_tables *tables);
long sealhip_dft_tables_plan(const sealhip_dft_tables *tables, sealhip_dft_plan *plan);
long sealhip_dft_tables_stage(const sealhip_dft_tables *tables, uint32_t stage, const uint64_t **plain_ntt);
/* coeffs_to_slots: ct: count x 2 x k x N at the tables' level k, not modified; stage by stage the BSGS product with the merged
   rescale, then sigma_(2N-1) of the result and ONE streaming kernel for both outputs:
       re = c' + sigma(c'),   im = -i (c' - sigma(c'))      (the last stage's values carry the 1/2),
   multiplication by i being the dyadic product with NTT(X^(N/2)). out_re, out_im: count x 2 x (k - n_stages) x N each.
   slots_to_coeffs: ct_re, ct_im: count x 2 x k x N; c = re + i im in one streaming kernel, then the stages;
   out: count x 2 x (k - n_stages) x N. The words are those of the same stages issued one by one through
   sealhip_evaluator_rotate_vector_bsgs_plain_rescale with the tables, composed with sealhip_evaluator_apply_galois, add, sub
   and the dyadic product. galois_elts[i] is the Galois element of galois_keys[i] (n_keys of them), as for
   sealhip_evaluator_rotate_vector_bsgs_plain.
   ct_re, ct_im, out_re and out_im must be 16-byte aligned: the split and the merge load and store two words at a time.
   Checks: NULL pointers -> E_POINTER; then, also on host-only contexts, tables made on another context, one of those four
   pointers not 16-byte aligned, tables of the other direction, a step (or, for
   coeffs_to_slots, element 2N - 1) whose key is absent ("Galois key not present"), a key with fewer digits than its stage's
   level, an output overlapping an input or the other output -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then
   a host-only context -> COR_E_INVALIDOPERATION. With a transparency sink: one flag per output ciphertext, written by a
   read pass over the result -- coeffs_to_slots: count flags for out_re, then count for out_im. Nothing synchronises. The
   temporaries (count x plan.temp_bytes_per_item bytes) are a block of the context's pool (sealhip_pool_stats counts it as
   in use) that the tables hold per calling thread, replaced by a larger one on demand and released by
   sealhip_dft_tables_destroy: capturable after one call with the same tables at a batch at least as large. */
long sealhip_evaluator_coeffs_to_slots(sealhip_context *ctx, const sealhip_dft_tables *tables, const uint64_t *ct, size_t count,
                                       const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                       uint32_t n_keys, uint64_t *out_re, uint64_t *out_im);
long sealhip_evaluator_slots_to_coeffs(sealhip_context *ctx, const sealhip_dft_tables *tables, const uint64_t *ct_re,
                                       const uint64_t *ct_im, size_t count, const uint32_t *galois_elts,
                                       const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, uint64_t *out);

/* Encrypted matrix-vector products from a caller's matrix: the diagonals found, pre-rotated, encoded
   and laid out on the device for sealhip_evaluator_rotate_vector_bsgs_plain[_rescale]. CKKS only, both modes. The fork has no
   such method; tests/lintrans_ref.py restates the scan, the plan and the values.
   Notation: n = N/2 slots; d a power of two, 1 <= d <= n. M is a d x d complex matrix, row-major, M[i][j] at doubles
   2 (i d + j) (re) and 2 (i d + j) + 1 (im), 16-byte aligned. Diagonal c in [0, d) is the slot vector
       u_c[p] = M[p mod d][(p + c) mod d],   p < n,
   and for a ciphertext whose slots are z the result's slots are
       out[p] = sum_{c in D} u_c[p] * z[(p + c) mod n],
   D the diagonals in use (for the tables: those holding a non-zero entry). The formula is the definition; for a d-periodic
   z (a vector of d values tiled n/d times) it is M z, tiled.
   The plan, given the baby stride n1 (a power of two <= d; 0 = the default): c = g + b with b = c mod n1, g = c - b; the baby
   steps are the distinct b over D and the giant steps the distinct g, both ascending; cell [gi][bi] of the grid holds
       values[gi][bi][p] = gain * u_(g+b)[(p - g) mod n],
   zero when g + b is not in D. Step 0 on either axis is the identity and needs no key. The default n1 is the power of two
   that minimises nb + 2 ng over the NON-ZERO baby and giant steps, ties to the larger n1 (dense d = 2^r, r >= 1:
   2^ceil((r+1)/2), the homomorphic DFT's default).
   diag_mask_host: d bytes on the host, non-zero = the diagonal is in D; NULL = every diagonal.
   Checks of every entry, in this order: NULL pointers -> E_POINTER; then, also on host-only contexts, a BFV context, a d that
   is no power of two in [1, n], an n1 that is neither 0 nor a power of two <= d, a mask without a diagonal, a gain that is
   not finite or is zero, a matrix or values pointer that is not 16-byte aligned -> E_INVALIDARG; then a host-only context
   -> COR_E_INVALIDOPERATION where the entry needs the device.

   sealhip_linear_transform_plan: works on host-only contexts. baby_steps, giant_steps, key_steps may each be NULL (the plan
   alone: n_baby, n_giant and n_key_steps say how many there are); what is given holds `capacity` entries, fewer than the
   list needs -> E_INVALIDARG. key_steps: the sorted distinct non-zero steps of both axes, the Galois keys the client makes. */
typedef struct sealhip_lintrans_plan
{
    uint32_t d, n_diagonals;      /* |D| */
    uint32_t n1, n_baby, n_giant; /* the table is n_giant x n_baby x n_key x N words */
    uint32_t n_key_steps;
    uint64_t table_words;
    uint64_t temp_bytes_per_item; /* pool bytes the tables hold per ciphertext of a transform: 0, its temporaries are the
                                     BSGS pipeline's, in the calling thread's arena */
} sealhip_lintrans_plan;
typedef struct sealhip_linear_transform sealhip_linear_transform;
long sealhip_linear_transform_plan(const sealhip_context *ctx, uint32_t d, const uint8_t *diag_mask_host, uint32_t n1,
                                   sealhip_lintrans_plan *plan, int32_t *baby_steps, int32_t *giant_steps, uint32_t *key_steps,
                                   uint32_t capacity);
/* The occupancy scan alone: diag_mask_host[c] = 1 if diagonal c of the DEVICE matrix holds a non-zero entry, re or im
   (-0.0 is zero), else 0; an entry that is not finite -> E_INVALIDARG (the mask is then unspecified). One kernel, one
   workgroup per diagonal, then one copy of d bytes. Synchronises; not capturable. */
long sealhip_linear_transform_diagonals(sealhip_context *ctx, const double *matrix_dev, uint32_t d, uint8_t *diag_mask_host);
/* The generator alone: values = n_giant x n_baby x n complex doubles {re, im}, the grid above for the diagonals of
   diag_mask_host; the products are re * gain and im * gain, two IEEE multiplies. sealhip_linear_transform_values reads a
   DEVICE matrix and writes DEVICE memory with one gather kernel; it stages the plan's steps from the host and synchronises
   (not capturable). _values_host reads and writes HOST memory with the same function, also on host-only contexts, and gives
   the same bits. */
long sealhip_linear_transform_values(sealhip_context *ctx, const double *matrix_dev, uint32_t d, const uint8_t *diag_mask_host,
                                     uint32_t n1, double gain, double *values_dev);
long sealhip_linear_transform_values_host(const sealhip_context *ctx, const double *matrix_host, uint32_t d,
                                          const uint8_t *diag_mask_host, uint32_t n1, double gain, double *values_host);
/* The tables of one matrix: the occupancy scan (a non-finite entry, or a matrix without a non-zero entry -- an empty sum
   would be a transparent ciphertext -- -> E_INVALIDARG), the plan over the diagonals found, then the grid chunk by chunk:
   as many cells as the calling thread's arena cap holds go values -> sealhip_ckks_encode at k = n_key and `scale`, into
   plan.table_words words of device memory (out of memory -> E_OUTOFMEMORY, nothing is kept). The encoder's refusals pass
   through ("scale out of bounds", "encoded values are too large"). Synchronises; not capturable. The plaintexts are at the
   key level, so one object serves every ciphertext level. _tables_steps: n_baby and n_giant steps (either may be NULL);
   _tables_plain: the device pointer that is valid as plain_ntt of sealhip_evaluator_rotate_vector_bsgs_plain[_rescale] with
   those steps. Destroy the tables before their context, not while a call that reads them is in flight, and not during a
   graph capture (COR_E_INVALIDOPERATION, the tables stay). */
long sealhip_linear_transform_create(sealhip_context *ctx, const double *matrix_dev, uint32_t d, uint32_t n1, double scale,
                                     double gain, sealhip_linear_transform **tables);
long sealhip_linear_transform_destroy(sealhip_linear_transform *tables);
long sealhip_linear_transform_tables_plan(const sealhip_linear_transform *tables, sealhip_lintrans_plan *plan, double *scale);
long sealhip_linear_transform_tables_steps(const sealhip_linear_transform *tables, int32_t *baby_steps, int32_t *giant_steps);
long sealhip_linear_transform_tables_plain(const sealhip_linear_transform *tables, const uint64_t **plain_ntt);
/* The transform: ct is count x 2 x k x N in NTT form, not modified. rescale == 0: the words of
   sealhip_evaluator_rotate_vector_bsgs_plain with the tables' steps and plaintexts, out: count x 2 x k x N; the result's
   scale is the ciphertext's times the tables'. rescale != 0: the words of sealhip_evaluator_rotate_vector_bsgs_plain_rescale,
   2 <= k, out: count x 2 x (k-1) x N, the scale divided by q_(k-1). galois_elts[i] is the Galois element of galois_keys[i].
   Checks: NULL pointers -> E_POINTER; then, also on host-only contexts, tables made on another context, the BSGS entry's own
   argument errors (k outside its levels, a step whose key is absent -- "Galois key not present" --, a key with fewer digits
   than the level, out overlapping ct) -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only context
   -> COR_E_INVALIDOPERATION. Nothing synchronises; capturable under the BSGS entry's conditions (after one call with the
   same keys); transparency sink as the BSGS entry: one flag per output ciphertext. */
long sealhip_evaluator_linear_transform(sealhip_context *ctx, const sealhip_linear_transform *tables, uint32_t k,
                                        const uint64_t *ct, size_t count, const uint32_t *galois_elts,
                                        const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys, int32_t rescale,
                                        uint64_t *out);

/* Towards CKKS bootstrapping: ModRaise and the double-angle step of EvalMod. CKKS only, both modes.
   The fork has neither; tests/bootstrap_ref.py restates ModRaise over the oracle's transforms.

   mod_raise: a level-1 ciphertext decrypts under s to m(X) modulo q_0. With centre(x) = x for x <= (q_0 - 1) / 2 and
   x - q_0 otherwise, the centred coefficients of c_0, c_1 mod q_0 are re-read modulo q_0 .. q_(k_out-1); the result decrypts
   to m + q_0 I for an integer polynomial I with |I_j| <= (h + 1) / 2 when the secret has Hamming weight h.
   ct: count x 2 x k_in x N in NTT form, not modified. Only the q_0 rows are read (dropping rows is CKKS's mod_switch_to),
   so any k_in >= 1 is accepted. out: count x 2 x k_out x N, 2 <= k_out <= first level: row 0 of every polynomial is the
   input's row 0, row i >= 1 is NTT_i(centre(INTT_0(row 0)) mod q_i), canonical. ct and out must be 16-byte aligned.
   Checks, in this order: NULL pointers -> E_POINTER; then, also on host-only contexts, a BFV context, k_in or k_out outside
   the ciphertext levels, k_out < 2, out overlapping ct, an operand not 16-byte aligned -> E_INVALIDARG; then count == 0 ->
   S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION. The 2 N words per ciphertext of temporaries
   come from the lane's arena, in chunks when the batch exceeds it; nothing synchronises; capturable after one warm-up call
   at a batch at least as large. With a transparency sink: one flag per output ciphertext, by a read pass over out.

   double_angle: out = 2 ct^2 - 1 for ct at scale `scale`, from level k to k - 1, in one call:
       (2 c_0^2 - rint(scale^2), 4 c_0 c_1, 2 c_1^2), relinearized with the rescale merged into the key switch's mod-down.
   *out_scale = scale * scale / (double) q_(k-1), formed in that order in doubles. The words are those of
   sealhip_evaluator_dot_product({ct}, {ct}) without keys, sealhip_evaluator_linear_combination_levels with weight 2 and the
   constant rint(-rint(scale * scale)) mod q_r, and sealhip_evaluator_relinearize_rescale, issued one by one; one streaming
   kernel replaces the first two (2 words read and 3 written per coefficient where they move 11).
   ct: count x 2 x k x N, not modified; out: count x 2 x (k-1) x N; relin_keys as for sealhip_evaluator_relinearize (required;
   only index 0 is read). Checks and order are those of sealhip_evaluator_dot_product_rescale, with a scale that is not
   finite and positive, or whose square is not finite, -> E_INVALIDARG next to the level's, and a ct that is not 16-byte
   aligned -> E_INVALIDARG after the overlap check (the kernel loads it two words at a time); out_scale is written once the
   checks have passed, also for an empty batch. Capturable under dot_product_rescale's conditions; with a transparency
   sink: one flag per output ciphertext, written by the kernel that stores the result. */
long sealhip_evaluator_mod_raise(sealhip_context *ctx, uint32_t k_in, const uint64_t *ct, size_t count, uint32_t k_out,
                                 uint64_t *out);
long sealhip_evaluator_double_angle(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale,
                                    const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out,
                                    double *out_scale);

/* EvalMod, the scaled sine of CKKS bootstrapping (csrc/evalmod_plan.hpp). CKKS only, both modes.
   After ModRaise a coefficient is c = m + q_0 I. K is the caller's bound on I: K >= max|I| + 1, where |I_j| <= (h + 1) / 2
   for a secret of Hamming weight h (sealhip_generate_secret_key does not sample sparse secrets: with its ternary secrets h
   is about 2 N / 3 and no practical K covers I; sealhip_generate_sparse_secret_key makes a secret of a chosen weight, and
   sealhip_evaluator_bootstrap_encapsulated runs ModRaise alone under it). For slots holding x = c / (q_0 K) in [-1, 1] at scale `scale`, eval_mod evaluates
   the degree-`degree` Chebyshev interpolant of cos((2 pi K x - pi / 2) / 2^r) with sealhip_evaluator_evaluate_polynomial_ckks'
   pipeline and applies sealhip_evaluator_double_angle r times (0 <= r <= 8): the slots then hold sin(2 pi c / q_0) =
   sin(2 pi m / q_0), which is 2 pi m / q_0 up to the relative error (2 pi m / q_0)^2 / 6 -- |m| / q_0 sets the precision
   floor of a bootstrapping, whatever the degree.
   sealhip_evalmod_coeffs: the degree + 1 coefficients (lowest degree first), by interpolation at the Chebyshev nodes with
   the sums formed in long double; needs no context.
   sealhip_evaluator_evalmod_plan: works on host-only contexts. With L_0 the polynomial plan's out level for (k, degree,
   n_baby) -- n_baby as for the polynomial evaluator, 0 its default --, step i = 1 .. r runs at level L_0 - i + 1. The scales
   are planned backwards, t_r = scale_out (0: scale), t_(i-1) = sqrt(t_i * (double) q_(L_0 - i)); the polynomial is evaluated
   with scale_out = t_0 (poly_scale_out); scales[0 .. r] are the forward values s_0 = t_0, s_i = s_(i-1) * s_(i-1) /
   (double) q_(L_0 - i), and scales[r] is the result's scale: scale_out up to |s_r / scale_out - 1| <= 2^(r+3) 2^-53.
   E_INVALIDARG: a BFV context, k outside the ciphertext levels, K < 1, r > 8, degree < 1 or above 1023, the polynomial
   plan's refusals, an out level L_0 - r below 1 ("end of modulus switching chain reached"), or a scale s_i or an element's
   scale of the polynomial plan that is not finite, positive and below 2^62 ("scale out of bounds"): the primes at the EvalMod
   levels are then too far from `scale` -- they should be near it.
   sealhip_evaluator_eval_mod: ct: count x 2 x k x N, not modified; out: count x 2 x plan.out_level x N; *out_level and
   *out_scale (either may be NULL) receive plan.out_level and scales[r]. The words are those of
   sealhip_evaluator_evaluate_polynomial_ckks with basis 1, the library's coefficients and scale_out = poly_scale_out, followed
   by r calls of sealhip_evaluator_double_angle at scales[0 .. r-1]. Checks: NULL pointers -> E_POINTER; then, also on
   host-only contexts, the plan's refusals, missing or short relinearization keys, out overlapping ct -> E_INVALIDARG; then
   count == 0 -> S_OK; then a host-only context -> COR_E_INVALIDOPERATION. Temporaries (count x plan.temp_bytes_per_item
   bytes at most) are blocks of the context's pool; NOT capturable, because the polynomial evaluator is not. ct and out need
   no more than their 8-byte alignment: the double-angle steps read pool blocks. With a transparency sink: one flag per
   output ciphertext. */
#define SEALHIP_EVALMOD_MAX_DOUBLINGS 8
typedef struct sealhip_evalmod_plan
{
    uint32_t K, r, degree, n_baby;   /* n_baby: the polynomial plan's baby steps m */
    uint32_t poly_level, out_level;  /* L_0 and L_0 - r */
    uint32_t n_products, reserved;   /* key-switched products: the polynomial's and the r steps */
    double poly_scale_out;           /* t_0 */
    double scales[SEALHIP_EVALMOD_MAX_DOUBLINGS + 1]; /* s_0 .. s_r, the rest 0 */
    uint64_t temp_bytes_per_item;
} sealhip_evalmod_plan;
long sealhip_evalmod_coeffs(uint32_t K, uint32_t r, uint32_t degree, double *coeffs);
long sealhip_evaluator_evalmod_plan(const sealhip_context *ctx, uint32_t k, double scale, uint32_t K, uint32_t r, uint32_t degree,
                                    uint32_t n_baby, double scale_out, sealhip_evalmod_plan *plan);
long sealhip_evaluator_eval_mod(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale, uint32_t K,
                                uint32_t r, uint32_t degree, uint32_t n_baby, double scale_out,
                                const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out,
                                uint32_t *out_level, double *out_scale);

/* CKKS bootstrapping in one call: bootstrap(ct) takes a ciphertext that has run out of levels and
   returns one at a usable level with the same scale. Full packing only (sparse packing stays out). The chain is
       mod_raise to k_top (the raised ciphertext is DECLARED to have scale S = (double) q_0 * K)
       -> coeffs_to_slots with gain 1: the slots hold x = c / (q_0 K) in [-1, 1]
       -> eval_mod (K, r, degree, n_baby) ONCE over the 2 count real and imaginary halves, scale_out = S
       -> slots_to_coeffs with gain (double) q_0 / (2 pi s_r), s_r the scale EvalMod ends at.
   The output coefficients are m again, so the result has the caller's scale whatever it was: the bootstrap takes no scale
   argument. K is the caller's bound on the integer polynomial I of ModRaise, K >= max|I| + 1 (see EvalMod above: K grows with
   the Hamming weight of the secret the raise runs under, which sealhip_evaluator_bootstrap_encapsulated below makes a sparse
   one of the caller's choice while the working key stays dense). The relative error of the sine step is
   (2 pi m / q_0)^2 / 6: |m| / q_0 sets the precision floor of the result, next to the CKKS noise of the chain.
   sealhip_evaluator_bootstrap_plan: works on host-only contexts. c2s_stages / s2c_stages and their optional n_baby lists are
   sealhip_evaluator_dft_plan's. key_steps as for sealhip_evaluator_dft_plan: the union of both transforms' sorted distinct
   rotation steps; element 2N - 1 is needed too (needs_conjugation). E_INVALIDARG: either transform's or EvalMod's refusals,
   an out level below 1.
   sealhip_bootstrap_tables_create: two sealhip_dft_tables with those gains, the coefficient vector, and (on first use) one
   block of the context's pool per calling thread for the intermediates -- count x plan.temp_bytes_per_item bytes, CoeffToSlot's
   out_re and out_im contiguous in it; a larger batch takes a larger block, _destroy releases all of them. Synchronises; not
   capturable; destroy the tables before their context and not during a graph capture (COR_E_INVALIDOPERATION).
   sealhip_evaluator_bootstrap: ct: count x 2 x k_in x N in NTT form (only its q_0 rows are read), out: count x 2 x
   plan.out_level x N, both 16-byte aligned. galois_elts / galois_keys as for sealhip_evaluator_coeffs_to_slots; relin_keys
   as for sealhip_evaluator_relinearize. Checks: NULL pointers -> E_POINTER; then, also on host-only contexts (where the
   first always applies, tables being made on a device), tables made on another context, k_in outside the ciphertext levels, a pointer not 16-byte aligned, a step or element 2N - 1 whose key is
   absent ("Galois key not present"), a key with fewer digits than its level needs, missing relinearization keys, out
   overlapping ct -> E_INVALIDARG; then count == 0 -> S_OK; then a host-only context -> COR_E_INVALIDOPERATION. NOT
   capturable (EvalMod is not). With a transparency sink: one flag per output ciphertext, by a read pass over out. */
typedef struct sealhip_bootstrap_plan
{
    uint32_t k_top, c2s_out_level, evalmod_out_level, out_level; /* the level after each part */
    uint32_t needs_conjugation, n_key_steps;
    double raise_scale;           /* S = (double) q_0 * K */
    double s2c_gain;              /* (double) q_0 / (2 pi s_r) */
    uint64_t table_words;         /* device words of both transforms' tables */
    uint64_t temp_bytes_per_item; /* the intermediates the tables hold, per ciphertext (the parts' own workspaces come on top) */
    sealhip_evalmod_plan evalmod;
} sealhip_bootstrap_plan;
typedef struct sealhip_bootstrap_tables sealhip_bootstrap_tables;
long sealhip_evaluator_bootstrap_plan(const sealhip_context *ctx, uint32_t k_top, const uint32_t *c2s_stages, uint32_t n_c2s,
                                      const uint32_t *c2s_n_baby, const uint32_t *s2c_stages, uint32_t n_s2c,
                                      const uint32_t *s2c_n_baby, uint32_t K, uint32_t r, uint32_t degree, uint32_t n_baby,
                                      sealhip_bootstrap_plan *plan, uint32_t *key_steps, uint32_t key_steps_capacity);
long sealhip_bootstrap_tables_create(sealhip_context *ctx, uint32_t k_top, const uint32_t *c2s_stages, uint32_t n_c2s,
                                     const uint32_t *c2s_n_baby, const uint32_t *s2c_stages, uint32_t n_s2c,
                                     const uint32_t *s2c_n_baby, uint32_t K, uint32_t r, uint32_t degree, uint32_t n_baby,
                                     sealhip_bootstrap_tables **tables);
long sealhip_bootstrap_tables_destroy(sealhip_bootstrap_tables *tables);
long sealhip_bootstrap_tables_plan(const sealhip_bootstrap_tables *tables, sealhip_bootstrap_plan *plan);
long sealhip_evaluator_bootstrap(sealhip_context *ctx, const sealhip_bootstrap_tables *tables, uint32_t k_in, const uint64_t *ct,
                                 size_t count, const uint32_t *galois_elts, const sealhip_kswitch_key *const *galois_keys,
                                 uint32_t n_keys, const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                 uint64_t *out);

/* Linear combinations of ciphertexts with scalar weights, both schemes, both modes:
       out_s = sum_{i < n_terms} W[s][i] * X_i  (+ K[s] on c_0)      for s < n_sums
   formed by one streaming kernel that loads every operand word once per tile of 4 sums: no transforms, no lifted plaintexts,
   no partial sums written and re-read.
   terms: a host array of n_terms device pointers, as sealhip_evaluator_dot_product takes them; each points at a batch
   count x size x k x N of ciphertexts at level k, all of the same size >= 2 (BFV in coefficient form, CKKS in NTT form).
   Pointers may repeat; the operands are never modified. weights: DEVICE memory, n_sums x n_terms x k words, W[s][i][r] a
   canonical residue modulo q_r. constant: DEVICE memory, n_sums x k words, or NULL; K[s][r] is added to polynomial 0 only --
   BFV at coefficient 0 (a constant polynomial in coefficient form), CKKS at every coefficient (a constant polynomial in NTT
   form). out: n_sums x count x size x k x N, sum-major as for sealhip_evaluator_apply_galois_dot_plain; it overlaps no term
   and neither table. Weights and constants are shared across the batch; weights of zero are legal and contribute nothing.
   Every output word is the canonical residue of the integer sum, so it is word for word the composition of
   multiply_poly_scalar_coeffmod per term and row, add_poly_coeffmod left to right, the constant added last. Operand or
   weight words at or above their prime give unspecified words.
   Checks: NULL pointers (ctx, weights, out, terms and each of its entries) -> E_POINTER; then, also on host-only contexts,
   k outside the ciphertext levels, size < 2 or > 16 (SEAL_CIPHERTEXT_SIZE_MIN / _MAX, util/defines.h:56-57, the bounds
   sealhip_evaluator_multiply and _relinearize apply), n_terms == 0 or n_sums == 0 with count > 0, out overlapping a term or a
   table -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION.
   Runs on the calling thread's lane, takes nothing from the arena and synchronises nothing; the term pointers travel in
   kernel arguments, so the call is capturable after one warm-up call. With a transparency sink: one flag per output
   ciphertext (n_sums x count flags, in output order), written by the kernel that stores it. */
long sealhip_evaluator_linear_combination(sealhip_context *ctx, uint32_t k, const uint64_t *const *terms, uint32_t n_terms,
                                          uint32_t size, size_t count, const uint64_t *weights, const uint64_t *constant,
                                          uint32_t n_sums, uint64_t *out);

/* The same sums over CKKS terms that keep their own level and size, both modes. A CKKS
   mod_switch_to_next only drops the last row, so a ciphertext at level k_t >= k holds the level-k ciphertext in place: the
   kernel reads rows r < k of every polynomial at the term's own row stride, and nothing is dropped to level k by a copy
   first. term_levels, term_sizes: HOST arrays of n_terms entries; term i is a device batch count x term_sizes[i] x
   term_levels[i] x N in NTT form, with k <= term_levels[i] <= the first level and 2 <= term_sizes[i] <= size; a term of fewer
   polynomials than size contributes nothing to the others. weights, constant and out are laid out at level k exactly as for
   sealhip_evaluator_linear_combination, and so are the capacity of a launch (16 terms, 4 sums) and the arithmetic per word.
   The words are those of the composition: drop each term to its first k rows, pad it with zero polynomials to size, then
   tests/poly_eval_ref.linear_combination; with every term at level k and size `size` they are those of
   sealhip_evaluator_linear_combination. One term with weight 1 is a one-pass mod_switch_to any lower level.
   Checks: NULL pointers (ctx, weights, out; with n_terms > 0 terms, each of its entries, term_levels, term_sizes) ->
   E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, a BFV context ("CKKS only": a BFV
   mod_switch_to_next is not a row drop), a term level below k or above the first level, size < 2 or > 16, a term size
   < 2 or > size, n_terms == 0 or n_sums == 0 with count > 0, out overlapping a term or a table -> E_INVALIDARG; then
   count == 0 -> S_OK, nothing launched; then a host-only context -> COR_E_INVALIDOPERATION.
   Runs on the calling thread's lane, takes nothing from the arena and synchronises nothing; pointers, levels and sizes
   travel in kernel arguments, so the call is capturable after one warm-up call. Transparency flags as for
   sealhip_evaluator_linear_combination. */
long sealhip_evaluator_linear_combination_levels(sealhip_context *ctx, uint32_t k, const uint64_t *const *terms,
                                                 const uint32_t *term_levels, const uint32_t *term_sizes, uint32_t n_terms,
                                                 uint32_t size, size_t count, const uint64_t *weights, const uint64_t *constant,
                                                 uint32_t n_sums, uint64_t *out);

/* Polynomial evaluation on ciphertexts: out = p(ct) = sum_e coeffs[e] ct^e by Paterson-Stockmeyer
   over the two entries above. BFV in STRICT mode. ct: count x 2 x k x N, coefficient form, not modified; out: count x 2 x k
   x N, overlapping nothing; both device memory. coeffs: HOST memory, degree + 1 words below t, shared by the batch.
   Trailing zero coefficients are trimmed first; with d what remains, m = n_baby, or ceil(sqrt(d + 1)) when n_baby is 0, and
   g = ceil((d + 1) / m):
     baby powers   B_1 = ct, B_e = relinearize(multiply(B_ceil(e/2), B_floor(e/2))) for 2 <= e <= min(m, d);
     giant powers  G_1 = B_m, G_j = relinearize(multiply(G_ceil(j/2), G_floor(j/2))) for 2 <= j < g -- only those that a
                   surviving term needs or that a needed one is built from;
     inner sums    I_j = sum_{1 <= i < m} w(c_{jm+i}) B_i + K(c_{jm}) for j < g in ONE sealhip_evaluator_linear_combination,
                   w(c)[r] = (c - t [c >= (t+1)/2]) mod q_r, the residue multiply_plain uses for a one-coefficient plaintext,
                   K(c)[r] the word multiply_add_plain_with_scaling_variant adds at coefficient 0 for that plaintext;
     outer sum     out = I_0 + sealhip_evaluator_dot_product({G_j}, {I_j}, j >= 1 with I_j not identically zero, relin_keys):
                   one inverse transform, one floor and one relinearization for the whole sum; with g == 1, out = I_0
                   (with g > 1 the inner sum that holds c_d is not zero, so there is such a j).
   What defines the words is the restatement over the oracle in tests/poly_eval_ref.py.
   relin_keys as for sealhip_evaluator_relinearize (only index 0 is read); with d == 1 no key is needed and it may be NULL.
   Checks: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, a CKKS context
   ("BFV only"), BFV in PARITY mode ("STRICT"), a coefficient >= t, d < 1 after trimming (a constant is not an operation on
   a ciphertext), n_baby == 1 or n_baby > d + 1, more outer terms than sealhip_evaluator_dot_product_max_terms(k), with
   d >= 2 missing keys or a key with fewer digits than the level, out overlapping ct -> E_INVALIDARG; then count == 0 ->
   S_OK; then a host-only context -> COR_E_INVALIDOPERATION.
   Temporaries -- (m - 1) + (g - 1) + g size-2 batches, the products' size-3 scratch and the two small tables -- are blocks
   of the context's pool (sealhip_pool_*), taken and released in stream order on the calling lane, and the coefficients
   travel in kernel arguments: nothing synchronises, but unlike sealhip_evaluator_linear_combination this entry allocates
   (until the pool is warm) and is therefore NOT capturable. With a transparency sink: one flag per output ciphertext, from the kernel that stores out (g == 1) or a
   read pass over it. CKKS polynomial evaluation needs per-power scale and level bookkeeping: it is
   sealhip_evaluator_evaluate_polynomial_ckks below. */
long sealhip_evaluator_evaluate_polynomial(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                           const uint64_t *coeffs, uint32_t degree, uint32_t n_baby,
                                           const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys, uint64_t *out);

/* Polynomial evaluation on CKKS ciphertexts with planned levels and scales, both modes:
   out = p(ct), p = sum_e coeffs[e] x^e (basis 0) or sum_e coeffs[e] T_e(x) (basis 1: Chebyshev polynomials of the first kind,
   for messages in [-1, 1]), by Paterson-Stockmeyer. The plan -- gemini-seal_amd/csrc/poly_plan.hpp, restated in
   tests/poly_eval_ckks_ref.py, which also defines the words -- with d the degree after trimming trailing zeros, m = n_baby
   or ceil(sqrt(d + 1)), g = ceil((d + 1) / m), delta(e) = ceil(log2 e), s the input scale and dbl(q) a prime as a double
   (all scale arithmetic is IEEE double in the order written):
     baby elements E_1 = ct, E_e from E_hi, E_lo (hi = ceil(e/2), lo = floor(e/2)) at level L = lev(hi), 2 <= e <= min(m, d):
                   monomial   E_e = dot_product_rescale({E_hi}, {E_lo});
                   Chebyshev  E_e = relinearize_rescale(2 E_hi E_lo - T_{hi-lo}), the subtraction BEFORE the rescale with the
                              integer rint(sc(hi) sc(lo)) (a constant, hi == lo) or rint(sc(hi) sc(lo) / sc(1)) (the weight of
                              E_1, read in place at level L) in one sealhip_evaluator_linear_combination_levels;
                   lev(e) = k - delta(e), sc(e) = sc(hi) sc(lo) / dbl(q_{L-1});
     chunks        monomial: c_{jm} .. c_{jm+m-1}; Chebyshev: the T_m-adic expansion p = sum_j r_j(x) T_m(x)^j by repeated
                   division by T_m (the chunk coefficients grow by up to about 2^(g-1));
     giant powers  Y_1 = E_m, Y_j = dot_product_rescale({Y_hi}, {Y_lo}) at level k - delta(m) - delta(j), only those needed;
     inner sums    with mi = m - 1, L_in = k - delta(mi), J the j >= 1 whose chunk is not identically zero, L_out =
                   min(L_in - 1, min_J lev(Y_j)), Sigma = scale_out dbl(q_{L_out-1}), tau_j = Sigma / sc(Y_j), tau_0 =
                   scale_out: the weight of E_i in sum j is rint(chunk_j[i] (tau_j dbl(q_{L_in-1}) / sc(i))), its constant
                   rint(chunk_j[0] (tau_j dbl(q_{L_in-1}))); all sums of {0} u J in ONE linear_combination_levels at level
                   L_in over E_1 .. E_mi, each read at its own level, then ONE rescale_to_next of the whole batch;
     result        I_0 (level L_in - 1) when J is empty, else dot_product_rescale({Y_j}, {I_j}, j in J) at level L_out plus
                   I_0 at level L_out - 1. Its scale is scale_out exactly, by construction.
   rint rounds half to even; the integer is reduced per prime exactly, whatever its size.
   The plan query fills *plan and, when not NULL, the HOST tables inner_weights [g][m - 1][inner_level] and inner_constants
   [g][inner_level] (rows of sums that are not formed stay zero); it works on host-only contexts. temp_bytes_per_item: the
   pool blocks the evaluation takes per item of the batch (the small tables, a few KiB per call, are not counted).
   coeffs: HOST doubles, degree + 1 of them. scale_out: 0 means the input scale. ct: count x 2 x k x N (NTT form, not
   modified); out: count x 2 x out_level x N, overlapping nothing; *out_level and *out_scale (may be NULL) get the plan's.
   Checks, in this order: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside the ciphertext levels, a BFV
   context ("CKKS only"), a non-finite or non-positive scale, a non-finite coefficient, basis > 1, d < 1, n_baby == 1 or
   > d + 1, out_level < 1 ("end of modulus switching chain reached"), with d >= 2 missing keys or a key with fewer digits
   than level k needs, out overlapping ct -> E_INVALIDARG; then count == 0 -> S_OK; then a host-only context ->
   COR_E_INVALIDOPERATION. (The plan query has no keys, no buffers and no batch: its checks end with out_level.)
   Temporaries are blocks of the context's pool, taken and released in stream order on the calling lane; the tables travel
   in kernel arguments: nothing synchronises, but the entry may allocate and is NOT capturable. With a transparency sink: one
   flag per output ciphertext from a read pass over out. */
typedef struct sealhip_poly_plan
{
    uint32_t d, m, g;
    uint32_t inner_level; /* L_in: the level the inner sums are formed at */
    uint32_t out_level;
    uint32_t n_products;  /* key-switched products: baby elements, giant powers, the outer sum */
    double out_scale;
    uint64_t temp_bytes_per_item;
} sealhip_poly_plan;
long sealhip_evaluator_polynomial_plan_ckks(sealhip_context *ctx, uint32_t k, double scale, const double *coeffs, uint32_t degree,
                                            uint32_t basis, uint32_t n_baby, double scale_out, sealhip_poly_plan *plan,
                                            uint64_t *inner_weights, uint64_t *inner_constants);
long sealhip_evaluator_evaluate_polynomial_ckks(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count, double scale,
                                                const double *coeffs, uint32_t degree, uint32_t basis, uint32_t n_baby,
                                                double scale_out, const sealhip_kswitch_key *const *relin_keys,
                                                uint32_t n_relin_keys, uint64_t *out, uint32_t *out_level, double *out_scale);

/* ---------------------------------------------------------------- decrypt-side arithmetic */
/* Decryptor::dot_product_ct_sk_array (decryptor.cpp:218-265): out[count][k][N] = c_0 + sum_{i>=1} c_i * s^i, in the form
   of the ciphertext (is_ntt_form). sk_powers_ntt = the Decryptor's secret_key_array_: (size-1) polynomials s, s^2, ...
   in NTT form, each with the key level's row stride (n_key_moduli x N); device memory. */
long sealhip_decryptor_dot_product_ct_sk(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                                         const uint64_t *sk_powers_ntt, int32_t is_ntt_form, uint64_t *out);
/* RNSTool::decrypt_scale_and_round (rns.cpp:1070-1126), BFV: in[count][k][N] -> out[count][N] coefficients mod t */
long sealhip_decrypt_scale_and_round(sealhip_context *ctx, uint32_t k, const uint64_t *in, size_t count, uint64_t *out);
/* Decryptor::invariant_noise_budget (decryptor.cpp:269-325) for a BFV batch: budgets[i] (host memory) of ciphertext i,
   ct[count][size][k][N] in coefficient form, sk_powers_ntt as for sealhip_decryptor_dot_product_ct_sk.
   Synchronises once; not capturable. */
long sealhip_decryptor_invariant_noise_budget(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size,
                                              size_t count, const uint64_t *sk_powers_ntt, int32_t *budgets);
/* Decryptor::decrypt (decryptor.cpp:51-150): BFV (is_ntt_form must be 0): plain[count][N] coefficients mod t
   (dot product + decrypt_scale_and_round); CKKS (is_ntt_form must be 1): plain[count][k][N] in NTT form.
   Device memory, temporaries from the lane arena, no synchronisation (capturable).
   Both entries: NULL pointers -> E_POINTER; then, also on host-only contexts, k outside 1..n_key_moduli or size outside
   2..16 -> E_INVALIDARG ("encrypted is not valid for encryption parameters"); a CKKS context asking for a noise budget ->
   COR_E_INVALIDOPERATION ("unsupported scheme"); a BFV decrypt with is_ntt_form != 0 or a CKKS decrypt with is_ntt_form
   == 0 -> E_INVALIDARG; then a host-only context -> COR_E_INVALIDOPERATION. count = 0 -> S_OK, nothing launched. A batch
   larger than the lane's arena is processed in chunks. */
long sealhip_decryptor_decrypt(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                               const uint64_t *sk_powers_ntt, int32_t is_ntt_form, uint64_t *plain);

/* ---------------------------------------------------------------- HIP graphs for launch-bound small batches */
/* Small batches are bound by kernel launches (one multiply+relinearize of a single N=2^15 ciphertext is ~25 launches):
   a fixed sequence of operations on fixed device buffers can be captured once from the context's stream and replayed as
   one hipGraph launch. Run the sequence once before capturing (tables, the arena and the NTT tickets are allocated on
   first use; allocation and synchronisation are not capturable); entry points that synchronise (is_transparent,
   ckks_encode, the wire format) cannot be captured. An operation that fails during a capture aborts and discards the
   capture (the error message says so). A graph replays on the lane (thread) it was captured on, whichever thread
   launches it; it goes stale -- launch fails with COR_E_INVALIDOPERATION -- when that lane's workspace is re-allocated
   or any key-switch key of the context is destroyed. Operand buffers are the caller's: they must outlive the graph. */
typedef struct sealhip_graph sealhip_graph;
long sealhip_graph_capture_begin(sealhip_context *ctx);
long sealhip_graph_capture_end(sealhip_context *ctx, sealhip_graph **graph);
long sealhip_graph_launch(sealhip_context *ctx, sealhip_graph *graph);
long sealhip_graph_destroy(sealhip_context *ctx, sealhip_graph *graph);

/* ---------------------------------------------------------------- encrypt-side arithmetic */
/* util::encrypt_zero_symmetric (util/rlwe.cpp:204-300) with the random samples handed in (sampling and the CSPRNG
   stay on the host): ct[count][2][rows][N] = ([-(a*s + e)]_q, a) over key primes 0..rows-1 (rows = n_key_moduli for
   key generation, keygenerator.cpp:347; rows = the level's k for Encryptor::encrypt_zero_internal, encryptor.cpp:183).
   a_ntt[count][rows][N]: uniform residues, taken to be in NTT form as the reference samples them (:245-249);
   noise[count][N]: small signed error coefficients (sample_poly_normal, :61-95); sk_ntt: rows x N, NTT form.
   is_ntt_form != 0 leaves the ciphertext in NTT form (CKKS, keys), 0 in coefficient form (BFV). Device memory. */
long sealhip_encrypt_zero_symmetric(sealhip_context *ctx, uint32_t rows, int32_t is_ntt_form, const uint64_t *a_ntt,
                                    const int32_t *noise, const uint64_t *sk_ntt, size_t count, uint64_t *ct);
/* util::encrypt_zero_asymmetric (util/rlwe.cpp:140-202): ct[count][2][rows][N], ct_j = pk_j * u + e_j.
   pk_ntt[2][rows][N] (NTT form); u[count][N] ternary (sample_poly_ternary, :25-59); noise[count][2][N]. */
long sealhip_encrypt_zero_asymmetric(sealhip_context *ctx, uint32_t rows, int32_t is_ntt_form, const uint64_t *pk_ntt,
                                     const int32_t *u, const int32_t *noise, size_t count, uint64_t *ct);
/* util::multiply_add_plain_with_scaling_variant / multiply_sub_plain_with_scaling_variant
   (util/scalingvariant.cpp:15-52 / :54-92) on c_0 of every ciphertext: the last step of Encryptor::encrypt for BFV
   (encryptor.cpp:221-225) and Evaluator::add_plain_inplace / sub_plain_inplace for BFV (evaluator.cpp:1338-1342).
   plain[count][N] coefficients < t (plain_item_stride words apart; 0 = one plaintext for all);
   ct[count][size][k][N] in place. */
long sealhip_multiply_add_plain_with_scaling_variant(sealhip_context *ctx, uint32_t k, const uint64_t *plain,
                                                     size_t plain_item_stride, uint64_t *ct, uint32_t size, size_t count,
                                                     int32_t subtract);
/* Evaluator::add_plain_inplace / sub_plain_inplace (evaluator.cpp:1290-1435): BFV = the scaling variant above;
   CKKS = add/sub_poly_coeffmod of the NTT-form plaintext plain[count][k][N] on c_0. */
long sealhip_evaluator_add_plain(sealhip_context *ctx, uint32_t k, uint64_t *ct, uint32_t size, size_t count,
                                 const uint64_t *plain, size_t plain_item_stride, int32_t subtract);

/* ---------------------------------------------------------------- Encryptor (encryptor.cpp:106-259), batched */
/* Encryptor::encrypt / encrypt_zero(parms_id) with a public key, for a batch: ct[count][2][k][N] at level k.
   pk_ntt: the key-level public key, 2 x n_key x N, NTT form (device). Below the key level the zero encryption runs over
   the k + 1 primes of the previous level and is divided and rounded by q_k (encryptor.cpp:141-176): with nsp special
   primes the previous level of the first level has k_first + 1 rows, not n_key.
   plain == NULL: encrypt_zero at level k (1..n_key). Otherwise BFV: plain[count][N] < t, k must be the first level
   (k_first = n_key - nsp); CKKS: plain[count][k][N] in NTT form at level k (1..k_first). plain_item_stride: words between
   consecutive plaintexts, 0 = one plaintext for all. u[count][N] (sample_poly_ternary), noise[count][2][N] (e_0, e_1 of
   sample_poly_normal): int32 samples (device). BFV ciphertexts come out in coefficient form, CKKS in NTT form.
   Checks, before any device work: NULL ctx / pk_ntt / u / noise / ct -> E_POINTER; k outside 1..n_key -> E_INVALIDARG
   ("parms_id is not valid for encryption parameters"); a plaintext at a level it cannot take -> E_INVALIDARG ("plain is
   not valid for encryption parameters"); then a host-only context -> COR_E_INVALIDOPERATION. count = 0 -> S_OK, nothing
   launched. Stream-ordered on the calling thread's lane; temporaries from its arena, in chunks. */
long sealhip_encryptor_encrypt(sealhip_context *ctx, uint32_t k, const uint64_t *pk_ntt, const uint64_t *plain,
                               size_t plain_item_stride, const int32_t *u, const int32_t *noise, size_t count,
                               uint64_t *ct);
/* Encryptor::encrypt_symmetric / encrypt_zero_symmetric (rlwe.cpp:204-300) for a batch at level k, same plaintext rules:
   c_1 = sample_poly_uniform(BlakePRNG(seed_i)) expanded on the device from seeds_host[count][8] (host; the seed
   BlakePRNGFactory().create() drew), c_0 = -(a s + e) [+ the plaintext]. sk_ntt: n_key x N (NTT form, device);
   noise[count][N] int32 (device). save_seed != 0 selects the reference's seeded branch: for BFV, a is sampled in coefficient
   form and c_1 stays that sample; the branch is dropped when k x N < 9 words (:225-230), as the reference drops it. ct
   always receives both polynomials (c_1 as Ciphertext::expand_seed would restore it); write the Serializable<> stream with
   sealhip_ciphertext_save_seeded. Checks as sealhip_encryptor_encrypt (NULL seeds_host / sk_ntt / noise / ct ->
   E_POINTER). Not capturable (the seeds are staged on the host). */
long sealhip_encryptor_encrypt_symmetric(sealhip_context *ctx, uint32_t k, const uint64_t *sk_ntt,
                                         const uint64_t *plain, size_t plain_item_stride, const uint64_t *seeds_host,
                                         const int32_t *noise, int32_t save_seed, size_t count, uint64_t *ct);

/* ---------------------------------------------------------------- BatchEncoder */
/* 1 when the context can batch: BFV with a prime plain modulus = 1 (mod 2N) (context.cpp:262-275, qualifiers().using_batching) */
long sealhip_context_using_batching(const sealhip_context *ctx, int32_t *using_batching);
/* BatchEncoder::encode (batchencoder.cpp:113-154): values[count][n_values] (n_values <= N, each < t; missing slots are
   zero) -> plain[count][N] coefficients; BatchEncoder::decode (:339-376): plain[count][N] -> values[count][N].
   E_INVALIDARG when the parameters do not support batching. Device memory. */
long sealhip_batch_encode(sealhip_context *ctx, const uint64_t *values, size_t n_values, size_t count, uint64_t *plain);
long sealhip_batch_decode(sealhip_context *ctx, const uint64_t *plain, size_t count, uint64_t *values);
/* the vector<int64_t> overloads (batchencoder.cpp:156-198, :378-420): values in (-t/2, t/2]; a negative value is stored as
   t + v, a decoded slot above t/2 comes back as v - t */
long sealhip_batch_encode_int64(sealhip_context *ctx, const int64_t *values, size_t n_values, size_t count, uint64_t *plain);
long sealhip_batch_decode_int64(sealhip_context *ctx, const uint64_t *plain, size_t count, int64_t *values);

/* CKKSEncoder::encode (ckks.h:405-617) / decode (:623-747), double precision. values: complex numbers as (re, im) pairs
   of doubles in device memory. encode: values[count][n_values] (n_values <= N/2; the other slots are zero) -> plain
   [count][k][N] in NTT form at `scale`; decode: plain[count][k][N] -> values[count][N/2]. Every floating-point operation
   is issued in the reference's order without contraction, so the outputs equal the reference's bits given the same root
   tables (host libm). E_INVALIDARG: "scale out of bounds", "encoded values are too large", "values_size is too large". */
long sealhip_ckks_encode(sealhip_context *ctx, uint32_t k, const double *values, size_t n_values, size_t count, double scale,
                         uint64_t *plain);
long sealhip_ckks_decode(sealhip_context *ctx, uint32_t k, const uint64_t *plain, size_t count, double scale, double *values);
/* CKKSEncoder::encode(double value, ...) (ckks.cpp:80-216): `value` in every slot = the constant polynomial round(value*scale);
   plain[count][k][N] (the same plaintext `count` times), NTT form. Errors as the reference: "scale out of bounds", "encoded
   value is too large". sealhip_ckks_encode_int64: CKKSEncoder::encode(int64_t value, ...) (ckks.cpp:218-275), scale 1. */
long sealhip_ckks_encode_value(sealhip_context *ctx, uint32_t k, double value, double scale, size_t count, uint64_t *plain);
long sealhip_ckks_encode_int64(sealhip_context *ctx, uint32_t k, int64_t value, size_t count, uint64_t *plain);

/* Ciphertext::resize (ciphertext.cpp:84-124) over a device-resident batch: dst[count][dst_size][k][N] receives the first
   min(src_size, dst_size) polynomials of every src[count][src_size][k][N]; added polynomials are zero (IntArray::resize).
   What a chain needs between relinearize (which leaves the batch stride at its old size) and the next multiply. */
long sealhip_ciphertext_resize(sealhip_context *ctx, uint32_t k, const uint64_t *src, uint32_t src_size, uint64_t *dst,
                               uint32_t dst_size, size_t count);

/* ---------------------------------------------------------------- ciphertext wire format */
/* What Ciphertext::save_members writes ahead of the coefficient words (ciphertext.cpp:170-188). */
typedef struct sealhip_ciphertext_info
{
    uint64_t parms_id[4];         /* parms_id_type (4 x uint64 Blake2 hash, computed by the host library)  */
    uint32_t is_ntt_form;
    uint32_t size;                /* polynomials                                                           */
    uint32_t coeff_modulus_size;  /* k                                                                     */
    uint32_t seeded;              /* 1: c_1 was replaced by a PRNG seed (ciphertext.cpp:189-208)           */
    uint64_t poly_modulus_degree; /* N                                                                     */
    double scale;
    uint64_t data_words;          /* uint64 words stored in the stream                                     */
    uint64_t total_bytes;         /* SEALHeader::size of the whole object                                  */
} sealhip_ciphertext_info;
/* Registers the parms_id of level k (k = n_key_moduli: the key level). The binding copies them from
   SEALContext::get_context_data(...)->parms_id() once per context (context.cpp:455-540 builds the chain);
   the loader uses them the way is_metadata_valid_for does (valcheck.cpp:67-105). */
long sealhip_context_set_parms_id(sealhip_context *ctx, uint32_t k, const uint64_t parms_id[4]);
/* Serialization::LoadHeader + the metadata of Ciphertext::load_members, no context needed (serialization.cpp:137-176,
   ciphertext.cpp:248-267). Errors as the reference: bad magic/size/compression -> COR_E_INVALIDOPERATION
   ("loaded SEALHeader is invalid" / "incompatible version"), truncated input -> E_UNEXPECTED ("I/O error"). */
long sealhip_ciphertext_peek(const void *bytes, size_t len, sealhip_ciphertext_info *info);
/* Ciphertext::load (ciphertext.cpp:228-330, uncompressed stream): validates the metadata against the context and
   copies the coefficient words from `bytes` (host) straight into dst_device (capacity in words). A seeded ciphertext
   (info->seeded: one stored polynomial + a 64-byte seed, what Encryptor::encrypt_symmetric(...).save() writes) is expanded
   like Ciphertext::expand_seed does (:126-133): c_1 is re-sampled on the device from the seed (sealhip_expand_seed) with
   the reference's BlakePRNG (BLAKE2Xb, randomgen.cpp:63-73) and sample_poly_uniform (util/rlwe.cpp:101-129), the same words
   as the host implementation csrc/blake2xb.cpp; dst_device receives both polynomials. */
long sealhip_ciphertext_load(sealhip_context *ctx, const void *bytes, size_t len, sealhip_ciphertext_info *info,
                             uint64_t *dst_device, size_t capacity_words);
/* Ciphertext::load for a batch of `count` streams (a std::vector<Ciphertext> arriving from clients): stream i (lens[i]
   bytes) lands at dst_device + i * item_stride_words and its metadata in infos[i]. Seeded and unseeded streams may be mixed.
   Every stream is checked as sealhip_ciphertext_load checks it, with the same errors and messages, before anything is
   written: when stream i fails the call returns its error and dst_device is unchanged. A stride below an item's size x k x N
   is "destination buffer is too small". The seeded items of one level are expanded in one sealhip_expand_seed launch (per
   arena chunk); the call synchronises once, at the end. */
long sealhip_ciphertext_load_many(sealhip_context *ctx, const void *const *streams, const size_t *lens, size_t count,
                                  sealhip_ciphertext_info *infos, uint64_t *dst_device, size_t item_stride_words);
/* Ciphertext::save_size(compr_mode_type::none) (ciphertext.cpp:135-168) and Ciphertext::save: the stream is written
   into `bytes` (host) with the coefficient words copied straight from src_device. */
long sealhip_ciphertext_save_size(const sealhip_context *ctx, uint32_t size, uint32_t k, size_t *bytes);
long sealhip_ciphertext_save(sealhip_context *ctx, const sealhip_ciphertext_info *info, const uint64_t *src_device,
                             void *bytes, size_t capacity, size_t *written);
/* Serializable<Ciphertext>::save (ciphertext.cpp:189-208) of a seeded encryption: the metadata of info (size must be 2),
   the k x N words of c_0 from src_device, then the 64-byte seed of c_1. Stream size:
   sealhip_ciphertext_save_size(ctx, 1, k) + 64; bytes == NULL: size query. Synchronises once. Loads back through
   sealhip_ciphertext_load, which expands the seed. */
long sealhip_ciphertext_save_seeded(sealhip_context *ctx, const sealhip_ciphertext_info *info,
                                    const uint64_t *src_device, const uint64_t seed[8], void *bytes,
                                    size_t capacity, size_t *written);
/* KSwitchKeys::load (kswitchkeys.cpp:87-150; RelinKeys / GaloisKeys streams, uncompressed): loads keys_[index] -- RelinKeys:
   index = key_power - 2 (relinkeys.h:61-68), GaloisKeys: index = (galois_elt - 1) / 2 (galoiskeys.h:52-55) -- with its
   decomposition digits concatenated straight from the stream into HBM. *key = NULL when that slot is empty; n_slots (may
   be NULL) receives keys_.size(). Needs the key level's parms_id registered (k = n_key_moduli). Seeded digits (keys saved
   as Serializable<RelinKeys>) are expanded on the device as in sealhip_ciphertext_load, all digits of the slot in one
   launch. */
long sealhip_kswitch_key_load_stream(sealhip_context *ctx, const void *bytes, size_t len, uint32_t index,
                                     sealhip_kswitch_key **key, uint64_t *n_slots);
/* Ciphertext::expand_seed on the host (works on host-only contexts): out_host[rows][N] = the words of c_1 for `seed`
   (random_seed_type: 8 x uint64) over the first `rows` key primes. sealhip_debug_blake2xb: the BLAKE2Xb function under it. */
long sealhip_expand_seed_host(sealhip_context *ctx, uint32_t rows, const uint64_t seed[8], uint64_t *out_host);
long sealhip_debug_blake2xb(void *out, size_t outlen, const void *in, size_t inlen, const void *key, size_t keylen);
/* Ciphertext::expand_seed on the device for a batch: out_device + i * item_stride_words receives the rows x N words of c_1
   for seed i (seeds_host: count x 8 words, the random_seed_type layout), word for word what sealhip_expand_seed_host
   computes. item_stride_words 0 means rows x N; 2 x k x N with out_device = ct + k x N fills the c_1 of a ciphertext batch.
   rows outside 1..n_key_moduli, or a nonzero stride below rows x N -> E_INVALIDARG (null pointers -> E_POINTER first);
   count 0 -> S_OK, nothing launched. Runs on the calling thread's lane in stream order (the seeds are staged before it
   returns). DESIGN.md "Seed expansion" describes the kernels. */
long sealhip_expand_seed(sealhip_context *ctx, uint32_t rows, const uint64_t *seeds_host, size_t count, uint64_t *out_device,
                         size_t item_stride_words);
/* Test hook of sealhip_expand_seed for the calling thread's lane: candidates provisioned per seed beyond rows x N (rounded
   up to whole 4096-byte PRNG buffers). < 0 restores the computed default; 0 sends every rejection through the in-kernel
   continuation. It never changes the words, only which path produces them. */
long sealhip_debug_seed_slack(sealhip_context *ctx, int64_t extra_candidates_per_seed);
/* KSwitchKeys::save (kswitchkeys.cpp:43-85 under Serialization::Save, uncompressed): writes a RelinKeys / GaloisKeys stream
   whose keys_[i] is keys[i] (NULL = unused slot, keys_dim2 = 0) with the digit words copied straight from HBM. bytes == NULL:
   only the size is reported in *written. Needs the key level's parms_id registered. The stream round-trips through
   sealhip_kswitch_key_load_stream and is what the reference's KSwitchKeys::load reads. */
long sealhip_kswitch_keys_save(sealhip_context *ctx, const sealhip_kswitch_key *const *keys, uint32_t n_slots, void *bytes,
                               size_t capacity, size_t *written);
/* ---------------------------------------------------------------- KeyGenerator (keygenerator.cpp:146-240, :325-398) */
/* KeyGenerator::relin_keys(count, save_seed) (keygenerator.cpp:146-175) and galois_keys(galois_elts, save_seed) (:177-240)
   with the random samples handed in: keys[i] receives an ordinary key-switch key handle (usable by relinearize, apply_galois,
   rotate_vector, the saves and sealhip_kswitch_key_destroy, like a loaded one) whose digits are generate_one_kswitch_key
   (:325-369) for the new key sk^(i+2) (relin; slot index i) or apply_galois_ntt(sk, galois_elts[i]) (Galois; slot index
   (elt - 1) / 2). For digit j < d = ceil(n_ct / nsp):
     c1 = sample_poly_uniform(BlakePRNG(seed_j)) over the n_key key primes, taken as NTT form (util/rlwe.cpp:245-249),
     c0 = -(NTT(e_j) + c1 * sk) (:266-284), and c0[r] += (prod of the special primes mod q_r) * new_key[r] for r in
     [j*nsp, min((j+1)*nsp, n_ct)) (keygenerator.cpp:350-366).
   sk_ntt: n_key x N, NTT form (device). seeds_host: n_keys x d x 8 words (random_seed_type, BlakePRNGFactory().create()'s
   seed; host). noise: n_keys x d x N int32 (sample_poly_normal's signed values; device). Every word equals the reference's
   given the same samples. keep_seeds: save_seed -- the handle keeps the d seeds (host memory) for
   sealhip_kswitch_keys_save_seeded (the reference drops save_seed below n_key x N = 9 words, rlwe.cpp:225-230, which no
   context reaches: n_key >= 2, N >= 8).
   Checks before any device work (also on host-only contexts): null pointers -> E_POINTER; an even element, one >= 2N or a
   repeated one -> E_INVALIDARG ("Galois element is not valid"); count > 14 -> E_INVALIDARG ("invalid count"); parameters
   without batching (Galois keys) -> COR_E_INVALIDOPERATION. Every context uses key switching (sealhip_context_create
   refuses a single prime). count / n_elts = 0 -> S_OK, nothing launched (on a device context). On any error every keys[i] is NULL and nothing
   leaks. Runs on the calling thread's lane and synchronises once, at the end; not capturable. Creating keys does not
   make captured graphs stale (sealhip_kswitch_key_load does not either); destroying them does. */
long sealhip_generate_relin_keys(sealhip_context *ctx, const uint64_t *sk_ntt, uint32_t count, const uint64_t *seeds_host,
                                 const int32_t *noise, int32_t keep_seeds, sealhip_kswitch_key **keys);
long sealhip_generate_galois_keys(sealhip_context *ctx, const uint64_t *sk_ntt, const uint32_t *galois_elts, uint32_t n_elts,
                                  const uint64_t *seeds_host, const int32_t *noise, int32_t keep_seeds,
                                  sealhip_kswitch_key **keys);
/* Serializable<RelinKeys / GaloisKeys>::save (KSwitchKeys::save with seeded digits): sealhip_kswitch_keys_save's stream,
   but every digit is written as Ciphertext::save_members writes a ciphertext with the seed marker (ciphertext.cpp:189-208):
   metadata of size 2, the words of c0 only, then the 64-byte seed of c1. Every non-NULL key must carry seeds (made with
   keep_seeds), else E_INVALIDARG. bytes == NULL: size query. Round-trips through sealhip_kswitch_key_load_stream, which
   expands the seeds on the device. */
long sealhip_kswitch_keys_save_seeded(sealhip_context *ctx, const sealhip_kswitch_key *const *keys, uint32_t n_slots,
                                      void *bytes, size_t capacity, size_t *written);
/* ---------------------------------------------------------------- RLWE samples from seeds */
/* The ternary polynomials (u, the secret key) and the noise polynomials (e, e_0, e_1) of encryption and key generation,
   drawn on the device from 64-byte seeds, so that only seeds cross from the host. The rule is the library's own (the
   streams are NOT the reference's sample_poly_ternary / sample_poly_normal streams); the noise LAW is the reference's.
     stream word m of seed S = the little-endian 64-bit word at byte 8m of BlakePRNG(S) (the words under
       sealhip_expand_seed, before its rotate-and-mask);
     item i draws n_ternary ternary polynomials, then n_noise noise polynomials; coefficient j of polynomial p comes from
       word pN + j alone (fixed consumption: no rejection);
     ternary: mulhi64(w, 3) - 1; noise: with r = w >> 1, magnitude = #{m in 0..18 : r >= T_m}, negative when w & 1, where
       T_m are the 19 constants of csrc/sample_map.hpp: trunc(X), X ~ N(0, 3.2^2) conditioned on |X| <= 19.2
       (util/rlwe.cpp:57-99), to within 2^-40 in statistical distance.
   sealhip_sample_polys: out_device + i * item_stride_words (int32 words) receives out[i][p][N] for seed i (seeds_host: count
   x 8 words). item_stride_words 0 means (n_ternary + n_noise) x N. Checks: null pointers -> E_POINTER; then, also on
   host-only contexts, n_ternary + n_noise outside 1..16, a nonzero stride below (n_ternary + n_noise) x N, a stride that
   is no multiple of 4 or an out_device that is not 16-byte aligned (the kernel stores 16 bytes at a time) -> E_INVALIDARG;
   then a host-only context -> COR_E_INVALIDOPERATION; count 0 -> S_OK, nothing launched. Runs on the calling thread's lane
   in stream order; the seeds are staged before it returns (not capturable). The PRNG roots it derives are erased from the
   arena in stream order; out_device is the caller's to erase (sealhip_memset_zero).
   sealhip_sample_polys_host: the same words into host memory, computed on the host (works on host-only contexts; no
   alignment rule).
   sealhip_debug_sample_map: the kernel's own map functions on n caller-supplied words (device): kind 0 ternary, 1 noise;
   other kinds -> E_INVALIDARG. The only way to reach the high thresholds: streams exceed magnitude 15 once in 10^7 draws. */
long sealhip_sample_polys(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary, uint32_t n_noise,
                          int32_t *out_device, size_t item_stride_words);
long sealhip_sample_polys_host(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary,
                               uint32_t n_noise, int32_t *out_host, size_t item_stride_words);
/* sealhip_sample_polys with the two kinds in two arrays, the layouts sealhip_encryptor_encrypt takes its samples in:
   ternary_device[count][n_ternary][N] and noise_device[count][n_noise][N] (the same samples: polynomial p of item i still
   comes from words [pN, (p+1)N) of seed i, ternary ones first). An array whose count is 0 may be NULL. Checks as
   sealhip_sample_polys (both pointers 16-byte aligned). */
long sealhip_sample_polys_split(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t n_ternary,
                                uint32_t n_noise, int32_t *ternary_device, int32_t *noise_device);
long sealhip_debug_sample_map(sealhip_context *ctx, const uint64_t *words_device, size_t n, int32_t kind, int32_t *out_device);
/* KeyGenerator::generate_sk (keygenerator.cpp:66-103) from a seed: sk_ntt_device (n_key x N words) receives the ternary
   polynomial sealhip_sample_polys(seed, 1, 0) lifted over the n_key key primes (-1 -> q_j - 1) in NTT form. The
   coefficient-form scratch is erased in stream order. null pointers -> E_POINTER; a host-only context ->
   COR_E_INVALIDOPERATION. Stream-ordered on the calling thread's lane; not capturable. */
long sealhip_generate_secret_key(sealhip_context *ctx, const uint64_t seed_host[8], uint64_t *sk_ntt_device);
/* ---------------------------------------------------------------- fixed-weight secrets and encapsulation */
/* The fixed-weight rule (the library's own): the polynomial of weight h, 1 <= h <= N, of seed S is
     w_i, i < N = stream words [0, N) of BlakePRNG(S), the words sealhip_sample_polys' ternary polynomial 0 would consume;
     rank_i = #{ j : w_j < w_i, or w_j == w_i and j < i }, a permutation of 0 .. N-1;
     coefficient i = 0 when rank_i >= h, else -1 when w_i & 1, else +1.
   The weight is exactly h; consumption is fixed at N words (no rejection, no continuation). The support is the set of the h
   smallest words: uniform over h-subsets for i.i.d. uniform words, and bit 0 is an independent fair sign unless two words
   agree in their upper 63 bits, so the statistical distance from (uniform subset x uniform signs) is at most N^2 / 2^64
   (2^-32 at N = 2^16). The device counts ranks in constant time (every lane compares its words with all N; no branch, loop
   bound, address or LDS index depends on a word; h and N are public).
   sealhip_sample_fixed_weight: out_device + i * item_stride_words receives out[i][N] (int32) for seed i. Checks, alignment
   and stride rules, lane, staging, erasure (the raw-word scratch included), host-only and empty-batch behaviour are
   sealhip_sample_polys' with one polynomial; h outside 1..N -> E_INVALIDARG.
   sealhip_sample_fixed_weight_host: the same words computed on the host (works on host-only contexts).
   sealhip_debug_fixed_weight_map: the rank kernel itself on caller-supplied words_device[n_polys][N] -> out_device[n_polys][N]
   (both 16-byte aligned), as sealhip_debug_sample_map: the only way to reach ties and the extreme words.
   sealhip_generate_sparse_secret_key: sealhip_generate_secret_key with the fixed-weight polynomial of weight h in place of the
   ternary one: the same lift (-1 -> q_j - 1), transform and erasure of the coefficient-form scratch; both schemes. */
long sealhip_sample_fixed_weight(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t h, int32_t *out_device,
                                 size_t item_stride_words);
long sealhip_sample_fixed_weight_host(sealhip_context *ctx, const uint64_t *seeds_host, size_t count, uint32_t h,
                                      int32_t *out_host, size_t item_stride_words);
long sealhip_debug_fixed_weight_map(sealhip_context *ctx, const uint64_t *words_device, size_t n_polys, uint32_t h,
                                    int32_t *out_device);
long sealhip_generate_sparse_secret_key(sealhip_context *ctx, const uint64_t seed_host[8], uint32_t h, uint64_t *sk_ntt_device);
/* Key-switch keys from one secret to ANOTHER: generate_one_kswitch_key with the new key handed in. keys[i] switches what is
   encrypted under sk_from_ntt[i] (n_keys x n_key x N, NTT form, device) to sk_to_ntt; no Galois element, no power of sk.
   seeds_host, noise, keep_seeds, the checks, errors, lane and synchronisation are sealhip_generate_relin_keys'; the handles are
   ordinary key-switch keys. level, 1 <= level <= n_ct (else E_INVALIDARG): n_ct gives the full key; a smaller level
   zero-fills, in both components, the data-prime rows r >= level of every digit and every digit j >= ceil(level / nsp). The
   key then serves key switches at levels <= level only (above it every entry answers E_INVALIDARG, "kswitch_keys is not
   valid for encryption parameters"), and cannot keep seeds (keep_seeds -> E_INVALIDARG: a seed gives back the c_1 rows
   left out). Encapsulation makes its dense -> sparse key with level = 1: an encryption under the sparse secret is then
   published modulo q_0 times the special primes only, not modulo the whole key modulus, where a sparse secret has the
   least margin. */
long sealhip_generate_switching_keys(sealhip_context *ctx, const uint64_t *sk_to_ntt, const uint64_t *sk_from_ntt,
                                     uint32_t n_keys, uint32_t level, const uint64_t *seeds_host, const int32_t *noise,
                                     int32_t keep_seeds, sealhip_kswitch_key **keys);
/* Re-encryption under another secret: out[count][2][k][N] = (c_0, 0) + switch_key(c_1) of ct[count][2][k][N] -- the words of
   sealhip_switch_key_inplace on a copy of ct whose c_1 is zeroed, with target c_1. A size-2 ciphertext under the key's
   source secret becomes one under its target secret. Both schemes (CKKS in NTT form, BFV in coefficient form), both modes.
   Checks before any device work: null pointers -> E_POINTER; k outside 1..n_ct, a key that does not serve level k (fewer
   digits than it needs, or made for a lower level), out overlapping ct -> E_INVALIDARG; then a host-only context ->
   COR_E_INVALIDOPERATION; count 0 -> S_OK. Transparency flag as sealhip_evaluator_apply_galois. */
long sealhip_evaluator_switch_secret(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                     const sealhip_kswitch_key *key, uint64_t *out);
/* sealhip_evaluator_bootstrap with ModRaise alone under a sparse secret: the q_0 rows of ct -> switch_secret at level 1 with
   to_sparse -> mod_raise to k_top -> switch_secret at k_top with to_dense -> the same CoeffToSlot / EvalMod / SlotToCoeff.
   The input, the output and every other key are under the working (dense) secret; K bounds the I of the SPARSE secret:
   |I_j| <= (h + 1) / 2. to_sparse: dense -> sparse, made with level = 1; to_dense: sparse -> dense at the full level. Checks
   are sealhip_evaluator_bootstrap's, then the two keys' (null -> E_POINTER; one that does not serve its level ->
   E_INVALIDARG). Not capturable; the intermediates are the tables' block and the lane arena. */
long sealhip_evaluator_bootstrap_encapsulated(sealhip_context *ctx, const sealhip_bootstrap_tables *tables, uint32_t k_in,
                                              const uint64_t *ct, size_t count, const uint32_t *galois_elts,
                                              const sealhip_kswitch_key *const *galois_keys, uint32_t n_keys,
                                              const sealhip_kswitch_key *const *relin_keys, uint32_t n_relin_keys,
                                              const sealhip_kswitch_key *to_sparse, const sealhip_kswitch_key *to_dense,
                                              uint64_t *out);
/* RGSW ciphertexts and the external product: the RLWE x RGSW product of Chillotti, Gama, Georgieva,
   Izabachene ("TFHE", J. Cryptology 2020) in this library's hybrid gadget, whose noise growth is additive. An RGSW
   encryption of a small polynomial m is two ordinary key-switch keys: K_b made with new_key = m and K_a made with
   new_key = m s. For a size-2 ciphertext (c_0, c_1) with phase c_0 + c_1 s,
       ct (x) rgsw = KS(c_0; K_b) + KS(c_1; K_a)
   has phase m (c_0 + c_1 s) + e_ks, e_ks ONE key switch's error (2 nd digit terms, one mod-down). The fork has no such
   method: what defines the words is the composition from entries this header already has -- sealhip_switch_key_partial
   on c_0 with K_b and on c_1 with K_a over all digits, the word-wise sum, sealhip_switch_key_finish with n_partials = 2 into
   a copy of the base -- restated over the oracle in tests/rgsw_ref.py. The fused entries decompose both components into
   one set of 2 nd digits, form ONE inner product with one reduction per word and run ONE mod-down; modular sums are
   associative, so the words are the composition's.

   sealhip_rgsw owns one device block [half][digit][component][n_key][N], half 0 = K_b, half 1 = K_a, each half in the
   layout of sealhip_kswitch_key_load.
   sealhip_generate_rgsw: n objects from m_coeff (n x N int32, DEVICE, coefficient form, small signed values). m is lifted
     over the key primes as a secret key is (-v -> q_j - v) and transformed, m s is a dyadic product with sk_ntt, and half h
     of message i is generated by the code behind sealhip_generate_switching_keys from seeds_host[i][h] (n x 2 x digits x 8
     words, HOST) and noise[i][h] (n x 2 x digits x N int32, DEVICE): every word is what that entry gives for
     sk_from = {NTT(m_i), NTT(m_i) (.) sk} with the same samples. level as there (1 .. n_ct). The lifted m and m s live in
     scratch that is erased in stream order. Checks: NULL ctx or sk_ntt, and with n > 0 NULL m_coeff, seeds_host, noise or
     out -> E_POINTER (every out[i] is NULL after any failure); then, also on host-only contexts, level outside 1 .. n_ct ->
     E_INVALIDARG; then a host-only context -> COR_E_INVALIDOPERATION; n == 0 -> S_OK; during a graph capture ->
     COR_E_INVALIDOPERATION. Allocates, and synchronises the calling thread's lane before it returns.
     Unlike sealhip_generate_switching_keys (at most 14 keys) there is no limit on n: the 2 n halves are assembled in
     batches. The scratch is erased before it is freed on the failure paths too.
   sealhip_rgsw_create: the object from two ordinary key handles (for example loaded from a stream), a device copy; refuses
     digit counts or levels that differ (E_INVALIDARG). sealhip_rgsw_export: keys[0] = K_b, keys[1] = K_a as two ordinary,
     owned key handles holding copies of the halves (the saves and the partial / finish entries work on them); both NULL
     after a failure. sealhip_rgsw_destroy: as sealhip_kswitch_key_destroy -- it waits for every lane, and graphs captured
     earlier are stale afterwards.

   The evaluator entries work on `count` size-2 ciphertexts at level k (count x 2 x k x N, DEVICE; CKKS in NTT form in both
   modes; BFV in coefficient form on a STRICT context -- PARITY BFV's in-bundle rows are the fork's quirk and do not
   decrypt) with ONE rgsw shared by the batch.
   sealhip_evaluator_external_product: out = base + ct (x) rgsw; base (count x 2 x k x N) may be NULL, meaning zero.
   sealhip_evaluator_cmux: out = ct0 + (ct1 - ct0) (x) rgsw, i.e. ct1 where rgsw encrypts 1 and ct0 where it encrypts 0; one
     streaming kernel reads both operands once and writes the difference and the copy of ct0 the mod-down adds into. The
     words are sealhip_evaluator_external_product(sub(ct1, ct0), base = ct0)'s.
   sealhip_evaluator_select: cts: count x 2^l x 2 x k x N; out: count x 2 x k x N = cts[.][index] for the index whose bit t
     (least significant first) rgsw_bits[t] encrypts. Level t = 0 .. l - 1 computes W'[i] = cmux(rgsw_bits[t]; W[2i],
     W[2i+1]): one prepare launch and one external product batched over count * 2^(l-t-1) pairs. l == 0 is a copy. The
     working sets between the levels (2^(l-1) + 2^(l-2) ciphertexts per item) and the differences (2^(l-1)) are parked in the
     lane's arena under a raised floor and take at most half of its cap; a batch that does not fit is walked in chunks of
     items and sealhip_debug_chunk_log ends with (count, items per chunk); when one item does not fit -> E_OUTOFMEMORY with
     a message that names both sizes.
   Checks, in this order: NULL ctx, ciphertext operands, out, rgsw (select: with l > 0 the list and every entry) ->
   E_POINTER; then, also on host-only contexts: k outside the ciphertext levels, (select) l > 16, BFV in PARITY mode, an
   operand, base or out not 16-byte aligned, out overlapping an operand or base -> E_INVALIDARG; then a host-only context
   -> COR_E_INVALIDOPERATION; then an rgsw that does not serve level k (fewer digits than the level needs, or made for a
   lower level: "rgsw is not valid for encryption parameters") -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched.
   With a transparency sink: one flag per output ciphertext, from the (last) mod-down, or from a read pass for l == 0.
   Nothing synchronises; capturable once the arena has its size (after one call of the same shape).
   sealhip_debug_ext_mac_plan: what the inner product's launcher would run for a chunk of `count` items at level k, with no
     launch: out[0] = 1 (the loop kernel) or 2 (the items family), out[1] = the instance's ND2 (0 for the loop kernel),
     out[2] = 1 when the 2 nd-term sum does not fit 128 bits and is reduced between its halves, out[3] = the item group. */
typedef struct sealhip_rgsw sealhip_rgsw;
long sealhip_generate_rgsw(sealhip_context *ctx, const uint64_t *sk_ntt, const int32_t *m_coeff, uint32_t n, uint32_t level,
                           const uint64_t *seeds_host, const int32_t *noise, sealhip_rgsw **out);
long sealhip_rgsw_create(sealhip_context *ctx, const sealhip_kswitch_key *key_b, const sealhip_kswitch_key *key_a,
                         sealhip_rgsw **out);
long sealhip_rgsw_export(sealhip_context *ctx, const sealhip_rgsw *rgsw, sealhip_kswitch_key **keys);
long sealhip_rgsw_destroy(sealhip_context *ctx, sealhip_rgsw *rgsw);
long sealhip_evaluator_external_product(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t count,
                                        const sealhip_rgsw *rgsw, const uint64_t *base, uint64_t *out);
long sealhip_evaluator_cmux(sealhip_context *ctx, uint32_t k, const uint64_t *ct0, const uint64_t *ct1, size_t count,
                            const sealhip_rgsw *rgsw, uint64_t *out);
long sealhip_evaluator_select(sealhip_context *ctx, uint32_t k, const uint64_t *cts, size_t count, uint32_t l,
                              const sealhip_rgsw *const *rgsw_bits, uint64_t *out);
long sealhip_debug_ext_mac_plan(sealhip_context *ctx, uint32_t k, size_t count, int32_t out[4]);
/* Blind rotation: the accumulator loop of programmable bootstrapping (Chillotti, Gama, Georgieva,
   Izabachene, "TFHE", J. Cryptology 2020, Alg. 3) over the external product above, with the two pieces a caller cannot
   compose without leaving the device per sample: a monomial product whose exponent differs per batch item, and the LWE
   modulus switch from q to 2N that makes those exponents. The fork has no such method; tests/blind_rotate_ref.py restates
   every entry over the oracle on top of tests/rgsw_ref.py.

   The ring is Z_q[X]/(X^N + 1); an exponent e is an integer in [0, 2N) with X^N = -1; e' = e mod N, sgn = -1 for e >= N.
   Coefficient form (BFV, STRICT): (X^e c)[x] = sgn c[x - e'] for x >= e' and -sgn c[N + x - e'] for x < e'. NTT form (CKKS,
   both modes): position c of row r holds the value at psi_r^(2 brev(c) + 1), so NTT(X^e)[c] = psi_r^(e (2 brev(c) + 1) mod 2N)
   with psi^(N + j) = -psi^j: the words of the forward transform of the one-hot row followed by the dyadic product. The
   powers come from a resident table of psi_r^j, j < N, per ciphertext prime (16 N bytes per prime, 512 KiB at N = 2^15),
   built on first use. An exponent >= 2N is reduced mod 2N by the kernel; the array is not scanned on the host.

   sealhip_evaluator_multiply_monomial: out[i] = X^(e_i) ct[i] - minus_one * ct[i] on both components, count size-2
     ciphertexts at level k in the scheme's form, e_i = exps_dev[i * exps_stride] (uint32, DEVICE). ct holds n_ct = 1
     ciphertext (shared by the batch) or n_ct = count. minus_one != 0 gives (X^e - 1) ct, the target of a blind-rotation step.
   sealhip_evaluator_blind_rotate: tv: n_tv size-2 ciphertexts, n_tv = 1 (shared) or count; exps_dev: count x (1 + n_steps)
     uint32 (DEVICE); rgsw_list[0 .. n_steps).
         acc_0[i] = X^(exps[i][0]) tv[i]
         acc_t[i] = acc_(t-1)[i] + ((X^(exps[i][t]) - 1) acc_(t-1)[i]) (x) rgsw_list[t-1],   t = 1 .. n_steps
         out[i]   = acc_(n_steps)[i]
     Where rgsw_list[t-1] encrypts a bit beta_t the phase of out[i] is X^(exps[i][0] + sum_t beta_t exps[i][t]) phase(tv) plus
     n_steps key-switch errors; nothing multiplies. The words are those of the step-by-step composition
     multiply_monomial(minus_one = 1) then sealhip_evaluator_external_product(target, base = acc). The accumulator lives in
     out from step 0 on; a step is one streaming launch (reads acc, writes the target into the arena) and one external
     product whose mod-down adds into acc in place. A batch that does not fit the arena is walked in chunks of items with
     the whole step loop inside a chunk; sealhip_debug_chunk_log ends with (count, items per chunk). No host read or
     synchronisation between steps; capturable after one call of the same shape. With a transparency sink: one flag per
     output, from the last step's mod-down, or from a read pass when n_steps == 0 (and for multiply_monomial).
   Checks of these two, in this order: NULL ctx, ct / tv, exps_dev, out, (n_steps > 0) the list and every entry -> E_POINTER;
   then, also on host-only contexts: k outside the ciphertext levels, n_ct / n_tv neither 1 nor count, BFV in PARITY mode, ct / tv
   or out not 16-byte aligned, exps_dev not 4-byte aligned, out overlapping ct / tv or exps -> E_INVALIDARG; then a host-only
   context -> COR_E_INVALIDOPERATION; then an rgsw that does not serve level k ("rgsw is not valid for encryption
   parameters") -> E_INVALIDARG; then count == 0 -> S_OK, nothing launched.

   sealhip_lwe_mod_switch: lwe_a[n_samples][1][N], lwe_b[n_samples][1] (DEVICE) are samples at level 1 (one prime q = q_0) as
     sealhip_evaluator_extract_lwe writes them at k = 1. With ms(x) = floor((2N x + floor(q / 2)) / q) mod 2N, exact in integers
     (a value that rounds to 2N wraps to 0), exps_out (DEVICE) receives blind_rotate's layout, n_samples x (1 + n_steps):
         exps[i][0] = -(ms(b_i) + b_offset) mod 2N
         binary secret  (ternary == 0): n_steps = N,  exps[i][1 + j] = -ms(a_ij) mod 2N
         ternary secret (ternary != 0): n_steps = 2N, exps[i][1 + 2j] = -ms(a_ij) mod 2N against RGSW([s_j = 1]) and
                                                      exps[i][2 + 2j] = +ms(a_ij)        against RGSW([s_j = -1])
     so that blind_rotate's out = X^(-phi~) tv with phi~ = ms(b) + b_offset + sum_j ms(a_j) s_j, and
     |phi~ - b_offset - 2N phi / q| <= (1 + ||s||_1) / 2. The constant coefficient of X^(-phi~) tv is tv[phi~] for phi~ < N and
     -tv[phi~ - N] above. Checks: NULL ctx, lwe_a, lwe_b, exps_out -> E_POINTER; then, also on host-only contexts: a context
     whose level 1 is not a ciphertext level, lwe_a not 16-byte, lwe_b not 8-byte or exps_out not 4-byte aligned, exps_out
     overlapping an input -> E_INVALIDARG; then a host-only context -> COR_E_INVALIDOPERATION; n_samples == 0 -> S_OK.
   sealhip_generate_blind_rotation_keys: out receives n_steps = n_lwe (binary) or 2 n_lwe (ternary) owned sealhip_rgsw, the
     encryptions of the constant polynomials [s_j = 1] (at 2j for ternary, with [s_j = -1] at 2j + 1) of lwe_secret_dev
     (n_lwe int32, DEVICE, values in {-1, 0, 1}). A kernel writes the indicators as m_coeff and the code behind
     sealhip_generate_rgsw does the rest: every word is that entry's for the indicator messages with the same samples
     (seeds_host: n_steps x 2 x digits x 8 words, HOST; noise: n_steps x 2 x digits x N int32, DEVICE). The indicators are
     erased in stream order. Checks and behaviour as sealhip_generate_rgsw with n = n_steps. */
long sealhip_evaluator_multiply_monomial(sealhip_context *ctx, uint32_t k, const uint64_t *ct, size_t n_ct, size_t count,
                                         const uint32_t *exps_dev, size_t exps_stride, int32_t minus_one, uint64_t *out);
long sealhip_lwe_mod_switch(sealhip_context *ctx, const uint64_t *lwe_a, const uint64_t *lwe_b, size_t n_samples,
                            int32_t ternary, uint32_t b_offset, uint32_t *exps_out);
long sealhip_generate_blind_rotation_keys(sealhip_context *ctx, const uint64_t *sk_ntt, const int32_t *lwe_secret_dev,
                                          uint32_t n_lwe, int32_t ternary, uint32_t level, const uint64_t *seeds_host,
                                          const int32_t *noise, sealhip_rgsw **out);
long sealhip_evaluator_blind_rotate(sealhip_context *ctx, uint32_t k, const uint64_t *tv, size_t n_tv, size_t count,
                                    const uint32_t *exps_dev, uint32_t n_steps, const sealhip_rgsw *const *rgsw_list,
                                    uint64_t *out);
/* stream-ordered hipMemsetAsync(dptr, 0, bytes) on the calling thread's lane: erases scratch that held secret samples
   before it goes back to a pool (the reference's clear_on_destruction pool, util/rlwe.cpp:141). Does not synchronise. */
long sealhip_memset_zero(sealhip_context *ctx, void *dptr, size_t bytes);
/* is_data_valid_for (valcheck.cpp:284-317) on device-resident ciphertexts: valid[i] = 1 iff every coefficient of
   ciphertext i is below its row's prime (what an ingesting service checks before evaluating untrusted input). */
long sealhip_is_data_valid_for(sealhip_context *ctx, uint32_t k, const uint64_t *ct, uint32_t size, size_t count,
                               uint8_t *valid);

#ifdef __cplusplus
}
#endif
#endif /* SEALHIP_H */
