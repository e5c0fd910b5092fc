// poly.hip -- coefficient-wise kernels (native/src/seal/util/polyarithsmallmod.{h,cpp}) and the
// Galois automorphisms (native/src/seal/util/galois.cpp) over batches of RNS rows.
// All of these are pure HBM streaming: 16-byte loads/stores, two coefficients per lane.
#include "engine.hpp"
#include "instance_dispatch.hpp"

#include <algorithm>

namespace sealhip
{
    namespace
    {
        template <int OP>
        __device__ __forceinline__ u64 apply_op(u64 a, u64 b, u64 scalar, const PrimeDev &P)
        {
            if (OP == 0)
                return mul_mod(a, b, P.p, P.cr0, P.cr1); // dyadic_product_coeffmod, polyarithsmallmod.cpp:63-117
            if (OP == 1)
                return add_mod(a, b, P.p);
            if (OP == 2)
                return sub_mod(a, b, P.p);
            if (OP == 3)
                return neg_mod(a, P.p);
            if (OP == 5)
                return barrett_reduce_63(a, P.p, P.cr1); // modulo_poly_coeffs_63, polyarithsmallmod.h:98-120
            return mul_mod(a, scalar, P.p, P.cr0, P.cr1); // multiply_poly_scalar_coeffmod, :15-61
        }

        template <int OP>
        __global__ __launch_bounds__(kThreads) void poly_op_kernel(const u64 *__restrict__ a,
                                                                   const u64 *__restrict__ b, u64 scalar,
                                                                   u64 *__restrict__ r,
                                                                   const PrimeDev *__restrict__ primes, RowMap map,
                                                                   int logn, std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs;
                 i += stride)
            {
                const std::size_t row = (2 * i) >> logn;
                const unsigned short pid = map.prime[row % map.rows];
                if (pid == kSkipRow)
                    continue;
                const PrimeDev &P = primes[pid];
                const ulonglong2 va = reinterpret_cast<const ulonglong2 *>(a)[i];
                ulonglong2 vb = va;
                if (OP == 0 || OP == 1 || OP == 2)
                    vb = reinterpret_cast<const ulonglong2 *>(b)[i];
                ulonglong2 out;
                out.x = apply_op<OP>(va.x, vb.x, scalar, P);
                out.y = apply_op<OP>(va.y, vb.y, scalar, P);
                reinterpret_cast<ulonglong2 *>(r)[i] = out;
            }
        }

        // out[I] = sum over i1 + i2 = I of a[i1] (.) b[i2], each term reduced (dyadic_product_coeffmod) and
        // accumulated with add_poly_coeffmod, exactly as evaluator.cpp:376-420 / :493-520 do.
        __global__ __launch_bounds__(kThreads) void tensor_product_kernel(
            const u64 *__restrict__ a, int sa, std::size_t a_stride, const u64 *__restrict__ b, int sb,
            std::size_t b_stride, u64 *__restrict__ out, std::size_t out_stride, const PrimeDev *__restrict__ primes,
            RowMap map, int logn, std::size_t npairs_per_item, std::size_t count, unsigned *__restrict__ tflags, int square)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t poly_words = static_cast<std::size_t>(map.rows) << logn;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t item = i / npairs_per_item;
                const std::size_t off = 2 * (i - item * npairs_per_item); // word offset inside one polynomial
                const PrimeDev &P = primes[map.prime[off >> logn]];
                const u64 *pa = a + item * a_stride + off;
                const u64 *pb = b + item * b_stride + off;
                u64 *po = out + item * out_stride + off;
                if (square)
                {
                    // Evaluator::square on a size-2 operand (bfv_square evaluator.cpp:644-657, ckks_square :752-760): x_0^2, x_0 x_1
                    // added to itself, x_1^2 -- two polynomials read instead of four, three products instead of four
                    const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(pa);
                    const ulonglong2 a1 = *reinterpret_cast<const ulonglong2 *>(pa + poly_words);
                    ulonglong2 c0, c1, c2;
                    c0.x = mul_mod(a0.x, a0.x, P.p, P.cr0, P.cr1);
                    c0.y = mul_mod(a0.y, a0.y, P.p, P.cr0, P.cr1);
                    c1.x = mul_mod(a0.x, a1.x, P.p, P.cr0, P.cr1);
                    c1.y = mul_mod(a0.y, a1.y, P.p, P.cr0, P.cr1);
                    c1.x = add_mod(c1.x, c1.x, P.p);
                    c1.y = add_mod(c1.y, c1.y, P.p);
                    c2.x = mul_mod(a1.x, a1.x, P.p, P.cr0, P.cr1);
                    c2.y = mul_mod(a1.y, a1.y, P.p, P.cr0, P.cr1);
                    *reinterpret_cast<ulonglong2 *>(po) = c0;
                    *reinterpret_cast<ulonglong2 *>(po + poly_words) = c1;
                    *reinterpret_cast<ulonglong2 *>(po + 2 * poly_words) = c2;
                    note_nonzero(tflags, item, c1.x | c1.y | c2.x | c2.y);
                    continue;
                }
                if (sa == 2 && sb == 2)
                {
                    const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(pa);
                    const ulonglong2 a1 = *reinterpret_cast<const ulonglong2 *>(pa + poly_words);
                    const ulonglong2 b0 = *reinterpret_cast<const ulonglong2 *>(pb);
                    const ulonglong2 b1 = *reinterpret_cast<const ulonglong2 *>(pb + poly_words);
                    ulonglong2 c0, c1, c2;
                    c0.x = mul_mod(a0.x, b0.x, P.p, P.cr0, P.cr1);
                    c0.y = mul_mod(a0.y, b0.y, P.p, P.cr0, P.cr1);
                    c1.x = add_mod(mul_mod(a1.x, b0.x, P.p, P.cr0, P.cr1), mul_mod(a0.x, b1.x, P.p, P.cr0, P.cr1), P.p);
                    c1.y = add_mod(mul_mod(a1.y, b0.y, P.p, P.cr0, P.cr1), mul_mod(a0.y, b1.y, P.p, P.cr0, P.cr1), P.p);
                    c2.x = mul_mod(a1.x, b1.x, P.p, P.cr0, P.cr1);
                    c2.y = mul_mod(a1.y, b1.y, P.p, P.cr0, P.cr1);
                    *reinterpret_cast<ulonglong2 *>(po) = c0;
                    *reinterpret_cast<ulonglong2 *>(po + poly_words) = c1;
                    *reinterpret_cast<ulonglong2 *>(po + 2 * poly_words) = c2;
                    note_nonzero(tflags, item, c1.x | c1.y | c2.x | c2.y);
                    continue;
                }
                const int dest = sa + sb - 1;
                for (int I = 0; I < dest; I++)
                {
                    const int last1 = I < sa - 1 ? I : sa - 1;
                    const int first2 = I < sb - 1 ? I : sb - 1;
                    const int first1 = I - first2;
                    ulonglong2 acc;
                    acc.x = 0;
                    acc.y = 0;
                    for (int i1 = first1; i1 <= last1; i1++)
                    {
                        const int i2 = I - i1;
                        const ulonglong2 va = *reinterpret_cast<const ulonglong2 *>(pa + i1 * poly_words);
                        const ulonglong2 vb = *reinterpret_cast<const ulonglong2 *>(pb + i2 * poly_words);
                        acc.x = add_mod(mul_mod(va.x, vb.x, P.p, P.cr0, P.cr1), acc.x, P.p);
                        acc.y = add_mod(mul_mod(va.y, vb.y, P.p, P.cr0, P.cr1), acc.y, P.p);
                    }
                    *reinterpret_cast<ulonglong2 *>(po + I * poly_words) = acc;
                    if (I >= 1)
                        note_nonzero(tflags, item, acc.x | acc.y);
                }
            }
        }

        // Ciphertext inner product: out = sum over the group's terms of the (2,2) tensor product
        // a_t (x) b_t, one lane per coefficient pair of one row of one item, addressed as in tensor_product_kernel. The three
        // sums c_0 = a_0 b_0, c_1 = a_1 b_0 + a_0 b_1, c_2 = a_1 b_1 are plain 128-bit integers (ntt_bounds.hpp section 8: at
        // most kDotGroup terms of canonical operands cannot wrap) that are reduced ONCE per output word; the canonical residue
        // is that of the composition of dyadic products and modular additions. The next term's loads are issued before the
        // current term is accumulated. REDUCE: the operands are any 64-bit words (lazily transformed rows) and are brought to
        // the canonical residue as they are loaded. add_partial: the canonical sums of the groups before this one are added in.
        struct DotLoad
        {
            ulonglong2 a0, a1, b0, b1;
        };
        __device__ __forceinline__ DotLoad dot_load(const u64 *pa, const u64 *pb, std::size_t poly_words)
        {
            DotLoad v;
            v.a0 = *reinterpret_cast<const ulonglong2 *>(pa);
            v.a1 = *reinterpret_cast<const ulonglong2 *>(pa + poly_words);
            v.b0 = *reinterpret_cast<const ulonglong2 *>(pb);
            v.b1 = *reinterpret_cast<const ulonglong2 *>(pb + poly_words);
            return v;
        }
        __device__ __forceinline__ u64 dot_canonical(u64 x, u64 p, u64 cr1)
        {
            const u64 r = barrett_lazy(x, cr1, p); // cr1 = floor(2^64 / p): [0, 2p) for every 64-bit x
            return r >= p ? r - p : r;
        }
        __device__ __forceinline__ void dot_add_word(u64 &lo, u64 &hi, u64 w)
        {
            const u64 nl = lo + w;
            hi += nl < lo;
            lo = nl;
        }
        template <bool REDUCE>
        __global__ __launch_bounds__(kThreads) void tensor_dot_kernel(DotTerms terms, std::size_t a_stride, std::size_t b_stride,
                                                                      u64 *out01, std::size_t out01_stride,
                                                                      u64 *out2, std::size_t out2_stride,
                                                                      const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                      std::size_t npairs_per_item, std::size_t count,
                                                                      unsigned *__restrict__ tflags, int add_partial)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t poly_words = static_cast<std::size_t>(map.rows) << logn;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t item = i / npairs_per_item;
                const std::size_t off = 2 * (i - item * npairs_per_item); // word offset inside one polynomial
                const unsigned short pid = map.prime[off >> logn];
                if (pid == kSkipRow)
                    continue;
                const u64 p = primes[pid].p, cr0 = primes[pid].cr0, cr1 = primes[pid].cr1;
                const std::size_t ao = item * a_stride + off, bo = item * b_stride + off;
                u64 lo[3][2] = {}, hi[3][2] = {};
                DotLoad next = dot_load(terms.a[0] + ao, terms.b[0] + bo, poly_words);
                for (int t = 0; t < terms.n; t++)
                {
                    DotLoad v = next;
                    if (t + 1 < terms.n)
                        next = dot_load(terms.a[t + 1] + ao, terms.b[t + 1] + bo, poly_words);
                    if (REDUCE)
                    {
                        v.a0.x = dot_canonical(v.a0.x, p, cr1), v.a0.y = dot_canonical(v.a0.y, p, cr1);
                        v.a1.x = dot_canonical(v.a1.x, p, cr1), v.a1.y = dot_canonical(v.a1.y, p, cr1);
                        v.b0.x = dot_canonical(v.b0.x, p, cr1), v.b0.y = dot_canonical(v.b0.y, p, cr1);
                        v.b1.x = dot_canonical(v.b1.x, p, cr1), v.b1.y = dot_canonical(v.b1.y, p, cr1);
                    }
                    mac128(lo[0][0], hi[0][0], v.a0.x, v.b0.x);
                    mac128(lo[0][1], hi[0][1], v.a0.y, v.b0.y);
                    mac128(lo[1][0], hi[1][0], v.a1.x, v.b0.x);
                    mac128(lo[1][1], hi[1][1], v.a1.y, v.b0.y);
                    mac128(lo[1][0], hi[1][0], v.a0.x, v.b1.x);
                    mac128(lo[1][1], hi[1][1], v.a0.y, v.b1.y);
                    mac128(lo[2][0], hi[2][0], v.a1.x, v.b1.x);
                    mac128(lo[2][1], hi[2][1], v.a1.y, v.b1.y);
                }
                u64 *po0 = out01 + item * out01_stride + off, *po2 = out2 + item * out2_stride + off;
                if (add_partial)
                {
                    const ulonglong2 q0 = *reinterpret_cast<const ulonglong2 *>(po0);
                    const ulonglong2 q1 = *reinterpret_cast<const ulonglong2 *>(po0 + poly_words);
                    const ulonglong2 q2 = *reinterpret_cast<const ulonglong2 *>(po2);
                    dot_add_word(lo[0][0], hi[0][0], q0.x), dot_add_word(lo[0][1], hi[0][1], q0.y);
                    dot_add_word(lo[1][0], hi[1][0], q1.x), dot_add_word(lo[1][1], hi[1][1], q1.y);
                    dot_add_word(lo[2][0], hi[2][0], q2.x), dot_add_word(lo[2][1], hi[2][1], q2.y);
                }
                ulonglong2 c0, c1, c2;
                c0.x = barrett_reduce_128(lo[0][0], hi[0][0], p, cr0, cr1);
                c0.y = barrett_reduce_128(lo[0][1], hi[0][1], p, cr0, cr1);
                c1.x = barrett_reduce_128(lo[1][0], hi[1][0], p, cr0, cr1);
                c1.y = barrett_reduce_128(lo[1][1], hi[1][1], p, cr0, cr1);
                c2.x = barrett_reduce_128(lo[2][0], hi[2][0], p, cr0, cr1);
                c2.y = barrett_reduce_128(lo[2][1], hi[2][1], p, cr0, cr1);
                *reinterpret_cast<ulonglong2 *>(po0) = c0;
                *reinterpret_cast<ulonglong2 *>(po0 + poly_words) = c1;
                *reinterpret_cast<ulonglong2 *>(po2) = c2;
                note_nonzero(tflags, item, c1.x | c1.y | c2.x | c2.y);
            }
        }

        // Linear combinations of ciphertexts: out_s = sum over the group's terms of w[s][t] * x_t for the
        // S sums of a tile, one lane per coefficient pair of one row of one polynomial of one item. Each operand pair is loaded
        // ONCE and accumulated into every sum as plain 128-bit integers (ntt_bounds.hpp lincomb_group_admits: a group of
        // canonical operands and weights, the partial sum and the constant cannot wrap); every output word is reduced once,
        // so it is the canonical residue of the composition of scalar products and modular additions. The next term's loads
        // are issued before the current term is accumulated. The weights of a row are the same for every lane of a block that
        // does not straddle rows: the kernel then derives the row from the block's first pair, which keeps the row, the prime's
        // constants and the weights in scalar registers (lincomb_lane is instantiated once per case).
        template <int S>
        __device__ __forceinline__ void lincomb_lane(const LinTerms &terms, std::size_t xo, const u64 *__restrict__ wr, int k,
                                                     std::size_t w_sum_stride, const u64 *__restrict__ kr, bool k_x, bool k_y,
                                                     u64 p, u64 cr0, u64 cr1, u64 *po, std::size_t out_sum_stride, int add_partial,
                                                     unsigned *tflags, std::size_t flag_sum_stride, std::size_t item)
        {
            u64 lo[S][2] = {}, hi[S][2] = {};
            ulonglong2 next = *reinterpret_cast<const ulonglong2 *>(terms.x[0] + xo);
            for (int t = 0; t < terms.n; t++)
            {
                const ulonglong2 v = next;
                if (t + 1 < terms.n)
                    next = *reinterpret_cast<const ulonglong2 *>(terms.x[t + 1] + xo);
                const u64 *wt = wr + static_cast<std::size_t>(t) * k;
#pragma unroll
                for (int s = 0; s < S; s++)
                {
                    const u64 ws = wt[s * w_sum_stride];
                    mac128(lo[s][0], hi[s][0], v.x, ws);
                    mac128(lo[s][1], hi[s][1], v.y, ws);
                }
            }
#pragma unroll
            for (int s = 0; s < S; s++)
            {
                u64 *ps = po + s * out_sum_stride;
                if (add_partial)
                {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(ps);
                    dot_add_word(lo[s][0], hi[s][0], q.x), dot_add_word(lo[s][1], hi[s][1], q.y);
                }
                if (kr != nullptr)
                {
                    const u64 kv = kr[static_cast<std::size_t>(s) * k];
                    dot_add_word(lo[s][0], hi[s][0], k_x ? kv : 0), dot_add_word(lo[s][1], hi[s][1], k_y ? kv : 0);
                }
                ulonglong2 c;
                c.x = barrett_reduce_128(lo[s][0], hi[s][0], p, cr0, cr1);
                c.y = barrett_reduce_128(lo[s][1], hi[s][1], p, cr0, cr1);
                *reinterpret_cast<ulonglong2 *>(ps) = c;
                if (tflags != nullptr)
                    note_nonzero(tflags + s * flag_sum_stride, item, c.x | c.y);
            }
        }
        template <int S>
        __global__ __launch_bounds__(kThreads) void lincomb_kernel(LinTerms terms, std::size_t x_stride, const u64 *__restrict__ w,
                                                                   std::size_t w_sum_stride, const u64 *__restrict__ constant,
                                                                   int const_mode, u64 *out, std::size_t out_sum_stride,
                                                                   const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                   std::size_t npairs_per_item, std::size_t count,
                                                                   unsigned *tflags, std::size_t flag_sum_stride, int add_partial)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            const int k = map.rows;
            // a row is 2^(logn - 1) pairs: from kThreads pairs per row on, a block covers pairs of ONE row of one item
            const bool block_in_row = (static_cast<std::size_t>(1) << logn) >= 2 * static_cast<std::size_t>(kThreads);
            for (std::size_t base = blockIdx.x * static_cast<std::size_t>(blockDim.x); base < total; base += stride)
            {
                const std::size_t i = base + threadIdx.x;
                if (i >= total)
                    continue;
                if (block_in_row)
                {
                    const std::size_t item = base / npairs_per_item; // (uniform: what the block's first pair says)
                    const std::size_t row = (2 * (base - item * npairs_per_item)) >> logn;
                    const int r = static_cast<int>(row % k);
                    const bool poly0 = row < static_cast<std::size_t>(k);
                    const unsigned short pid = map.prime[r];
                    if (pid == kSkipRow)
                        continue;
                    const std::size_t off = 2 * (i - item * npairs_per_item);
                    const bool k_x = poly0 && (const_mode == 2 || (off & nmask) == 0), k_y = poly0 && const_mode == 2;
                    lincomb_lane<S>(terms, item * x_stride + off, w + r, k, w_sum_stride,
                                    constant != nullptr && poly0 ? constant + r : nullptr, k_x, k_y, primes[pid].p, primes[pid].cr0,
                                    primes[pid].cr1, out + item * x_stride + off, out_sum_stride, add_partial,
                                    poly0 ? nullptr : tflags, flag_sum_stride, item);
                }
                else
                {
                    const std::size_t item = i / npairs_per_item;
                    const std::size_t off = 2 * (i - item * npairs_per_item);
                    const std::size_t row = off >> logn;
                    const int r = static_cast<int>(row % k);
                    const bool poly0 = row < static_cast<std::size_t>(k);
                    const unsigned short pid = map.prime[r];
                    if (pid == kSkipRow)
                        continue;
                    const bool k_x = poly0 && (const_mode == 2 || (off & nmask) == 0), k_y = poly0 && const_mode == 2;
                    lincomb_lane<S>(terms, item * x_stride + off, w + r, k, w_sum_stride,
                                    constant != nullptr && poly0 ? constant + r : nullptr, k_x, k_y, primes[pid].p, primes[pid].cr0,
                                    primes[pid].cr1, out + item * x_stride + off, out_sum_stride, add_partial,
                                    poly0 ? nullptr : tflags, flag_sum_stride, item);
                }
            }
        }

        // Sums of ciphertexts against rows of plaintexts: out_s = sum over the group's terms of
        // x_t (.) P[s][t] for the S sums of a tile, everything in NTT form, so the weight of a word is the plaintext's word at
        // the same row and slot. The shape is lincomb_lane's: each operand pair is loaded ONCE per tile and accumulated into
        // every sum as plain 128-bit integers (lincomb_group_admits covers it: the same products and the partial sum, no
        // constant), one reduction per output word, the next term's operand load issued before the current term is
        // accumulated. Term t of item c is at x + c * item_stride + t * term_stride, plaintext (s, t) at
        // pl + s * plain_sum_stride + t * plain_words.
        template <int S>
        __device__ __forceinline__ void dot_plain_lane(const u64 *__restrict__ x, std::size_t term_stride, int n,
                                                       const u64 *__restrict__ pl, std::size_t plain_words,
                                                       std::size_t plain_sum_stride, u64 p, u64 cr0, u64 cr1, u64 *po,
                                                       std::size_t out_sum_stride, int add_partial, unsigned *tflags,
                                                       std::size_t flag_sum_stride, std::size_t item)
        {
            u64 lo[S][2] = {}, hi[S][2] = {};
            ulonglong2 next = *reinterpret_cast<const ulonglong2 *>(x);
            for (int t = 0; t < n; t++)
            {
                const ulonglong2 v = next;
                if (t + 1 < n)
                    next = *reinterpret_cast<const ulonglong2 *>(x + static_cast<std::size_t>(t + 1) * term_stride);
                const u64 *pt = pl + static_cast<std::size_t>(t) * plain_words;
#pragma unroll
                for (int s = 0; s < S; s++)
                {
                    const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(pt + s * plain_sum_stride);
                    mac128(lo[s][0], hi[s][0], v.x, w.x);
                    mac128(lo[s][1], hi[s][1], v.y, w.y);
                }
            }
#pragma unroll
            for (int s = 0; s < S; s++)
            {
                u64 *ps = po + s * out_sum_stride;
                if (add_partial)
                {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(ps);
                    dot_add_word(lo[s][0], hi[s][0], q.x), dot_add_word(lo[s][1], hi[s][1], q.y);
                }
                ulonglong2 c;
                c.x = barrett_reduce_128(lo[s][0], hi[s][0], p, cr0, cr1);
                c.y = barrett_reduce_128(lo[s][1], hi[s][1], p, cr0, cr1);
                *reinterpret_cast<ulonglong2 *>(ps) = c;
                if (tflags != nullptr)
                    note_nonzero(tflags + s * flag_sum_stride, item, c.x | c.y);
            }
        }
        // One lane per coefficient pair of one row of one polynomial of one item; as in lincomb_kernel, a block that cannot
        // straddle rows (N >= 2 kThreads) derives the row from its first pair, which keeps the prime's constants scalar.
        template <int S>
        __global__ __launch_bounds__(kThreads) void dot_plain_kernel(const u64 *__restrict__ x, std::size_t term_stride,
                                                                     std::size_t item_stride, int n, const u64 *__restrict__ plain,
                                                                     std::size_t plain_sum_stride, u64 *out,
                                                                     std::size_t out_sum_stride, const PrimeDev *__restrict__ primes,
                                                                     RowMap map, int logn, std::size_t npairs_per_item,
                                                                     std::size_t count, unsigned *tflags,
                                                                     std::size_t flag_sum_stride, int add_partial)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            const std::size_t k = static_cast<std::size_t>(map.rows);
            const bool block_in_row = (static_cast<std::size_t>(1) << logn) >= 2 * static_cast<std::size_t>(kThreads);
            for (std::size_t base = blockIdx.x * static_cast<std::size_t>(blockDim.x); base < total; base += stride)
            {
                const std::size_t i = base + threadIdx.x;
                if (i >= total)
                    continue;
                // (uniform where the block lies in one row: what the block's first pair says)
                const std::size_t item = (block_in_row ? base : i) / npairs_per_item;
                const std::size_t row = (2 * ((block_in_row ? base : i) - item * npairs_per_item)) >> logn;
                const std::size_t r = row % k;
                const unsigned short pid = map.prime[r];
                const std::size_t off = 2 * (i - item * npairs_per_item); // word offset inside the ciphertext
                dot_plain_lane<S>(x + item * item_stride + off, term_stride, n, plain + (r << logn) + (off & nmask), k << logn,
                                  plain_sum_stride, primes[pid].p, primes[pid].cr0, primes[pid].cr1, out + item * term_stride + off,
                                  out_sum_stride, add_partial, row < k ? nullptr : tflags, flag_sum_stride, item);
            }
        }

        // The same sums over terms at their own level and size: a CKKS mod_switch_to_next only drops the
        // last row, so a term at level rows[t] >= k holds the level-k ciphertext in place at its own row stride, and a term of
        // size[t] polynomials is the size-`size` ciphertext whose further polynomials are zero. Term t's word for (item, j, r)
        // is at ((item * size[t] + j) * rows[t] + r) * N; a term with size[t] <= j contributes nothing to polynomial j. The
        // arithmetic per output word, the group, the partial sum and the flags are lincomb_lane's. Uniform (a block inside one
        // row): item, j and r are the block's, so the term's base and whether it takes part are scalar and the block skips its
        // load and its products together. Otherwise (N < 2 kThreads, a block straddles rows and polynomials) no lane branches:
        // a term that takes no part is read at polynomial 0 and multiplied by zero.
        template <int S, bool Uniform>
        __device__ __forceinline__ void lincomb_levels_lane(const LinLevelTerms &terms, std::size_t item, int j, int r,
                                                            std::size_t col, int logn, const u64 *__restrict__ wr, int k,
                                                            std::size_t w_sum_stride, const u64 *__restrict__ kr, bool k_x,
                                                            bool k_y, u64 p, u64 cr0, u64 cr1, u64 *po,
                                                            std::size_t out_sum_stride, int add_partial, unsigned *tflags,
                                                            std::size_t flag_sum_stride)
        {
            u64 lo[S][2] = {}, hi[S][2] = {};
            const auto word = [&](int t, bool live) {
                const std::size_t jt = Uniform || live ? static_cast<std::size_t>(j) : 0;
                const std::size_t row = (item * terms.size[t] + jt) * terms.rows[t] + static_cast<std::size_t>(r);
                return *reinterpret_cast<const ulonglong2 *>(terms.x[t] + (row << logn) + col);
            };
            bool live_next = j < static_cast<int>(terms.size[0]);
            ulonglong2 next = {};
            if (!Uniform || live_next)
                next = word(0, live_next);
            for (int t = 0; t < terms.n; t++)
            {
                const ulonglong2 v = next;
                const bool live = live_next;
                if (t + 1 < terms.n)
                {
                    live_next = j < static_cast<int>(terms.size[t + 1]);
                    if (!Uniform || live_next)
                        next = word(t + 1, live_next);
                }
                if (Uniform && !live)
                    continue;
                const u64 *wt = wr + static_cast<std::size_t>(t) * k;
#pragma unroll
                for (int s = 0; s < S; s++)
                {
                    const u64 ws = Uniform || live ? wt[s * w_sum_stride] : 0;
                    mac128(lo[s][0], hi[s][0], v.x, ws);
                    mac128(lo[s][1], hi[s][1], v.y, ws);
                }
            }
#pragma unroll
            for (int s = 0; s < S; s++)
            {
                u64 *ps = po + s * out_sum_stride;
                if (add_partial)
                {
                    const ulonglong2 q = *reinterpret_cast<const ulonglong2 *>(ps);
                    dot_add_word(lo[s][0], hi[s][0], q.x), dot_add_word(lo[s][1], hi[s][1], q.y);
                }
                if (kr != nullptr)
                {
                    const u64 kv = kr[static_cast<std::size_t>(s) * k];
                    dot_add_word(lo[s][0], hi[s][0], k_x ? kv : 0), dot_add_word(lo[s][1], hi[s][1], k_y ? kv : 0);
                }
                ulonglong2 c;
                c.x = barrett_reduce_128(lo[s][0], hi[s][0], p, cr0, cr1);
                c.y = barrett_reduce_128(lo[s][1], hi[s][1], p, cr0, cr1);
                *reinterpret_cast<ulonglong2 *>(ps) = c;
                if (tflags != nullptr)
                    note_nonzero(tflags + s * flag_sum_stride, item, c.x | c.y);
            }
        }
        template <int S>
        __global__ __launch_bounds__(kThreads) void lincomb_levels_kernel(LinLevelTerms terms, std::size_t out_stride,
                                                                          const u64 *__restrict__ w, std::size_t w_sum_stride,
                                                                          const u64 *__restrict__ constant, int const_mode,
                                                                          u64 *out, std::size_t out_sum_stride,
                                                                          const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                          std::size_t npairs_per_item, std::size_t count,
                                                                          unsigned *tflags, std::size_t flag_sum_stride,
                                                                          int add_partial)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            const int k = map.rows;
            // a row is 2^(logn - 1) pairs: from kThreads pairs per row on, a block covers pairs of ONE row of one item
            const bool block_in_row = (static_cast<std::size_t>(1) << logn) >= 2 * static_cast<std::size_t>(kThreads);
            for (std::size_t base = blockIdx.x * static_cast<std::size_t>(blockDim.x); base < total; base += stride)
            {
                const std::size_t i = base + threadIdx.x;
                if (i >= total)
                    continue;
                if (block_in_row)
                {
                    const std::size_t item = base / npairs_per_item; // (uniform: what the block's first pair says)
                    const std::size_t row = (2 * (base - item * npairs_per_item)) >> logn;
                    const int j = static_cast<int>(row / k), r = static_cast<int>(row % k);
                    const unsigned short pid = map.prime[r];
                    if (pid == kSkipRow)
                        continue;
                    const std::size_t off = 2 * (i - item * npairs_per_item);
                    const bool k_x = j == 0 && (const_mode == 2 || (off & nmask) == 0), k_y = j == 0 && const_mode == 2;
                    lincomb_levels_lane<S, true>(terms, item, j, r, off & nmask, logn, w + r, k, w_sum_stride,
                                                 constant != nullptr && j == 0 ? constant + r : nullptr, k_x, k_y, primes[pid].p,
                                                 primes[pid].cr0, primes[pid].cr1, out + item * out_stride + off, out_sum_stride,
                                                 add_partial, j == 0 ? nullptr : tflags, flag_sum_stride);
                }
                else
                {
                    const std::size_t item = i / npairs_per_item;
                    const std::size_t off = 2 * (i - item * npairs_per_item);
                    const std::size_t row = off >> logn;
                    const int j = static_cast<int>(row / k), r = static_cast<int>(row % k);
                    const unsigned short pid = map.prime[r];
                    if (pid == kSkipRow)
                        continue;
                    const bool k_x = j == 0 && (const_mode == 2 || (off & nmask) == 0), k_y = j == 0 && const_mode == 2;
                    lincomb_levels_lane<S, false>(terms, item, j, r, off & nmask, logn, w + r, k, w_sum_stride,
                                                  constant != nullptr && j == 0 ? constant + r : nullptr, k_x, k_y, primes[pid].p,
                                                  primes[pid].cr0, primes[pid].cr1, out + item * out_stride + off, out_sum_stride,
                                                  add_partial, j == 0 ? nullptr : tflags, flag_sum_stride);
                }
            }
        }

        // The tables of a polynomial's inner sums from its coefficients mod t (launch_poly_tables). One lane per (coefficient,
        // row): the weight is plain_lift_centered_kernel's word, the constant scaling_variant_kernel's at coefficient 0.
        constexpr int kPolyCoeffChunk = 64;
        struct PolyCoeffs
        {
            u64 c[kPolyCoeffChunk];
        };
        __global__ __launch_bounds__(kThreads) void poly_tables_kernel(PolyCoeffs cs, std::size_t first, int n, std::size_t ms,
                                                                       ScalingArgs sc, const PrimeDev *__restrict__ primes,
                                                                       u64 *__restrict__ w, u64 *__restrict__ constant)
        {
            const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
            if (i >= n * sc.k)
                return;
            const int r = i % sc.k;
            const u64 c = cs.c[i / sc.k];
            const std::size_t e = first + static_cast<std::size_t>(i / sc.k), j = e / ms, ii = e - j * ms;
            const PrimeDev &P = primes[r];
            if (ii == 0)
                constant[j * sc.k + r] = mul_add_mod(sc.div[r], c, scaling_variant_fix(sc, c), P.p, P.cr0, P.cr1);
            else
            {
                const u64 inc = P.p - barrett_reduce_63(sc.t, P.p, P.cr1);
                w[(j * (ms - 1) + ii - 1) * sc.k + r] = barrett_reduce_63(c + (c >= sc.threshold ? inc : 0), P.p, P.cr1);
            }
        }

        __global__ __launch_bounds__(kThreads) void copy_rows_kernel(const u64 *__restrict__ src,
                                                                     std::size_t src_stride, u64 *__restrict__ dst,
                                                                     std::size_t dst_stride,
                                                                     std::size_t pairs_per_poly, std::size_t npolys)
        {
            const std::size_t total = pairs_per_poly * npolys;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t poly = i / pairs_per_poly;
                const std::size_t off = 2 * (i - poly * pairs_per_poly);
                *reinterpret_cast<ulonglong2 *>(dst + poly * dst_stride + off) =
                    *reinterpret_cast<const ulonglong2 *>(src + poly * src_stride + off);
            }
        }

        // NTT form: out[i] = in[table[i]] (galois.cpp:188-214); coefficient form: out[(i*g) mod N] = +-in[i]
        // (galois.cpp:144-186). One coefficient per lane: the permutation defeats wider accesses on one side.
        __global__ __launch_bounds__(kThreads) void galois_kernel(const u64 *__restrict__ in, u64 *__restrict__ out,
                                                                  const PrimeDev *__restrict__ primes, RowMap map,
                                                                  int logn, std::size_t total, std::uint32_t elt,
                                                                  const std::uint32_t *__restrict__ table)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t row = i >> logn;
                const std::size_t c = i & nmask;
                if (table)
                {
                    out[i] = in[(row << logn) + table[c]];
                }
                else
                {
                    const u64 p = primes[map.prime[row % map.rows]].p;
                    const u64 raw = static_cast<u64>(c) * elt;
                    u64 v = in[i];
                    if ((raw >> logn) & 1)
                        v = neg_mod(v, p);
                    out[(row << logn) + (raw & nmask)] = v;
                }
            }
        }

        // Evaluator-level linear operations on batches of ciphertexts whose sizes may differ
        // (evaluator.cpp:65-232: negate_inplace, add_inplace, sub_inplace) and multiply_plain_ntt (:1605-1646).
        // OP 0: a + b (missing polynomials of the shorter operand count as absent: the tail of the longer one is
        // copied), OP 1: a - b (tail of b negated, :216-220), OP 2: -a, OP 3: a (.) plain, the plaintext rows
        // broadcast over the polynomials of the ciphertext.
        template <int OP>
        __global__ __launch_bounds__(kThreads) void ct_linear_kernel(const u64 *__restrict__ a, int sa,
                                                                     const u64 *__restrict__ b, int sb,
                                                                     std::size_t b_item_stride, u64 *__restrict__ out,
                                                                     const PrimeDev *__restrict__ primes, RowMap map,
                                                                     int logn, std::size_t pairs_per_poly,
                                                                     std::size_t count)
        {
            const int so = OP <= 1 ? (sa > sb ? sa : sb) : sa;
            const std::size_t total = pairs_per_poly * so * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t poly_words = pairs_per_poly * 2;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t item = i / (pairs_per_poly * so);
                const std::size_t rem = i - item * pairs_per_poly * so;
                const int j = static_cast<int>(rem / pairs_per_poly);
                const std::size_t off = 2 * (rem - j * pairs_per_poly);
                const PrimeDev &P = primes[map.prime[off >> logn]];
                ulonglong2 va, vb, r;
                va.x = va.y = vb.x = vb.y = 0;
                const bool has_a = j < sa;
                if (has_a)
                    va = *reinterpret_cast<const ulonglong2 *>(a + (item * sa + j) * poly_words + off);
                if (OP <= 1)
                {
                    const bool has_b = j < sb;
                    if (has_b)
                        vb = *reinterpret_cast<const ulonglong2 *>(b + (item * sb + j) * poly_words + off);
                    if (has_a && has_b)
                    {
                        r.x = OP == 0 ? add_mod(va.x, vb.x, P.p) : sub_mod(va.x, vb.x, P.p);
                        r.y = OP == 0 ? add_mod(va.y, vb.y, P.p) : sub_mod(va.y, vb.y, P.p);
                    }
                    else if (has_a)
                        r = va;
                    else
                    {
                        r.x = OP == 0 ? vb.x : neg_mod(vb.x, P.p);
                        r.y = OP == 0 ? vb.y : neg_mod(vb.y, P.p);
                    }
                }
                else if (OP == 2)
                {
                    r.x = neg_mod(va.x, P.p);
                    r.y = neg_mod(va.y, P.p);
                }
                else
                {
                    vb = *reinterpret_cast<const ulonglong2 *>(b + item * b_item_stride + off);
                    r.x = mul_mod(va.x, vb.x, P.p, P.cr0, P.cr1);
                    r.y = mul_mod(va.y, vb.y, P.p, P.cr0, P.cr1);
                }
                *reinterpret_cast<ulonglong2 *>(out + (item * so + j) * poly_words + off) = r;
            }
        }

        // Ciphertext::is_transparent (ciphertext.h:471-476): flag[item] != 0 iff some word of polynomials 1.. is non-zero
        __global__ __launch_bounds__(kThreads) void nonzero_tail_kernel(const u64 *__restrict__ ct,
                                                                        std::size_t item_words,
                                                                        std::size_t skip_words, std::size_t count,
                                                                        unsigned *__restrict__ flag)
        {
            const std::size_t tail_pairs = (item_words - skip_words) / 2;
            const std::size_t total = tail_pairs * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t item = i / tail_pairs;
                const std::size_t off = 2 * (i - item * tail_pairs);
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(ct + item * item_words + skip_words + off);
                if ((v.x | v.y) != 0 && flag[item] == 0)
                    flag[item] = 1; // benign race: every writer stores the same value
            }
        }

        // is_data_valid_for (valcheck.cpp:284-317): flag[item] != 0 iff some coefficient is not below its row's prime
        __global__ __launch_bounds__(kThreads) void out_of_range_kernel(const u64 *__restrict__ ct, std::size_t item_words,
                                                                        std::size_t count,
                                                                        const PrimeDev *__restrict__ primes, RowMap map,
                                                                        int logn, unsigned *__restrict__ flag)
        {
            const std::size_t item_pairs = item_words / 2;
            const std::size_t total = item_pairs * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t item = i / item_pairs;
                const std::size_t off = 2 * (i - item * item_pairs);
                const u64 p = primes[map.prime[(off >> logn) % map.rows]].p;
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(ct + item * item_words + off);
                if ((v.x >= p || v.y >= p) && flag[item] == 0)
                    flag[item] = 1; // benign race: every writer stores the same value
            }
        }

        // multiply_plain_normal's lift of a plaintext into the RNS base when every q_i > t (fast plain lift,
        // evaluator.cpp:1583-1592): temp_r[i] = plain[i] + (plain[i] >= threshold ? q_r - t : 0)
        __global__ __launch_bounds__(kThreads) void plain_lift_kernel(const u64 *__restrict__ plain,
                                                                      std::size_t plain_stride, u64 *__restrict__ out,
                                                                      const PrimeDev *__restrict__ primes, RowMap map,
                                                                      int logn, u64 t, u64 threshold,
                                                                      std::size_t nplains)
        {
            const std::size_t n = static_cast<std::size_t>(1) << logn;
            const std::size_t total = nplains * map.rows * n;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t c = i & (n - 1);
                const std::size_t row = i >> logn;
                const std::size_t item = row / map.rows;
                const u64 p = primes[map.prime[row % map.rows]].p;
                const u64 v = plain[item * plain_stride + c];
                out[i] = v + (v >= threshold ? p - t : 0);
            }
        }

        // transform_to_ntt(Plaintext)'s lift (evaluator.cpp:1682-1737). Both reference branches -- v + (q_r - t) for
        // v >= thr when every q_r > t, the multi-word v + (Q - t) decomposed otherwise -- give the canonical residue of
        // the centred value: out = (v - t [v >= thr]) mod q_r, formed as the canonical residue of
        // v + (q_r - t mod q_r) [v >= thr] < t + q_r < 2^62 (t < 2^61). Coefficients at or beyond coeff_count are zero and
        // are not read.
        __global__ __launch_bounds__(kThreads) void plain_lift_centered_kernel(const u64 *__restrict__ plain,
                                                                               std::size_t coeff_count, std::size_t plain_stride,
                                                                               u64 *__restrict__ out,
                                                                               const PrimeDev *__restrict__ primes, RowMap map,
                                                                               int logn, u64 t, u64 threshold, std::size_t nplains)
        {
            const std::size_t n = static_cast<std::size_t>(1) << logn;
            const std::size_t total = nplains * map.rows * n;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total;
                 i += stride)
            {
                const std::size_t c = i & (n - 1);
                const std::size_t row = i >> logn;
                const std::size_t item = row / map.rows;
                const PrimeDev &P = primes[map.prime[row % map.rows]];
                const u64 v = c < coeff_count ? plain[item * plain_stride + c] : 0;
                const u64 inc = P.p - barrett_reduce_63(t, P.p, P.cr1);
                out[i] = barrett_reduce_63(v + (v >= threshold ? inc : 0), P.p, P.cr1);
            }
        }

        // Decryptor::dot_product_ct_sk_array (decryptor.cpp:246-256, :265): out = sum_{i>=1} ct_i (.) s^i, each term
        // reduced (dyadic_product_coeffmod) and accumulated with add_poly_coeffmod; with add_c0 also + ct_0 (NTT-form
        // ciphertexts; coefficient-form ones add c_0 after the inverse NTT). ct polys 1.. may hold lazy NTT values.
        __global__ __launch_bounds__(kThreads) void dot_sk_kernel(const u64 *__restrict__ ct, int size,
                                                                  std::size_t ct_item_stride,
                                                                  const u64 *__restrict__ sk, std::size_t sk_power_stride,
                                                                  u64 *out,
                                                                  const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                  std::size_t pairs_per_poly, std::size_t count, int add_c0)
        {
            const std::size_t total = pairs_per_poly * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t poly_words = pairs_per_poly * 2;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t item = i / pairs_per_poly;
                const std::size_t off = 2 * (i - item * pairs_per_poly);
                const PrimeDev &P = primes[map.prime[off >> logn]];
                ulonglong2 acc;
                acc.x = acc.y = 0;
                if (add_c0 == 2)
                    acc = *reinterpret_cast<const ulonglong2 *>(out + item * poly_words + off);
                for (int j = 1; j < size; j++)
                {
                    const ulonglong2 c = *reinterpret_cast<const ulonglong2 *>(ct + item * ct_item_stride + j * poly_words + off);
                    const ulonglong2 s = *reinterpret_cast<const ulonglong2 *>(sk + (j - 1) * sk_power_stride + off);
                    acc.x = add_mod(acc.x, mul_mod(c.x, s.x, P.p, P.cr0, P.cr1), P.p);
                    acc.y = add_mod(acc.y, mul_mod(c.y, s.y, P.p, P.cr0, P.cr1), P.p);
                }
                if (add_c0)
                {
                    const ulonglong2 c0 = *reinterpret_cast<const ulonglong2 *>(ct + item * ct_item_stride + off);
                    acc.x = add_mod(acc.x, c0.x, P.p);
                    acc.y = add_mod(acc.y, c0.y, P.p);
                }
                *reinterpret_cast<ulonglong2 *>(out + item * poly_words + off) = acc;
            }
        }
    } // namespace

    hipError_t launch_poly_op(const Engine &e, PolyOp op, const u64 *a, const u64 *b, u64 scalar, u64 *r,
                              std::size_t nrows, const RowMap &map)
    {
        const std::size_t npairs = (nrows << e.logn) / 2;
        if (npairs == 0)
            return hipSuccess;
        const unsigned grid = grid_for(npairs);
        ProfScope prof(e, "poly_op", 0);
        switch (op)
        {
        case PolyOp::Dyadic:
            poly_op_kernel<0><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        case PolyOp::Add:
            poly_op_kernel<1><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        case PolyOp::Sub:
            poly_op_kernel<2><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        case PolyOp::Negate:
            poly_op_kernel<3><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        case PolyOp::Scalar:
            poly_op_kernel<4><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        case PolyOp::Mod63:
            poly_op_kernel<5><<<grid, kThreads, 0, e.lane().stream>>>(a, b, scalar, r, e.d_primes, map, e.logn, npairs);
            break;
        }
        return hipGetLastError();
    }

    hipError_t launch_tensor_product(const Engine &e, const u64 *a, int sa, std::size_t a_stride, const u64 *b, int sb,
                                     std::size_t b_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                     const RowMap &map, bool square)
    {
        if (square && (sa != 2 || sb != 2 || a != b))
            return hipErrorInvalidValue; // the square form is that of ONE size-2 operand
        const std::size_t pairs = (static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "tensor_product", 0);
        tensor_product_kernel<<<grid_for(pairs * count), kThreads, 0, e.lane().stream>>>(
            a, sa, a_stride, b, sb, b_stride, out, out_stride, e.d_primes, map, e.logn, pairs, count, e.lane().tsink_arm,
            square ? 1 : 0);
        return hipGetLastError();
    }

    hipError_t launch_tensor_dot(const Engine &e, const DotTerms &terms, std::size_t a_stride, std::size_t b_stride, u64 *out01,
                                 std::size_t out01_stride, u64 *out2, std::size_t out2_stride, std::size_t count,
                                 const RowMap &map, bool reduce_on_load, bool add_partial)
    {
        static_assert(bounds::dot_group_admits(kDotGroup, bounds::kDotAccOperandBits), "a group's sums fit 128 bits");
        if (terms.n < 1 || terms.n > kDotGroup || map.rows < 1 || map.rows > kMaxRows)
            return hipErrorInvalidValue;
        const std::size_t pairs = (static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "tensor_dot", 0);
        const unsigned grid = grid_for(pairs * count);
        if (reduce_on_load)
            tensor_dot_kernel<true><<<grid, kThreads, 0, e.lane().stream>>>(terms, a_stride, b_stride, out01, out01_stride, out2,
                                                                            out2_stride, e.d_primes, map, e.logn, pairs, count,
                                                                            e.lane().tsink_arm, add_partial ? 1 : 0);
        else
            tensor_dot_kernel<false><<<grid, kThreads, 0, e.lane().stream>>>(terms, a_stride, b_stride, out01, out01_stride, out2,
                                                                             out2_stride, e.d_primes, map, e.logn, pairs, count,
                                                                             e.lane().tsink_arm, add_partial ? 1 : 0);
        return hipGetLastError();
    }

    namespace
    {
        // The double-angle step's front: out = 2 a^2 + C as a size-3 ciphertext,
        //     o_0 = 2 a_0^2 + C_r,   o_1 = 4 a_0 a_1,   o_2 = 2 a_1^2      (mod the row's prime),
        // in ONE pass: 2 words read and 3 written per coefficient, where tensor_dot_kernel followed by lincomb_levels_kernel
        // moves 11. The operands are canonical and the primes at most 61 bits, so 4 a_0 a_1 < 2^124 and 2 a_0^2 + C_r < 2^124:
        // each output is one 128-bit integer reduced ONCE, hence the canonical residue -- the very word the two passes leave.
        // a[count][2][rows][N], out[count][3][rows][N]; one lane per coefficient pair; the constants travel in the arguments.
        struct SquareAffineConsts
        {
            u64 c[kMaxModuli];
        };
        __device__ __forceinline__ u64 square_affine_word(u64 x, u64 y, int shift, u64 c, u64 p, u64 cr0, u64 cr1)
        {
            u64 lo = x * y, hi = mulhi(x, y);
            hi = (hi << shift) | (lo >> (64 - shift));
            lo <<= shift;
            dot_add_word(lo, hi, c);
            return barrett_reduce_128(lo, hi, p, cr0, cr1);
        }
        __global__ __launch_bounds__(kThreads) void square_affine_kernel(const u64 *__restrict__ a, u64 *__restrict__ out,
                                                                         SquareAffineConsts consts,
                                                                         const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                         std::size_t npairs_per_item, std::size_t count)
        {
            const std::size_t total = npairs_per_item * count;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t poly_words = static_cast<std::size_t>(map.rows) << logn;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t item = i / npairs_per_item;
                const std::size_t off = 2 * (i - item * npairs_per_item); // word offset inside one polynomial
                const int row = static_cast<int>(off >> logn);
                const unsigned short pid = map.prime[row];
                const u64 p = primes[pid].p, cr0 = primes[pid].cr0, cr1 = primes[pid].cr1, c = consts.c[row];
                const u64 *pa = a + item * 2 * poly_words + off;
                const ulonglong2 a0 = *reinterpret_cast<const ulonglong2 *>(pa);
                const ulonglong2 a1 = *reinterpret_cast<const ulonglong2 *>(pa + poly_words);
                u64 *po = out + item * 3 * poly_words + off;
                store_stream2(po, square_affine_word(a0.x, a0.x, 1, c, p, cr0, cr1),
                              square_affine_word(a0.y, a0.y, 1, c, p, cr0, cr1));
                store_stream2(po + poly_words, square_affine_word(a0.x, a1.x, 2, 0, p, cr0, cr1),
                              square_affine_word(a0.y, a1.y, 2, 0, p, cr0, cr1));
                store_stream2(po + 2 * poly_words, square_affine_word(a1.x, a1.x, 1, 0, p, cr0, cr1),
                              square_affine_word(a1.y, a1.y, 1, 0, p, cr0, cr1));
            }
        }
    } // namespace

    hipError_t launch_square_affine(const Engine &e, const u64 *a, u64 *out, std::size_t count, const RowMap &map,
                                    const u64 *constant)
    {
        if (map.rows < 1 || map.rows > kMaxModuli)
            return hipErrorInvalidValue;
        const std::size_t pairs = (static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        SquareAffineConsts consts{};
        for (int r = 0; r < map.rows; r++)
        {
            if (map.prime[r] == kSkipRow)
                return hipErrorInvalidValue;
            consts.c[r] = constant[r];
        }
        ProfScope prof(e, "square_affine", 0);
        square_affine_kernel<<<grid_for(pairs * count), kThreads, 0, e.lane().stream>>>(a, out, consts, e.d_primes, map, e.logn,
                                                                                       pairs, count);
        return hipGetLastError();
    }

    hipError_t launch_lincomb(const Engine &e, const LinTerms &terms, int size, std::size_t x_stride, const u64 *w,
                              std::size_t w_sum_stride, const u64 *constant, int const_mode, u64 *out, std::size_t out_sum_stride,
                              int n_sums, std::size_t count, const RowMap &map, bool add_partial, std::size_t flag_sum_stride)
    {
        static_assert(bounds::lincomb_group_admits(kLinGroup, bounds::kDotAccOperandBits), "a group's sums fit 128 bits");
        if (terms.n < 1 || terms.n > kLinGroup || n_sums < 1 || n_sums > kLinTile || size < 1 || map.rows < 1 ||
            map.rows > kMaxRows || (constant && const_mode != 1 && const_mode != 2))
            return hipErrorInvalidValue;
        const std::size_t pairs = (static_cast<std::size_t>(size) * map.rows << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "lincomb", 0);
        const unsigned grid = grid_for(pairs * count);
        // (one instance per number of sums in a tile: n_sums was checked against the range above)
        dispatch_int<1, kLinTile>(n_sums, [&](auto s) {
            lincomb_kernel<decltype(s)::value><<<grid, kThreads, 0, e.lane().stream>>>(
                terms, x_stride, w, w_sum_stride, constant, const_mode, out, out_sum_stride, e.d_primes, map, e.logn, pairs, count,
                e.lane().tsink_arm, flag_sum_stride, add_partial ? 1 : 0);
        });
        return hipGetLastError();
    }

    hipError_t launch_dot_plain(const Engine &e, const u64 *x, int size, std::size_t item_stride, int n_terms, const u64 *plain,
                                std::size_t plain_sum_stride, u64 *out, std::size_t out_sum_stride, int n_sums, std::size_t count,
                                const RowMap &map, bool add_partial, std::size_t flag_sum_stride)
    {
        // the products and the partial sum of lincomb_kernel, without its constant: the same predicate admits the group
        static_assert(bounds::lincomb_group_admits(kLinGroup, bounds::kDotAccOperandBits), "a group's sums fit 128 bits");
        if (n_terms < 1 || n_terms > kLinGroup || n_sums < 1 || n_sums > kLinTile || size < 1 || map.rows < 1 ||
            map.rows > kMaxRows)
            return hipErrorInvalidValue;
        for (int r = 0; r < map.rows; r++)
            if (map.prime[r] == kSkipRow)
                return hipErrorInvalidValue;
        const std::size_t term_stride = static_cast<std::size_t>(size) * map.rows << e.logn;
        const std::size_t pairs = term_stride / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "dot_plain", 0);
        const unsigned grid = grid_for(pairs * count);
        dispatch_int<1, kLinTile>(n_sums, [&](auto s) {
            dot_plain_kernel<decltype(s)::value><<<grid, kThreads, 0, e.lane().stream>>>(
                x, term_stride, item_stride, n_terms, plain, plain_sum_stride, out, out_sum_stride, e.d_primes, map, e.logn, pairs,
                count, e.lane().tsink_arm, flag_sum_stride, add_partial ? 1 : 0);
        });
        return hipGetLastError();
    }

    hipError_t launch_lincomb_levels(const Engine &e, const LinLevelTerms &terms, int size, std::size_t out_stride, const u64 *w,
                                     std::size_t w_sum_stride, const u64 *constant, int const_mode, u64 *out,
                                     std::size_t out_sum_stride, int n_sums, std::size_t count, const RowMap &map,
                                     bool add_partial, std::size_t flag_sum_stride)
    {
        static_assert(bounds::lincomb_group_admits(kLinGroup, bounds::kDotAccOperandBits), "a group's sums fit 128 bits");
        if (terms.n < 1 || terms.n > kLinGroup || n_sums < 1 || n_sums > kLinLevelsTile || size < 1 || map.rows < 1 ||
            map.rows > kMaxRows || (constant && const_mode != 1 && const_mode != 2))
            return hipErrorInvalidValue;
        for (int t = 0; t < terms.n; t++) // (what keeps every load inside its term)
            if (terms.rows[t] < map.rows || terms.size[t] < 1 || terms.size[t] > size)
                return hipErrorInvalidValue;
        const std::size_t pairs = (static_cast<std::size_t>(size) * map.rows << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "lincomb_levels", 0);
        const unsigned grid = grid_for(pairs * count);
        // (a smaller tile instantiates fewer kernels: the range is the tile)
        dispatch_int<1, kLinLevelsTile>(n_sums, [&](auto s) {
            lincomb_levels_kernel<decltype(s)::value><<<grid, kThreads, 0, e.lane().stream>>>(
                terms, out_stride, w, w_sum_stride, constant, const_mode, out, out_sum_stride, e.d_primes, map, e.logn, pairs, count,
                e.lane().tsink_arm, flag_sum_stride, add_partial ? 1 : 0);
        });
        return hipGetLastError();
    }

    hipError_t launch_poly_tables(const Engine &e, int k, const u64 *coeffs, std::size_t n_coeffs, std::size_t ms, u64 *w,
                                  u64 *constant)
    {
        if (k < 1 || k > kMaxModuli || ms < 2)
            return hipErrorInvalidValue;
        ScalingArgs sc{};
        fill_scaling_args(e, k, sc);
        ProfScope prof(e, "poly_tables", 0);
        for (std::size_t first = 0; first < n_coeffs; first += kPolyCoeffChunk)
        {
            PolyCoeffs cs{};
            const int n = static_cast<int>(std::min<std::size_t>(kPolyCoeffChunk, n_coeffs - first));
            for (int i = 0; i < n; i++)
                cs.c[i] = coeffs[first + i];
            poly_tables_kernel<<<grid_for(static_cast<std::size_t>(n) * k), kThreads, 0, e.lane().stream>>>(cs, first, n, ms, sc,
                                                                                                            e.d_primes, w, constant);
        }
        return hipGetLastError();
    }

    namespace
    {
        struct RowValues
        {
            u64 v[kMaxModuli];
        };
        // dst[count][rows][N]: row r of every item filled with vals.v[r] (the single-value CKKS encodings, ckks.cpp:80-260)
        __global__ __launch_bounds__(kThreads) void fill_rows_kernel(u64 *__restrict__ dst, RowValues vals, int rows, int logn,
                                                                    std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs; i += stride)
            {
                const u64 v = vals.v[((2 * i) >> logn) % rows];
                ulonglong2 o;
                o.x = v;
                o.y = v;
                reinterpret_cast<ulonglong2 *>(dst)[i] = o;
            }
        }
    } // namespace

    hipError_t launch_fill_rows(const Engine &e, u64 *dst, const u64 *row_values, int rows, std::size_t count)
    {
        if (rows < 1 || rows > kMaxModuli)
            return hipErrorInvalidValue;
        const std::size_t npairs = (count * static_cast<std::size_t>(rows) << e.logn) / 2;
        if (!npairs)
            return hipSuccess;
        RowValues rv{};
        for (int r = 0; r < rows; r++)
            rv.v[r] = row_values[r];
        ProfScope prof(e, "fill_rows", 0);
        fill_rows_kernel<<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(dst, rv, rows, e.logn, npairs);
        return hipGetLastError();
    }

    namespace
    {
        struct PutWords
        {
            u64 v[kPutWords];
        };
        __global__ __launch_bounds__(kThreads) void put_words_kernel(u64 *__restrict__ dst, PutWords words, int n)
        {
            const int i = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
            if (i < n)
                dst[i] = words.v[i];
        }
    } // namespace

    hipError_t launch_put_words(const Engine &e, u64 *dst, const u64 *words, std::size_t n)
    {
        ProfScope prof(e, "put_words", 0);
        for (std::size_t first = 0; first < n; first += kPutWords)
        {
            PutWords pw{};
            const int m = static_cast<int>(std::min<std::size_t>(kPutWords, n - first));
            for (int i = 0; i < m; i++)
                pw.v[i] = words[first + i];
            put_words_kernel<<<grid_for(static_cast<std::size_t>(m)), kThreads, 0, e.lane().stream>>>(dst + first, pw, m);
        }
        return hipGetLastError();
    }

    hipError_t launch_copy_rows(const Engine &e, const u64 *src, std::size_t src_poly_stride, u64 *dst,
                                std::size_t dst_poly_stride, std::size_t npolys, int rows)
    {
        const std::size_t pairs = (static_cast<std::size_t>(rows) << e.logn) / 2;
        if (pairs * npolys == 0)
            return hipSuccess;
        ProfScope prof(e, "copy_rows", 0);
        copy_rows_kernel<<<grid_for(pairs * npolys), kThreads, 0, e.lane().stream>>>(src, src_poly_stride, dst,
                                                                             dst_poly_stride, pairs, npolys);
        return hipGetLastError();
    }

    hipError_t launch_galois(const Engine &e, const u64 *in, u64 *out, std::size_t nrows, const RowMap &map,
                             std::uint32_t elt, const std::uint32_t *table)
    {
        const std::size_t total = nrows << e.logn;
        if (total == 0)
            return hipSuccess;
        ProfScope prof(e, "galois", 0);
        galois_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(in, out, e.d_primes, map, e.logn, total, elt, table);
        return hipGetLastError();
    }
    hipError_t launch_ct_linear(const Engine &e, CtLinearOp op, const u64 *a, int sa, const u64 *b, int sb,
                                std::size_t b_item_stride, u64 *out, std::size_t count, const RowMap &map)
    {
        const std::size_t pairs = (static_cast<std::size_t>(map.rows) << e.logn) / 2;
        const int so = (op == CtLinearOp::Add || op == CtLinearOp::Sub) ? (sa > sb ? sa : sb) : sa;
        if (pairs * so * count == 0)
            return hipSuccess;
        ProfScope prof(e, "ct_linear", 0);
        const unsigned grid = grid_for(pairs * so * count);
        switch (op)
        {
        case CtLinearOp::Add:
            ct_linear_kernel<0><<<grid, kThreads, 0, e.lane().stream>>>(a, sa, b, sb, b_item_stride, out, e.d_primes, map, e.logn,
                                                                pairs, count);
            break;
        case CtLinearOp::Sub:
            ct_linear_kernel<1><<<grid, kThreads, 0, e.lane().stream>>>(a, sa, b, sb, b_item_stride, out, e.d_primes, map, e.logn,
                                                                pairs, count);
            break;
        case CtLinearOp::Negate:
            ct_linear_kernel<2><<<grid, kThreads, 0, e.lane().stream>>>(a, sa, b, sb, b_item_stride, out, e.d_primes, map, e.logn,
                                                                pairs, count);
            break;
        case CtLinearOp::MulPlain:
            ct_linear_kernel<3><<<grid, kThreads, 0, e.lane().stream>>>(a, sa, b, sb, b_item_stride, out, e.d_primes, map, e.logn,
                                                                pairs, count);
            break;
        }
        return hipGetLastError();
    }

    // flags[item] |= "some word of [data + item * item_stride, + words) is non-zero" (the read pass the fused kernels avoid)
    hipError_t launch_nonzero_words(const Engine &e, const u64 *data, std::size_t item_stride, std::size_t words,
                                    std::size_t count, unsigned *flags)
    {
        if (words == 0 || count == 0)
            return hipSuccess;
        if (words > item_stride)
            return hipErrorInvalidValue;
        ProfScope prof(e, "nonzero_tail", 0);
        // (item_words = stride, skip = stride - words, base shifted back so that the tail is [data, data + words))
        nonzero_tail_kernel<<<grid_for(words / 2 * count), kThreads, 0, e.lane().stream>>>(
            data - (item_stride - words), item_stride, item_stride - words, count, flags);
        return hipGetLastError();
    }

    hipError_t launch_nonzero_tail(const Engine &e, const u64 *ct, std::size_t item_words, std::size_t skip_words,
                                   std::size_t count, unsigned *flags)
    {
        if (item_words <= skip_words || count == 0)
            return hipSuccess;
        ProfScope prof(e, "nonzero_tail", 0);
        nonzero_tail_kernel<<<grid_for((item_words - skip_words) / 2 * count), kThreads, 0, e.lane().stream>>>(
            ct, item_words, skip_words, count, flags);
        return hipGetLastError();
    }

    hipError_t launch_out_of_range(const Engine &e, const u64 *ct, std::size_t item_words, std::size_t count,
                                   const RowMap &map, unsigned *flags)
    {
        if (item_words == 0 || count == 0)
            return hipSuccess;
        ProfScope prof(e, "out_of_range", 0);
        out_of_range_kernel<<<grid_for(item_words / 2 * count), kThreads, 0, e.lane().stream>>>(ct, item_words, count, e.d_primes,
                                                                                        map, e.logn, flags);
        return hipGetLastError();
    }

    hipError_t launch_plain_lift(const Engine &e, const u64 *plain, std::size_t plain_stride, u64 *out, std::size_t nplains,
                                 const RowMap &map, u64 t)
    {
        const std::size_t total = (nplains * map.rows) << e.logn;
        if (total == 0)
            return hipSuccess;
        ProfScope prof(e, "plain_lift", 0);
        plain_lift_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(plain, plain_stride, out, e.d_primes, map, e.logn, t,
                                                                    (t + 1) >> 1, nplains);
        return hipGetLastError();
    }
    hipError_t launch_plain_lift_centered(const Engine &e, const u64 *plain, std::size_t coeff_count, std::size_t plain_stride,
                                          u64 *out, std::size_t nplains, const RowMap &map, u64 t)
    {
        const std::size_t total = (nplains * map.rows) << e.logn;
        if (total == 0)
            return hipSuccess;
        ProfScope prof(e, "plain_lift_centered", 0);
        plain_lift_centered_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(plain, coeff_count, plain_stride, out,
                                                                                       e.d_primes, map, e.logn, t, (t + 1) >> 1,
                                                                                       nplains);
        return hipGetLastError();
    }
    hipError_t launch_dot_sk(const Engine &e, const u64 *ct, int size, std::size_t ct_item_stride, const u64 *sk_powers,
                             std::size_t sk_power_stride, u64 *out, std::size_t count, const RowMap &map, int add_c0)
    {
        const std::size_t pairs = (static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (pairs * count == 0)
            return hipSuccess;
        ProfScope prof(e, "dot_sk", 0);
        dot_sk_kernel<<<grid_for(pairs * count), kThreads, 0, e.lane().stream>>>(ct, size, ct_item_stride, sk_powers, sk_power_stride,
                                                                         out, e.d_primes, map, e.logn, pairs, count,
                                                                         add_c0);
        return hipGetLastError();
    }
} // namespace sealhip
