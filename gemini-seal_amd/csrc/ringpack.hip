// ringpack.hip -- ring packing: the LWE sample of one coefficient of a ciphertext, its embedding
// back into the ring, and the merge step of PackLWEs / the field trace (Chen, Dai, Kim, Song, "Efficient Homomorphic
// Conversion Between (Ring) LWE Ciphertexts", Alg. 2 and 3) fused around the key switch; and the other direction, the step
// of the oblivious expansion of one ciphertext into n (the Expand of Angel, Chen, Laine, Setty, "PIR
// with compressed queries and amortized query processing", Fig. 3), fused the same way. The fork has no such method.
// All of these are HBM streaming in the style of poly.hip: two coefficients per lane, every store 16 bytes wide and
// coalesced, every permutation (the reversed read of a sample, the monomial shift, the automorphism) on the load side.
#include "engine.hpp"
#include "instance_dispatch.hpp"

namespace sealhip
{
    namespace
    {
        // -x for i > j, x otherwise: the sign split of the negacyclic wrap; 0 stays 0 (neg_mod)
        __device__ __forceinline__ u64 neg_if(bool neg, u64 v, u64 p)
        {
            return neg ? neg_mod(v, p) : v;
        }

        // a[i] = c_1[j - i] for i <= j, -c_1[N + j - i] for i > j; b = c_0[j]: b + <a, s> = (c_0 + c_1 s)[j].
        // One lane per pair (i, i + 1) of one row of one sample; the lane of the pair i = 0 also stores the row's b.
        __global__ __launch_bounds__(kThreads) void lwe_extract_kernel(const u64 *__restrict__ ct, std::size_t ct_stride,
                                                                       const std::uint32_t *__restrict__ idx, std::size_t n_idx,
                                                                       u64 *__restrict__ lwe_a, u64 *__restrict__ lwe_b,
                                                                       const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                       std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            const std::size_t k = static_cast<std::size_t>(map.rows);
            for (std::size_t t = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; t < npairs; t += stride)
            {
                const std::size_t word = 2 * t;
                const std::size_t i = word & nmask;
                const std::size_t row = word >> logn; // (item * n_idx + sample) * k + r; below 2^32 (the launcher): 32-bit divisions
                const unsigned row32 = static_cast<unsigned>(row), k32 = static_cast<unsigned>(k);
                const unsigned n32 = static_cast<unsigned>(n_idx), ci = row32 / k32;
                const std::size_t r = row32 - ci * k32;
                const std::size_t item = ci / n32, sample = ci - static_cast<unsigned>(item) * n32;
                const u64 p = primes[map.prime[r]].p;
                const std::size_t j = idx[sample];
                const u64 *c0 = ct + item * ct_stride + (r << logn);
                const u64 *c1 = c0 + (k << logn);
                const u64 a0 = neg_if(i > j, c1[(j - i) & nmask], p);
                const u64 a1 = neg_if(i + 1 > j, c1[(j - i - 1) & nmask], p);
                store_stream2(lwe_a + word, a0, a1);
                if (i == 0)
                    lwe_b[row] = c0[j];
            }
        }

        struct PackWeights // w_r and its Shoup companion, per ciphertext row
        {
            u64 w[kMaxModuli], ws[kMaxModuli];
        };

        // The inverse map scaled by w_r: c_0 = w b at coefficient 0 (NTT_C0: at every slot, the transform of that constant),
        // c_1[0] = w a[0], c_1[N - i] = -w a[i]. Sample (item, j) of lwe_a[items][n][k][N] goes to out[jj][item][2][k][N]
        // (sample-major, so that both halves of every merge step are contiguous batches), where jj walks the samples
        // j0 .. j0 + c - 1 and then j_hi + j0 .. j_hi + j0 + c - 1: the two operands of c merges of the first step (the whole
        // item: j0 = 0, c = n). One lane per pair of one row of one ciphertext, both polynomials.
        template <bool NTT_C0>
        __global__ __launch_bounds__(kThreads) void lwe_embed_kernel(const u64 *__restrict__ lwe_a, const u64 *__restrict__ lwe_b,
                                                                     std::size_t n, std::size_t items, std::size_t j0, std::size_t c_grp,
                                                                     std::size_t j_hi, u64 *__restrict__ out,
                                                                     const PrimeDev *__restrict__ primes, RowMap map,
                                                                     PackWeights wt, int logn, std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            const std::size_t k = static_cast<std::size_t>(map.rows);
            for (std::size_t t = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; t < npairs; t += stride)
            {
                const std::size_t word = 2 * t;
                const std::size_t c = word & nmask;
                const std::size_t row = word >> logn; // (j * items + item) * k + r; below 2^32 (the launcher): 32-bit divisions
                const unsigned row32 = static_cast<unsigned>(row), k32 = static_cast<unsigned>(k);
                const unsigned items32 = static_cast<unsigned>(items), ci32 = row32 / k32, j32 = ci32 / items32;
                const std::size_t ci = ci32; // ciphertext of the output
                const std::size_t r = row32 - ci32 * k32, item = ci32 - j32 * items32;
                const std::size_t j = j32 < c_grp ? j0 + j32 : j_hi + j0 + (j32 - c_grp);
                const u64 p = primes[map.prime[r]].p;
                const u64 w = wt.w[r], ws = wt.ws[r];
                const std::size_t src_row = (item * n + j) * k + r;
                const u64 *a = lwe_a + (src_row << logn);
                const u64 x0 = c == 0 ? a[0] : neg_mod(a[(nmask + 1) - c], p);
                const u64 x1 = neg_mod(a[nmask - c], p);
                u64 *o0 = out + ((ci * 2 * k + r) << logn) + c;
                store_stream2(o0 + (k << logn), mulmod_shoup(x0, w, ws, p), mulmod_shoup(x1, w, ws, p));
                const u64 b = mulmod_shoup(lwe_b[src_row], w, ws, p);
                store_stream2(o0, (NTT_C0 || c == 0) ? b : 0, NTT_C0 ? b : 0);
            }
        }

        // (X^s B)[x] in coefficient form: B[x - s], with the sign of the wrap
        __device__ __forceinline__ u64 shifted(const u64 *__restrict__ b, std::size_t x, std::size_t s, std::size_t nmask, u64 p)
        {
            return neg_if(x < s, b[(x - s) & nmask], p);
        }

        // One merge step of the pack (HAS_ODD) or one step of the trace (!HAS_ODD: O absent, E - O = E), without the key
        // switch: with O = X^s B,
        //     out = ((E_0 + O_0) + sigma_g(E_0 - O_0), E_1 + O_1),    target = sigma_g(E_1 - O_1),
        // so that out + key_switch(target) is (E + O) + apply_galois(E - O, g). Ciphertext x of E, B and out is [2][k][N] at
        // x * 2kN words, target x is [k][N]. One lane per pair of output coefficients of one row of one ciphertext.
        // FORM 0, coefficient form: coefficient c of sigma_g(D) is +-D[c g^{-1} mod 2N] (ginv = g^{-1} mod 2N).
        // FORM 1, NTT form: O = M (.) B with M = NTT(X^s) as {word, Shoup companion} pairs, sigma_g(D)[c] = D[T[c]].
        template <int FORM, bool HAS_ODD>
        __global__ __launch_bounds__(kThreads) void pack_merge_kernel(const u64 *__restrict__ E, const u64 *__restrict__ B,
                                                                      u64 *__restrict__ out, u64 *__restrict__ target,
                                                                      const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                      std::size_t npairs, std::uint32_t shift, std::uint32_t ginv,
                                                                      const std::uint32_t *__restrict__ table,
                                                                      const ulonglong2 *__restrict__ mono)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const std::size_t k = static_cast<std::size_t>(map.rows);
            const std::size_t poly = k << logn;
            for (std::size_t t = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; t < npairs; t += stride)
            {
                const std::size_t word = 2 * t;
                const std::size_t c = word & nmask;
                const std::size_t row = word >> logn; // x * k + r; below 2^32 (the launcher): a 32-bit division
                const unsigned row32 = static_cast<unsigned>(row), x32 = row32 / static_cast<unsigned>(k);
                const std::size_t x = x32, r = row32 - x32 * static_cast<unsigned>(k);
                const unsigned short pid = map.prime[r];
                const u64 p = primes[pid].p;
                const u64 *e0 = E + x * 2 * poly + (r << logn), *e1 = e0 + poly;
                const u64 *b0 = HAS_ODD ? B + x * 2 * poly + (r << logn) : nullptr, *b1 = HAS_ODD ? b0 + poly : nullptr;
                const ulonglong2 ve0 = *reinterpret_cast<const ulonglong2 *>(e0 + c);
                const ulonglong2 ve1 = *reinterpret_cast<const ulonglong2 *>(e1 + c);
                const u64 s0[2] = { ve0.x, ve0.y }, s1[2] = { ve1.x, ve1.y };
                u64 o0[2], o1[2], tg[2];
                if (FORM == 0)
                {
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t cc = c + h;
                        const std::size_t u = (cc * ginv) & (2 * N - 1), i = u & nmask;
                        u64 d0 = e0[i], d1 = e1[i];
                        o0[h] = s0[h];
                        o1[h] = s1[h];
                        if (HAS_ODD)
                        {
                            d0 = sub_mod(d0, shifted(b0, i, shift, nmask, p), p);
                            d1 = sub_mod(d1, shifted(b1, i, shift, nmask, p), p);
                            o0[h] = add_mod(o0[h], shifted(b0, cc, shift, nmask, p), p);
                            o1[h] = add_mod(o1[h], shifted(b1, cc, shift, nmask, p), p);
                        }
                        o0[h] = add_mod(o0[h], neg_if(u >= N, d0, p), p);
                        tg[h] = neg_if(u >= N, d1, p);
                    }
                }
                else
                {
                    const uint2 tt = *reinterpret_cast<const uint2 *>(table + c);
                    const std::size_t ti[2] = { tt.x, tt.y };
                    const ulonglong2 *m = HAS_ODD ? mono + (static_cast<std::size_t>(pid) << logn) : nullptr;
                    ulonglong2 vb0, vb1;
                    if (HAS_ODD)
                    {
                        vb0 = *reinterpret_cast<const ulonglong2 *>(b0 + c);
                        vb1 = *reinterpret_cast<const ulonglong2 *>(b1 + c);
                    }
                    const u64 q0[2] = { HAS_ODD ? vb0.x : 0, HAS_ODD ? vb0.y : 0 };
                    const u64 q1[2] = { HAS_ODD ? vb1.x : 0, HAS_ODD ? vb1.y : 0 };
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t i = ti[h];
                        u64 d0 = e0[i], d1 = e1[i];
                        o0[h] = s0[h];
                        o1[h] = s1[h];
                        if (HAS_ODD)
                        {
                            const ulonglong2 mc = m[c + h], mi = m[i];
                            d0 = sub_mod(d0, mulmod_shoup(b0[i], mi.x, mi.y, p), p);
                            d1 = sub_mod(d1, mulmod_shoup(b1[i], mi.x, mi.y, p), p);
                            o0[h] = add_mod(o0[h], mulmod_shoup(q0[h], mc.x, mc.y, p), p);
                            o1[h] = add_mod(o1[h], mulmod_shoup(q1[h], mc.x, mc.y, p), p);
                        }
                        o0[h] = add_mod(o0[h], d0, p);
                        tg[h] = d1;
                    }
                }
                u64 *po = out + x * 2 * poly + (r << logn) + c;
                store_stream2(po, o0[0], o0[1]);
                store_stream2(po + poly, o1[0], o1[1]);
                store_stream2(target + x * poly + (r << logn) + c, tg[0], tg[1]);
            }
        }
    } // namespace

    namespace
    {
        // the kernels divide the row index with 32-bit arithmetic: no buffer a device holds has 2^32 rows
        bool rows_exceed_32_bits(const Engine &e, std::size_t npairs)
        {
            return ((2 * npairs) >> e.logn) >> 32 != 0;
        }
    } // namespace

    hipError_t launch_lwe_extract(const Engine &e, const u64 *ct, std::size_t ct_stride, std::size_t count,
                                  const std::uint32_t *idx, std::size_t n_idx, u64 *lwe_a, u64 *lwe_b, const RowMap &map_q)
    {
        const std::size_t npairs = (count * n_idx * static_cast<std::size_t>(map_q.rows) << e.logn) / 2;
        if (!npairs)
            return hipSuccess;
        if (rows_exceed_32_bits(e, npairs))
            return hipErrorInvalidValue;
        ProfScope prof(e, "lwe_extract", 0);
        lwe_extract_kernel<<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(ct, ct_stride, idx, n_idx, lwe_a, lwe_b, e.d_primes,
                                                                               map_q, e.logn, npairs);
        return hipGetLastError();
    }

    hipError_t launch_lwe_embed(const Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n, std::size_t items,
                                std::size_t j0, std::size_t c, std::size_t n_out, u64 *out, const RowMap &map_q, const u64 *w,
                                const u64 *w_shoup, bool ntt_c0)
    {
        if (map_q.rows < 1 || map_q.rows > kMaxModuli)
            return hipErrorInvalidValue;
        const std::size_t npairs = (n_out * items * static_cast<std::size_t>(map_q.rows) << e.logn) / 2;
        if (!npairs)
            return hipSuccess;
        if (rows_exceed_32_bits(e, npairs) || j0 + c > n || (n_out != c && (n_out != 2 * c || n / 2 + j0 + c > n)))
            return hipErrorInvalidValue;
        PackWeights wt{};
        for (int r = 0; r < map_q.rows; r++)
        {
            wt.w[r] = w[r];
            wt.ws[r] = w_shoup[r];
        }
        ProfScope prof(e, "lwe_embed", 0);
        dispatch_bool(ntt_c0, [&](auto c0) {
            lwe_embed_kernel<decltype(c0)::value><<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(
                lwe_a, lwe_b, n, items, j0, c, n / 2, out, e.d_primes, map_q, wt, e.logn, npairs);
        });
        return hipGetLastError();
    }

    hipError_t launch_pack_merge(const Engine &e, const u64 *E, const u64 *B, u64 *out, u64 *target, std::size_t ncts,
                                 const RowMap &map_q, std::uint32_t shift, std::uint32_t ginv, const std::uint32_t *table,
                                 const u64 *mono)
    {
        const std::size_t npairs = (ncts * static_cast<std::size_t>(map_q.rows) << e.logn) / 2;
        if (!npairs)
            return hipSuccess;
        if (rows_exceed_32_bits(e, npairs))
            return hipErrorInvalidValue;
        ProfScope prof(e, "pack_merge", 0);
        dispatch_bool(table != nullptr, [&](auto ntt) {
            dispatch_bool(B != nullptr, [&](auto odd) {
                pack_merge_kernel<decltype(ntt)::value ? 1 : 0, decltype(odd)::value>
                    <<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(E, B, out, target, e.d_primes, map_q, e.logn, npairs, shift,
                                                                         ginv, table, reinterpret_cast<const ulonglong2 *>(mono));
            });
        });
        return hipGetLastError();
    }

    // ------------------------------------------------------------------------------------------
    // Oblivious expansion: one step of the tree, fused around the key switch
    // ------------------------------------------------------------------------------------------
    namespace
    {
        struct NoWeights // what an unscaled step carries for the normalisation: nothing
        {
        };
        // a loaded word, times w_r where the step normalises (SCALED: step 1 alone)
        template <bool SCALED, class W>
        __device__ __forceinline__ u64 expand_word(u64 v, const W &wt, std::size_t r, u64 p)
        {
            if constexpr (SCALED)
                return mulmod_shoup(v, wt.w[r], wt.ws[r], p);
            else
                return v;
        }

        // (X^(-s) E)[x] in coefficient form: E[x + s], with the sign of the wrap
        __device__ __forceinline__ u64 shifted_down(const u64 *__restrict__ e, std::size_t x, std::size_t s, std::size_t N, u64 p)
        {
            return neg_if(x + s >= N, e[(x + s) & (N - 1)], p);
        }

        // One step of the expansion without its key switch: with O = X^(-s) E,
        //     out_even = (E_0 + sigma_g(E_0), E_1),  target_even = sigma_g(E_1),
        //     out_odd  = (O_0 + sigma_g(O_0), O_1),  target_odd  = sigma_g(O_1),
        // so that out + key_switch(target) is E + apply_galois(E, g) and O + apply_galois(O, g). Source x is [2][k][N] at
        // x * src_stride words; with x = item * 2^log_grp + j its even result is ciphertext item * out_item + j of out and
        // its odd one out_odd ciphertexts behind it; the targets ([k][N] each) likewise with tgt_item and tgt_odd. One lane
        // per pair of output coefficients of one row of one source; every permutation is on the load side.
        // FORM 0, coefficient form: coefficient c of sigma_g(D) is +-D[c g^{-1} mod 2N] (ginv = g^{-1} mod 2N).
        // FORM 1, NTT form: O = M (.) E with M = NTT(X^(-s)) as {word, Shoup companion} pairs, sigma_g(D)[c] = D[T[c]].
        // SCALED: every loaded word of E is multiplied by w_r first (the normalisation, which step 1 applies).
        template <int FORM, bool SCALED>
        __global__ __launch_bounds__(kThreads) void expand_step_kernel(
            const u64 *__restrict__ E, std::size_t src_stride, u64 *__restrict__ out, u64 *__restrict__ target,
            const PrimeDev *__restrict__ primes, RowMap map, int logn, std::size_t npairs, int log_grp, std::size_t out_item,
            std::size_t out_odd, std::size_t tgt_item, std::size_t tgt_odd, std::uint32_t shift, std::uint32_t ginv,
            const std::uint32_t *__restrict__ table, const ulonglong2 *__restrict__ mono,
            std::conditional_t<SCALED, PackWeights, NoWeights> wt)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const std::size_t k = static_cast<std::size_t>(map.rows);
            const std::size_t poly = k << logn;
            for (std::size_t t = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; t < npairs; t += stride)
            {
                const std::size_t word = 2 * t;
                const std::size_t c = word & nmask;
                const std::size_t row = word >> logn; // x * k + r; below 2^32 (the launcher): a 32-bit division
                const unsigned row32 = static_cast<unsigned>(row), x32 = row32 / static_cast<unsigned>(k);
                const std::size_t x = x32, r = row32 - x32 * static_cast<unsigned>(k);
                const std::size_t item = x >> log_grp, j = x - (item << log_grp);
                const unsigned short pid = map.prime[r];
                const u64 p = primes[pid].p;
                const u64 *e0 = E + x * src_stride + (r << logn), *e1 = e0 + poly;
                const ulonglong2 ve0 = *reinterpret_cast<const ulonglong2 *>(e0 + c);
                const ulonglong2 ve1 = *reinterpret_cast<const ulonglong2 *>(e1 + c);
                const u64 s0[2] = { expand_word<SCALED>(ve0.x, wt, r, p), expand_word<SCALED>(ve0.y, wt, r, p) };
                const u64 s1[2] = { expand_word<SCALED>(ve1.x, wt, r, p), expand_word<SCALED>(ve1.y, wt, r, p) };
                u64 ev0[2], ev1[2], evt[2], od0[2], od1[2], odt[2];
                if (FORM == 0)
                {
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t cc = c + h;
                        const std::size_t u = (cc * ginv) & (2 * N - 1), i = u & nmask;
                        const bool neg = u >= N;
                        const u64 d0 = expand_word<SCALED>(e0[i], wt, r, p), d1 = expand_word<SCALED>(e1[i], wt, r, p);
                        ev0[h] = add_mod(s0[h], neg_if(neg, d0, p), p);
                        ev1[h] = s1[h];
                        evt[h] = neg_if(neg, d1, p);
                        const u64 q0 = expand_word<SCALED>(shifted_down(e0, cc, shift, N, p), wt, r, p);
                        const u64 q1 = expand_word<SCALED>(shifted_down(e1, cc, shift, N, p), wt, r, p);
                        const u64 g0 = expand_word<SCALED>(shifted_down(e0, i, shift, N, p), wt, r, p);
                        const u64 g1 = expand_word<SCALED>(shifted_down(e1, i, shift, N, p), wt, r, p);
                        od0[h] = add_mod(q0, neg_if(neg, g0, p), p);
                        od1[h] = q1;
                        odt[h] = neg_if(neg, g1, p);
                    }
                }
                else
                {
                    const uint2 tt = *reinterpret_cast<const uint2 *>(table + c);
                    const std::size_t ti[2] = { tt.x, tt.y };
                    const ulonglong2 *m = mono + (static_cast<std::size_t>(pid) << logn);
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t i = ti[h];
                        const ulonglong2 mc = m[c + h], mi = m[i];
                        const u64 d0 = expand_word<SCALED>(e0[i], wt, r, p), d1 = expand_word<SCALED>(e1[i], wt, r, p);
                        ev0[h] = add_mod(s0[h], d0, p);
                        ev1[h] = s1[h];
                        evt[h] = d1;
                        od0[h] = add_mod(mulmod_shoup(s0[h], mc.x, mc.y, p), mulmod_shoup(d0, mi.x, mi.y, p), p);
                        od1[h] = mulmod_shoup(s1[h], mc.x, mc.y, p);
                        odt[h] = mulmod_shoup(d1, mi.x, mi.y, p);
                    }
                }
                const std::size_t at = (r << logn) + c;
                u64 *po = out + (item * out_item + j) * 2 * poly + at;
                store_stream2(po, ev0[0], ev0[1]);
                store_stream2(po + poly, ev1[0], ev1[1]);
                store_stream2(po + out_odd * 2 * poly, od0[0], od0[1]);
                store_stream2(po + out_odd * 2 * poly + poly, od1[0], od1[1]);
                u64 *pt = target + (item * tgt_item + j) * poly + at;
                store_stream2(pt, evt[0], evt[1]);
                store_stream2(pt + tgt_odd * poly, odt[0], odt[1]);
            }
        }
    } // namespace

    hipError_t launch_expand_step(const Engine &e, const u64 *E, std::size_t src_stride, std::size_t nsrc, int log_grp, u64 *out,
                                  std::size_t out_item, std::size_t out_odd, u64 *target, std::size_t tgt_item, std::size_t tgt_odd,
                                  const RowMap &map_q, std::uint32_t shift, std::uint32_t ginv, const std::uint32_t *table,
                                  const u64 *mono, const u64 *w, const u64 *w_shoup)
    {
        if (map_q.rows < 1 || map_q.rows > kMaxModuli)
            return hipErrorInvalidValue;
        const std::size_t npairs = (nsrc * static_cast<std::size_t>(map_q.rows) << e.logn) / 2;
        if (!npairs)
            return hipSuccess;
        // (a group's results must not reach into the odd half or the next item; the NTT form needs its rows)
        const std::size_t grp = static_cast<std::size_t>(1) << log_grp;
        if (rows_exceed_32_bits(e, npairs) || log_grp < 0 || shift < 1 || shift >= e.n || out_odd < grp || tgt_odd < grp ||
            (nsrc > grp && (out_item < out_odd + grp || tgt_item < tgt_odd + grp)) || (table != nullptr) != (mono != nullptr) ||
            (w != nullptr) != (w_shoup != nullptr))
            return hipErrorInvalidValue;
        ProfScope prof(e, "expand_step", 0);
        const unsigned grid = grid_for(npairs);
        dispatch_bool(table != nullptr, [&](auto ntt) {
            dispatch_bool(w != nullptr, [&](auto scaled) {
                constexpr int form = decltype(ntt)::value ? 1 : 0;
                constexpr bool sc = decltype(scaled)::value;
                std::conditional_t<sc, PackWeights, NoWeights> wt{};
                if constexpr (sc)
                    for (int r = 0; r < map_q.rows; r++)
                    {
                        wt.w[r] = w[r];
                        wt.ws[r] = w_shoup[r];
                    }
                expand_step_kernel<form, sc><<<grid, kThreads, 0, e.lane().stream>>>(
                    E, src_stride, out, target, e.d_primes, map_q, e.logn, npairs, log_grp, out_item, out_odd, tgt_item, tgt_odd,
                    shift, ginv, table, reinterpret_cast<const ulonglong2 *>(mono), wt);
            });
        });
        return hipGetLastError();
    }
} // namespace sealhip
