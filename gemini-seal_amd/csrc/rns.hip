// rns.hip -- BEHZ base conversions and modulus switching (native/src/seal/util/rns.cpp:731-1068) as
// column-parallel kernels: one lane owns one coefficient column of one item and walks the RNS rows,
// so every global access is a coalesced row segment; the per-prime constants are wave-uniform
// (scalar loads). All outputs are canonical residues, so constants are fused where the reference
// multiplies twice (e.g. m_tilde * q^_i^{-1}).
#include <type_traits>

#include "engine.hpp"
#include "instance_dispatch.hpp"

namespace sealhip
{
    namespace
    {
        // compile-time loop: f(std::integral_constant<int, I>{}) for I = 0 .. N-1
        template <int N, int I = 0, class F>
        __device__ __forceinline__ void static_for(F &&f)
        {
            if constexpr (I < N)
            {
                f(std::integral_constant<int, I>{});
                static_for<N, I + 1>(f);
            }
        }

        // The level constants never change after the context is built. Reading them through the constant address
        // space tells the compiler so: scalar loads that can be merged and hoisted above the kernel's own stores
        // (through a plain pointer every constant is re-fetched, and waited for, right before its use).
        template <class T>
        __device__ __forceinline__ const __attribute__((address_space(4))) T *kc(const T *p)
        {
            return (const __attribute__((address_space(4))) T *)p;
        }

        // One row's constants at a time: the row pointer and the row's result each pass through an empty asm statement. Such
        // statements keep their order, so a row's scalar loads cannot be requested before the preceding row's result
        // exists. Left alone, the straight-line row loops of the exact-K instances request every row's constants up front
        // (sched_barrier orders the machine scheduler only, instruction selection has sunk the arithmetic below the loads
        // by then) and spill scalar registers to vector lanes.
        template <class T>
        __device__ __forceinline__ const __attribute__((address_space(4))) T *row_window(
            const __attribute__((address_space(4))) T *row)
        {
            asm volatile("" : "+s"(row));
            return row;
        }
        __device__ __forceinline__ void row_done(u64 &v)
        {
            asm volatile("" : "+v"(v));
        }

        struct Cols
        {
            std::size_t item, c;
        };
        __device__ __forceinline__ bool column(std::size_t count, int logn, Cols &out)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            out.item = i >> logn;
            out.c = i & ((static_cast<std::size_t>(1) << logn) - 1);
            return out.item < count;
        }

        // t[i] = x_i * (q^_i)^{-1} mod q_i  (first loop of fast_convert_array, rns.cpp:476-485)
        // then out_j = sum_i t[i] * M[j][i] mod p_j  (dot_product_mod, rns.cpp:487-495)
        template <int KMAX>
        __device__ __forceinline__ u64 dot_mod(const u64 (&t)[KMAX], int k, const u64 *__restrict__ mrow,
                                               const PrimeDev &P)
        {
            u64 lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < KMAX; i++)
                if (i < k)
                    mac128(lo, hi, t[i], mrow[i]);
            return barrett_reduce_128(lo, hi, P.p, P.cr0, P.cr1);
        }

        // fastbconv_m_tilde (rns.cpp:1025-1068): k rows -> |Bsk|+1 rows
        template <int KMAX>
        __global__ __launch_bounds__(kThreads) void fastbconv_m_tilde_kernel(
            const RnsDev *__restrict__ d, const PrimeDev *__restrict__ primes, const u64 *__restrict__ in,
            std::size_t in_stride, u64 *__restrict__ out, std::size_t out_stride, std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k, nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            u64 t[KMAX];
#pragma unroll
            for (int i = 0; i < KMAX; i++)
                if (i < k)
                {
                    const PrimeDev &Q = primes[d->q_prime[i]];
                    t[i] = mul_mod(pin[i * N], d->q_mt_inv[i], Q.p, Q.cr0, Q.cr1);
                }
            for (int j = 0; j < nB; j++)
                pout[j * N] = dot_mod<KMAX>(t, k, d->q_to_Bsk + j * k, primes[d->bsk_prime[j]]);
            u64 acc = 0; // modulus 2^32: only the low word matters
#pragma unroll
            for (int i = 0; i < KMAX; i++)
                if (i < k)
                    acc += t[i] * d->q_to_mt[i];
            pout[nB * N] = acc & 0xFFFFFFFFull;
        }

        // centred reduction of r_m_tilde modulo the row's prime p (rns.cpp:969-973)
        __device__ __forceinline__ u64 centred_r_m_tilde(u64 r_mt, u64 p)
        {
            u64 temp = r_mt;
            if (temp >= (1ull << 31))
                temp += p - (1ull << 32);
            return temp;
        }
        // sm_mrq (rns.cpp:925-981)
        __device__ __forceinline__ u64 sm_mrq_one(u64 in_b, u64 r_mt, const RnsDev *d, int j, const PrimeDev &Bp)
        {
            u64 temp = r_mt; // (centred_r_m_tilde: the unit kernel keeps the statement, which the compiler lays out otherwise)
            if (temp >= (1ull << 31))
                temp += Bp.p - (1ull << 32);
            return mul_mod(mul_add_mod(d->prod_q_mod_Bsk[j], temp, in_b, Bp.p, Bp.cr0, Bp.cr1), d->inv_mt_mod_Bsk[j],
                           Bp.p, Bp.cr0, Bp.cr1);
        }
        template <class DP>
        __device__ __forceinline__ u64 r_m_tilde(u64 in_mt, DP d)
        {
            const u64 temp = (in_mt * d->inv_prod_q_mod_mt) & 0xFFFFFFFFull;
            return temp ? (1ull << 32) - temp : 0;
        }

        __global__ __launch_bounds__(kThreads) void sm_mrq_kernel(const RnsDev *__restrict__ d,
                                                                  const PrimeDev *__restrict__ primes,
                                                                  const u64 *__restrict__ in, std::size_t in_stride,
                                                                  u64 *__restrict__ out, std::size_t out_stride,
                                                                  std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            const u64 r_mt = r_m_tilde(pin[nB * N], d);
            for (int j = 0; j < nB; j++)
                pout[j * N] = sm_mrq_one(pin[j * N], r_mt, d, j, primes[d->bsk_prime[j]]);
        }

        // fused fastbconv_m_tilde + sm_mrq (evaluator.cpp:345-348): k rows -> |Bsk| rows. The step-by-step form, for k > 32
        __global__ __launch_bounds__(kThreads) void bfv_lift_kernel(const RnsDev *__restrict__ d,
                                                                    const PrimeDev *__restrict__ primes,
                                                                    const u64 *__restrict__ in, std::size_t in_stride,
                                                                    u64 *__restrict__ out, std::size_t out_stride,
                                                                    std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k, nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            u64 t[kMaxModuli];
            u64 acc = 0;
#pragma unroll
            for (int i = 0; i < kMaxModuli; i++)
                if (i < k)
                {
                    const PrimeDev &Q = primes[d->q_prime[i]];
                    t[i] = mul_mod(pin[i * N], d->q_mt_inv[i], Q.p, Q.cr0, Q.cr1);
                    acc += t[i] * d->q_to_mt[i];
                }
            const u64 r_mt = r_m_tilde(acc & 0xFFFFFFFFull, d);
            for (int j = 0; j < nB; j++)
            {
                const PrimeDev &Bp = primes[d->bsk_prime[j]];
                const u64 conv = dot_mod<kMaxModuli>(t, k, d->q_to_Bsk + j * k, Bp);
                pout[j * N] = sm_mrq_one(conv, r_mt, d, j, Bp);
            }
        }

        // Constant-folded variant of bfv_lift_kernel (k <= 32): the chain
        //   conv_j = sum_i t_i M_ji mod b;  u = (prod_q*temp + conv_j) mod b;  out = u * m_tilde^{-1} mod b
        // (rns.cpp:1062-1067 + :960-980) is a composition of exact modular operations, so it equals
        //   out = ( sum_i t_i*(M_ji*m_tilde^{-1}) + temp*(prod_q*m_tilde^{-1}) ) mod b
        // with ONE 128-bit accumulation and ONE reduction per output instead of three. The constants carry the factor 2^64,
        // which the Montgomery reduction removes. Two families of kernels compute it (and the fused floor below):
        //   exact k     K = 1 .. bounds::kBehzExactMaxK primes, known at compile time, launched only where the host proved
        //               that every REDC lands below 2p (RnsDev::redc_small): no guards and no branches in the row loops, the
        //               constants of a dot product are one packed row (wide scalar loads), the dot products are carry-free
        //               (dotacc.hpp) at the split S the host selected for the level (RnsDev::dot_split)
        //   run-time k  any k <= kBehzGeneric: guarded loops, the constants in separate arrays, 128-bit multiply-accumulate

        // Exact k, the floor's three dot products (the lift's row writes the same steps out, see there):
        // (head * chead +) sum_i v[i] * c[i] mod p, canonical. c is packed (dot_pack<S>); `last` says whether the
        // last of K + 1 values takes part (the optional extra prime of B); K values all do. KIND names the dot product's
        // operand classes (bounds::behz_dot_shape); kind 2, the m_sk row, has no head term.
        // The values' constants start at c[C0]. p and ninv (and rdp below) come as pointers, read after the products: a
        // caller that has the word passes its local's address, one that has not passes the table's.
        template <int KIND, int K, int C0, int S, int NV, class CP, class PP, class NP>
        __device__ __forceinline__ u64 dot_redc_exact(const Split<S> &head, u64 chead, const Split<S> (&v)[NV], bool last,
                                                      CP c, PP p, NP ninv)
        {
            constexpr int H = KIND == 2 ? 0 : 1;
            u64 lo, hi;
            BehzDot<S, KIND, K> acc; // carry-free accumulation (dotacc.hpp), same integer sum
            if constexpr (H != 0)
                acc.template add<0>(head, chead);
            static_for<NV>([&](auto I) {
                if (I.value < K || last)
                    acc.template add<I.value + H>(v[I.value], c[I.value + C0]);
            });
            acc.finish(lo, hi);
            const u64 pv = *p;
            return redc_canonical_hs(lo, hi, pv, *ninv);
        }
        // Run-time k: head * chead + sum_{i < n} v[i] * row[i] mod p, canonical (`small`: the REDC lands below 2p)
        template <int NV, class CP, class PP, class NP, class RP>
        __device__ __forceinline__ u64 dot_redc_guarded(u64 head, u64 chead, const u64 (&v)[NV], CP row, int n, PP p,
                                                        NP ninv, RP rdp, bool small)
        {
            u64 lo = head * chead, hi = mulhi(head, chead);
#pragma unroll
            for (int i = 0; i < NV; i++)
                if (i < n)
                    mac128(lo, hi, v[i], row[i]);
            const u64 pv = *p;
            return redc_finish(redc128(lo, hi, pv, *ninv), pv, *rdp, small);
        }

        // The lift at an exact K.
        // TOP: one lane per column PAIR (c, c + N/2); after a row's two outputs are formed the lane
        // applies the forward NTT's top layer to them (ForwardLazy, ntt.cpp:245-252, the very function the NTT kernel's load
        // phase would run on these two words) and stores the results. The transform that follows is launched with
        // kNttTopDone: its workgroups then read their own half only, and the layer's products are computed once per pair
        // instead of once per workgroup.
        template <int K, bool TOP, int S>
        __global__ __launch_bounds__(kThreads) void bfv_lift_exact_kernel(const RnsDev *__restrict__ d_,
                                                                          const PrimeDev *__restrict__, // (RnsDev has the rows' primes)
                                                                          const u64 *__restrict__ in, std::size_t in_stride,
                                                                          u64 *__restrict__ out, std::size_t out_stride,
                                                                          std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, TOP ? logn - 1 : logn, cc))
                return;
            constexpr int NC = TOP ? 2 : 1; // columns per lane
            const auto *d = kc(d_);         // read-only for the lifetime of the context: constant address space
            const int nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            u64 t[NC][K];
            u64 acc[NC] = {};
#pragma unroll
            for (int i = 0; i < K; i++)
            {
                const u64 qp = d->q_p[i];
#pragma unroll
                for (int h = 0; h < NC; h++)
                {
                    t[h][i] = mulmod_shoup_hs(pin[i * N + h * (N >> 1)], d->q_mt_inv[i], d->q_mt_inv_s[i], qp); // exact canonical product
                    acc[h] += t[h][i] * d->q_to_mt[i];
                }
            }
            u64 r_mt[NC];
#pragma unroll
            for (int h = 0; h < NC; h++)
                r_mt[h] = r_m_tilde(acc[h] & 0xFFFFFFFFull, d);
            Split<S> ts[NC][K];
            static_for<K>([&](auto I) {
#pragma unroll
                for (int h = 0; h < NC; h++)
                    ts[h][I.value] = Split<S>(t[h][I.value]);
            });
            const auto *Lrows = kc(d->lift_rows);
            const auto row_out = [&](int j) {
                // the row {L2, L1[0..K-1], p, -p^-1}, split for the dot product, is one contiguous run of scalar loads
                const auto *row = row_window(Lrows + j * (K + 3));
                const u64 bp = row[K + 1];
                const u64 ninv = row[K + 2];
                u64 v[NC];
#pragma unroll
                for (int h = 0; h < NC; h++)
                {
                    // (dot_redc_exact<0, K, 1> written out: inside this column loop the call leaves the one-column instances
                    //  another schedule, with scalar registers spilled to vector lanes at K = 15)
                    u64 lo, hi;
                    BehzDot<S, 0, K> acc2; // carry-free accumulation (dotacc.hpp), same integer sum
                    acc2.template add<0>(Split<S>(centred_r_m_tilde(r_mt[h], bp)), row[0]);
                    static_for<K>([&](auto I) { acc2.template add<I.value + 1>(ts[h][I.value], row[I.value + 1]); });
                    acc2.finish(lo, hi);
                    v[h] = redc_canonical_hs(lo, hi, bp, ninv);
                }
                if constexpr (TOP)
                {
                    butterfly_fwd_hs<true>(v[0], v[1], d->b_w1[j], d->b_w1s[j], 0 - bp, bp << 1);
                    pout[j * N + (N >> 1)] = v[1];
                }
                pout[j * N] = v[0];
            };
            // |Bsk| is k + 1 or k + 2 (rns.cpp:568-573): with an exact K only the last row is a run-time question, the
            // others are straight-line code whose scalar loads overlap the neighbouring rows' arithmetic
            static_for<K + 1>([&](auto J) { row_out(J.value); });
            if (nB == K + 2)
                row_out(K + 1);
        }

        // The lift at a run-time k <= kBehzGeneric
        __global__ __launch_bounds__(kThreads) void bfv_lift_guarded_kernel(const RnsDev *__restrict__ d_,
                                                                            const PrimeDev *__restrict__, // (RnsDev has the rows' primes)
                                                                            const u64 *__restrict__ in, std::size_t in_stride,
                                                                            u64 *__restrict__ out, std::size_t out_stride,
                                                                            std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const auto *d = kc(d_); // read-only for the lifetime of the context: constant address space
            const int k = d->k, nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            u64 t[kBehzGeneric];
            u64 acc = 0;
#pragma unroll
            for (int i = 0; i < kBehzGeneric; i++)
                if (i < k)
                {
                    t[i] = mulmod_shoup_hs(pin[i * N], d->q_mt_inv[i], d->q_mt_inv_s[i], d->q_p[i]); // exact canonical product
                    acc += t[i] * d->q_to_mt[i];
                }
            const u64 r_mt = r_m_tilde(acc & 0xFFFFFFFFull, d);
            const bool small = d->redc_small != 0;
            const auto *L1m = kc(d->lift_L1m);
            const auto *L2m = kc(d->lift_L2m);
            for (int j = 0; j < nB; j++)
            {
                const u64 bp = d->b_p[j];
                const u64 ninv = d->b_ninv[j];
                pout[j * N] = dot_redc_guarded(centred_r_m_tilde(r_mt, bp), L2m[j], t, L1m + j * k, k, &bp, &ninv, &d->b_rdp[j], small);
            }
        }

        // Constant-folded variant of bfv_floor_sk_kernel (k <= 32); see RnsDev for the folded constants.
        // Every output is the same canonical residue as the step-by-step version: only exact modular
        // identities are used ((b - c)*g == -c*g, (x*t)*g == x*(t*g), mul_add_mod(a,b,c) == a*b + c (mod q)).
        // One coefficient of an inverse-NTT output whose top layer was deferred (kNttDeferTop): BackwardLazyLast
        // (ntt.cpp:274-281) on the pair (c mod N/2, c mod N/2 + N/2), this lane's side of the butterfly only, without the
        // multiplication: its constant (n^{-1} or w * n^{-1}) is folded into the constant the
        // value is multiplied with next (RnsDev::floor_F0_top / floor_G1m_top). REDUCE brings the value below 2p (operands
        // of the carry-free dot products must stay below 2^61); a Shoup product takes it as it is.
        template <bool REDUCE>
        __device__ __forceinline__ u64 before_top(u64 u, u64 v, bool is_hi, u64 two_p)
        {
            const u64 vv = is_hi ? two_p - v : v; // (a select, not a branch: a uniform branch here splits the row loop into
            u64 r = u + vv;                       //  blocks the scalar loads cannot be scheduled across); r < 4p
            if (REDUCE)
                r = r >= two_p ? r - two_p : r;
            return r;
        }
        // The column of this lane where the inverse NTT's top layer was deferred; is_hi: it lies in the upper half of its row.
        // The lanes of columns c and c + N/2 read the same 2(k + |Bsk| + 1) words. Blocks
        // are dealt round-robin over the 8 XCDs (one L2 each): physical blocks b and b + 8 run on the same XCD at
        // about the same time, so they are given the lower and the upper half of the same 256 columns and the second
        // read comes from L2 instead of HBM (the halves used to be half a grid apart: 37 row passes instead of 22).
        // logn >= 14 here: the blocks of an item are a multiple of 16. Everything is derived from the block index, so
        // the compiler knows is_hi is uniform and reads the tables selected by it with scalar loads.
        __device__ __forceinline__ bool deferred_column(std::size_t count, std::size_t N, Cols &cc, bool &is_hi)
        {
            const std::size_t per_item = N / kThreads, bid = blockIdx.x;
            cc.item = bid / per_item;
            if (cc.item >= count)
                return false;
            const unsigned pl = static_cast<unsigned>(bid - cc.item * per_item), r = pl & 15u;
            is_hi = (r >> 3) != 0;
            cc.c = (is_hi ? N >> 1 : 0) + static_cast<std::size_t>(((pl >> 4) << 3) | (r & 7u)) * kThreads + threadIdx.x;
            return true;
        }
        // The Shenoy-Kumaresan correction's sign and magnitude (rns.cpp:898-909) from the two m_sk words
        struct SkAlpha
        {
            bool neg;
            u64 a2;
        };
        template <class DP>
        __device__ __forceinline__ SkAlpha sk_alpha(u64 diff, u64 mp, DP d) // diff = conv_sk - fl_sk, kept positive
        {
            const u64 alpha = mulmod_shoup(diff, d->inv_prod_B_mod_msk, d->inv_prod_B_mod_msk_s, mp);
            const bool neg = alpha > (mp >> 1); // rns.cpp:909
            return { neg, neg ? mp - alpha : alpha };
        }

        // The floor at an exact K
        template <int K, bool DEFER, int S>
        __global__ __launch_bounds__(kThreads) void bfv_floor_sk_exact_kernel(const RnsDev *__restrict__ d_,
                                                                              const PrimeDev *__restrict__, // (RnsDev has the rows' primes)
                                                                              const u64 *__restrict__ in,
                                                                              std::size_t in_stride, u64 *__restrict__ out,
                                                                              std::size_t out_stride, std::size_t count,
                                                                              int logn, int mont, unsigned *__restrict__ tflags)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const std::size_t half = N >> 1;
            Cols cc;
            bool is_hi = false;
            if (DEFER ? !deferred_column(count, N, cc, is_hi) : !column(count, logn, cc))
                return;
            const auto *d = kc(d_); // read-only for the lifetime of the context: constant address space
            const int B = d->B;     // K or K + 1
            // every test against B is a compile-time fact except for the one optional extra prime of B (index K): no
            // branches inside the row loops, so scalar loads and arithmetic of neighbouring rows overlap
            const bool extraB = B > K;
            const auto lt_B = [&](int j) { return j < K || (j == K && extraB); };
            const auto le_B = [&](int j) { return j <= K || (j == K + 1 && extraB); };
            const u64 *pin = in + cc.item * in_stride + cc.c;
            const u64 *pitem = in + cc.item * in_stride;
            const std::size_t c_lo = cc.c & (half - 1);
            u64 *pout = out + cc.item * out_stride + cc.c;
            // every input word of this column is requested before any arithmetic: one exposed memory latency per
            // thread instead of one per output row (the loads used to sit in the row loops)
            u64 ru[2 * K + 2], rv[2 * K + 2];
#pragma unroll
            for (int i = 0; i < K; i++)
            {
                ru[i] = DEFER ? pitem[i * N + c_lo] : pin[i * N];
                rv[i] = DEFER ? pitem[i * N + c_lo + half] : 0;
            }
            static_for<K + 2>([&](auto J) {
                constexpr int j = J.value;
                if (le_B(j))
                {
                    ru[K + j] = DEFER ? pitem[(K + j) * N + c_lo] : pin[(K + j) * N];
                    rv[K + j] = DEFER ? pitem[(K + j) * N + c_lo + half] : 0;
                }
            });
            __builtin_amdgcn_sched_barrier(0);
            u64 t[K];
            // mont (kernel-uniform): the input words carry the Montgomery factor 2^-64 of the tensor product formed inside
            // the inverse NTT; the constants of the first product of every input then carry 2^64 on top
            const int top_sel = (mont ? 2 : 0) + (is_hi ? 1 : 0); // scalar: selects a table by address arithmetic
            // {F0, its Shoup quotient, q_i} sit next to each other, one short scalar load per input row, requested
            // as the loop goes (a batch of all 3K constants up front held 6K scalar registers through the first rows and
            // pushed the row constants to scratch)
            const auto *first = kc(d->floor_first) + (DEFER ? top_sel : 4) * (K * 3);
#pragma unroll
            for (int i = 0; i < K; i++)
            {
                const u64 cF0 = first[3 * i], cF0s = first[3 * i + 1];
                const u64 qp = first[3 * i + 2];
                if (DEFER) // (u +- v) * (n^{-1} or w n^{-1}) * F0 with ONE canonical Shoup product
                    t[i] = mulmod_shoup_hs(before_top<false>(ru[i], rv[i], is_hi, qp << 1), cF0, cF0s, qp);
                else
                    t[i] = mulmod_shoup_hs(ru[i], cF0, cF0s, qp);
            }
            u64 tb[K + 1];
            u64 fl_sk = 0;
            Split<S> ts[K], tbs[K + 1];
            static_for<K>([&](auto I) { ts[I.value] = Split<S>(t[I.value]); });
            // the row {G1, G2[0..K-1], p, -p^-1} of this launch's table, split at S, in one run of scalar loads
            const auto *Frows = kc(d->floor_rows) + (DEFER ? top_sel : 4) * (d->nB * (K + 3));
            // (compile-time row indices: a `#pragma unroll` gives up on these loops from K = 15 on and leaves
            //  run-time indexed register arrays, i.e. scratch)
            static_for<K + 2>([&](auto J) {
                constexpr int j = J.value;
                if (le_B(j))
                {
                    const auto *row = row_window(Frows + j * (K + 3));
                    const u64 bp = row[K + 1];
                    const u64 ninv = row[K + 2];
                    const u64 x = DEFER ? before_top<true>(ru[K + j], rv[K + j], is_hi, bp << 1) : ru[K + j];
                    u64 v = dot_redc_exact<1, K, 1>(Split<S>(x), row[0], ts, false, row, &bp, &ninv);
                    row_done(v);
                    if (lt_B(j))
                        tb[j < K + 1 ? j : 0] = v;
                    else
                        fl_sk = v;
                    // one row's constants at a time: left alone the scheduler requests the constants of every row up front
                    // and spills scalar registers to scratch
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
            const u64 mp = d->b_p[B];
            const auto *BtoMsk = kc(d->B_to_mskp);
            static_for<K + 1>([&](auto J) {
                if (lt_B(J.value))
                    tbs[J.value] = Split<S>(tb[J.value]);
            });
            const u64 conv_sk = dot_redc_exact<2, K, 0>(Split<S>(), 0, tbs, extraB, BtoMsk, &mp, &d->b_ninv[B]);
            const SkAlpha al = sk_alpha(conv_sk + (mp - fl_sk), mp, d);
            const bool neg = al.neg;
            const Split<S> a2s(al.a2);
            const auto *Qrows = kc(d->q_rows); // rows {pB, nB, B_to_q[i][0..B-1], p, -p^-1}, split at S
            u64 nz = 0;                        // OR of the words this column stores (transparency sink)
            const auto q_row = [&](int i) {
                const auto *qrow = Qrows + i * (B + 4);
                const u64 c = neg ? qrow[0] : qrow[1];
                const u64 w = dot_redc_exact<3, K, 2>(a2s, c, tbs, extraB, qrow, qrow + (B + 2), qrow + (B + 3));
                pout[i * N] = w;
                nz |= w;
                __builtin_amdgcn_sched_barrier(0);
            };
            static_for<K>([&](auto I) { q_row(I.value); });
            note_nonzero(tflags, cc.item, nz); // (the launcher passes the sink for polynomials 1.. of the product only)
        }

        // The floor at a run-time k <= kBehzGeneric
        template <bool DEFER>
        __global__ __launch_bounds__(kThreads) void bfv_floor_sk_guarded_kernel(const RnsDev *__restrict__ d_,
                                                                                const PrimeDev *__restrict__, // (RnsDev has the rows' primes)
                                                                                const u64 *__restrict__ in,
                                                                                std::size_t in_stride, u64 *__restrict__ out,
                                                                                std::size_t out_stride, std::size_t count,
                                                                                int logn, int mont, unsigned *__restrict__ tflags)
        {
            constexpr int KA = kBehzGeneric; // array extent
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const std::size_t half = N >> 1;
            Cols cc;
            bool is_hi = false;
            if (DEFER ? !deferred_column(count, N, cc, is_hi) : !column(count, logn, cc))
                return;
            const auto *d = kc(d_); // read-only for the lifetime of the context: constant address space
            const int k = d->k, B = d->B; // B is k or k + 1
            const u64 *pin = in + cc.item * in_stride + cc.c;
            const u64 *pitem = in + cc.item * in_stride;
            const std::size_t c_lo = cc.c & (half - 1);
            u64 *pout = out + cc.item * out_stride + cc.c;
            // every input word of this column is requested before any arithmetic: one exposed memory latency per
            // thread instead of one per output row (the loads used to sit in the row loops)
            u64 ru[2 * KA + 2], rv[2 * KA + 2];
#pragma unroll
            for (int i = 0; i < KA; i++)
                if (i < k)
                {
                    ru[i] = DEFER ? pitem[i * N + c_lo] : pin[i * N];
                    rv[i] = DEFER ? pitem[i * N + c_lo + half] : 0;
                }
#pragma unroll
            for (int j = 0; j < KA + 2; j++)
                if (j <= B)
                {
                    ru[KA + j] = DEFER ? pitem[(k + j) * N + c_lo] : pin[(k + j) * N];
                    rv[KA + j] = DEFER ? pitem[(k + j) * N + c_lo + half] : 0;
                }
            __builtin_amdgcn_sched_barrier(0);
            u64 t[KA];
            // mont (kernel-uniform): the input words carry the Montgomery factor 2^-64 of the tensor product formed inside
            // the inverse NTT; the constants of the first product of every input then carry 2^64 on top
            const int top_sel = (mont ? 2 : 0) + (is_hi ? 1 : 0); // scalar: selects a table by address arithmetic
            // the constants of the first loop, requested as one batch of scalar loads while the vector loads are in flight
            // (inside the loop every iteration waited for its own three)
            const auto *F0t = DEFER ? kc(d->floor_F0_top[top_sel]) : kc(d->floor_F0);
            const auto *F0ts = DEFER ? kc(d->floor_F0_top_s[top_sel]) : kc(d->floor_F0_s);
#pragma unroll
            for (int i = 0; i < KA; i++)
                if (i < k)
                {
                    const u64 cF0 = F0t[i], cF0s = F0ts[i];
                    const u64 qp = d->q_p[i];
                    if (DEFER) // (u +- v) * (n^{-1} or w n^{-1}) * F0 with ONE canonical Shoup product
                        t[i] = mulmod_shoup_hs(before_top<false>(ru[i], rv[i], is_hi, qp << 1), cF0, cF0s, qp);
                    else
                        t[i] = mulmod_shoup_hs(ru[i], cF0, cF0s, qp);
                }
            u64 tb[KA + 1];
            u64 fl_sk = 0;
            const bool small = d->redc_small != 0;
            const auto *G1m = DEFER ? kc(d->floor_G1m_top[top_sel]) : kc(d->floor_G1m);
            const auto *G2m = kc(d->floor_G2m);
            for (int j = 0; j < KA + 2; j++)
                if (j <= B)
                {
                    const u64 bp = d->b_p[j];
                    const u64 ninv = d->b_ninv[j];
                    const u64 x = DEFER ? before_top<true>(ru[KA + j], rv[KA + j], is_hi, bp << 1) : ru[KA + j];
                    const u64 v = dot_redc_guarded(x, G1m[j], t, G2m + j * k, k, &bp, &ninv, &d->b_rdp[j], small);
                    if (j < B)
                        tb[j < KA + 1 ? j : 0] = v;
                    else
                        fl_sk = v;
                    // one row's constants at a time: left alone the scheduler requests the constants of every row up front
                    // and spills scalar registers to scratch
                    __builtin_amdgcn_sched_barrier(0);
                }
            const u64 mp = d->b_p[B];
            const u64 conv_sk = dot_redc_guarded(0, 0, tb, kc(d->B_to_mskm), B, &mp, &d->b_ninv[B], &d->b_rdp[B], small);
            const SkAlpha al = sk_alpha(conv_sk + (mp - fl_sk), mp, d);
            const auto *pBm = kc(d->pBm);
            const auto *nBm = kc(d->nBm);
            const auto *BtoQ = kc(d->B_to_qm);
            u64 nz = 0; // OR of the words this column stores (transparency sink)
            for (int i = 0; i < k; i++)
            {
                const u64 w = dot_redc_guarded(al.a2, al.neg ? pBm[i] : nBm[i], tb, BtoQ + i * B, B, &d->q_p[i], &d->q_ninv[i], &d->q_rdp[i], small);
                pout[i * N] = w;
                nz |= w;
                __builtin_amdgcn_sched_barrier(0);
            }
            note_nonzero(tflags, cc.item, nz); // (the launcher passes the sink for polynomials 1.. of the product only)
        }

        // fast_floor (rns.cpp:983-1023), optionally preceded by the multiplication by t of
        // evaluator.cpp:432-434: (k + |Bsk|) rows -> |Bsk| rows
        template <int KMAX>
        __global__ __launch_bounds__(kThreads) void fast_floor_kernel(const RnsDev *__restrict__ d,
                                                                      const PrimeDev *__restrict__ primes,
                                                                      const u64 *__restrict__ in, std::size_t in_stride,
                                                                      u64 *__restrict__ out, std::size_t out_stride,
                                                                      std::size_t count, int logn, int mul_t)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k, nB = d->nB;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            u64 t[KMAX];
#pragma unroll
            for (int i = 0; i < KMAX; i++)
                if (i < k)
                {
                    const PrimeDev &Q = primes[d->q_prime[i]];
                    u64 x = pin[i * N];
                    if (mul_t)
                        x = mul_mod(x, d->t, Q.p, Q.cr0, Q.cr1);
                    t[i] = mul_mod(x, d->q_inv[i], Q.p, Q.cr0, Q.cr1);
                }
            for (int j = 0; j < nB; j++)
            {
                const PrimeDev &Bp = primes[d->bsk_prime[j]];
                const u64 conv = dot_mod<KMAX>(t, k, d->q_to_Bsk + j * k, Bp);
                u64 x = pin[(k + j) * N];
                if (mul_t)
                    x = mul_mod(x, d->t, Bp.p, Bp.cr0, Bp.cr1);
                pout[j * N] = mul_mod(x + (Bp.p - conv), d->inv_prod_q_mod_Bsk[j], Bp.p, Bp.cr0, Bp.cr1);
            }
        }

        // Shenoy-Kumaresan tail shared by fastbconv_sk and the fused kernel (rns.cpp:880-922)
        template <int KMAX>
        __device__ __forceinline__ void sk_finish(const RnsDev *d, const PrimeDev *primes, const u64 (&tb)[KMAX + 1],
                                                  u64 in_sk, u64 *pout, std::size_t N)
        {
            const int k = d->k, B = d->B;
            const PrimeDev &Msk = primes[d->bsk_prime[B]];
            u64 lo = 0, hi = 0;
#pragma unroll
            for (int i = 0; i < KMAX + 1; i++)
                if (i < B)
                    mac128(lo, hi, tb[i], d->B_to_msk[i]);
            const u64 conv_sk = barrett_reduce_128(lo, hi, Msk.p, Msk.cr0, Msk.cr1);
            const u64 alpha = mul_mod(conv_sk + (Msk.p - in_sk), d->inv_prod_B_mod_msk, Msk.p, Msk.cr0, Msk.cr1);
            const bool neg = alpha > (Msk.p >> 1);
            for (int i = 0; i < k; i++)
            {
                const PrimeDev &Q = primes[d->q_prime[i]];
                u64 l2 = 0, h2 = 0;
                const u64 *mrow = d->B_to_q + i * B;
#pragma unroll
                for (int a = 0; a < KMAX + 1; a++)
                    if (a < B)
                        mac128(l2, h2, tb[a], mrow[a]);
                const u64 conv = barrett_reduce_128(l2, h2, Q.p, Q.cr0, Q.cr1);
                const u64 pB = d->prod_B_mod_q[i];
                pout[i * N] = neg ? mul_add_mod(pB, Msk.p - alpha, conv, Q.p, Q.cr0, Q.cr1)
                                  : mul_add_mod(Q.p - pB, alpha, conv, Q.p, Q.cr0, Q.cr1);
            }
        }

        // fastbconv_sk (rns.cpp:853-923): |Bsk| rows -> k rows
        template <int KMAX>
        __global__ __launch_bounds__(kThreads) void fastbconv_sk_kernel(const RnsDev *__restrict__ d,
                                                                        const PrimeDev *__restrict__ primes,
                                                                        const u64 *__restrict__ in,
                                                                        std::size_t in_stride, u64 *__restrict__ out,
                                                                        std::size_t out_stride, std::size_t count,
                                                                        int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int B = d->B;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 tb[KMAX + 1];
#pragma unroll
            for (int i = 0; i < KMAX + 1; i++)
                if (i < B)
                {
                    const PrimeDev &Bp = primes[d->bsk_prime[i]];
                    tb[i] = mul_mod(pin[i * N], d->B_inv[i], Bp.p, Bp.cr0, Bp.cr1);
                }
            sk_finish<KMAX>(d, primes, tb, pin[B * N], out + cc.item * out_stride + cc.c, N);
        }

        // fused BEHZ steps (6)-(8) of evaluator.cpp:427-444: (k+|Bsk|) rows -> k rows. The step-by-step form, for k > 32
        __global__ __launch_bounds__(kThreads) void bfv_floor_sk_kernel(const RnsDev *__restrict__ d,
                                                                        const PrimeDev *__restrict__ primes,
                                                                        const u64 *__restrict__ in,
                                                                        std::size_t in_stride, u64 *__restrict__ out,
                                                                        std::size_t out_stride, std::size_t count,
                                                                        int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k, B = d->B;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 t[kMaxModuli];
#pragma unroll
            for (int i = 0; i < kMaxModuli; i++)
                if (i < k)
                {
                    const PrimeDev &Q = primes[d->q_prime[i]];
                    const u64 x = mul_mod(pin[i * N], d->t, Q.p, Q.cr0, Q.cr1);
                    t[i] = mul_mod(x, d->q_inv[i], Q.p, Q.cr0, Q.cr1);
                }
            u64 tb[kMaxModuli + 1];
            u64 in_sk = 0;
#pragma unroll
            for (int j = 0; j < kMaxModuli + 2; j++)
                if (j <= B)
                {
                    const PrimeDev &Bp = primes[d->bsk_prime[j]];
                    const u64 conv = dot_mod<kMaxModuli>(t, k, d->q_to_Bsk + j * k, Bp);
                    const u64 x = mul_mod(pin[(k + j) * N], d->t, Bp.p, Bp.cr0, Bp.cr1);
                    const u64 fl = mul_mod(x + (Bp.p - conv), d->inv_prod_q_mod_Bsk[j], Bp.p, Bp.cr0, Bp.cr1);
                    if (j < B)
                    {
                        if (j < kMaxModuli + 1)
                            tb[j < kMaxModuli + 1 ? j : 0] = mul_mod(fl, d->B_inv[j], Bp.p, Bp.cr0, Bp.cr1);
                    }
                    else
                        in_sk = fl;
                }
            sk_finish<kMaxModuli>(d, primes, tb, in_sk, out + cc.item * out_stride + cc.c, N);
        }

        // divide_and_round_q_last_inplace (rns.cpp:731-775); writes out_rows rows (k-1, or k to mirror the
        // reference's clobbered last row)
        __global__ __launch_bounds__(kThreads) void divround_bfv_kernel(const RnsDev *__restrict__ d,
                                                                        const PrimeDev *__restrict__ primes,
                                                                        const u64 *__restrict__ in,
                                                                        std::size_t in_stride, u64 *__restrict__ out,
                                                                        std::size_t out_stride, std::size_t count,
                                                                        int logn, int out_rows)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            const PrimeDev &L = primes[d->q_prime[k - 1]];
            const u64 half = L.p >> 1;
            const u64 last = barrett_reduce_63(pin[(k - 1) * N] + half, L.p, L.cr1);
            for (int i = 0; i < k - 1; i++)
            {
                const PrimeDev &Q = primes[d->q_prime[i]];
                u64 temp = barrett_reduce_63(last, Q.p, Q.cr1);
                temp = sub_mod(temp, barrett_reduce_63(half, Q.p, Q.cr1), Q.p);
                const u64 v = sub_mod(pin[i * N], temp, Q.p);
                pout[i * N] = mul_mod(v, d->inv_q_last_mod_q[i], Q.p, Q.cr0, Q.cr1);
            }
            if (out_rows == k)
                pout[(k - 1) * N] = last;
        }

        // divide_and_round_q_last_ntt_inplace, part before the forward NTTs (rns.cpp:800-827); `last` is the
        // already inverse-transformed last row and is updated in place like the reference does
        __global__ __launch_bounds__(kThreads) void rescale_pre_kernel(const RnsDev *__restrict__ d,
                                                                       const PrimeDev *__restrict__ primes,
                                                                       u64 *__restrict__ last_row,
                                                                       std::size_t last_stride,
                                                                       u64 *__restrict__ temp, std::size_t temp_stride,
                                                                       std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            u64 *plast = last_row + cc.item * last_stride + cc.c;
            u64 *ptemp = temp + cc.item * temp_stride + cc.c;
            const PrimeDev &L = primes[d->q_prime[k - 1]];
            const u64 half = L.p >> 1;
            const u64 last = barrett_reduce_63(*plast + half, L.p, L.cr1);
            *plast = last;
            for (int i = 0; i < k - 1; i++)
            {
                const PrimeDev &Q = primes[d->q_prime[i]];
                const u64 v = Q.p < L.p ? barrett_reduce_63(last, Q.p, Q.cr1) : last;
                ptemp[i * N] = v + (Q.p - barrett_reduce_63(half, Q.p, Q.cr1));
            }
        }

        // ... and the part after them (rns.cpp:841-849)
        __global__ __launch_bounds__(kThreads) void rescale_post_kernel(const RnsDev *__restrict__ d,
                                                                        const PrimeDev *__restrict__ primes,
                                                                        const u64 *__restrict__ in,
                                                                        std::size_t in_stride,
                                                                        const u64 *__restrict__ temp,
                                                                        std::size_t temp_stride, u64 *__restrict__ out,
                                                                        std::size_t out_stride, std::size_t count,
                                                                        int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * in_stride + cc.c;
            const u64 *ptemp = temp + cc.item * temp_stride + cc.c;
            u64 *pout = out + cc.item * out_stride + cc.c;
            for (int i = 0; i < k - 1; i++)
            {
                const PrimeDev &Q = primes[d->q_prime[i]];
                const u64 v = pin[i * N] + (Q.p << 2) - ptemp[i * N];
                pout[i * N] = mul_mod(v, d->inv_q_last_mod_q[i], Q.p, Q.cr0, Q.cr1);
            }
        }

        inline unsigned blocks_for(std::size_t count, int logn)
        {
            return static_cast<unsigned>(((count << logn) + kThreads - 1) / kThreads);
        }

        // RNSTool::decrypt_scale_and_round (rns.cpp:1070-1126): k rows -> one row of coefficients mod t. The two scalar
        // multiplications before the base conversion are folded into one constant; everything else as written there.
        __global__ __launch_bounds__(kThreads) void decrypt_scale_and_round_kernel(const RnsDev *__restrict__ d,
                                                                                   const PrimeDev *__restrict__ primes,
                                                                                   const u64 *__restrict__ in,
                                                                                   u64 *__restrict__ out,
                                                                                   std::size_t count, int logn)
        {
            Cols cc;
            if (!column(count, logn, cc))
                return;
            const int k = d->k;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const u64 *pin = in + cc.item * (static_cast<std::size_t>(k) * N) + cc.c;
            const u64 t = d->t, gamma = d->dsr_gamma;
            const PrimeDev &G = primes[d->gamma_prime];
            u64 lt = 0, ht = 0, lg = 0, hg = 0;
            for (int i = 0; i < k; i++)
            {
                const u64 qi = primes[d->q_prime[i]].p;
                const u64 y = mulmod_shoup(pin[i * N], d->dsr_scale[i], d->dsr_scale_s[i], qi); // :1076-1082 + :476-485
                mac128(lt, ht, y, d->dsr_to_t[i]);                                             // :487-495
                mac128(lg, hg, y, d->dsr_to_g[i]);
            }
            // reductions mod t (any modulus below 2^61: plain 128-bit remainder) and mod gamma (Barrett)
            const unsigned __int128 st = (static_cast<unsigned __int128>(ht) << 64) | lt;
            u64 vt = static_cast<u64>(st % t);
            u64 vg = barrett_reduce_128(lg, hg, G.p, G.cr0, G.cr1);
            vt = static_cast<u64>((static_cast<unsigned __int128>(vt) * d->dsr_neg_inv_q_t) % t); // :1091-1096
            vg = mul_mod(vg, d->dsr_neg_inv_q_g, G.p, G.cr0, G.cr1);
            u64 r;
            if (vg > (gamma >> 1)) // :1107-1117
            {
                const u64 a = vt + (gamma - vg) % t;
                r = a >= t ? a - t : a;
            }
            else
            {
                const u64 b = vg % t;
                r = vt >= b ? vt - b : vt + t - b;
            }
            if (r) // :1120-1124
                r = static_cast<u64>((static_cast<unsigned __int128>(r) * d->dsr_inv_gamma_t) % t);
            out[cc.item * N + cc.c] = r;
        }
    } // namespace

    namespace
    {
        // The unit kernels are instantiated for row counts rounded up to 4, 8, 16, 32 and 64 (kMaxModuli):
        // f(integral_constant<int, KM>) for the smallest of them that holds k. (The two fused step-by-step kernels run
        // for k > 32 only and have the one extent kMaxModuli.)
        template <class F>
        void dispatch_k_bucket(int k, F &&f)
        {
            static_assert(kMaxModuli == 64, "the largest bucket holds every level");
            dispatch_among<4, 8, 16, 32, 64>(k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : (k <= 32 ? 32 : 64))), f);
        }
    } // namespace

    hipError_t launch_fastbconv_m_tilde(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                        std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        const unsigned grid = blocks_for(count, e.logn);
        ProfScope prof(e, "fastbconv_m_tilde", 0);
        dispatch_k_bucket(h.k, [&](auto km) {
            fastbconv_m_tilde_kernel<decltype(km)::value><<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out,
                                                                                                  out_stride, count, e.logn);
        });
        return hipGetLastError();
    }

    hipError_t launch_sm_mrq(const Engine &e, const RnsDev *d, const RnsDev &, const u64 *in, std::size_t in_stride,
                             u64 *out, std::size_t out_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "sm_mrq", 0);
        sm_mrq_kernel<<<blocks_for(count, e.logn), kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out,
                                                                            out_stride, count, e.logn);
        return hipGetLastError();
    }

    namespace
    {
        // The fused BEHZ kernels' exact-k instances: f(K, S) for the plan's code K = 1 .. 15, S the split the level's
        // tables are packed with (RnsDev::dot_split: 30, else 31). false: the code names the run-time-k kernel.
        template <class F>
        bool dispatch_behz_exact(int code, int dot_split, F &&f)
        {
            return dispatch_int<1, bounds::kBehzExactMaxK>(code, [&](auto k) {
                dispatch_bool(dot_split == 30,
                              [&](auto s30) { f(k, std::integral_constant<int, decltype(s30)::value ? 30 : 31>{}); });
            });
        }
    } // namespace

    bool bfv_lift_can_apply_top(const Engine &e, int k, bool redc_small)
    {
        // (STRICT: the caller also asks ntt_strict_top_done_ok -- only the dense forward schedule starts below the top layer;
        //  the layer itself is the same butterfly on canonical words either way: nothing can wrap in it)
        return redc_small && k >= 1 && k <= bounds::kBehzExactMaxK && e.logn >= 14;
    }

    // the instance code a plan names must be one this level can run (plan_bfv_multiply, pipeline.cpp)
    static bool behz_instance_ok(const RnsDev &h, const BfvMulPlan &plan, int code)
    {
        if (plan.k != h.k || plan.redc_small != (h.redc_small != 0))
            return false;
        if (code == kBehzStepwise)
            return h.k > 32;
        if (code == kBehzGeneric)
            return h.k <= 32;
        return code == h.k && h.redc_small && h.k <= bounds::kBehzExactMaxK && (h.dot_split == 30 || h.dot_split == 31);
    }

    hipError_t launch_bfv_lift(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in, std::size_t in_stride,
                               u64 *out, std::size_t out_stride, std::size_t count, const BfvMulPlan &plan)
    {
        if (!count)
            return hipSuccess;
        const bool top_layer = plan.lift_top;
        if (!behz_instance_ok(h, plan, plan.lift_kernel) || (top_layer && !bfv_lift_can_apply_top(e, h.k, h.redc_small)))
            return hipErrorInvalidValue;
        const unsigned grid = blocks_for(count, top_layer ? e.logn - 1 : e.logn);
        ProfScope prof(e, "bfv_lift", 0);
        if (plan.lift_kernel == kBehzStepwise)
            bfv_lift_kernel<<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out, out_stride, count, e.logn);
        else if (!dispatch_behz_exact(plan.lift_kernel, h.dot_split, [&](auto k, auto split) {
                     dispatch_bool(top_layer, [&](auto top) { // (only the exact-k instances apply the top layer)
                         bfv_lift_exact_kernel<decltype(k)::value, decltype(top)::value, decltype(split)::value>
                             <<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out, out_stride, count, e.logn);
                     });
                 }))
            bfv_lift_guarded_kernel<<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out, out_stride, count,
                                                                            e.logn);
        return hipGetLastError();
    }

    hipError_t launch_fast_floor(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                 std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count, int mul_t)
    {
        if (!count)
            return hipSuccess;
        const unsigned grid = blocks_for(count, e.logn);
        ProfScope prof(e, "fast_floor", 0);
        dispatch_k_bucket(h.k, [&](auto km) {
            fast_floor_kernel<decltype(km)::value><<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out,
                                                                                           out_stride, count, e.logn, mul_t);
        });
        return hipGetLastError();
    }

    hipError_t launch_fastbconv_sk(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        const unsigned grid = blocks_for(count, e.logn);
        ProfScope prof(e, "fastbconv_sk", 0);
        dispatch_k_bucket(h.k, [&](auto km) {
            fastbconv_sk_kernel<decltype(km)::value><<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out,
                                                                                             out_stride, count, e.logn);
        });
        return hipGetLastError();
    }

    hipError_t launch_bfv_floor_sk(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                   const BfvMulPlan &plan)
    {
        if (!count)
            return hipSuccess;
        const int deferred_top = plan.deferred_top;
        if (!behz_instance_ok(h, plan, plan.floor_kernel))
            return hipErrorInvalidValue;
        const unsigned grid = blocks_for(count, e.logn);
        // transparency sink armed for this launch (pipeline.cpp SinkArm: polynomials 1.. of a product): the fused kernel
        // notes non-zero words as it stores them; the step-by-step kernels are followed by the read pass instead
        unsigned *tflags = e.lane().tsink_arm;
        ProfScope prof(e, "bfv_floor_sk", 0);
        if (plan.floor_kernel != kBehzStepwise)
        {
            // (both families have the form that applies the deferred top layer)
            const int mont = deferred_top == 2 ? 1 : 0;
            dispatch_bool(deferred_top != 0, [&](auto top) {
                if (!dispatch_behz_exact(plan.floor_kernel, h.dot_split, [&](auto k, auto split) {
                        bfv_floor_sk_exact_kernel<decltype(k)::value, decltype(top)::value, decltype(split)::value>
                            <<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out, out_stride, count, e.logn,
                                                                     mont, tflags);
                    }))
                    bfv_floor_sk_guarded_kernel<decltype(top)::value><<<grid, kThreads, 0, e.lane().stream>>>(
                        d, e.d_primes, in, in_stride, out, out_stride, count, e.logn, mont, tflags);
            });
            return hipGetLastError();
        }
        if (deferred_top)
            return hipErrorInvalidValue;
        bfv_floor_sk_kernel<<<grid, kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out, out_stride, count, e.logn);
        hipError_t err = hipGetLastError();
        if (err == hipSuccess && tflags)
            err = launch_nonzero_words(e, out, out_stride, static_cast<std::size_t>(h.k) << e.logn, count, tflags);
        return err;
    }

    hipError_t launch_divround_bfv(const Engine &e, const RnsDev *d, const RnsDev &, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                   int out_rows)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "divround_bfv", 0);
        divround_bfv_kernel<<<blocks_for(count, e.logn), kThreads, 0, e.lane().stream>>>(d, e.d_primes, in, in_stride, out,
                                                                                  out_stride, count, e.logn, out_rows);
        return hipGetLastError();
    }

    hipError_t launch_rescale_pre(const Engine &e, const RnsDev *d, const RnsDev &, u64 *last,
                                  std::size_t last_stride, u64 *temp, std::size_t temp_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "rescale_pre", 0);
        rescale_pre_kernel<<<blocks_for(count, e.logn), kThreads, 0, e.lane().stream>>>(d, e.d_primes, last, last_stride,
                                                                                 temp, temp_stride, count, e.logn);
        return hipGetLastError();
    }

    hipError_t launch_rescale_post(const Engine &e, const RnsDev *d, const RnsDev &, const u64 *in,
                                   std::size_t in_stride, const u64 *temp, std::size_t temp_stride, u64 *out,
                                   std::size_t out_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "rescale_post", 0);
        rescale_post_kernel<<<blocks_for(count, e.logn), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, in, in_stride, temp, temp_stride, out, out_stride, count, e.logn);
        return hipGetLastError();
    }
    hipError_t launch_decrypt_scale_and_round(const Engine &e, const RnsDev *d, const RnsDev &, const u64 *in, u64 *out,
                                              std::size_t count)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "decrypt_scale_and_round", 0);
        const std::size_t lanes = count << e.logn;
        decrypt_scale_and_round_kernel<<<static_cast<unsigned>((lanes + kThreads - 1) / kThreads), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, in, out, count, e.logn);
        return hipGetLastError();
    }
} // namespace sealhip
