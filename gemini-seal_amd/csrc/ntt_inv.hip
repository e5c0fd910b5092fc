// ntt_inv.hip -- single-pass inverse NTT for N = 2^14 .. 2^16 (the half-row kernel and its whole-row and quarter-row
// forms, ntt_half.hpp), the streaming top-layer passes, and their launcher.
#include <utility>

#include "ntt_half.hpp"

namespace sealhip
{
    namespace
    {
        // ----------------------------------------------------------------------------------------
        // Single-pass inverse NTT for logn = 14..16: the mirror image of ntt_fwd_half_kernel. The
        // Gentleman-Sande layers on index bits 0..T-1 only pair coefficients inside one half of the row, so
        // a workgroup transforms its half entirely on chip (final arrangement first, then rounds 3, 2, 1,
        // ascending bits) and stores lazy values in [0, 2p). The top layer (gap N/2, with n^{-1} folded
        // in, ntt.cpp:393-402) needs both halves and is applied by ntt_inv_top_kernel, a pure streaming
        // pass (or, inside the pipelines, by the consumer kernel).
        // ---- inverse rounds as stage pipelines (ntt_half.hpp Stage, as ntt_fwd.hip RoundStage / RoundPipe; layers ascend W = 1, 2, 3, 4)
        // Lazy-sum schedule of the inverse (only when the caller accepts any representative of the stored values and every
        // prime of the launch is small enough, select_inv_half): the conditional subtraction of the sum output is dropped
        // on all but two of the T on-chip layers; those two (the middle one and the last) reduce with barrett_lazy
        // instead. Values entering layer l are below 2^shift(l) * p; the difference operand gets that bound added.
        // (the schedule, its worst-case recurrence and the admission predicate live in ntt_bounds.hpp)
        // Round 4: the MODE 1 layers of the lazy schedule (all but two) take the level-2 quotient (devmath.hpp mulhi_apx2,
        // butterflies_inv_apx2): their products land below 4p, which is what the unreduced sum of such a layer is bounded by
        // anyway, so shift(), mode() and the admission predicate are what they were (ntt_bounds.hpp section 1).
        // kInvLazySum: the sparse schedule (two reducing layers; primes with head-room), kInvDense (round 4): the DENSE schedule for primes
        // up to 2^60 -- every third layer and the last reduce their sums with the single-precision quotient estimate, values
        // never pass 16p (ntt_bounds.hpp section 1): the 60-bit Bsk rows of a BFV multiply and ciphertext primes of 56-60 bits
        // no longer pay a conditional subtraction in every butterfly.
        template <int LZ>
        constexpr bool kLazy = LZ == kInvLazySum || LZ == kInvDense;
        template <int T, int LZ = kInvLazySum>
        struct InvLazy
        {
            static constexpr int sched = LZ == kInvDense ? 1 : 0;
            static constexpr int mode(int l)
            {
                return bounds::inv_lazy_mode(T, l, sched);
            }
            static constexpr int shift(int l)
            {
                return bounds::inv_lazy_shift(T, l, sched);
            }
            // what butterflies_inv_hs gets for a reducing layer: Barrett (sparse) or the quotient estimate (dense)
            static constexpr int reduce_mode = LZ == kInvDense ? 3 : 2;
        };
        // Floating-point schedule of the inverse (LZ == kInvFp64, primes below 2^50, inputs below 2p): sums double the bound per
        // layer, so both outputs of layers 1, 5, 9, 13 are brought back to [-p/2, p/2]: 2p -> 4p -> 8p | 0.5p -> p -> 2p ->
        // 4p -> 8p | ...; a difference is at most 8p too, its product below (0.5 + 8p 2^-52) p <= 2.5p. Every magnitude stays
        // at or below 8p < 2^53: exact (devmath.hpp). The last layer's outputs are canonicalised by the store instead.
        // p << shift as a value of its own at every use. The subtraction u - y + addend is a 64-bit v_sub / v_subb pair; the
        // second reads the carry, so its other operand cannot be a scalar register and the compiler keeps the addend's high
        // dword in a VECTOR register -- and, because the same shift recurs in layers far apart, kept it there (or in scratch:
        // three spilled dwords in <16, 1, true>) across whole rounds. An opaque scalar copy per layer ends that live range.
        __device__ __forceinline__ u64 lazy_addend(u64 neg_p, int shift)
        {
            u64 a = (0 - neg_p) << shift;
            asm volatile("" : "+s"(a));
            return a;
        }
        template <int T>
        constexpr bool fp_inv_reduce_after(int layer)
        {
            return bounds::fp_inv_reduce_after_layer(T, layer);
        }
        template <int T, int R, bool UNIFORM, int K, int LZ = kInvExact>
        struct RoundStageInv : Stage<T, R, 1 + K / kStagesPerLayer, (K % kStagesPerLayer) * kIL, UNIFORM, LZ == kInvFp64>
        {
            static constexpr int W = 1 + K / kStagesPerLayer;
            using S = Stage<T, R, W, (K % kStagesPerLayer) * kIL, UNIFORM, LZ == kInvFp64>;
            using S::bit;
            using S::slot;
            static constexpr int layer = (T - 12) + 4 * (3 - R) + (W - 1); // 0-based on-chip layer index
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64 (&w)[kIL], const u64 (&ws)[kIL], u64 two_p,
                                                       u64 neg_p, u64 rdp, ZeroPairs &zp)
            {
                if constexpr (LZ == kInvFp64)
                {
                    const double pd = fp_of(two_p), pinv = fp_of(neg_p);
#pragma unroll
                    for (int j = 0; j < kIL; j++)
                    {
                        fp_butterfly_inv(x[slot(j)], x[slot(j) | bit], w[j], pd, pinv);
                        if constexpr (fp_inv_reduce_after<T>(layer))
                        {
                            x[slot(j)] = fp_bits(fp_reduce(fp_of(x[slot(j)]), pd, pinv));
                            x[slot(j) | bit] = fp_bits(fp_reduce(fp_of(x[slot(j) | bit]), pd, pinv));
                        }
                    }
                    return;
                }
                u64 u[kIL], y[kIL];
#pragma unroll
                for (int j = 0; j < kIL; j++)
                {
                    u[j] = x[slot(j)];
                    y[j] = x[slot(j) | bit];
                }
                if constexpr (kLazy<LZ> && InvLazy<T, LZ>::mode(layer) == 1)
                    butterflies_inv_apx2<UNIFORM, kIL>(u, y, w, ws, neg_p, lazy_addend(neg_p, InvLazy<T, LZ>::shift(layer)), zp.z);
                else if constexpr (kLazy<LZ>)
                    butterflies_inv_hs<UNIFORM, kIL, InvLazy<T, LZ>::mode(layer) == 1 ? 1 : InvLazy<T, LZ>::reduce_mode>(
                        u, y, w, ws, neg_p, lazy_addend(neg_p, InvLazy<T, LZ>::shift(layer)), rdp);
                else
                    butterflies_inv_hs<UNIFORM, kIL>(u, y, w, ws, neg_p, two_p); // BackwardLazy, ntt.cpp:265-272
#pragma unroll
                for (int j = 0; j < kIL; j++)
                {
                    x[slot(j)] = u[j];
                    x[slot(j) | bit] = y[j];
                }
            }
        };
        template <int T, int R, bool UNIFORM, int LZ, int K = 0, int NLAYERS = 4>
        struct RoundPipeInv
        {
            static constexpr int NST = NLAYERS * (16 / kIL); // (NLAYERS = 3: the whole-row form applies the round's last layer itself)
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64 (&w)[kIL], const u64 (&ws)[kIL],
                                                       const u64 *__restrict__ tw, int jb, int N, u64 two_p, u64 neg_p,
                                                       u64 rdp, ZeroPairs &zp)
            {
                u64 wn[kIL], wsn[kIL];
                if constexpr (K + 1 < NST)
                    RoundStageInv<T, R, UNIFORM, K + 1, LZ>::load(wn, wsn, tw, jb, N);
                __builtin_amdgcn_sched_barrier(0);
                RoundStageInv<T, R, UNIFORM, K, LZ>::run(x, w, ws, two_p, neg_p, rdp, zp);
                if constexpr (K + 1 < NST)
                    RoundPipeInv<T, R, UNIFORM, LZ, K + 1, NLAYERS>::run(x, wn, wsn, tw, jb, N, two_p, neg_p, rdp, zp);
            }
        };

        // first phase of the inverse: the 2^f consecutive coefficients that share the filler slot bits G run their low
        // layers (index bits 0 .. f-1, ascending); group twiddles in the order used: layer W = 0 (2^(f-1) entries),
        // W = 1, ..., W = f-1 (1 entry): ntt_half.hpp GroupTw. All coefficients are loaded before (one exposed latency),
        // twiddles are requested one stage (FinalStage<T>::SG groups) ahead.
        template <int T, int G, int LZ>
        __device__ __forceinline__ void h_first_group_regs(u64 (&x)[32], const u64x2 *tg, u64 neg_p, u64 two_p, u64 rdp, ZeroPairs &zp)
        {
            constexpr int f = T - 12;
            static_assert(LZ != kInvLazySum || f - 1 < bounds::inv_lazy_r1(T), "sparse schedule: the first layers are never the reducing ones");
            int base = 0;
#pragma unroll
            for (int W = 0; W < f; W++)
            {
                const int bit = 1 << W;
                const u64 addend = kLazy<LZ> ? lazy_addend(neg_p, InvLazy<T, LZ>::shift(W)) : two_p; // layer index = W
#pragma unroll
                for (int e = 0; e < (1 << f); e++)
                {
                    if (e & bit)
                        continue;
                    const int s = (G << f) | e;
                    const u64x2 Wv = tg[base + (e >> (W + 1))];
                    if constexpr (LZ == kInvFp64)
                    {
                        const double pd = fp_of(two_p), pinv = fp_of(neg_p);
                        fp_butterfly_inv(x[s], x[s | bit], Wv.x, pd, pinv);
                        if (fp_inv_reduce_after<T>(W))
                        {
                            x[s] = fp_bits(fp_reduce(fp_of(x[s]), pd, pinv));
                            x[s | bit] = fp_bits(fp_reduce(fp_of(x[s | bit]), pd, pinv));
                        }
                        continue;
                    }
                    const u64 u = x[s], v = x[s | bit];
                    u64 tt = u + v;
                    if (!kLazy<LZ>)
                        tt = tt >= two_p ? tt - two_p : tt;
                    else if (InvLazy<T, LZ>::mode(W) != 1) // (dense schedule at N = 2^16: its layer 2 is one of the first three)
                        tt = reduce_small_quot(tt, __uint_as_float(static_cast<unsigned>(rdp)), neg_p);
                    x[s] = tt;
                    // (W is a constant after unrolling: the branch folds)
                    // (level-2 quotient in the non-reducing layers of the first round too -- sparse schedule only: the dense
                    //  plain instances spill four dwords with the pairs live here)
                    if (LZ == kInvLazySum && InvLazy<T, kInvLazySum>::mode(W) == 1)
                        x[s | bit] = mulmod_lazy_apx2<false>(u - v + addend, Wv.x, Wv.y, neg_p, zp.z[(e >> (W + 1)) & 1]);
                    else
                        x[s | bit] = mulmod_lazy_hs<false>(u - v + addend, Wv.x, Wv.y, neg_p);
                }
                base += 1 << (f - 1 - W);
            }
        }
        template <int T, int ST, int LZ, int I = 0>
        struct FirstStage
        {
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64x2 *tg, u64 neg_p, u64 two_p, u64 rdp, ZeroPairs &zp)
            {
                h_first_group_regs<T, ST * FinalStage<T>::SG + I, LZ>(x, tg + I * FinalStage<T>::NTW, neg_p, two_p, rdp, zp);
                if constexpr (I + 1 < FinalStage<T>::SG)
                    FirstStage<T, ST, LZ, I + 1>::run(x, tg, neg_p, two_p, rdp, zp);
            }
        };
        // AHEAD: the next stage's twiddles are requested before this stage is computed (two stages of twiddles live: 48
        // registers at f = 2). Off at f = 3 (they do not fit), in the lazy fused-tensor instances, which come out of their
        // products at the register cap, and in the exact whole-row instance (the request then follows the stage: its latency is
        // exposed once per stage; round 3: with this, fresh_tid and lazy_addend no single-pass kernel spills any more).
        template <int T, int ST, int LZ, bool AHEAD = FinalStage<T>::PIPE>
        struct FirstPipe
        {
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64x2 *cur, const u64 *__restrict__ tw, int jb,
                                                       int N, u64 neg_p, u64 two_p, u64 rdp, ZeroPairs &zp)
            {
                u64x2 next[FinalStage<T>::SG * FinalStage<T>::NTW];
                if constexpr (ST + 1 < FinalStage<T>::NS && AHEAD)
                    StageTw<T, ST + 1, false, LZ == kInvFp64>::load(next, tw, jb, N);
                __builtin_amdgcn_sched_barrier(0);
                FirstStage<T, ST, LZ>::run(x, cur, neg_p, two_p, rdp, zp);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (ST + 1 < FinalStage<T>::NS && !AHEAD)
                    StageTw<T, ST + 1, false, LZ == kInvFp64>::load(next, tw, jb, N);
                if constexpr (ST + 1 < FinalStage<T>::NS)
                    FirstPipe<T, ST + 1, LZ, AHEAD>::run(x, next, tw, jb, N, neg_p, two_p, rdp, zp);
            }
        };

        // ---- ciphertext tensor product formed on load (evaluator.cpp:376-420 for two size-2 operands): output polynomial I
        // of an item is c_0 = a_0 b_0, c_1 = a_0 b_1 + a_1 b_0, c_2 = a_1 b_1 over the forward-transformed rows X[s] (s = 0, 1:
        // a; s = 2, 3: b) of the same prime. The reference reduces every product with Barrett and adds with one conditional
        // subtraction; its results are canonical residues that only feed this inverse transform, so any representative of
        // the same residue class below 2p gives the same final output. Here: carry-free 128-bit sum of products (operands
        // below 2^61) and ONE Montgomery reduction, which leaves the factor 2^-64; the consumer's constants carry 2^64
        // (RnsDev::floor_*_topM). The operands must make that reduction land below 2p: below 4p for primes under 2^59
        // (what the lazy forward transform stores), below 2p for primes up to 2^61 -- the wrapped 60-bit Bsk rows hold
        // arbitrary 64-bit words (which dyadic_product_coeffmod accepts, polyarithsmallmod.cpp:63-117), so the forward
        // launch that produces them reduces every word with barrett_lazy before it stores it (kNttReduceOut).
        struct DyadicSrc
        {
            const u64 *x;                        // forward-transformed operands: item-major, 4 polynomials of kb rows
            std::size_t item_stride, poly_stride; // words
            int kb;
            // Evaluator::square (evaluator.cpp:560-702): TWO polynomials per item; c_0 = x_0^2, c_1 = x_0 x_1 added to itself
            // (:650-651), c_2 = x_1^2
            int square;
        };
        // IL words in lock step: t_j = (sum of NP products of operands below 2^61) * 2^-64 mod p as a Montgomery reduction,
        // t_j < sum / 2^64 + p. 4 multiplier instructions per product (the operands' upper halves are below 2^29, so the
        // middle sums cannot overflow), 3 for m = lo * (-p^-1) mod 2^64, 4 + one carry for floor(m p / 2^64).
        // Program-ordered (volatile) like the butterflies: consecutive instructions belong to different words, and the
        // carry of the high product is read IL >= 3 instructions after it is written.
        template <int IL, int NP>
        __device__ __forceinline__ void dyadic_redc(u64 (&t)[IL], const u64 (&a)[NP][IL], const u64 (&b)[NP][IL], u64 p, u64 ninv)
        {
            static_assert(IL >= 3, "the carry of the high product is read IL instructions after its producer");
            typedef unsigned __int128 u128;
            u64 P0[NP][IL], M[IL], H[IL], cy[IL] = {};
#pragma unroll
            for (int q = 0; q < NP; q++)
            {
#pragma unroll
                for (int j = 0; j < IL; j++)
                    P0[q][j] = mul64v<false>(static_cast<u32>(a[q][j]), static_cast<u32>(b[q][j]), cy[j]);
#pragma unroll
                for (int j = 0; j < IL; j++)
                    M[j] = q == 0 ? mul64v<false>(static_cast<u32>(a[q][j]), static_cast<u32>(b[q][j] >> 32), cy[j])
                                  : mad64v<false>(static_cast<u32>(a[q][j]), static_cast<u32>(b[q][j] >> 32), M[j], cy[j]);
#pragma unroll
                for (int j = 0; j < IL; j++)
                    M[j] = mad64v<false>(static_cast<u32>(a[q][j] >> 32), static_cast<u32>(b[q][j]), M[j], cy[j]);
#pragma unroll
                for (int j = 0; j < IL; j++)
                    H[j] = q == 0 ? mul64v<false>(static_cast<u32>(a[q][j] >> 32), static_cast<u32>(b[q][j] >> 32), cy[j])
                                  : mad64v<false>(static_cast<u32>(a[q][j] >> 32), static_cast<u32>(b[q][j] >> 32), H[j], cy[j]);
            }
            u64 lo[IL], hi[IL], m[IL], A[IL], B[IL], carry[IL], mh[IL];
            u32 cb[IL];
            const u32 p0 = static_cast<u32>(p), p1 = static_cast<u32>(p >> 32);
#pragma unroll
            for (int j = 0; j < IL; j++)
            {
                u128 X = (static_cast<u128>(H[j]) << 64) + (static_cast<u128>(M[j]) << 32);
#pragma unroll
                for (int q = 0; q < NP; q++)
                    X += P0[q][j];
                lo[j] = static_cast<u64>(X);
                hi[j] = static_cast<u64>(X >> 64);
                m[j] = lo[j] * ninv;
            }
#pragma unroll
            for (int j = 0; j < IL; j++)
                A[j] = mad64v<true>(static_cast<u32>(m[j] >> 32), p0, static_cast<u64>(__umulhi(static_cast<u32>(m[j]), p0)), cy[j]);
#pragma unroll
            for (int j = 0; j < IL; j++)
                asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(B[j]), "=s"(carry[j]) : "v"(static_cast<u32>(m[j])), "s"(p1), "v"(A[j]));
#pragma unroll
            for (int j = 0; j < IL; j++)
                asm volatile("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(cb[j]) : "s"(carry[j]));
#pragma unroll
            for (int j = 0; j < IL; j++)
                mh[j] = mad64v<true>(static_cast<u32>(m[j] >> 32), p1,
                                     static_cast<u64>(static_cast<u32>(B[j] >> 32)) | (static_cast<u64>(cb[j]) << 32), cy[j]);
#pragma unroll
            for (int j = 0; j < IL; j++)
                t[j] = hi[j] + mh[j] + (lo[j] != 0); // lo + m p is a multiple of 2^64: its low word carries iff lo != 0
        }
        // The inverse starts in arrangement 4 (runs of 2^f consecutive coefficients per lane) and loads its rows that way:
        // 16-byte pieces at a 2^f * 8-byte stride per instruction for f >= 2, the mirror image of the store pattern at
        // ntt_fwd.hip kStoreExchange. Loading in arrangement 1 and moving to arrangement 4 through the LDS measured no gain
        // (profiles/r02/ntt_store_pattern.txt): the second load instruction of a line hits in the CU's L1.

        // the half row's 32 words per lane, arrangement 4, as products of two (c_0, c_2) or four (c_1) input rows
        // SAME: b is a (a square: one load). TWICE: the product added to itself, t + t below 4p brought back below 2p with
        // one conditional subtraction (the reference's add_poly_coeffmod of the product with itself: same residue).
        template <int T, bool SAME = false, bool TWICE = false>
        __device__ __forceinline__ void h_load_dyadic2(u64 (&x)[32], const u64 *__restrict__ a, const u64 *__restrict__ b,
                                                       int jloc, u64 p, u64 ninv)
        {
#pragma unroll
            for (int batch = 0; batch < 4; batch++)
            {
                ulonglong2 va[4], vb[4];
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int idx = jloc + Arr<T, 4>::slot_index((batch * 4 + i) * 2);
                    va[i] = *reinterpret_cast<const ulonglong2 *>(a + idx);
                    if constexpr (SAME)
                        vb[i] = va[i];
                    else
                        vb[i] = *reinterpret_cast<const ulonglong2 *>(b + idx);
                }
#pragma unroll
                for (int g = 0; g < 2; g++)
                {
                    const u64 aa[1][4] = { { va[2 * g].x, va[2 * g].y, va[2 * g + 1].x, va[2 * g + 1].y } };
                    const u64 bb[1][4] = { { vb[2 * g].x, vb[2 * g].y, vb[2 * g + 1].x, vb[2 * g + 1].y } };
                    u64 t[4];
                    dyadic_redc<4, 1>(t, aa, bb, p, ninv);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                    {
                        if constexpr (TWICE)
                        {
                            const u64 d = t[j] << 1, two_p = p << 1; // t below 2p <= 2^62
                            t[j] = d >= two_p ? d - two_p : d;
                        }
                        x[(batch * 4 + 2 * g) * 2 + j] = t[j];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        template <int T>
        __device__ __forceinline__ void h_load_dyadic4(u64 (&x)[32], const u64 *__restrict__ a0, const u64 *__restrict__ b1,
                                                       const u64 *__restrict__ a1, const u64 *__restrict__ b0, int jloc, u64 p,
                                                       u64 ninv)
        {
#pragma unroll
            for (int batch = 0; batch < 8; batch++)
            {
                ulonglong2 v0[2], v1[2], v2[2], v3[2];
#pragma unroll
                for (int i = 0; i < 2; i++)
                {
                    const int idx = jloc + Arr<T, 4>::slot_index((batch * 2 + i) * 2);
                    v0[i] = *reinterpret_cast<const ulonglong2 *>(a0 + idx);
                    v1[i] = *reinterpret_cast<const ulonglong2 *>(b1 + idx);
                    v2[i] = *reinterpret_cast<const ulonglong2 *>(a1 + idx);
                    v3[i] = *reinterpret_cast<const ulonglong2 *>(b0 + idx);
                }
                const u64 aa[2][4] = { { v0[0].x, v0[0].y, v0[1].x, v0[1].y }, { v2[0].x, v2[0].y, v2[1].x, v2[1].y } };
                const u64 bb[2][4] = { { v1[0].x, v1[0].y, v1[1].x, v1[1].y }, { v3[0].x, v3[0].y, v3[1].x, v3[1].y } };
                u64 t[4];
                dyadic_redc<4, 2>(t, aa, bb, p, ninv);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    x[batch * 4 + j] = t[j];
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // WHOLE: the same workgroup shape (2^T coefficients, T = LOGN - 1) applied to a whole row of a ring of 2^T coefficients:
        // one workgroup per row, all T layers on chip -- the last of them is the row's top layer (BackwardLazyLast with
        // n^-1 folded in, ntt.cpp:274-281) -- so the standalone inverse is ONE launch that reads and writes the row once,
        // instead of the half-row kernel plus the streaming top-layer pass. All three arithmetic forms, N = 2^14 and 2^15.
        // QUARTER (round 4): the same shape applied to a QUARTER of a row of a ring of 2^(T + 2) coefficients -- for N = 2^16, where a
        // half row is 1024 lanes and the whole register file of a CU (one workgroup per CU, phases that cannot overlap: 0.38 FP64 /
        // 0.30 integer of the roofline), the N = 2^15 shape on quarter rows keeps two workgroups per CU (0.51 / 0.40 on the same
        // bytes, profiles/r04/n65536_quarter_row_projection.txt). It finishes index bits 0 .. T - 1 = 0 .. 13; the two layers
        // above (gap N/4 and the top layer, n^-1 folded in) are ntt_inv_top2_kernel's, one streaming radix-4 pass.
        template <int LOGN, int LZ, bool DY, bool WHOLE = false, bool QUARTER = false>
        __global__ __launch_bounds__(1 << (LOGN - 6), 4) void ntt_inv_half_kernel(u64 *__restrict__ data,
                                                                                  const PrimeDev *__restrict__ primes,
                                                                                  RowMap map, std::size_t nrows,
                                                                                  std::size_t chunk,
                                                                                  const u64 *__restrict__ src,
                                                                                  std::size_t src_poly_stride,
                                                                                  LiveSlots live, DyadicSrc dy,
                                                                                  int canonical = 0)
        {
            static_assert(!WHOLE || !DY, "whole-row form: plain transforms");
            static_assert(!QUARTER || (!DY && !WHOLE), "quarter-row form: plain transforms");
            constexpr int T = LOGN - 1;
            constexpr int LOGR = WHOLE ? T : (QUARTER ? T + 2 : LOGN); // log2 of the row length
            constexpr int N = 1 << LOGR;
            extern __shared__ u64 lds[];
            const int wave_base = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) & ~63); // (see fresh_tid)
            int half = 0, position;
            std::size_t poly;
            if constexpr (DY)
            {
                // The three output polynomials of one (item, prime) read the same four input rows (c_0: a_0 b_0, c_1: all
                // four, c_2: a_1 b_1): enumerate them next to each other -- v = (prime position, item, output) -- so that the six
                // workgroups run on one XCD at the same time and every input half row is fetched from HBM once and found in
                // that XCD's L2 by its second reader (prime-major as before: the twiddle tables stay L2-resident).
                // live.slot[] is sorted by slot = I * kb + r, i.e. three runs of the same nr prime rows.
                const unsigned xcd = blockIdx.x & 7u;
                const std::size_t slot = blockIdx.x >> 3, npolys = nrows / map.rows;
                half = static_cast<int>(slot & 1);
                const std::size_t v = static_cast<std::size_t>(xcd) * chunk + (slot >> 1);
                if ((slot >> 1) >= chunk || v >= npolys * static_cast<std::size_t>(live.n))
                    return;
                const int nr = live.n / 3;
                const std::size_t pr = v / 3;
                position = static_cast<int>(v - pr * 3) * nr + static_cast<int>(pr / npolys);
                poly = pr % npolys;
            }
            // one, two or four workgroups per live row; `half` counts quarters in the quarter-row form (gbase = half << T)
            else if (!block_place<WHOLE ? 0 : (QUARTER ? 2 : 1)>(blockIdx.x, nrows / map.rows, live.n, chunk, poly, position, half))
                return;
            const std::size_t row = poly * map.rows + live.slot[position];
            const unsigned short pid = map.prime[row % map.rows];
            const PrimeDev P = primes[pid];
            constexpr bool FP = LZ == kInvFp64; // two_p / neg_p then carry the bits of p and 1/p as doubles (see fp_reduce_all)
            static_assert(!FP || !DY, "the floating-point instance serves plain half transforms only");
            const u64 p = P.p, two_p = FP ? fp_bits(P.p_d) : P.two_p;
            const u64 *tw = FP ? reinterpret_cast<const u64 *>(P.inv_d) : P.inv;
            const int gbase = half << T;
            u64 *halfp = data + (row << LOGR) + gbase;
            // optional out-of-place input (polynomial-strided rows of another buffer): saves a copy kernel
            const u64 *inp = src ? src + (row / map.rows) * src_poly_stride + ((row % map.rows) << LOGR) + gbase : halfp;
            u64 x[32];
            const u64 neg_p = FP ? fp_bits(P.pinv_d) : 0 - p;
            // what the reducing layers of the lazy schedules read: floor(2^64 / p) (sparse: Barrett) or the bits of the
            // single-precision quotient constant (dense)
            const u64 rdp = LZ == kInvLazySum ? P.rdp : (LZ == kInvDense ? static_cast<u64>(__float_as_uint(small_quot_const(p))) : 0);
            {
                // every coefficient of the half row first (16 x 16 bytes per lane in flight at once), the twiddles of
                // the first stage with them
                // (jl: the loads' own copy of the lane's index, see fresh_tid)
                const int jloc = Arr<T, 4>::tid_index(fresh_tid(wave_base)), jl = Arr<T, 4>::tid_index(fresh_tid(wave_base));
                u64x2 tg0[FinalStage<T>::SG * FinalStage<T>::NTW];
                if constexpr (!DY)
                    StageTw<T, 0, false, LZ == kInvFp64>::load(tg0, tw, gbase + jloc, N);
                if constexpr (DY)
                {
                    // map.rows = 3 * kb: slot = I * kb + r selects the output polynomial I and the prime row r
                    const int slot = live.slot[position], I = slot / dy.kb, r = slot - I * dy.kb;
                    const u64 *xr = dy.x + poly * dy.item_stride + (static_cast<std::size_t>(r) << LOGN) + gbase;
                    const std::size_t ps = dy.poly_stride;
                    if (dy.square) // (launch-uniform) two polynomials per item
                    {
                        if (I == 1)
                            h_load_dyadic2<T, false, true>(x, xr, xr + ps, jl, p, P.ninv);
                        else
                            h_load_dyadic2<T, true>(x, xr + (I >> 1) * ps, nullptr, jl, p, P.ninv);
                    }
                    else if (I == 1) // block-uniform
                        h_load_dyadic4<T>(x, xr, xr + 3 * ps, xr + ps, xr + 2 * ps, jl, p, P.ninv);
                    else if (I == 0)
                        h_load_dyadic2<T>(x, xr, xr + 2 * ps, jl, p, P.ninv);
                    else
                        h_load_dyadic2<T>(x, xr + ps, xr + 3 * ps, jl, p, P.ninv);
                    // (the first stage's twiddles only now: held across the products they cost 24 registers of scratch)
                    StageTw<T, 0, false, LZ == kInvFp64>::load(tg0, tw, gbase + jloc, N);
                }
                else
                {
#pragma unroll
                    for (int s = 0; s < 32; s += 2)
                    {
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(inp + jl + Arr<T, 4>::slot_index(s));
                        x[s] = FP ? fp_bits(fp_from_u64(v.x)) : v.x; // (inputs below 2p < 2^52)
                        x[s + 1] = FP ? fp_bits(fp_from_u64(v.y)) : v.y;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                ZeroPairs zp1; // (devmath.hpp mulhi_apx2: the first round's own pairs, written here, dead after it)
                if constexpr (LZ == kInvLazySum)
                    zp1.init();
                FirstPipe<T, 0, LZ, FinalStage<T>::PIPE && !(DY && kLazy<LZ>) && !(WHOLE && LZ == kInvExact)>::run(x, tg0, tw, gbase + jloc, N, neg_p,
                                                                                                         two_p, rdp, zp1);
            }
            const int jb3 = gbase + Arr<T, 3>::tid_index(fresh_tid(wave_base));
            u64 w0[kIL], ws0[kIL];
            RoundStageInv<T, 3, false, 0, LZ>::load(w0, ws0, tw, jb3, N); // lands while the exchange runs
            __builtin_amdgcn_sched_barrier(0);
            h_exchange<T, 4, 3>(x, lds, fresh_tid(wave_base));
            ZeroPairs zp; // (devmath.hpp mulhi_apx2; written again where each phase starts)
            if constexpr (kLazy<LZ>)
                zp.init();
            RoundPipeInv<T, 3, false, LZ>::run(x, w0, ws0, tw, jb3, N, two_p, neg_p, rdp, zp);
            const int jb2 = gbase + Arr<T, 2>::tid_index(fresh_tid(wave_base));
            RoundStageInv<T, 2, false, 0, LZ>::load(w0, ws0, tw, jb2, N);
            __builtin_amdgcn_sched_barrier(0);
            h_exchange<T, 3, 2>(x, lds, fresh_tid(wave_base));
            if constexpr (kLazy<LZ>)
                zp.init();
            RoundPipeInv<T, 2, false, LZ>::run(x, w0, ws0, tw, jb2, N, two_p, neg_p, rdp, zp);
            RoundStageInv<T, 1, true, 0, LZ>::load(w0, ws0, tw, gbase, N); // block-uniform twiddles -> scalar loads
            h_exchange<T, 2, 1>(x, lds, fresh_tid(wave_base));
            if constexpr (kLazy<LZ>)
                zp.init();
            if constexpr (WHOLE)
            {
                RoundPipeInv<T, 1, true, LZ, 0, 3>::run(x, w0, ws0, tw, gbase, N, two_p, neg_p, rdp, zp);
                // the row's top layer: slot bit 4 of arrangement 1 is index bit T - 1
                if constexpr (FP)
                {
                    // (inputs at most 4p in magnitude)
                    const double pd = fp_of(two_p), pinv = fp_of(neg_p);
                    const double c_sum = static_cast<double>(P.inv_n), c_diff = static_cast<double>(P.inv_n_w);
#pragma unroll
                    for (int s2 = 0; s2 < 16; s2++)
                    {
                        const double u = fp_of(x[s2]), v = fp_of(x[s2 | 16]);
                        x[s2] = fp_bits(fp_mulmod(u + v, c_sum, pd, pinv));
                        x[s2 | 16] = fp_bits(fp_mulmod(u - v, c_diff, pd, pinv));
                    }
                }
                else
                {
                    // BackwardLazyLast as ntt_inv_top_kernel applies it; with lazy sums the operands are below
                    // 2^shift(T - 1) p, so that multiple of p keeps the difference non-negative
                    const u64 addend = kLazy<LZ> ? (0 - neg_p) << InvLazy<T, LZ>::shift(T - 1) : two_p;
#pragma unroll
                    for (int s2 = 0; s2 < 16; s2++)
                    {
                        const u64 u = x[s2], v = x[s2 | 16];
                        u64 tt = u + v;
                        if (LZ == kInvExact)
                            tt = tt >= two_p ? tt - two_p : tt;
                        u64 a0 = mulmod_lazy_hs<true>(tt, P.inv_n, P.inv_n_shoup, neg_p);
                        u64 a1 = mulmod_lazy_hs<true>(u - v + addend, P.inv_n_w, P.inv_n_w_shoup, neg_p);
                        if (canonical)
                        {
                            a0 = a0 >= p ? a0 - p : a0;
                            a1 = a1 >= p ? a1 - p : a1;
                        }
                        x[s2] = a0;
                        x[s2 | 16] = a1;
                    }
                }
            }
            else
                RoundPipeInv<T, 1, true, LZ>::run(x, w0, ws0, tw, gbase, N, two_p, neg_p, rdp, zp);
            {
                const int jb = Arr<T, 1>::tid_index(fresh_tid(wave_base));
#pragma unroll
                for (int s = 0; s < 32; s += 2)
                {
                    if constexpr (FP) // canonical residues: below 2p as the consumers of the lazy form expect, and exact
                        store_nt(halfp + jb + Arr<T, 1>::slot_index(s), fp_to_u64(fp_canonical(fp_of(x[s]), fp_of(two_p), fp_of(neg_p))),
                                 fp_to_u64(fp_canonical(fp_of(x[s + 1]), fp_of(two_p), fp_of(neg_p))));
                    else
                        store_nt(halfp + jb + Arr<T, 1>::slot_index(s), x[s], x[s + 1]);
                }
            }
        }

        // top inverse layer (gap N/2): x0 = (u+v)*n^-1, x1 = (u-v+2p)*(w*n^-1)  (BackwardLazyLast, ntt.cpp:274-281)
        __global__ __launch_bounds__(256) void ntt_inv_top_kernel(u64 *__restrict__ data,
                                                                  const PrimeDev *__restrict__ primes, RowMap map,
                                                                  int logn, std::size_t npairs, int flags)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t half = static_cast<std::size_t>(1) << (logn - 1);
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs; i += stride)
            {
                // i enumerates 16-byte pairs of the lower halves: row = i / (N/4), pair inside the half = i % (N/4)
                const std::size_t row = i >> (logn - 2);
                const std::size_t off = (i & ((half >> 1) - 1)) * 2;
                const unsigned short pid = map.prime[row % map.rows];
                if (pid == kSkipRow)
                    continue;
                const PrimeDev &P = primes[pid];
                const u64 p = P.p, two_p = P.two_p;
                u64 *lo = data + (row << logn) + off;
                u64 *hi = lo + half;
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(lo);
                const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(hi);
                ulonglong2 r0, r1;
                u64 t0 = a.x + b.x, t1 = a.y + b.y;
                t0 = t0 >= two_p ? t0 - two_p : t0;
                t1 = t1 >= two_p ? t1 - two_p : t1;
                r0.x = mulmod_lazy(t0, P.inv_n, P.inv_n_shoup, p);
                r0.y = mulmod_lazy(t1, P.inv_n, P.inv_n_shoup, p);
                r1.x = mulmod_lazy(a.x - b.x + two_p, P.inv_n_w, P.inv_n_w_shoup, p);
                r1.y = mulmod_lazy(a.y - b.y + two_p, P.inv_n_w, P.inv_n_w_shoup, p);
                if (flags & kNttCanonical)
                {
                    r0.x = r0.x >= p ? r0.x - p : r0.x;
                    r0.y = r0.y >= p ? r0.y - p : r0.y;
                    r1.x = r1.x >= p ? r1.x - p : r1.x;
                    r1.y = r1.y >= p ? r1.y - p : r1.y;
                }
                *reinterpret_cast<ulonglong2 *>(lo) = r0;
                *reinterpret_cast<ulonglong2 *>(hi) = r1;
            }
        }

        // The two layers a quarter-row inverse leaves undone, as one streaming pass (N = 2^16): the layer on index bit logn - 2
        // (gap N/4: BackwardLazy, ntt.cpp:265-272, twiddles (N + j) >> (logn - 1) = entries 2 and 3 of the table for the lower and
        // the upper pair) and the top layer (BackwardLazyLast with n^-1 folded in, :274-281), on the four words
        // (j, j + N/4, j + N/2, j + 3N/4) of a row -- the reference's operations in the reference's order, so the `_lazy`
        // entry keeps its representatives. One lane per 16-byte pair of the first quarter.
        __global__ __launch_bounds__(256) void ntt_inv_top2_kernel(u64 *__restrict__ data, const PrimeDev *__restrict__ primes,
                                                                   RowMap map, int logn, std::size_t nitems, int flags)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t quarter = static_cast<std::size_t>(1) << (logn - 2);
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < nitems; i += stride)
            {
                const std::size_t row = i >> (logn - 3); // N/8 pairs per row
                const std::size_t off = (i & ((quarter >> 1) - 1)) * 2;
                const unsigned short pid = map.prime[row % map.rows];
                if (pid == kSkipRow)
                    continue;
                const PrimeDev &P = primes[pid];
                const u64 p = P.p, two_p = P.two_p;
                const u64x2 WA = ((tw_global_t)P.inv)[2], WB = ((tw_global_t)P.inv)[3];
                u64 *q0 = data + (row << logn) + off;
                ulonglong2 x[4], y[4];
#pragma unroll
                for (int r = 0; r < 4; r++)
                    x[r] = *reinterpret_cast<const ulonglong2 *>(q0 + r * quarter);
                const auto lazy_pair = [&](u64 u, u64 v, u64 w, u64 ws, u64 &s, u64 &d) { // BackwardLazy
                    u64 tt = u + v;
                    s = tt >= two_p ? tt - two_p : tt;
                    d = mulmod_lazy(u - v + two_p, w, ws, p);
                };
                const auto last_pair = [&](u64 u, u64 v, u64 &lo, u64 &hi) { // BackwardLazyLast
                    u64 tt = u + v;
                    tt = tt >= two_p ? tt - two_p : tt;
                    lo = mulmod_lazy(tt, P.inv_n, P.inv_n_shoup, p);
                    hi = mulmod_lazy(u - v + two_p, P.inv_n_w, P.inv_n_w_shoup, p);
                    if (flags & kNttCanonical)
                    {
                        lo = lo >= p ? lo - p : lo;
                        hi = hi >= p ? hi - p : hi;
                    }
                };
                u64 s01, d01, s23, d23;
                lazy_pair(x[0].x, x[1].x, WA.x, WA.y, s01, d01);
                lazy_pair(x[2].x, x[3].x, WB.x, WB.y, s23, d23);
                last_pair(s01, s23, y[0].x, y[2].x);
                last_pair(d01, d23, y[1].x, y[3].x);
                lazy_pair(x[0].y, x[1].y, WA.x, WA.y, s01, d01);
                lazy_pair(x[2].y, x[3].y, WB.x, WB.y, s23, d23);
                last_pair(s01, s23, y[0].y, y[2].y);
                last_pair(d01, d23, y[1].y, y[3].y);
#pragma unroll
                for (int r = 0; r < 4; r++)
                    *reinterpret_cast<ulonglong2 *>(q0 + r * quarter) = y[r];
            }
        }

        // The instances that serve a ring of 2^LOGN, in the order of kInvInstances (ntt_select.hpp; null where the table says
        // the instance does not serve this ring size), for kernel_table (ntt_half.hpp): launch_half_inv launches from that table
        // and ntt_inv_half_init registers from it. The whole-row form of a ring is the half-row kernel of the ring twice as
        // large, the quarter-row form that of the ring half as large (inv_kernel_logn).
        using InvKernel = void (*)(u64 *, const PrimeDev *, RowMap, std::size_t, std::size_t, const u64 *, std::size_t, LiveSlots,
                                   DyadicSrc, int);
        struct InvTable
        {
            using Kernel = InvKernel;
            static constexpr int count = kInvInstanceCount;
            template <int LOGN, int I>
            static Kernel at()
            {
                constexpr InvInstance inst = kInvInstances[I];
                if constexpr (inv_instance_at(LOGN, inst))
                    return &ntt_inv_half_kernel<inv_kernel_logn(inst.shape, LOGN), inst.sched, inst.tensor_load(), inst.shape == kShapeWhole,
                                                inst.shape == kShapeQuarter>;
                else
                    return nullptr;
            }
        };
        // a shape's exchange buffer: half of the 2^(KLOGN - 1) coefficients a workgroup of ntt_inv_half_kernel<KLOGN, ..> holds
        constexpr int inv_lds_bytes(int shape, int logn)
        {
            return hpad(1 << (inv_kernel_logn(shape, logn) - 2)) * 8;
        }

        // Which shape and schedule run, and which top pass follows, is select_inv_half's decision (ntt_select.hpp; the
        // instances and who launches them: DESIGN.md section 6). Here: the facts it decides on and the launches.
        // (A one-launch standalone inverse by sibling hand-off -- the second finisher of a row applying the top layer to
        //  both halves -- was measured in round 2 and brought nothing; its cross-workgroup publish
        //  rested on workgroup-scope fences, so the path was removed rather than kept as an unsupported option.)
        template <int LOGN>
        hipError_t launch_half_inv(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags,
                                   const u64 *src = nullptr, std::size_t src_poly_stride = 0,
                                   const DyadicSrc *dyadic = nullptr)
        {
            if (fp64_enabled() && (flags & (kNttAnyRep | kNttCanonical)) != 0 && !dyadic)
            {
                RowMap a, b;
                if (split_by_fp(e, map, a, b))
                {
                    const hipError_t err = launch_half_inv<LOGN>(e, data, nrows, a, flags, src, src_poly_stride);
                    return err != hipSuccess ? err : launch_half_inv<LOGN>(e, data, nrows, b, flags, src, src_poly_stride);
                }
            }
            if (nrows % map.rows != 0)
                return hipErrorInvalidValue;
            const LiveSlots live = live_slots(map);
            if (live.n == 0)
                return hipSuccess;
            u64 live_p[kMaxRows];
            for (int i = 0; i < live.n; i++)
                live_p[i] = e.tables[map.prime[live.slot[i]]].p;
            const InvChoice c = select_inv_half(InvFacts{ LOGN, flags, live_p, live.n, dyadic != nullptr, ntt_switches() });
            if (!c.valid)
                return hipErrorInvalidValue;
            const std::size_t chunk = ((nrows / map.rows) * live.n + 7) / 8; // live rows per XCD
            const std::size_t blocks = chunk * 8 * inv_blocks_per_row(c.shape); // (eight XCDs)
            if (chunk * 16 > 0x7fffffffull || blocks > 0x7fffffffull)
                return hipErrorInvalidValue;
            {
                ProfScope prof(e, "ntt_inv_half", transformed_rows(nrows, map));
                kernel_table<InvTable, LOGN>()[c.instance]<<<static_cast<unsigned>(blocks), 1 << (inv_kernel_logn(c.shape, LOGN) - 6),
                                                  inv_lds_bytes(c.shape, LOGN), e.lane().stream>>>(
                    data, e.d_primes, map, nrows, chunk, src, src_poly_stride, live, dyadic ? *dyadic : DyadicSrc{}, c.canon);
                const hipError_t err = hipGetLastError();
                if (err != hipSuccess || c.top == kTopNone)
                    return err;
            }
            // the streaming pass for what the kernel left: one lane per 16-byte pair of the first half (top layer) or of
            // the first quarter (radix-4 pass) of every row
            const bool radix4 = c.top == kTopRadix4;
            const std::size_t nitems = nrows << (LOGN - (radix4 ? 3 : 2));
            std::size_t grid = (nitems + 255) / 256;
            if (grid > 256u * 32u)
                grid = 256u * 32u;
            ProfScope prof(e, "ntt_inv_top", radix4 ? 0 : transformed_rows(nrows, map));
            if (radix4)
                ntt_inv_top2_kernel<<<static_cast<unsigned>(grid), 256, 0, e.lane().stream>>>(data, e.d_primes, map, LOGN, nitems, flags);
            else
                ntt_inv_top_kernel<<<static_cast<unsigned>(grid), 256, 0, e.lane().stream>>>(data, e.d_primes, map, LOGN, nitems, flags);
            return hipGetLastError();
        }
    } // namespace

    hipError_t ntt_inv_half(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags, const u64 *src,
                            std::size_t src_poly_stride)
    {
        return at_ring_size(e.logn, [&](auto logn) {
            return launch_half_inv<decltype(logn)::value>(e, data, nrows, map, flags, src, src_poly_stride);
        });
    }

    hipError_t ntt_inv_tensor(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags, const u64 *x,
                              std::size_t item_stride, std::size_t poly_stride, int kb, bool square)
    {
        const DyadicSrc dy{ x, item_stride, poly_stride, kb, square ? 1 : 0 };
        return at_ring_size(e.logn, [&](auto logn) {
            return launch_half_inv<decltype(logn)::value>(e, data, nrows, map, flags, nullptr, 0, &dy);
        });
    }

    hipError_t ntt_inv_half_init()
    {
        // the dynamic LDS limit of every instance that serves the ring
        return at_every_ring_size([](auto logn) {
            constexpr int LOGN = decltype(logn)::value;
            return set_dynamic_lds(kernel_table<InvTable, LOGN>(), InvTable::count,
                                   [](int i) { return inv_lds_bytes(kInvInstances[i].shape, LOGN); });
        });
    }
} // namespace sealhip
