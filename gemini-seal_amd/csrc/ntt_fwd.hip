// ntt_fwd.hip -- single-pass forward NTT for N = 2^14 .. 2^16 (the half-row kernel, ntt_half.hpp) and its launcher.
#include <cstring>
#include <utility>

#include "ntt_half.hpp"

namespace sealhip
{
    namespace
    {
        // STRICT == kSchedApprox (approximate Shoup quotient): which form (ntt_bounds.hpp section 2: bounds::kFwdApxLevel) -- 1: round 2's
        // (hi32(y0*s0) dropped, product below 3p); 2: round 4's carry-free quotient (devmath.hpp mulhi_apx2, below 4p).
        // The butterfly's second output is u - v + (that bound), so the bound is what the layers add.
        template <int STRICT>
        constexpr int kApx = STRICT == kSchedApprox ? bounds::kFwdApxLevel : 0;
        // The final round at N = 2^15 runs at the register cap (two stages of prefetched twiddles, 48 registers): four more for
        // zero-high pairs spill two coefficients. Its 32 butterflies (of 272) keep the level-1 quotient there -- a product
        // below 3p under a schedule that allows 4p, so the bounds of level 2 cover it (ntt_bounds.hpp section 2).
        constexpr int kFinalZeroPairs = 2;
        template <int T, int STRICT>
        constexpr int kFinalApx = (kApx<STRICT> == 2 && (T - 12) == 2) ? 1 : kApx<STRICT>;
        template <int STRICT>
        __device__ __forceinline__ u64 fwd_addend(u64 two_p, u64 neg_p)
        {
            if constexpr (STRICT != kSchedApprox)
                return two_p;
            u64 a = two_p << 1; // 4p (level 2), opaque: left visible the compiler rewrites (u << 1) + (2p << 1) as (u + 2p) << 1,
            asm("" : "+s"(a));  // two 64-bit instructions where v_lshl_add_u64 does it in one
            return a;
        }

        // Final-round stores. A lane finishes runs of 2^f consecutive coefficients; for f >= 2 storing them from there
        // means 16-byte pieces at a 2^f * 8-byte stride per instruction -- every 128-byte line is written by 2^(f-1)
        // different instructions, and a kernel that does nothing but these stores reaches 2.0 TB/s at f = 2 (3.0 at
        // f = 3) against 5.3 TB/s for the contiguous stores of f = 1 (profiles/r02/ntt_store_pattern.txt). So for
        // f >= 2 the finished values take one more trip through the LDS, back to arrangement 1 (a lane holds pairs, the
        // lanes of a wave are consecutive pairs), and every store instruction writes one contiguous kilobyte.
        // Which instances take the trip (bit mask): 1 the floating-point ones, 2 the integer ones at f = 2, 4 the integer
        // ones at f = 3. Inside the pipelines the integer instances are bound by instruction issue, not by their stores:
        // at f = 2 the extra exchange costs them 2 % (config 3: 18.8 vs 18.4 ms of forward transforms per 1024 pairs)
        // although the transform alone gains 6 %; the floating-point instances gain 10 % in the config-4 key switch.
        // Round 3: the transposition in registers instead. What is slow about the f >= 2 pattern is not the 16-byte pieces
        // as such but the *streaming* (nontemporal) stores of them: tools/ubench_store_pattern.hip writes the same half
        // rows at 1.9 TB/s nontemporal against 5.7 TB/s with plain stores (the L2 merges the two instructions' pieces),
        // and a nontemporal instruction is fast (5.5 TB/s) as soon as the wave as a whole covers contiguous memory --
        // which lane writes which piece does not matter (profiles/r03/store_pattern_ubench.txt). v_permlane32_swap
        // (lanes 32-63 of one register <-> lanes 0-31 of another) is exactly that transposition for f = 2: before,
        // lane (l5, r) holds pairs h = 0, 1 of its run; after swap(pair 0, pair 1) register h of lane (l5, r) holds pair
        // l5 of lane (h, r), so instruction h writes the 128 consecutive coefficients of half-wave h: one dword move per
        // dword, no LDS, no barrier. For f = 3 a v_permlane16_swap step (rows of 16 lanes) transposes the second bit.
        // Every f >= 2 instance takes the swap but mode 7, which keeps the trip: its store phase reads the product rows at
        // the same addresses (mode 7 has a floating-point instance only, ntt_select.hpp kFwdInstances).
        template <int T, int REDUCE>
        constexpr bool kStoreSwap = (T - 12) >= 2 && REDUCE != kTreatModDownStore;
        template <int T, int REDUCE>
        constexpr bool kStoreExchange = fwd_store_exchange(T, REDUCE); // (ntt_select.hpp: the instance table states where it exists)

        __device__ __forceinline__ void swap_half_waves(u64 &a, u64 &b) // lanes 32-63 of a <-> lanes 0-31 of b
        {
            const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(a), static_cast<unsigned>(b), false, false);
            const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<unsigned>(a >> 32), static_cast<unsigned>(b >> 32), false, false);
            a = lo[0] | (static_cast<u64>(hi[0]) << 32);
            b = lo[1] | (static_cast<u64>(hi[1]) << 32);
        }
        __device__ __forceinline__ void swap_rows16(u64 &a, u64 &b) // odd 16-lane rows of a <-> even rows of b
        {
            const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(a), static_cast<unsigned>(b), false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<unsigned>(a >> 32), static_cast<unsigned>(b >> 32), false, false);
            a = lo[0] | (static_cast<u64>(hi[0]) << 32);
            b = lo[1] | (static_cast<u64>(hi[1]) << 32);
        }
        // Final-round group G (2^f finished registers, runs of 2^f consecutive coefficients per lane) -> memory through the
        // register transposition: afterwards pair register i of lane L holds pair (L >> 4 or 5 bits) of the lane whose
        // those bits are i, so instruction i writes the i-th 128-coefficient piece of the wave's 2^(f+6) coefficients.
        template <int T, int G>
        __device__ __forceinline__ void h_store_group_swapped(u64 (&x)[32], u64 *__restrict__ rowp, int jb)
        {
            constexpr int f = T - 12;
            static_assert(f == 2 || f == 3, "register transposition: runs of 4 or 8 coefficients");
            constexpr int s = G << f;
            const int j = jb & ((1 << T) | ((1 << T) - 1));
            // lane part of the address: the wave's base, then r * 2^f + (the swapped lane bits) * 2
            // (the lane is index bits [f, f+6), everything above -- no filler bit is set in j -- is the base)
            const int tid = (j >> f) & 63;
            int base = j & ~((1 << (6 + f)) - 1);
            if constexpr (f == 2)
            {
                base += ((tid & 31) << 2) + (((tid >> 5) & 1) << 1);
                swap_half_waves(x[s], x[s + 2]);
                swap_half_waves(x[s + 1], x[s + 3]);
            }
            else
            {
                base += ((tid & 15) << 3) + (((tid >> 5) & 1) << 2) + (((tid >> 4) & 1) << 1);
#pragma unroll
                for (int e = 0; e < 4; e++)
                    swap_half_waves(x[s + e], x[s + 4 + e]);
#pragma unroll
                for (int e = 0; e < 2; e++)
                {
                    swap_rows16(x[s + e], x[s + 2 + e]);
                    swap_rows16(x[s + 4 + e], x[s + 6 + e]);
                }
            }
            u64 *dst = rowp + base + Arr<T, 4>::slot_index(s);
#pragma unroll
            for (int i = 0; i < (1 << (f - 1)); i++)
                store_nt(dst + i * 128, x[s + 2 * i], x[s + 2 * i + 1]);
        }

        // Where the final round's twiddles come from: get(W, e) is the twiddle of layer W's butterfly on element e of the group.
        // TwRegs: the group's prefetched registers (GroupTw, FinalPipe: f <= 2). TwMemory: loaded where they are used
        // (FinalGroups: f = 3, where two stages of 28 twiddle registers do not fit).
        template <int T>
        struct TwRegs
        {
            static constexpr bool from_memory = false;
            const u64x2 *tg;
            __device__ __forceinline__ u64x2 get(int W, int e) const
            {
                return tg[GroupTw<T, true>::at(W, e)];
            }
        };
        template <int T, int G, bool FP>
        struct TwMemory
        {
            static constexpr bool from_memory = true;
            const u64 *__restrict__ tw;
            int jb, N;
            __device__ __forceinline__ u64x2 get(int W, int e) const
            {
                const int i = ((N + jb) >> (Arr<T, 4>::slot_bit(W) + 1)) + Arr<T, 4>::tw_offset((G << (T - 12)) | e, W);
                u64x2 Wv;
                if constexpr (FP)
                {
                    Wv.x = ((twd_global_t)tw)[i];
                    Wv.y = 0;
                }
                else
                    Wv = ((tw_global_t)tw)[i];
                return Wv;
            }
        };

        // a finished pair of words of the final round -> the words that are stored (fin, rdp: see ntt_fwd_half_kernel)
        template <int STRICT, bool ROUT>
        __device__ __forceinline__ void h_finish_pair(u64 &a, u64 &b, u64 p, u64 two_p, u64 neg_p, u64 rdp, int fin)
        {
            if constexpr (STRICT == kSchedFp64)
            {
                // canonical residues always: they serve kNttCanonical and every any-representative consumer alike
                a = fp_to_u64(fp_canonical(fp_of(a), fp_of(two_p), fp_of(neg_p)));
                b = fp_to_u64(fp_canonical(fp_of(b), fp_of(two_p), fp_of(neg_p)));
            }
            else if (fin & 1)
            {
                if constexpr (STRICT == kSchedApprox)
                {
                    // canonical output of the approximate-quotient schedule (values below (2 + g log n) p <= 66p,
                    // ntt_bounds.hpp section 2): one step to [0, 2p), one conditional subtraction. fin & 4: the step is
                    // the single-precision quotient estimate (rdp then carries the bits of its constant), else Barrett
                    if (fin & 4)
                    {
                        const float cq = __uint_as_float(static_cast<unsigned>(rdp));
                        a = reduce_small_quot(a, cq, neg_p);
                        b = reduce_small_quot(b, cq, neg_p);
                    }
                    else
                    {
                        a = barrett_lazy_hs(a, rdp, neg_p);
                        b = barrett_lazy_hs(b, rdp, neg_p);
                    }
                }
                else
                {
                    a = a >= two_p ? a - two_p : a;
                    b = b >= two_p ? b - two_p : b;
                }
                a = a >= p ? a - p : a;
                b = b >= p ? b - p : b;
            }
            else if constexpr (ROUT && STRICT == kSchedDense)
            {
                // dense lazy schedule: words below 16p -> [0, 2p) (rdp carries the bits of the quotient constant)
                const float cq = __uint_as_float(static_cast<unsigned>(rdp));
                a = reduce_small_quot(a, cq, neg_p);
                b = reduce_small_quot(b, cq, neg_p);
            }
            else if constexpr (ROUT)
            {
                // kNttReduceOut: [0, 4p) -> [0, 2p), same residue. (The last layer reduces its first operand and its
                // product below 2p before it adds them -- ForwardLazyLast, ntt.cpp:254-261 -- so even on the 60-bit rows,
                // where earlier layers wrap, what it outputs is below 4p.)
                a = a >= two_p ? a - two_p : a;
                b = b >= two_p ? b - two_p : b;
            }
        }

        // final round, one group at a time: the low f index bits of the 2^f registers that share the filler
        // slot bits G are finished (layers f-1 .. 0) and stored right away, which bounds the live twiddles
        // SX: what happens to the finished words -- 0 stored from arrangement 4 as they are, 1 kept for the LDS trip
        // (kStoreExchange), 2 transposed in registers and stored group by group (kStoreSwap)
        template <int T, int STRICT, int G, bool ROUT, int SX, class TwSource>
        __device__ __forceinline__ void h_final_group(u64 (&x)[32], const TwSource &twiddles, u64 *__restrict__ rowp, int jb,
                                                      u64 p, u64 two_p, u64 neg_p, u64 rdp, int fin, ZeroPairs &zp)
        {
            constexpr int f = T - 12;
            // (twiddles from memory: f = 3, where kStoreSwap or kStoreExchange always holds)
            static_assert(SX != 0 || !TwSource::from_memory, "the store from arrangement 4 exists in the prefetched form only");
#pragma unroll
            for (int W = f - 1; W >= 0; W--)
            {
                const int gb = Arr<T, 4>::slot_bit(W);
                const int bit = 1 << W;
#pragma unroll
                for (int e = 0; e < (1 << f); e++)
                {
                    if (e & bit)
                        continue;
                    const int s = (G << f) | e;
                    const u64x2 Wv = twiddles.get(W, e);
                    if constexpr (STRICT == kSchedFp64)
                    {
                        fp_butterfly_fwd(x[s], x[s | bit], Wv.x, fp_of(two_p), fp_of(neg_p));
                        continue;
                    }
                    if (STRICT == kSchedHarvey)
                        x[s] = x[s] >= two_p ? x[s] - two_p : x[s];
                    else if (gb == 0 && !(fin & 2)) // fin & 2: the consumer takes any representative and nothing can wrap
                        x[s] = barrett_lazy_hs(x[s], rdp, neg_p);
                    if constexpr (kFinalApx<T, STRICT> == 2)
                        butterfly_fwd_apx2<false>(x[s], x[s | bit], Wv.x, Wv.y, neg_p, fwd_addend<STRICT>(two_p, neg_p), zp.z[(((e >> (W + 1)) << W) | (e & (bit - 1))) & (kFinalZeroPairs - 1)]);
                    else
                        butterfly_fwd_hs<false, kFinalApx<T, STRICT>>(x[s], x[s | bit], Wv.x, Wv.y, neg_p, fwd_addend<STRICT>(two_p, neg_p));
                }
            }
#pragma unroll
            for (int e = 0; e < (1 << f); e += 2)
            {
                const int s = (G << f) | e;
                ulonglong2 v;
                v.x = x[s];
                v.y = x[s + 1];
                h_finish_pair<STRICT, ROUT>(v.x, v.y, p, two_p, neg_p, rdp, fin);
                if constexpr (SX != 0)
                {
                    x[s] = v.x; // stored by h_store_rows after the trip back to arrangement 1, or transposed below
                    x[s + 1] = v.y;
                }
                else
                    store_nt(rowp + (jb & ((1 << T) | ((1 << T) - 1))) + Arr<T, 4>::slot_index(s), v.x, v.y);
            }
            if constexpr (SX == 2)
                h_store_group_swapped<T, G>(x, rowp, jb);
        }

        template <int T, int STRICT, int G, int NG, bool ROUT, int SX>
        struct FinalGroups
        {
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64 *__restrict__ tw, u64 *__restrict__ rowp,
                                                       int jb, int N, u64 p, u64 two_p, u64 neg_p, u64 rdp, int fin, ZeroPairs &zp)
            {
                h_final_group<T, STRICT, G, ROUT, SX>(x, TwMemory<T, G, STRICT == kSchedFp64>{ tw, jb, N }, rowp, jb, p, two_p, neg_p,
                                                      rdp, fin, zp);
                if ((G & 1) == 1)
                    __builtin_amdgcn_sched_barrier(0); // keep the compiler from hoisting every group's twiddle loads
                FinalGroups<T, STRICT, G + 1, NG, ROUT, SX>::run(x, tw, rowp, jb, N, p, two_p, neg_p, rdp, fin, zp);
            }
        };
        template <int T, int STRICT, int NG, bool ROUT, int SX>
        struct FinalGroups<T, STRICT, NG, NG, ROUT, SX>
        {
            __device__ static __forceinline__ void run(u64 (&)[32], const u64 *, u64 *, int, int, u64, u64, u64, u64, int, ZeroPairs &)
            {}
        };

        template <int T, int STRICT, bool ROUT, int SX, int ST, int I = 0>
        struct StageRun
        {
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64x2 *tg, u64 *__restrict__ rowp, int jb,
                                                       u64 p, u64 two_p, u64 neg_p, u64 rdp, int fin, ZeroPairs &zp)
            {
                h_final_group<T, STRICT, ST * FinalStage<T>::SG + I, ROUT, SX>(x, TwRegs<T>{ tg + I * FinalStage<T>::NTW }, rowp, jb, p,
                                                                          two_p, neg_p, rdp, fin, zp);
                if constexpr (I + 1 < FinalStage<T>::SG)
                    StageRun<T, STRICT, ROUT, SX, ST, I + 1>::run(x, tg, rowp, jb, p, two_p, neg_p, rdp, fin, zp);
            }
        };
        template <int T, int STRICT, bool ROUT, int SX, int ST>
        struct FinalPipe
        {
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64x2 *cur, const u64 *__restrict__ tw,
                                                       u64 *__restrict__ rowp, int jb, int N, u64 p, u64 two_p, u64 neg_p,
                                                       u64 rdp, int fin, ZeroPairs &zp)
            {
                u64x2 next[FinalStage<T>::SG * FinalStage<T>::NTW];
                if constexpr (ST + 1 < FinalStage<T>::NS)
                    StageTw<T, ST + 1, true, STRICT == kSchedFp64>::load(next, tw, jb, N);
                __builtin_amdgcn_sched_barrier(0);
                StageRun<T, STRICT, ROUT, SX, ST>::run(x, cur, rowp, jb, p, two_p, neg_p, rdp, fin, zp);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (ST + 1 < FinalStage<T>::NS)
                    FinalPipe<T, STRICT, ROUT, SX, ST + 1>::run(x, next, tw, rowp, jb, N, p, two_p, neg_p, rdp, fin, zp);
            }
        };

        // ---- a compute round as a pipeline of stages. Stage K = kIL butterflies of one layer (layers W = 4, 3, 2, 1,
        // 16 / kIL stages each). The twiddles of stage K+1 are requested before stage K is computed (pinned with
        // sched_barrier), the first stage's before the preceding LDS exchange: no twiddle latency is exposed.
        template <int T, int R, int STRICT, bool UNIFORM, int K>
        struct RoundStage : Stage<T, R, 4 - K / kStagesPerLayer, (K % kStagesPerLayer) * kIL, UNIFORM, STRICT == kSchedFp64>
        {
            using S = Stage<T, R, 4 - K / kStagesPerLayer, (K % kStagesPerLayer) * kIL, UNIFORM, STRICT == kSchedFp64>;
            using S::bit;
            using S::slot;
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64 (&w)[kIL], const u64 (&ws)[kIL], u64 two_p,
                                                       u64 neg_p, ZeroPairs &zp)
            {
                if constexpr (STRICT == kSchedFp64)
                {
#pragma unroll
                    for (int j = 0; j < kIL; j++)
                        fp_butterfly_fwd(x[slot(j)], x[slot(j) | bit], w[j], fp_of(two_p), fp_of(neg_p));
                    return;
                }
                u64 u[kIL], y[kIL];
#pragma unroll
                for (int j = 0; j < kIL; j++)
                {
                    u[j] = x[slot(j)];
                    y[j] = x[slot(j) | bit];
                    if (STRICT == kSchedHarvey)
                        u[j] = u[j] >= two_p ? u[j] - two_p : u[j];
                }
                if constexpr (kApx<STRICT> == 2)
                {
                    static_assert(kIL == 4, "two zero-high pairs for four lock-step butterflies");
                    butterflies_fwd_apx2<UNIFORM, kIL>(u, y, w, ws, neg_p, fwd_addend<STRICT>(two_p, neg_p), zp.z);
                }
                else
                    butterflies_fwd_hs<UNIFORM, kIL, kApx<STRICT>>(u, y, w, ws, neg_p, fwd_addend<STRICT>(two_p, neg_p)); // ForwardLazy, ntt.cpp:245-252
#pragma unroll
                for (int j = 0; j < kIL; j++)
                {
                    x[slot(j)] = u[j];
                    x[slot(j) | bit] = y[j];
                }
            }
        };
        template <int T, int R, int STRICT, bool UNIFORM, int K = 0>
        struct RoundPipe
        {
            static constexpr int NST = 4 * (16 / kIL);
            __device__ static __forceinline__ void run(u64 (&x)[32], const u64 (&w)[kIL], const u64 (&ws)[kIL],
                                                       const u64 *__restrict__ tw, int jb, int N, u64 two_p, u64 neg_p, ZeroPairs &zp)
            {
                u64 wn[kIL], wsn[kIL];
                if constexpr (K + 1 < NST)
                    RoundStage<T, R, STRICT, UNIFORM, K + 1>::load(wn, wsn, tw, jb, N);
                __builtin_amdgcn_sched_barrier(0);
                // (before on-chip layers 5 and 10 -- after round 2's first and round 3's second layer: see fp_reduce_all)
                if constexpr (STRICT == kSchedFp64 && K % (16 / kIL) == 0 && bounds::fp_fwd_reduce_before_layer(4 * (R - 1) + K / (16 / kIL)))
                    fp_reduce_all(x, two_p, neg_p);
                // dense lazy schedule (STRICT == kSchedDense, ntt_bounds.hpp section 2b): every word back below 2p before rounds 2 and 3
                if constexpr (STRICT == kSchedDense && K == 0 && bounds::fwd_dense_reduce_before_round(R))
                {
                    const float cq = small_quot_const(0 - neg_p);
#pragma unroll
                    for (int i = 0; i < 32; i++)
                        x[i] = reduce_small_quot(x[i], cq, neg_p);
                }
                RoundStage<T, R, STRICT, UNIFORM, K>::run(x, w, ws, two_p, neg_p, zp);
                if constexpr (K + 1 < NST)
                    RoundPipe<T, R, STRICT, UNIFORM, K + 1>::run(x, wn, wsn, tw, jb, N, two_p, neg_p, zp);
            }
        };

        constexpr int kLoadBatch = 4; // (lo, hi) 16-byte pairs per lane in flight during the load phase
        template <int T, int STRICT, int HALF, int REDUCE>
        __device__ __forceinline__ void h_load_top(u64 (&x)[32], const u64 *__restrict__ rowp,
                                                   const u64 *__restrict__ tw, int tid, u64 two_p, u64 neg_p, u64 cr1,
                                                   u64 aux_p = 0, u64 aux_cr1 = 0, const u64 *aux_top = nullptr)
        {
            const int jb = Arr<T, 1>::tid_index(tid);
            ZeroPairs zp;
            if constexpr (kApx<STRICT> == 2)
                zp.init();
            u64x2 W1;
            if constexpr (STRICT == kSchedFp64)
                W1.x = ((twd_const_t)tw)[1];
            else
                W1 = ((tw_const_t)tw)[1];
#pragma unroll
            for (int batch = 0; batch < 16 / kLoadBatch; batch++)
            {
                ulonglong2 lo[kLoadBatch], hi[kLoadBatch];
#pragma unroll
                for (int i = 0; i < kLoadBatch; i++)
                {
                    const int s = (batch * kLoadBatch + i) * 2;
                    const int idx = jb + Arr<T, 1>::slot_index(s);
                    lo[i] = *reinterpret_cast<const ulonglong2 *>(rowp + idx);
                    hi[i] = *reinterpret_cast<const ulonglong2 *>(rowp + (1 << T) + idx);
                }
                if constexpr (REDUCE == kTreatNegSpecialTop || REDUCE == kTreatModDownStore)
                {
                    // mode 4 on a source row whose top inverse layer was left to us: the pair (lo, hi) = (c, c + N/2) first
                    // goes through BackwardLazyLast w.r.t. the special prime P (inputs below 2P), then -(. mod P)
#pragma unroll
                    for (int i = 0; i < kLoadBatch; i++)
                    {
                        const auto top = [&](u64 &u, u64 &v) {
                            if constexpr (STRICT == kSchedFp64)
                            {
                                // aux_p / aux_cr1: P and 1/P as doubles; aux_top[0], [2]: n^-1 and w n^-1 as doubles
                                const double P = fp_of(aux_p), Pinv = fp_of(aux_cr1), ud = fp_from_u64(u), vd = fp_from_u64(v);
                                const double a0 = fp_canonical(fp_mulmod(ud + vd, fp_of(aux_top[0]), P, Pinv), P, Pinv);
                                const double a1 = fp_canonical(fp_mulmod(ud - vd, fp_of(aux_top[2]), P, Pinv), P, Pinv);
                                u = fp_bits(a0 != 0.0 ? P - a0 : 0.0);
                                v = fp_bits(a1 != 0.0 ? P - a1 : 0.0);
                            }
                            else
                            {
                                const u64 two_P = aux_p << 1;
                                u64 tt = u + v;
                                tt = tt >= two_P ? tt - two_P : tt;
                                u64 a0 = mulmod_lazy(tt, aux_top[0], aux_top[1], aux_p); // below 2P
                                u64 a1 = mulmod_lazy(u - v + two_P, aux_top[2], aux_top[3], aux_p);
                                a0 = a0 >= aux_p ? a0 - aux_p : a0;
                                a1 = a1 >= aux_p ? a1 - aux_p : a1;
                                u = a0 ? aux_p - a0 : 0;
                                v = a1 ? aux_p - a1 : 0;
                            }
                        };
                        top(lo[i].x, hi[i].x);
                        top(lo[i].y, hi[i].y);
                    }
                }
                if constexpr (REDUCE == kTreatNegSpecial)
                {
                    // CKKS mod-down with one special prime P (multi_special_primes.cpp:262-273): the word is a lazy value of
                    // the special row; the row being transformed holds (-(s mod P)) mod q. -(s mod P) is formed here as the
                    // integer P - r (0 for r = 0), which is below P < 2q: the lazy transform takes it as it is, so the
                    // separate pass that wrote these k rows and the read of them are gone.
#pragma unroll
                    for (int i = 0; i < kLoadBatch; i++)
                    {
                        const auto red = [&](u64 v) {
                            if constexpr (STRICT == kSchedFp64)
                            {
                                // floating-point instance: aux_p / aux_cr1 carry P and 1/P as doubles, v < 2^52; the word
                                // stays a double (the top layer below does not convert it again)
                                const double P = fp_of(aux_p), r = fp_canonical(fp_from_u64(v), P, fp_of(aux_cr1));
                                return fp_bits(r != 0.0 ? P - r : 0.0);
                            }
                            const u64 r = barrett_reduce_63(v, aux_p, aux_cr1);
                            return r ? aux_p - r : 0;
                        };
                        lo[i].x = red(lo[i].x);
                        lo[i].y = red(lo[i].y);
                        hi[i].x = red(hi[i].x);
                        hi[i].y = red(hi[i].y);
                    }
                }
                if constexpr (REDUCE == kTreatBarrett || REDUCE == kTreatCondSub) // gathered single-prime mod-up (multi_special_primes.cpp:103-107)
                {
                    const u64 p = STRICT == kSchedFp64 ? static_cast<u64>(fp_of(two_p)) : 0 - neg_p;
                    const auto red = [&](u64 v) {
                        if constexpr (REDUCE == kTreatCondSub)
                            return v >= p ? v - p : v; // source prime < 2p: the canonical residue is v or v - p
                        else
                            return barrett_reduce_63(v, p, cr1);
                    };
#pragma unroll
                    for (int i = 0; i < kLoadBatch; i++)
                    {
                        lo[i].x = red(lo[i].x);
                        lo[i].y = red(lo[i].y);
                        hi[i].x = red(hi[i].x);
                        hi[i].y = red(hi[i].y);
                    }
                }
#pragma unroll
                for (int i = 0; i < kLoadBatch; i += 2)
                {
                    // four butterflies in lock step (program-ordered asm: the products stay inside their batch instead
                    // of being sunk below the loads of the later batches, which used to spill loaded values)
                    const int s = (batch * kLoadBatch + i) * 2;
                    u64 u[4] = {lo[i].x, lo[i].y, lo[i + 1].x, lo[i + 1].y};
                    u64 y[4] = {hi[i].x, hi[i].y, hi[i + 1].x, hi[i + 1].y};
                    if constexpr (STRICT == kSchedFp64)
                    {
                        // inputs below 2^52 (select_fwd_half: residues, lazy gathered values, or the treatments above)
#pragma unroll
                        for (int j = 0; j < 4; j++)
                        {
                            if constexpr (REDUCE != kTreatNegSpecial && REDUCE != kTreatNegSpecialTop && REDUCE != kTreatModDownStore)
                            {
                                u[j] = fp_bits(fp_from_u64(u[j]));
                                y[j] = fp_bits(fp_from_u64(y[j]));
                            }
                            fp_butterfly_fwd(u[j], y[j], W1.x, fp_of(two_p), fp_of(neg_p));
                            x[s + j] = HALF ? y[j] : u[j];
                        }
                        continue;
                    }
                    const u64 w[4] = {W1.x, W1.x, W1.x, W1.x}, ws[4] = {W1.y, W1.y, W1.y, W1.y};
                    if (STRICT == kSchedHarvey)
                    {
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            u[j] = u[j] >= two_p ? u[j] - two_p : u[j];
                    }
                    if constexpr (kApx<STRICT> == 2)
                        butterflies_fwd_apx2<true, 4>(u, y, w, ws, neg_p, fwd_addend<STRICT>(two_p, neg_p), zp.z);
                    else
                        butterflies_fwd_hs<true, 4, kApx<STRICT>>(u, y, w, ws, neg_p, fwd_addend<STRICT>(two_p, neg_p));
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        x[s + j] = HALF ? y[j] : u[j];
                }
                // keep the next batch's loads from being hoisted over this batch's products: that costs registers
                // (spilled loaded values came back as HBM write traffic) and buys nothing (the load phase is bound by
                // the CU's load path, not by latency: profiles/r04/fwd_phases_exp_build.txt)
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // kNttSplitLast: the parity class HALF of the gathered row, src[2 i + HALF] for i < 2^T, in arrangement 1 -- no layer
        // is applied here. A slot pair (i, i + 1) lies in two neighbouring 16-byte pieces of the row, of which this workgroup
        // keeps one word each: as many 16-byte loads per lane as h_load_top issues (32), every line of the row read once by
        // each of the row's two workgroups.
        template <int T, int HALF, int REDUCE>
        __device__ __forceinline__ void h_load_split(u64 (&x)[32], const u64 *__restrict__ rowp, int tid, u64 p, u64 cr1)
        {
            static_assert(REDUCE == kTreatNone || REDUCE == kTreatBarrett || REDUCE == kTreatCondSub, "mod-up treatments only");
            const int jb = Arr<T, 1>::tid_index(tid);
#pragma unroll
            for (int batch = 0; batch < 16 / kLoadBatch; batch++)
            {
                ulonglong2 a[kLoadBatch], b[kLoadBatch];
#pragma unroll
                for (int i = 0; i < kLoadBatch; i++)
                {
                    const int idx = jb + Arr<T, 1>::slot_index((batch * kLoadBatch + i) * 2);
                    a[i] = *reinterpret_cast<const ulonglong2 *>(rowp + 2 * idx);
                    b[i] = *reinterpret_cast<const ulonglong2 *>(rowp + 2 * idx + 2);
                }
#pragma unroll
                for (int i = 0; i < kLoadBatch; i++)
                {
                    const int s = (batch * kLoadBatch + i) * 2;
                    u64 v0 = HALF ? a[i].y : a[i].x, v1 = HALF ? b[i].y : b[i].x;
                    if constexpr (REDUCE == kTreatCondSub)
                    {
                        v0 = v0 >= p ? v0 - p : v0; // source prime < 2p: the canonical residue is v or v - p
                        v1 = v1 >= p ? v1 - p : v1;
                    }
                    else if constexpr (REDUCE == kTreatBarrett)
                    {
                        v0 = barrett_reduce_63(v0, p, cr1);
                        v1 = barrett_reduce_63(v1, p, cr1);
                    }
                    x[s] = v0;
                    x[s + 1] = v1;
                }
                __builtin_amdgcn_sched_barrier(0); // (as in h_load_top: loaded values are not held across batches)
            }
        }

        // arrangement 1 -> memory: pairs, consecutive lanes 16 bytes apart
        template <int T>
        __device__ __forceinline__ void h_store_rows(const u64 (&x)[32], u64 *__restrict__ halfp, int tid)
        {
            const int jb = Arr<T, 1>::tid_index(tid);
#pragma unroll
            for (int s = 0; s < 32; s += 2)
                store_nt(halfp + jb + Arr<T, 1>::slot_index(s), x[s], x[s + 1]);
        }

        // reduce mode 7: the words of arrangement 1 are canonical residues t of temp_q (NTT form); what is stored is the rest of
        // the CKKS mod-down (NttSource::ModDownStore): v = (prod + t) * P^-1 mod q, into the ciphertext
        template <int T>
        __device__ __forceinline__ void h_store_moddown(const u64 (&x)[32], int tid, const u64 *__restrict__ prod_half,
                                                        u64 *__restrict__ ct_half, const u64 *__restrict__ c0_half, bool add_ct,
                                                        u64 inv_p, u64 inv_p_shoup, u64 p, unsigned *__restrict__ tflag)
        {
            const int jb = Arr<T, 1>::tid_index(tid);
            u64 nz = 0; // transparency sink: OR of the words stored into component 1 (tflag is null for component 0)
#pragma unroll
            for (int b = 0; b < 32; b += 8)
            {
                ulonglong2 pr[4], cc[4];
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int off = jb + Arr<T, 1>::slot_index(b + 2 * i);
                    pr[i] = *reinterpret_cast<const ulonglong2 *>(prod_half + off);
                    if (c0_half)
                        cc[i] = *reinterpret_cast<const ulonglong2 *>(c0_half + off);
                    else if (add_ct)
                        cc[i] = *reinterpret_cast<const ulonglong2 *>(ct_half + off);
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                {
                    const int off = jb + Arr<T, 1>::slot_index(b + 2 * i);
                    u64 v0 = mulmod_shoup(pr[i].x + x[b + 2 * i], inv_p, inv_p_shoup, p);
                    u64 v1 = mulmod_shoup(pr[i].y + x[b + 2 * i + 1], inv_p, inv_p_shoup, p);
                    if (c0_half || add_ct)
                    {
                        v0 = add_mod(v0, cc[i].x, p);
                        v1 = add_mod(v1, cc[i].y, p);
                    }
                    store_nt(ct_half + off, v0, v1);
                    nz |= v0 | v1;
                }
            }
            note_nonzero(tflag, 0, nz);
        }

        // SPLIT (kNttSplitLast): the workgroup transforms one parity class of the gathered row as a ring of
        // N/2 -- h_load_split instead of the top layer, the rounds' twiddle addressing of a ring of N/2 (tables: the first half
        // of PrimeDev::fwd), the store phase as it is, into the workgroup's half of the row. The consumer applies the last layer.
        template <int LOGN, int STRICT, int REDUCE, bool SPLIT = false>
        __global__ __launch_bounds__(1 << (LOGN - 6), 4) void ntt_fwd_half_kernel(
            u64 *__restrict__ data, const PrimeDev *__restrict__ primes, RowMap map, std::size_t nrows, int flags,
            unsigned *__restrict__ tickets, unsigned *__restrict__ timeout_flag, unsigned spin_limit, NttSource src,
            std::size_t chunk, LiveSlots live)
        {
            constexpr int T = LOGN - 1;
            constexpr int N = SPLIT ? 1 << (LOGN - 1) : 1 << LOGN; // the ring whose twiddles the rounds address
            static_assert(!SPLIT || ((STRICT == kSchedLazy || STRICT == kSchedApprox) && REDUCE <= kTreatCondSub), "kFwdSplitInstances");
            extern __shared__ u64 lds[];
            const int wave_base = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) & ~63); // (see fresh_tid)
            int half, position;
            std::size_t poly;
            if (!block_place<1>(blockIdx.x, nrows / map.rows, live.n, chunk, poly, position, half,
                                (flags & kNttPolyMajor) ? ((flags >> 16) & 0xFF) : 0))
                return;
            const std::size_t row = poly * map.rows + live.slot[position];
            const unsigned short pid = map.prime[row % map.rows];
            const PrimeDev P = primes[pid];
            constexpr bool FP = STRICT == kSchedFp64; // butterflies on the FP64 pipe (primes below 2^50, see fp_reduce_all)
            const u64 p = P.p, two_p = FP ? fp_bits(P.p_d) : P.two_p, rdp = P.rdp;
            const u64 *tw = FP ? reinterpret_cast<const u64 *>(P.fwd_d) : P.fwd;
            u64 *rowp = data + (row << LOGN);
            if constexpr (SPLIT)
                rowp += half << T; // (the rounds below run with gbase = 0: indices of the workgroup's own ring)
            u64 x[32];

            // ---- load both halves, top layer on the fly, arrangement 1 (block-uniform branch on the half)
            const u64 neg_p = FP ? fp_bits(P.pinv_d) : 0 - p;
            const u64 *srcp = rowp;
            if (src.base[0])
            {
                const unsigned short code = src.code[row % map.rows];
                if (code != kSkipRow)
                {
                    const int b = code >> 15;
                    srcp = src.base[b] + (row / map.rows) * src.poly_stride[b] +
                           (static_cast<std::size_t>(code & 0x3FFF) << LOGN);
                }
            }
            if constexpr (REDUCE == kTreatReduceOutTopDone)
            {
                // kNttTopDone: the producer applied the top layer; this workgroup's half, arrangement 1, nothing else
                const int jb1 = Arr<T, 1>::tid_index(fresh_tid(wave_base));
#pragma unroll
                for (int s = 0; s < 32; s += 2)
                {
                    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(rowp + (half << T) + jb1 + Arr<T, 1>::slot_index(s));
                    x[s] = v.x;
                    x[s + 1] = v.y;
                }
            }
            else if constexpr (SPLIT)
            {
                if (half)
                    h_load_split<T, 1, REDUCE>(x, srcp, fresh_tid(wave_base), p, P.cr1);
                else
                    h_load_split<T, 0, REDUCE>(x, srcp, fresh_tid(wave_base), p, P.cr1);
            }
            else if (half)
                h_load_top<T, STRICT, 1, REDUCE>(x, srcp, tw, fresh_tid(wave_base), two_p, neg_p, P.cr1, src.aux_p, src.aux_cr1, src.aux_top);
            else
                h_load_top<T, STRICT, 0, REDUCE>(x, srcp, tw, fresh_tid(wave_base), two_p, neg_p, P.cr1, src.aux_p, src.aux_cr1, src.aux_top);
            // The transform is in place and both workgroups of a row read BOTH halves: neither may store before
            // the other has finished loading. Ticket protocol (placement independent, bounded spin): every
            // wave bumps the row's counter once its loads have landed in registers; before its store phase
            // it waits until the counter shows all waves of both workgroups. Only a "finished reading" signal crosses workgroups, so
            // relaxed agent-scope atomics suffice (no payload is published).
            // The signal is sent after the first LDS exchange: its barriers are only passed once every wave of
            // the workgroup has consumed all of its loaded values in round 1, so no extra wait or barrier is needed.
            // (Sharing the top layer between the two workgroups instead -- each publishing the other's outputs -- measured
            //  slower: profiles/r04/sibling_top_exchange_ab.txt.)
            const int gbase = SPLIT ? 0 : half << T;
            // round 1: every lane index bit lies below the processed bits -> block-uniform twiddles
            u64 w0[kIL], ws0[kIL];
            RoundStage<T, 1, STRICT, true, 0>::load(w0, ws0, tw, gbase, N);
            if constexpr (FP)
                fp_reduce_all(x, two_p, neg_p);
            ZeroPairs zp; // (written again where each phase starts: two moves, and no register held across the exchanges)
            if constexpr (kApx<STRICT> == 2)
                zp.init();
            RoundPipe<T, 1, STRICT, true>::run(x, w0, ws0, tw, gbase, N, two_p, neg_p, zp);
            const int jb2 = gbase + Arr<T, 2>::tid_index(fresh_tid(wave_base));
            RoundStage<T, 2, STRICT, false, 0>::load(w0, ws0, tw, jb2, N); // lands while the exchange runs
            __builtin_amdgcn_sched_barrier(0);
            h_exchange<T, 1, 2>(x, lds, fresh_tid(wave_base));
            if (fresh_tid(wave_base) == 0 && tickets && !(flags & kNttDebugNoSignal))
                __hip_atomic_fetch_add(&tickets[row], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (kApx<STRICT> == 2)
                zp.init();
            RoundPipe<T, 2, STRICT, false>::run(x, w0, ws0, tw, jb2, N, two_p, neg_p, zp);
            const int jb3 = gbase + Arr<T, 3>::tid_index(fresh_tid(wave_base));
            RoundStage<T, 3, STRICT, false, 0>::load(w0, ws0, tw, jb3, N);
            __builtin_amdgcn_sched_barrier(0);
            h_exchange<T, 2, 3>(x, lds, fresh_tid(wave_base));
            if constexpr (kApx<STRICT> == 2)
                zp.init();
            RoundPipe<T, 3, STRICT, false>::run(x, w0, ws0, tw, jb3, N, two_p, neg_p, zp);
            const int jb4 = gbase + Arr<T, 4>::tid_index(fresh_tid(wave_base));
            u64x2 tg0[FinalStage<T>::SG * FinalStage<T>::NTW];
            if constexpr (FinalStage<T>::PIPE)
            {
                StageTw<T, 0, true, STRICT == kSchedFp64>::load(tg0, tw, jb4, N); // lands while the last exchange runs
                __builtin_amdgcn_sched_barrier(0);
            }
            h_exchange<T, 3, 4>(x, lds, fresh_tid(wave_base));
            static_assert(!bounds::fp_fwd_reduce_before_layer(12) && !bounds::fp_fwd_reduce_before_layer(13) &&
                              !bounds::fp_fwd_reduce_before_layer(14),
                          "the final round runs without a reduction (the schedule reduces inside rounds 2 and 3)");
            // ---- wait until the sibling workgroup has read its inputs (normally true ~tens of microseconds ago)
            const auto wait_for_sibling = [&] {
                if ((fresh_tid(wave_base) & 63) == 0 && tickets) // one poll per wave, no workgroup barrier
                {
                    unsigned spins = 0;
                    while (__hip_atomic_load(&tickets[row], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 2u)
                    {
                        __builtin_amdgcn_s_sleep(8);
                        if (++spins > spin_limit)
                        {
                            // never observed outside the tests that force it; do not hang the device: flag the launch as
                            // failed (host-mapped word, read by every host-visible synchronisation point) and fall through
                            __hip_atomic_store(timeout_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                            break;
                        }
                    }
                }
                // (the other lanes of the wave wait for lane 0 through re-convergence; every wave checks for itself
                //  that both workgroups of the row have finished reading)
            };
            constexpr bool XCH = kStoreExchange<T, REDUCE>;
            constexpr int SX = XCH ? 1 : (kStoreSwap<T, REDUCE> ? 2 : 0);
            if constexpr (!XCH)
                wait_for_sibling(); // the final round stores as it goes
            // ---- final round + store, group by group (arrangement 4: runs of 2^f consecutive coefficients per lane)
            // bit 0: canonicalising wrapper; bit 1: leave the last layer's first operand unreduced (kNttAnyRep)
            // bit 2 (approximate-quotient canonical launches on primes of at least 45 bits, select_fwd_half): the canonicalising
            // step estimates its small quotient in single precision (devmath.hpp reduce_small_quot)
            // (STRICT == kSchedDense, the dense lazy schedule: the last layer leaves its first operand as it is, the store reduces)
            // (SPLIT: the half ring's last layer is not the row's; the consumer reduces, select_fwd_half admitted the primes)
            const int fin = ((flags & kNttCanonical) ? 1 : 0) | (((flags & kNttAnyRep) || STRICT == kSchedDense || SPLIT) ? 2 : 0) | ((flags & kNttSmallQuot) ? 4 : 0);
            const u64 rdp_fin =
                ((STRICT == kSchedApprox && (flags & kNttSmallQuot)) || STRICT == kSchedDense) ? static_cast<u64>(__float_as_uint(small_quot_const(p))) : rdp;
            constexpr bool ROUT = REDUCE == kTreatReduceOut || REDUCE == kTreatReduceOutTopDone; // kNttReduceOut launches (never gathered: no load treatment to combine with)
            if constexpr (kFinalApx<T, STRICT> == 2)
                zp.init();
            if constexpr (FinalStage<T>::PIPE)
                FinalPipe<T, STRICT, ROUT, SX, 0>::run(x, tg0, tw, rowp, jb4, N, p, two_p, neg_p, rdp_fin, fin, zp);
            else
                FinalGroups<T, STRICT, 0, 1 << (5 - (T - 12)), ROUT, SX>::run(x, tw, rowp, jb4, N, p, two_p, neg_p, rdp_fin, fin, zp);
            if constexpr (XCH)
            {
                h_exchange<T, 4, 1>(x, lds, fresh_tid(wave_base));
                wait_for_sibling();
                if constexpr (REDUCE == kTreatModDownStore)
                {
                    // row = (polynomial pl of the launch, prime slot q): products at prod[pl][q], ciphertext component pl & 1
                    const std::size_t pl = row / map.rows, q = row % map.rows;
                    typedef const __attribute__((address_space(4))) u64 *kc_t;
                    const u64 ip = ((kc_t)src.md.inv_p)[q], ips = ((kc_t)src.md.inv_p_shoup)[q];
                    const u64 *prod_half = src.md.prod + pl * src.md.prod_stride + (q << LOGN) + gbase;
                    u64 *ct_half = src.md.ct + (pl >> 1) * src.md.ct_stride + (((pl & 1) * map.rows + q) << LOGN) + gbase;
                    const u64 *c0_half =
                        (src.md.c0_src && !(pl & 1)) ? src.md.c0_src + (pl >> 1) * src.md.c0_stride + (q << LOGN) + gbase : nullptr;
                    h_store_moddown<T>(x, fresh_tid(wave_base), prod_half, ct_half, c0_half, src.md.c0_src == nullptr, ip, ips, P.p,
                                       (src.md.tflags && (pl & 1)) ? src.md.tflags + (pl >> 1) : nullptr);
                }
                else
                    h_store_rows<T>(x, rowp + gbase, fresh_tid(wave_base));
            }
        }

        // The instances of a ring of 2^LOGN, in the order of kFwdInstances (ntt_select.hpp; null where the table says the
        // instance does not exist at this ring size), for kernel_table (ntt_half.hpp): launch_half launches from that table and
        // ntt_fwd_half_init registers from it.
        using FwdKernel = void (*)(u64 *, const PrimeDev *, RowMap, std::size_t, int, unsigned *, unsigned *, unsigned, NttSource,
                                   std::size_t, LiveSlots);
        struct FwdTable
        {
            using Kernel = FwdKernel;
            static constexpr int count = kFwdInstanceCount;
            template <int LOGN, int I>
            static Kernel at()
            {
                if constexpr (fwd_instance_at(LOGN, kFwdInstances[I]))
                    return &ntt_fwd_half_kernel<LOGN, kFwdInstances[I].sched, kFwdInstances[I].treatment>;
                else
                    return nullptr;
            }
        };
        struct FwdSplitTable // ... and those of kFwdSplitInstances
        {
            using Kernel = FwdKernel;
            static constexpr int count = kFwdSplitInstanceCount;
            template <int LOGN, int I>
            static Kernel at()
            {
                return &ntt_fwd_half_kernel<LOGN, kFwdSplitInstances[I].sched, kFwdSplitInstances[I].treatment, true>;
            }
        };

        // the facts select_fwd_half decides on, and its decision, for a launch on ring e.logn
        FwdChoice choose_fwd(const Engine &e, const RowMap &map, int flags, const NttSource &src, const LiveSlots &live)
        {
            u64 live_p[kMaxRows];
            FwdFacts f{};
            f.logn = e.logn;
            f.flags = flags;
            f.live = live_p;
            f.live_n = live.n;
            f.gathers = src.base[0] != nullptr;
            f.all_gathered = f.same_source = f.key_moduli_fp = true;
            for (int i = 0; i < live.n; i++)
            {
                live_p[i] = e.tables[map.prime[live.slot[i]]].p;
                if (f.gathers)
                {
                    f.all_gathered = f.all_gathered && src.code[live.slot[i]] != kSkipRow;
                    f.same_source = f.same_source && ((src.code[live.slot[i]] ^ src.code[live.slot[0]]) & ~kSrcReduce) == 0;
                }
            }
            for (std::size_t i = 0; f.gathers && f.key_moduli_fp && i < e.key_moduli.size(); i++)
                f.key_moduli_fp = e.key_moduli[i] < bounds::kFpInputBound;
            f.treatment = src.reduce_mode;
            f.aux_p = src.aux_p;
            f.sw = ntt_switches();
            f.suppress_signal = e.ntt_suppress_signal;
            return select_fwd_half(f);
        }

        // Which instance runs, and with which flags, is select_fwd_half's decision (ntt_select.hpp; the instances and who
        // launches them: DESIGN.md section 6). Here: the facts it decides on, the hand-off tickets, the launch.
        template <int LOGN>
        hipError_t launch_half(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags,
                               const NttSource &src)
        {
            constexpr int T = LOGN - 1;
            const std::size_t lds_bytes = static_cast<std::size_t>(hpad(1 << (T - 1))) * 8;
            if (nrows % map.rows != 0)
                return hipErrorInvalidValue;
            if (fp64_enabled() && (flags & (kNttAnyRep | kNttCanonical)) != 0 && (flags & kNttReduceOut) == 0 && !src.base[0])
            {
                RowMap a, b; // (in-place launches only: a gathered launch's sources are not known per row here)
                if (split_by_fp(e, map, a, b))
                {
                    const hipError_t err = launch_half<LOGN>(e, data, nrows, a, flags, src);
                    return err != hipSuccess ? err : launch_half<LOGN>(e, data, nrows, b, flags, src);
                }
            }
            const LiveSlots live = live_slots(map);
            if (live.n == 0)
                return hipSuccess;
            const std::size_t chunk = ((nrows / map.rows) * live.n + 7) / 8; // live rows per XCD
            const std::size_t blocks = chunk * 16;
            if (blocks > 0x7fffffffull)
                return hipErrorInvalidValue;
            const FwdChoice c = choose_fwd(e, map, flags, src, live);
            if (!c.valid)
                return hipErrorInvalidValue;
            // The transform is in place and both workgroups of a row read both halves: a ticket per row (zeroed for this
            // launch, stream-ordered) tells each when the other has finished loading -- unless the choice says that nothing
            // is handed off
            unsigned *tickets = c.tickets ? e.ntt_tickets(nrows) : nullptr;
            if (c.tickets && !tickets)
                return hipErrorOutOfMemory;
            NttSource ksrc = src;
            if (c.aux_as_doubles)
            {
                const double P = static_cast<double>(src.aux_p), Pinv = 1.0 / P;
                const double c0 = static_cast<double>(src.aux_top[0]), c2 = static_cast<double>(src.aux_top[2]);
                std::memcpy(&ksrc.aux_p, &P, 8);
                std::memcpy(&ksrc.aux_cr1, &Pinv, 8);
                std::memcpy(&ksrc.aux_top[0], &c0, 8);
                std::memcpy(&ksrc.aux_top[2], &c2, 8);
            }
            ProfScope prof(e, "ntt_fwd_half", transformed_rows(nrows, map));
            (c.split ? kernel_table<FwdSplitTable, LOGN>() : kernel_table<FwdTable, LOGN>())[c.instance]<<<static_cast<unsigned>(blocks), 1 << (LOGN - 6), lds_bytes, e.lane().stream>>>(
                data, e.d_primes, map, nrows, c.flags, tickets, e.lane().d_fault, e.ntt_spin_limit, ksrc, chunk, live);
            return hipGetLastError();
        }

    } // namespace

    hipError_t ntt_fwd_half(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags, const NttSource &src)
    {
        return at_ring_size(e.logn, [&](auto logn) { return launch_half<decltype(logn)::value>(e, data, nrows, map, flags, src); });
    }

    bool ntt_fwd_half_splits(const Engine &e, const RowMap &map, int flags, const NttSource &src)
    {
        const LiveSlots live = live_slots(map);
        if (e.logn < 14 || e.logn > 16 || live.n == 0)
            return false;
        const FwdChoice c = choose_fwd(e, map, flags | kNttSplitLast, src, live);
        return c.valid && c.split;
    }

    hipError_t ntt_fwd_half_init()
    {
        return at_every_ring_size([](auto logn) {
            constexpr int LOGN = decltype(logn)::value;
            const auto bytes = [](int) { return hpad(1 << (LOGN - 2)) * 8; };
            const hipError_t err = set_dynamic_lds(kernel_table<FwdTable, LOGN>(), FwdTable::count, bytes);
            return err != hipSuccess ? err : set_dynamic_lds(kernel_table<FwdSplitTable, LOGN>(), FwdSplitTable::count, bytes);
        });
    }
} // namespace sealhip
