// ntt_half.hpp -- what the single-pass NTT kernels for N = 2^14 .. 2^16 of both directions share (ntt_fwd.hip,
// ntt_inv.hip), and the entry points through which ntt.hip reaches them. Internal to the library.
#pragma once
#include <utility>

#include "engine.hpp"
#include "instance_dispatch.hpp"

// (library-internal: not exported from libsealhip.so)
#define SEALHIP_INTERNAL __attribute__((visibility("hidden")))

namespace sealhip
{
    // The environment switches (ntt_select.hpp NttSwitches), read once per process, defined in ntt.hip: the only getenv of
    // the NTT. SEALHIP_NTT_NO_FP64 switches the floating-point instances off; SEALHIP_NTT_EXACT_FWD switches the forward
    // transform's shortcuts off (the reference's own sequence). The STRICT-drop rule, the dense schedule and
    // ntt_strict_top_done_ok must agree about the latter within a process: all three read this one copy.
    SEALHIP_INTERNAL const NttSwitches &ntt_switches();
    SEALHIP_INTERNAL bool fp64_enabled();
    SEALHIP_INTERNAL bool exact_fwd();

    // single-pass transforms of rings of 2^14 .. 2^16 (e.logn), the caller has checked the ring size
    SEALHIP_INTERNAL hipError_t ntt_fwd_half(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags,
                                             const NttSource &src);
    SEALHIP_INTERNAL hipError_t ntt_inv_half(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags,
                                             const u64 *src = nullptr, std::size_t src_poly_stride = 0);
    // would this gathered launch, with kNttSplitLast added, select an instance of kFwdSplitInstances (else it is refused)
    SEALHIP_INTERNAL bool ntt_fwd_half_splits(const Engine &e, const RowMap &map, int flags, const NttSource &src);
    // inverse of the ciphertext tensor product formed on load (ntt_inv.hip DyadicSrc, launch_intt_tensor)
    SEALHIP_INTERNAL hipError_t ntt_inv_tensor(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, int flags,
                                               const u64 *x, std::size_t item_stride, std::size_t poly_stride, int kb,
                                               bool square);
    // the kernels' dynamic LDS limits (ntt_init_kernels)
    SEALHIP_INTERNAL hipError_t ntt_fwd_half_init();
    SEALHIP_INTERNAL hipError_t ntt_inv_half_init();

    namespace
    {
        // ----------------------------------------------------------------------------------------
        // Single-pass NTT for logn = 14..16 ("half-row" kernels). Described for the forward direction (ntt_fwd.hip); the
        // inverse (ntt_inv.hip) runs the same arrangements in the opposite order.
        //
        // After the top butterfly layer (gap N/2) the two halves of a row are independent sub-transforms.
        // One workgroup owns one half (2^T coefficients, T = logn-1): it reads BOTH halves with 16-byte
        // coalesced loads, applies the top layer on the fly (the sibling workgroup of the other half
        // recomputes the same products: +1/logn of the multiplies, and its reads of the shared half are
        // L2 hits when the two run on the same XCD, which the block -> (row, half) map arranges), and then
        // finishes all T remaining layers on chip: 32 coefficients per lane (5 index bits), radix-16 register
        // rounds, LDS exchanges between rounds. The LDS holds only half of the tile, so every exchange runs
        // in two phases keyed on index bit 0, which stays in the registers through all rounds ("sticky"):
        // coefficients with bit0 = p only ever move between slots with slot-bit0 = p. Only the exchange between
        // arrangements 1 and 2 crosses waves (workgroup barriers); the others stay inside a wave (see below).
        // HBM traffic: one read of the row (+ the sibling re-read, mostly from L2) and one write.
        //
        // Arrangement R (R = 1..3: compute rounds on index bits [T-4R, T-4R+4); R = 4: final round on the
        // remaining T-12 low bits): slot bit 0 <-> index bit 0 always; the other slot bits and the lane id
        // cover the rest as two runs of consecutive index bits.
        //
        // Round 4, wave-local arrangements. A workgroup has 2^(T-11) waves, and in
        // arrangements 2 and 3 the wave number of a lane (tid >> 6) is exactly index bits [11, T): the lane bits below
        // cover everything else. With arrangement 4's fillers on index bits [f+6, 11) instead of the top bits -- lane bits
        // 0..5 <-> index bits [f, f+6), wave number <-> bits [11, T) there as well -- a wave owns the SAME 2048 indices
        // (1024 LDS words, one contiguous range of the exchange buffer) from arrangement 2 to the store: the exchanges
        // 2 <-> 3 and 3 <-> 4 move data between lanes of one wave only. LDS instructions of a wave execute in order, so those
        // exchanges need no s_barrier at all (h_exchange): 4 workgroup barriers per transform instead of 12, and the eight
        // waves of a workgroup drift apart after round 1 -- one wave's exchange overlaps another's arithmetic inside the same
        // workgroup, where before every wave of it waited at the same barrier. Memory side unchanged per instruction (a wave
        // still covers 2^(f+6) consecutive coefficients per final-round group); its groups are now neighbours (a contiguous
        // 16 KB per wave) instead of 16 KB apart.
        template <int T, int R>
        struct Arr
        {
            static_assert(T >= 13 && T <= 15, "half-row shapes of N = 2^14 .. 2^16: 2^(T-5) lanes, i.e. 2^(T-11) waves <-> index bits [11, T)");
            static constexpr int beta = R <= 3 ? T - 4 * R : 0;
            static constexpr int f = T - 12; // low bits left for the final round (incl. bit 0)
            static constexpr int slot_bit(int w)
            {
                if (w == 0)
                    return 0;
                if (R <= 3)
                    return beta + (w - 1);
                if (w < f)
                    return w;
                return f + 6 + (w - f); // fillers: index bits [f+6, 11), just above the lane's
            }
            static constexpr int low_start = R <= 3 ? 1 : f;
            static constexpr int low_len = R <= 3 ? beta - 1 : T - 5;
            static constexpr int high_start = beta + 4;
            __device__ static __forceinline__ int tid_index(int tid)
            {
                if constexpr (R == 4)
                    return ((tid & 63) << f) | ((tid >> 6) << 11);
                int v = (tid & ((1 << low_len) - 1)) << low_start;
                if (R <= 3 && low_len < T - 5)
                    v |= (tid >> low_len) << high_start;
                return v;
            }
            // the wave number is index bits [11, T) in this arrangement
            static constexpr bool wave_owned = R == 2 || R == 3 || R == 4;
            static constexpr int slot_index(int s)
            {
                int r = 0;
                for (int w = 0; w < 5; w++)
                    if ((s >> w) & 1)
                        r |= 1 << slot_bit(w);
                return r;
            }
            // contribution of the slot bits above w to the twiddle index of a butterfly on slot bit w
            static constexpr int tw_offset(int s, int w)
            {
                int r = 0;
                for (int v = w + 1; v < 5; v++)
                    if ((s >> v) & 1)
                        r |= 1 << (slot_bit(v) - slot_bit(w) - 1);
                return r;
            }
        };

        // streaming 16-byte store / load: the transformed rows are not read again by this kernel, keeping them out of
        // the way of the twiddle tables in L2 is worth 4 % (nontemporal hint)
        typedef u64 u64x2_nt __attribute__((ext_vector_type(2)));
        __device__ __forceinline__ void store_nt(u64 *p, u64 a, u64 b)
        {
            u64x2_nt v;
            v.x = a;
            v.y = b;
            __builtin_nontemporal_store(v, reinterpret_cast<u64x2_nt *>(p));
        }

        // LDS image of the exchange buffer: two pad words per 32 and one more for the odd 16-word blocks. With
        // 2 * (e >> 5) alone the final arrangement (lanes two words apart) had two-way bank conflicts
        // (SQ_LDS_BANK_CONFLICT 2048 per row at N = 2^15); this form measures zero (tools/hpad_sweep.sh).
        __host__ __device__ constexpr int hpad(int e)
        {
            return e + 2 * (e >> 5) + ((e >> 4) & 1);
        }

        template <int T, int RA, int RB>
        __device__ __forceinline__ void h_exchange(u64 (&x)[32], u64 *lds, int tid)
        {
            const int pa = hpad(Arr<T, RA>::tid_index(tid) >> 1);
            const int pb = hpad(Arr<T, RB>::tid_index(tid) >> 1);
            // both arrangements wave-owned: every word a wave writes is read by the same wave and by no other. The LDS
            // executes a wave's instructions in order, so the hardware needs nothing; the fences keep the compiler from
            // moving a read above the writes it depends on (they emit no instruction at wavefront scope).
            constexpr bool LOCAL = Arr<T, RA>::wave_owned && Arr<T, RB>::wave_owned;
            const auto sync = [] {
                if constexpr (LOCAL)
                {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
                else
                    __syncthreads();
            };
#pragma unroll
            for (int phase = 0; phase < 2; phase++)
            {
#pragma unroll
                for (int s = 0; s < 32; s++)
                    if ((s & 1) == phase)
                        lds[pa + hpad(Arr<T, RA>::slot_index(s) >> 1)] = x[s];
                sync();
#pragma unroll
                for (int s = 0; s < 32; s++)
                    if ((s & 1) == phase)
                        x[s] = lds[pb + hpad(Arr<T, RB>::slot_index(s) >> 1)];
                sync();
            }
        }

        // Twiddle tables are read-only for the lifetime of a context: load them through the global
        // (address_space 1) or, when the index is wave-uniform, the constant (address_space 4, scalar cache)
        // address space instead of the generic pointer stored in PrimeDev (which would give flat loads).
        typedef u64 u64x2 __attribute__((ext_vector_type(2)));
        typedef const __attribute__((address_space(1))) u64x2 *tw_global_t;
        typedef const __attribute__((address_space(4))) u64x2 *tw_const_t;
        // the floating-point variant's tables hold one double per twiddle (PrimeDev::fwd_d / inv_d), moved as 64-bit words
        typedef const __attribute__((address_space(1))) u64 *twd_global_t;
        typedef const __attribute__((address_space(4))) u64 *twd_const_t;
        // In the floating-point instances (STRICT == kSchedFp64 forward, LZ == kInvFp64 inverse) the registers x[] hold the bit patterns
        // of doubles, the parameters named two_p / neg_p carry the bits of p and 1/p as doubles, and tw points to the
        // double table. Reduction schedule of the forward transform (ntt_bounds.hpp section 4 holds the derivation and the
        // recurrence the CPU test runs). With U = 2^50 >= p and B a bound on the magnitudes, a layer gives
        // |y*w mod p| <= (0.5 + 3 * 2^-53 |y|) p -- the quotient estimate's rounding, the relative 2^-52 of h * (1/p) AND the
        // exact rounding error l of the product -- so B' <= 1.375 B + 0.5 U: from a reduction (B = 0.5 U) FIVE layers stay
        // below 8 U = 2^53 (1.19, 2.13, 3.43, 5.22, 7.68), from raw inputs below 2^52 the top layer does (6 U). Hence: all
        // values to [-p/2, p/2] after the top layer, after round 2's first layer and after round 3's second (spans of 5, 5 and
        // at most 2 + 3 layers, the last followed by the canonicalisation): every operation is exact. (Round 2 reduced after
        // round 2's second layer and before the final round -- two spans of six layers, sound only under the bound
        // (0.5 + 2^-52 |y|) p, which ignores l: ADVICE r02.)
        __device__ __forceinline__ void fp_reduce_all(u64 (&x)[32], u64 p_bits, u64 pinv_bits)
        {
            const double p = fp_of(p_bits), pinv = fp_of(pinv_bits);
#pragma unroll
            for (int i = 0; i < 32; i++)
                x[i] = fp_bits(fp_reduce(fp_of(x[i]), p, pinv));
        }
        constexpr int kIL = 4; // butterflies advanced in lock step (devmath.hpp: butterflies_fwd_hs)
        using ZeroPairs = ZeroHi<2>; // devmath.hpp mulhi_apx2: written where a phase starts (two v_mov), each used by two of the four lock-step butterflies

        // ---- pipelined final round. A stage = SG groups; the twiddles of stage k+1 are requested before stage k is
        // computed and stored, so their L2 latency is covered by a stage of arithmetic instead of being exposed at
        // every sched_barrier. Twiddles of one group, in the order used: layer W = f-1 (1 entry), f-2 (2), ... 0.
        template <int T>
        struct FinalStage
        {
            static constexpr int f = T - 12;
            static constexpr int NTW = (1 << f) - 1;            // twiddles per group
            static constexpr int SG = f == 1 ? 4 : (f == 2 ? 2 : 1); // groups per stage
            static constexpr int NG = 1 << (5 - f);
            static constexpr int NS = NG / SG;
            static constexpr bool PIPE = f <= 2; // f = 3: two stages of 28 twiddle registers do not fit
        };

        // The twiddles of one group of 2^f registers (those that share the filler slot bits G), held in tg[] in the order the
        // direction uses its layers: DESC (forward) W = f-1 (1 entry), f-2 (2), ..., 0; else (inverse) W = 0 (2^(f-1) entries),
        // 1, ..., f-1 (1 entry). Entry o of layer W serves the butterflies of the elements e with e >> (W + 1) == o.
        template <int T, bool DESC>
        struct GroupTw
        {
            static constexpr int f = T - 12;
            static constexpr int at(int W, int e) // place in tg[] of the twiddle of layer W's butterfly on element e
            {
                return (DESC ? (1 << (f - 1 - W)) - 1 : (1 << f) - (1 << (f - W))) + (e >> (W + 1));
            }
            // loads issued in the order of tg[]
            template <int G, bool FP>
            __device__ static __forceinline__ void load(u64x2 *tg, const u64 *__restrict__ tw, int jb, int N)
            {
#pragma unroll
                for (int k = 0; k < f; k++)
                {
                    const int W = DESC ? f - 1 - k : k;
                    const int tb = (N + jb) >> (Arr<T, 4>::slot_bit(W) + 1);
#pragma unroll
                    for (int o = 0; o < (1 << (f - 1 - W)); o++)
                    {
                        const int e = o << (W + 1), s = (G << f) | e;
                        if constexpr (FP)
                            tg[at(W, e)].x = ((twd_global_t)tw)[tb + Arr<T, 4>::tw_offset(s, W)];
                        else
                            tg[at(W, e)] = ((tw_global_t)tw)[tb + Arr<T, 4>::tw_offset(s, W)];
                    }
                }
            }
        };
        template <int T, int ST, bool DESC, bool FP, int I = 0>
        struct StageTw // twiddle loads of stage ST (FinalStage<T>::SG groups)
        {
            __device__ static __forceinline__ void load(u64x2 *tg, const u64 *__restrict__ tw, int jb, int N)
            {
                GroupTw<T, DESC>::template load<ST * FinalStage<T>::SG + I, FP>(tg + I * FinalStage<T>::NTW, tw, jb, N);
                if constexpr (I + 1 < FinalStage<T>::SG)
                    StageTw<T, ST, DESC, FP, I + 1>::load(tg, tw, jb, N);
            }
        };

        // A stage of a compute round in arrangement R: kIL butterflies of layer W (slot bit W), the C-th .. (C+kIL-1)-th of its
        // 16. Its slots, and the loads of its twiddles: doubles moved as 64-bit words (FP) or (w, w') pairs; through the
        // scalar cache where the index is wave-uniform (UNIFORM), else global loads.
        template <int T, int R, int W, int C, bool UNIFORM, bool FP>
        struct Stage
        {
            static constexpr int bit = 1 << W;
            static constexpr int slot(int j)
            {
                return (((C + j) >> W) << (W + 1)) | ((C + j) & (bit - 1)); // the (C+j)-th slot with bit W clear
            }
            __device__ static __forceinline__ void load(u64 (&w)[kIL], u64 (&ws)[kIL], const u64 *__restrict__ tw, int jb,
                                                        int N)
            {
                const int tb = (N + jb) >> (Arr<T, R>::slot_bit(W) + 1);
#pragma unroll
                for (int j = 0; j < kIL; j++)
                {
                    u64x2 Wv;
                    if constexpr (FP)
                    {
                        Wv.x = UNIFORM ? ((twd_const_t)tw)[__builtin_amdgcn_readfirstlane(tb) + Arr<T, R>::tw_offset(slot(j), W)]
                                       : ((twd_global_t)tw)[tb + Arr<T, R>::tw_offset(slot(j), W)];
                        Wv.y = 0;
                    }
                    else if (UNIFORM)
                        Wv = ((tw_const_t)tw)[__builtin_amdgcn_readfirstlane(tb) + Arr<T, R>::tw_offset(slot(j), W)];
                    else
                        Wv = ((tw_global_t)tw)[tb + Arr<T, R>::tw_offset(slot(j), W)];
                    w[j] = Wv.x;
                    ws[j] = Wv.y;
                }
            }
        };
        constexpr int kStagesPerLayer = 16 / kIL;

        // XCD-aware block -> (row, part) map (speed only; any placement gives the same result). A row is transformed by
        // 2^PARTS_LOG2 workgroups: its two halves (the forward kernel, the half-row inverse), one (the whole-row inverse) or
        // four quarters (the quarter-row inverse). Blocks are dealt
        // round-robin over the 8 XCDs, each with its own 4 MB L2. Rows are enumerated prime-major
        // (v = position * npolys + poly, positions = the LIVE slots of a polynomial in slot order) and XCD x gets the
        // contiguous range [x*chunk, (x+1)*chunk): it then touches at most two primes, so their twiddle tables (512 KB
        // each at N=2^15) stay L2-resident instead of all rows_per_poly tables thrashing every L2 (measured: HBM reads
        // 583 -> 377 KB per row at N=2^15). Slots mapped to kSkipRow are left out of the enumeration: counting them
        // left the XCD that owned a skipped slot idle (the key-switch launches skip one slot in k+1, and the CKKS
        // special-row launches transform one slot in k+1: one XCD did all the work).
        // The parts of a row are consecutive blocks of one XCD. (The tensor-load inverse enumerates in an order of its own:
        // ntt_inv.hip.)
        struct LiveSlots
        {
            int n;
            unsigned short slot[kMaxRows];
        };
        inline LiveSlots live_slots(const RowMap &map)
        {
            LiveSlots ls{};
            for (int r = 0; r < map.rows; r++)
                if (map.prime[r] != kSkipRow)
                    ls.slot[ls.n++] = static_cast<unsigned short>(r);
            return ls;
        }
        // -> false when the block has nothing to do; else the polynomial index and the position among the live slots, and which half or quarter of
        // that row (`part`)
        // poly_major = g > 0 (two parts per row only: the key switch's digit launches, whose live rows all gather ONE source row): groups of g live
        // positions interleaved item by item, so that g readers of a source row run next to each other on one XCD and the row is
        // fetched from HBM n_live / g times instead of n_live times -- at the price of an XCD touching up to 2g twiddle tables
        // instead of two. Round 3, config 3 (integer instances, seven readers per source row, 512 KB per table): forward
        // transforms 17.34 ms per 1024 pairs at g = 1, 17.18 / 17.10 / 16.98 at g = 2 / 3 / 4, 17.13 at g = 7 (the tables start
        // to thrash the 4 MB L2); step 44.98 -> 44.51 ms at g = 4. Config 4 (FP64, eleven readers): the transforms gain 2.5 % at
        // g = 11 but the inner product, which reads what they wrote in the old order, loses as much: off there.
        // select_fwd_half (ntt_select.hpp): g = 4, integer launches only.
        template <int PARTS_LOG2>
        __device__ __forceinline__ bool block_place(unsigned bid, std::size_t npolys, int n_live, std::size_t chunk,
                                                    std::size_t &poly, int &position, int &part, int poly_major = 0)
        {
            static_assert(PARTS_LOG2 >= 0 && PARTS_LOG2 <= 2, "one, two or four workgroups per row");
            const unsigned xcd = bid & 7u;
            const std::size_t slot = bid >> 3;
            part = static_cast<int>(slot & ((1u << PARTS_LOG2) - 1));
            const std::size_t v = static_cast<std::size_t>(xcd) * chunk + (slot >> PARTS_LOG2);
            if ((slot >> PARTS_LOG2) >= chunk || v >= npolys * static_cast<std::size_t>(n_live))
                return false;
            if constexpr (PARTS_LOG2 == 1)
                if (poly_major)
                {
                    // groups of g consecutive live positions interleaved item by item: v = (group * npolys + poly) * g + b
                    // (g = n_live: item-major; the last group may be shorter)
                    const int g = poly_major;
                    const std::size_t full = static_cast<std::size_t>(n_live / g) * npolys * g; // rows in complete groups
                    if (v < full)
                    {
                        const std::size_t gp = v / g;
                        position = static_cast<int>(gp / npolys) * g + static_cast<int>(v - gp * g);
                        poly = gp % npolys;
                    }
                    else
                    {
                        const int rem = n_live % g; // > 0 here
                        const std::size_t u = v - full, gp = u / rem;
                        position = (n_live / g) * g + static_cast<int>(u - gp * rem);
                        poly = gp;
                    }
                    return true;
                }
            poly = v % npolys;
            position = static_cast<int>(v / npolys);
            return true;
        }

        // A fresh copy of the thread index. Everything a phase derives from it (coefficient indices, LDS addresses,
        // twiddle indices) is then computed where the phase starts instead of at the top of the kernel, where it
        // would sit in registers -- or in scratch, whose write-back showed up as +28 % HBM write traffic -- until used.
        // Round 3: not even threadIdx.x is kept (an opaque copy of it was, before). These kernels run at the 128-register cap, and the one value
        // every phase needs -- threadIdx.x -- was what the allocator spilled (1-6 dwords of scratch in eight inverse instances).
        // The wave's base index is uniform (an SGPR), the lane id comes from v_mbcnt: two full-rate instructions wherever a
        // phase starts, no register held across the rounds. (volatile: never merged with an earlier copy)
        __device__ __forceinline__ int fresh_tid(int wave_base)
        {
            int lane;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
            return wave_base + lane;
        }

        // rows a launch really transforms (rows mapped to kSkipRow are left alone): the unit count of the profiler
        inline double transformed_rows(std::size_t nrows, const RowMap &map)
        {
            int live = 0;
            for (int r = 0; r < map.rows; r++)
                live += map.prime[r] != kSkipRow;
            return static_cast<double>(nrows / map.rows) * live;
        }

        // A launch whose live rows mix primes below 2^50 with larger ones (the usual CKKS chain: 60-bit ends, 40-bit middle)
        // is issued as two: the rows that can take the floating-point instance, then the others. -> true when both kinds
        // are live; `fp_rows` / `rest` are the map with the other kind masked out.
        inline bool split_by_fp(const Engine &e, const RowMap &map, RowMap &fp_rows, RowMap &rest)
        {
            fp_rows = rest = map;
            int n_fp = 0, n_rest = 0;
            for (int r = 0; r < map.rows; r++)
            {
                if (map.prime[r] == kSkipRow)
                    continue;
                if (e.tables[map.prime[r]].p < kFpPrimeBound)
                {
                    rest.prime[r] = kSkipRow;
                    n_fp++;
                }
                else
                {
                    fp_rows.prime[r] = kSkipRow;
                    n_rest++;
                }
            }
            return n_fp > 0 && n_rest > 0;
        }

        // The kernels of a ring of 2^LOGN in the order of an instance table of ntt_select.hpp. Of names the table:
        // Of::Kernel, Of::count, and Of::at<LOGN, I>(), the kernel of instance I at that ring size or null where the table says
        // there is none. The launchers launch from this table and register from it.
        template <class Of, int LOGN, int... I>
        const typename Of::Kernel *kernel_table(std::integer_sequence<int, I...>)
        {
            static const typename Of::Kernel table[] = { Of::template at<LOGN, I>()... };
            return table;
        }
        template <class Of, int LOGN>
        const typename Of::Kernel *kernel_table()
        {
            return kernel_table<Of, LOGN>(std::make_integer_sequence<int, Of::count>{});
        }
        // the dynamic LDS limit of every kernel of a table (the default suffices for the 2^13-coefficient shape only)
        template <class Kernel, class Bytes>
        hipError_t set_dynamic_lds(const Kernel *table, int count, Bytes bytes_of)
        {
            for (int i = 0; i < count; i++)
                if (table[i])
                {
                    const hipError_t err =
                        hipFuncSetAttribute(reinterpret_cast<const void *>(table[i]), hipFuncAttributeMaxDynamicSharedMemorySize, bytes_of(i));
                    if (err != hipSuccess)
                        return err;
                }
            return hipSuccess;
        }
        // f(std::integral_constant<int, LOGN>{}) -> hipError_t at the ring size logn; at every ring size, until one fails
        template <class F>
        hipError_t at_ring_size(int logn, F &&f)
        {
            hipError_t err = hipErrorInvalidValue; // (no single-pass kernel for this ring)
            dispatch_among<14, 15, 16>(logn, [&](auto n) { err = f(n); });
            return err;
        }
        template <class F>
        hipError_t at_every_ring_size(F &&f)
        {
            hipError_t err = hipSuccess;
            for (int logn = 14; logn <= 16 && err == hipSuccess; logn++)
                err = at_ring_size(logn, f);
            return err;
        }
    } // namespace
} // namespace sealhip
