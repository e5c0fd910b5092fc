// dotacc.hpp -- the carry-free dot product of the fused BEHZ kernels with FOUR multiplier instructions per term.
//
// sum_i t_i * c_i. Both factors are split at bit S, not 32:
//   t = t1*2^S + t0 (t0 < 2^S),  c = c1*2^S + c0 likewise
//   L[.] += t0*c0,   M[.] += t0*c1, t1*c0,   H[.] += t1*c1
// every product goes to a 64-bit accumulator with ONE v_mad_u64_u32 and no carry handling, and
//   sum = L + M*2^S + H*2^(2S)
// is assembled once per dot product. The integer sum is the one multiply_accumulate_uint64 (uintarith.h:942-958) forms.
// DotAcc (devmath.hpp) cut the low product in two 16x32 pieces for the same guarantee: five multiplier instructions.
//
// How many products an accumulator takes before it can wrap depends on S and on how wide the operands are:
//   S = 31, operands below 2^61 (bounds::kDotAccOperandBits): t0*c0 < 2^62 (4 per accumulator), the cross products
//           < 2^61 (8), t1*c1 < 2^60 (16). Serves every prime the context admits (DotAcc31 below).
//   S = 30, operands below 2^60: every product is below 2^60, 16 per accumulator -- the dot products of a level with up to
//           8 primes keep ONE accumulator per part and finish() adds nothing together. The widths are those of the
//           operand classes of the kernels (bounds::behz_dot_shape): the host selects S = 30 per level where the level's
//           primes are admitted (bounds::behz_split_admits), S = 31 otherwise.
// The accumulator counts are derived from the widths by bounds::dotsplit_count, the predicate is bounds::dotsplit_ok
// (ntt_bounds.hpp section 5).
//
// The wave-uniform constants are split once on the host and stored as (c1 << 32) | c0 (dot_pack<S>): still 8 bytes per
// constant, and each half is a whole 32-bit scalar operand.
//
// Plain 64-bit arithmetic: the header compiles for the host too (tests/dotacc_check.cpp and tests/dotacc_split_check.cpp
// run it against unsigned __int128).
#pragma once

#include "ntt_bounds.hpp"

#if defined(__HIPCC__)
#define SEALHIP_HD __host__ __device__ __forceinline__
#else
#define SEALHIP_HD inline
#endif

namespace sealhip
{
    template <int S>
    constexpr unsigned long long dot_pack(unsigned long long c) // c < 2^(S + 32)
    {
        static_assert(S == 30 || S == 31, "split position");
        return ((c >> S) << 32) | (c & ((1ull << S) - 1));
    }
    template <int S>
    constexpr unsigned long long dot_unpack(unsigned long long pk)
    {
        return ((pk >> 32) << S) | (pk & 0xFFFFFFFFull);
    }
    constexpr unsigned long long dot_pack(int s, unsigned long long c) // the split as a run-time value (engine.cpp)
    {
        return s == 30 ? dot_pack<30>(c) : dot_pack<31>(c);
    }
    constexpr unsigned long long dot31_pack(unsigned long long c) { return dot_pack<31>(c); } // c < 2^61
    constexpr unsigned long long dot31_unpack(unsigned long long pk) { return dot_unpack<31>(pk); }

    template <int S>
    struct Split // the per-lane factor, split once and reused by every dot product it takes part in
    {
        static_assert(S == 30 || S == 31, "split position");
        unsigned t0, t1;
        SEALHIP_HD Split() : t0(0), t1(0) {}
        SEALHIP_HD explicit Split(unsigned long long t) // t < 2^(S + 32)
            : t0(static_cast<unsigned>(t) & ((1u << S) - 1)), t1(static_cast<unsigned>(t >> S))
        {}
    };
    using Split31 = Split<31>;

    // NTERMS products; the lane factor of term 0 is below 2^FIRST_BITS, those of the other terms below 2^LANE_BITS, the
    // constants below 2^CONST_BITS
    template <int S, int NTERMS, int FIRST_BITS, int LANE_BITS, int CONST_BITS>
    struct DotAccSplit
    {
        using u64 = unsigned long long;
        static constexpr bounds::DotShape kShape{ NTERMS, FIRST_BITS, LANE_BITS, CONST_BITS };
        static constexpr int NL = bounds::dotsplit_count(S, kShape, 0), NM = bounds::dotsplit_count(S, kShape, 1),
                             NH = bounds::dotsplit_count(S, kShape, 2);
        static_assert(NL >= 1 && NM >= 1 && NH >= 1 && bounds::dotsplit_ok(S, kShape, NL, NM, NH),
                      "carry-free accumulators: the products of these operand classes must fit (ntt_bounds.hpp section 5)");
        u64 l[NL] = {}, m[NM] = {}, h[NH] = {};
        // cpk = dot_pack<S>(c), wave-uniform in the kernels (its halves are used whole: one scalar operand per v_mad_u64_u32)
        template <int IDX>
        SEALHIP_HD void add(const Split<S> &t, u64 cpk)
        {
            static_assert(IDX >= 0 && IDX < NTERMS, "term index");
            const unsigned c0 = static_cast<unsigned>(cpk), c1 = static_cast<unsigned>(cpk >> 32);
            l[IDX % NL] += static_cast<u64>(t.t0) * c0;
            m[(2 * IDX) % NM] += static_cast<u64>(t.t0) * c1;
            m[(2 * IDX + 1) % NM] += static_cast<u64>(t.t1) * c0;
            h[IDX % NH] += static_cast<u64>(t.t1) * c1;
        }
        // (lo, hi) = L + (M + H*2^S)*2^S, below 2^128 for every admitted shape
        SEALHIP_HD void finish(u64 &lo, u64 &hi) const
        {
            typedef unsigned __int128 u128;
            u128 s = m[0], r = l[0];
            for (int i = 1; i < NM; i++)
                s += m[i];
            for (int i = 0; i < NH; i++)
                s += static_cast<u128>(h[i]) << S;
            for (int i = 1; i < NL; i++)
                r += l[i];
            r += s << S;
            lo = static_cast<u64>(r);
            hi = static_cast<u64>(r >> 64);
        }
    };
    // split at 31, every operand below 2^61
    template <int NTERMS>
    using DotAcc31 = DotAccSplit<31, NTERMS, bounds::kDotAccOperandBits, bounds::kDotAccOperandBits, bounds::kDotAccOperandBits>;
    // the dot product `KIND` (bounds::behz_dot_shape) of the exact-k BEHZ instance of split S at level K
    template <int S, int KIND, int K>
    using BehzDot = DotAccSplit<S, bounds::behz_built_shape(S, KIND, K).nterms, bounds::behz_built_shape(S, KIND, K).first_bits,
                                bounds::behz_built_shape(S, KIND, K).lane_bits, bounds::behz_built_shape(S, KIND, K).const_bits>;
} // namespace sealhip
