// dotacc.hpp -- the carry-free dot product of the fused BEHZ kernels with FOUR multiplier instructions per term.
//
// sum_i t_i * c_i for operands below 2^61 (bounds::kDotAccOperandBits). Both factors are split at bit 31, not 32:
//   t = t1*2^31 + t0 (t0 < 2^31, t1 < 2^30),  c = c1*2^31 + c0 likewise
//   L[.] += t0*c0 (< 2^62: at most 4 per accumulator)
//   M[.] += t0*c1, t1*c0 (< 2^61 each: at most 8 per accumulator)
//   H[.] += t1*c1 (< 2^60: at most 16 per accumulator)
// every product goes to a 64-bit accumulator with ONE v_mad_u64_u32 and no carry handling, and
//   sum = L + M*2^31 + H*2^62
// is assembled once per dot product. The integer sum is the one multiply_accumulate_uint64 (uintarith.h:942-958) forms.
// DotAcc (devmath.hpp) cut the low product in two 16x32 pieces for the same guarantee: five multiplier instructions.
// The overflow predicate is bounds::dotacc31_ok (ntt_bounds.hpp section 5).
//
// The wave-uniform constants are split once on the host and stored as (c1 << 32) | c0 (dot31_pack): still 8 bytes per
// constant, and each half is a whole 32-bit scalar operand.
//
// Plain 64-bit arithmetic: the header compiles for the host too (tests/dotacc_check.cpp runs it against unsigned __int128).
#pragma once

#include "ntt_bounds.hpp"

#if defined(__HIPCC__)
#define SEALHIP_HD __host__ __device__ __forceinline__
#else
#define SEALHIP_HD inline
#endif

namespace sealhip
{
    constexpr unsigned long long dot31_pack(unsigned long long c) // c < 2^61
    {
        return ((c >> 31) << 32) | (c & 0x7FFFFFFFull);
    }
    constexpr unsigned long long dot31_unpack(unsigned long long pk)
    {
        return ((pk >> 32) << 31) | (pk & 0xFFFFFFFFull);
    }

    struct Split31 // the per-lane factor, split once and reused by every dot product it takes part in
    {
        unsigned t0, t1;
        SEALHIP_HD Split31() : t0(0), t1(0) {}
        SEALHIP_HD explicit Split31(unsigned long long t)
            : t0(static_cast<unsigned>(t) & 0x7FFFFFFFu), t1(static_cast<unsigned>(t >> 31))
        {}
    };

    template <int NTERMS>
    struct DotAcc31
    {
        static_assert(bounds::dotacc31_ok(NTERMS, bounds::kDotAccOperandBits),
                      "carry-free accumulators: NTERMS products of 61-bit operands must fit (ntt_bounds.hpp section 5)");
        using u64 = unsigned long long;
        static constexpr int NL = bounds::dotacc31_nl(NTERMS), NM = bounds::dotacc31_nm(NTERMS),
                             NH = bounds::dotacc31_nh(NTERMS);
        u64 l[NL] = {}, m[NM] = {}, h[NH] = {};
        // cpk = dot31_pack(c), wave-uniform in the kernels (its halves are used whole: one scalar operand per v_mad_u64_u32)
        template <int IDX>
        SEALHIP_HD void add(const Split31 &t, u64 cpk)
        {
            static_assert(IDX >= 0 && IDX < NTERMS, "term index");
            const unsigned c0 = static_cast<unsigned>(cpk), c1 = static_cast<unsigned>(cpk >> 32);
            l[IDX % NL] += static_cast<u64>(t.t0) * c0;
            m[(2 * IDX) % NM] += static_cast<u64>(t.t0) * c1;
            m[(2 * IDX + 1) % NM] += static_cast<u64>(t.t1) * c0;
            h[IDX % NH] += static_cast<u64>(t.t1) * c1;
        }
        // (lo, hi) = L + (M + H*2^31)*2^31, below 2^128 for every admitted NTERMS
        SEALHIP_HD void finish(u64 &lo, u64 &hi) const
        {
            typedef unsigned __int128 u128;
            u128 s = m[0], r = l[0];
            for (int i = 1; i < NM; i++)
                s += m[i];
            for (int i = 0; i < NH; i++)
                s += static_cast<u128>(h[i]) << 31;
            for (int i = 1; i < NL; i++)
                r += l[i];
            r += s << 31;
            lo = static_cast<u64>(r);
            hi = static_cast<u64>(r >> 64);
        }
    };
} // namespace sealhip
