// homdft_entry.hpp -- one entry of a stage matrix of the homomorphic DFT (homdft_plan.hpp) by its
// closed form, for the generator kernel (homdft.hip) and its host restatement (homdft.cpp): the same function, compiled for
// both sides with contraction off, over the same tables, so the two agree bit for bit.
//
// A forward stage of layers s0 .. s0+r-1: every non-zero is a single path product,
//     M[i][col] = prod over s with bit s-1 of col set of (-1)^(bit s-1 of i) omega_(s, i mod 2^(s-1)),
// and the inverse stage is its conjugate transpose over 2^r (the caller folds 2^-r into `gain`).
// roots: the encoder's table, entry t = exp(2 pi i bitrev(t) / 2N) as {re, im}; slot_map: the encoder's slot map, whose
// entry j < N/2 is bitrev((5^j mod 2N - 1) / 2) -- it doubles as the table of powers of 5.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SEALHIP_DFT_HD __host__ __device__
#else
#define SEALHIP_DFT_HD
#endif

namespace sealhip
{
    SEALHIP_DFT_HD inline std::uint32_t dft_bitrev(std::uint32_t x, int bits)
    {
        return __builtin_bitreverse32(x) >> (32 - bits);
    }

    // gain * M[row][col] for i = row, col in one block of the stage and equal below bit s0-1 (the caller checks)
    SEALHIP_DFT_HD inline void dft_stage_entry(const double *roots, const std::uint32_t *slot_map, int logn, int s0, int r,
                                           bool inverse, std::uint32_t row, std::uint32_t col, double gain, double &re,
                                           double &im)
    {
#pragma clang fp contract(off)
        const std::uint32_t i = inverse ? col : row, c = inverse ? row : col;
        double ar = gain, ai = 0.0;
        for (int s = s0; s < s0 + r; s++)
        {
            if (!((c >> (s - 1)) & 1u))
                continue;
            const std::uint32_t j = i & ((1u << (s - 1)) - 1u);
            const std::uint32_t pow5 = 2u * dft_bitrev(slot_map[j], logn) + 1u;         // 5^j mod 2N
            std::uint32_t e = (pow5 & ((4u << s) - 1u)) << (logn + 1 - (s + 2));      // omega_(s,j) = zeta^e, e < 2N
            const bool negate = ((e >> logn) ^ (i >> (s - 1))) & 1u;                    // zeta^N = -1, and the layer's sign
            e &= (1u << logn) - 1u;
            const std::uint32_t t = dft_bitrev(e, logn);
            double wr = roots[2 * t], wi = roots[2 * t + 1];
            if (negate)
            {
                wr = -wr;
                wi = -wi;
            }
            const double pr = ar * wr - ai * wi;
            ai = ar * wi + ai * wr;
            ar = pr;
        }
        re = ar;
        im = inverse ? -ai : ai;
    }
} // namespace sealhip
