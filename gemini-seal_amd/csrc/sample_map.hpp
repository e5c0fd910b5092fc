// sample_map.hpp -- the map from one 64-bit PRNG word to one RLWE sample, shared by the device
// kernels (seed_expand.hip) and the host restatement (blake2xb.cpp). One word, one sample: no rejection, no scan.
//   ternary: floor(3 w / 2^64) - 1 in {-1, 0, 1}; each value has probability 1/3 to within 2^-64.
//   noise:   the reference's sample_poly_normal law (util/rlwe.cpp:57-99): trunc(X) for X ~ N(0, 3.2^2) conditioned on
//            |X| <= 19.2 (globals.h: standard deviation 3.2, width multiplier 6). With r = w >> 1 uniform below 2^63, the
//            magnitude is the number of thresholds T_m <= r, and bit 0 of w is the sign (-0 = 0). T_m = 2^63 -
//            round(2^63 tail_m), tail_m = P(|X| >= m + 1) = (erfc((m+1)/(3.2 sqrt 2)) - erfc(6/sqrt 2)) / erf(6/sqrt 2).
// The thresholds are constants: they are never recomputed at run time, so no libm can change a word
// (tests/golden/noise_cdt.json holds the same 19 values; tests/test_sample_host.py checks both against the formula).
// All 19 comparisons always run: no branch and no table index depends on the word.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SEALHIP_SAMPLE_FN __host__ __device__ __forceinline__
#else
#define SEALHIP_SAMPLE_FN inline
#endif

namespace sealhip
{
    constexpr int kNoiseCdtSize = 19; // magnitudes 0 .. 19
    constexpr std::uint64_t kNoiseCdt[kNoiseCdtSize] = {
        0x1f67485e1414e400ULL, 0x3be85f5582810000ULL, 0x53644e2dedd21400ULL, 0x64f422f09cf1bc00ULL, 0x70dfcc250f890980ULL,
        0x7837f1b047d3fc80ULL, 0x7c535c45b5071480ULL, 0x7e690b1eb1011500ULL, 0x7f5eeb470d610900ULL, 0x7fc5bca5a5143d8cULL,
        0x7fecc2f990af3852ULL, 0x7ffa349ee365e98cULL, 0x7ffe68c004b14a13ULL, 0x7fff9a26cfa9533cULL, 0x7fffe8d1193b747aULL,
        0x7ffffb3514070e96ULL, 0x7fffff1c06e24ca0ULL, 0x7fffffdc665b1647ULL, 0x7ffffffe05c3f8adULL
    };

    enum SampleKind : std::int32_t
    {
        kSampleTernary = 0,
        kSampleNoise = 1
    };

    SEALHIP_SAMPLE_FN std::int32_t sample_ternary(std::uint64_t w)
    {
        // mulhi64(w, 3) from the two 32-bit halves (neither product overflows 64 bits)
        const std::uint64_t lo = (w & 0xFFFFFFFFULL) * 3, hi = (w >> 32) * 3 + (lo >> 32);
        return static_cast<std::int32_t>(hi >> 32) - 1;
    }

    SEALHIP_SAMPLE_FN std::int32_t sample_noise(std::uint64_t w)
    {
        const std::uint64_t r = w >> 1;
        std::int32_t mag = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int m = 0; m < kNoiseCdtSize; m++)
            mag += r >= kNoiseCdt[m] ? 1 : 0;
        const std::int32_t sign = -static_cast<std::int32_t>(w & 1); // 0 or -1
        return (mag ^ sign) - sign;
    }
} // namespace sealhip
