// decrypt.hip -- Decryptor::invariant_noise_budget (decryptor.cpp:269-325) for a batch of BFV ciphertexts, from the dot
// product c_0 + c_1 s + ... (canonical residues, coefficient form, pipeline.cpp op_dot_product_ct_sk):
//   w = t v mod q_i (multiply_poly_scalar_coeffmod), W = CRT(w) in [0, Q) (RNSBase::compose_array, rns.cpp:401-450),
//   |W| centred at Q/2 (poly_infty_norm_coeffmod, util/polyarithmod.cpp:17-48), norm = max_c |W_c|,
//   budget = max(0, bits(Q) - bits(norm) - 1).
// bits() is monotone, so the kernel reduces bit counts instead of integers: bits(norm) = max_c bits(|W_c|). No multi-limb
// integer leaves a lane; one int per lane goes through a wave shuffle and LDS, then one atomicMax per workgroup into the
// item's word (an integer max does not depend on arrival order).
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        constexpr int kWave = 64;

        // One lane per coefficient c of item `blockIdx.x / blocks_per_item`; bits_out[item] = max(bits_out[item], bits(|W_c|)).
        // t is folded into the CRT constant: t_inv_punct[r] = t (Q/q_r)^{-1} mod q_r, so w_r (Q/q_r)^{-1} costs one mul_mod.
        template <int KMAX>
        __global__ __launch_bounds__(kThreads) void noise_bits_kernel(const u64 *__restrict__ v, const NoiseBudgetDev *d_,
                                                                      const PrimeDev *__restrict__ primes, int logn,
                                                                      unsigned blocks_per_item, int *__restrict__ bits_out)
        {
            const NoiseBudgetDev &d = *d_;
            const int K = d.k;
            const std::size_t n = std::size_t(1) << logn;
            const unsigned item = blockIdx.x / blocks_per_item, part = blockIdx.x - item * blocks_per_item;
            const u64 *src = v + static_cast<std::size_t>(item) * static_cast<std::size_t>(K) * n;
            int local = 0;
            for (std::size_t c = static_cast<std::size_t>(part) * blockDim.x + threadIdx.x; c < n;
                 c += static_cast<std::size_t>(blocks_per_item) * blockDim.x)
            {
                u64 acc[KMAX];
#pragma unroll
                for (int l = 0; l < KMAX; l++)
                    acc[l] = 0;
                for (int r = 0; r < K; r++)
                {
                    const PrimeDev &P = primes[r];
                    const u64 y = mul_mod(src[(static_cast<std::size_t>(r) << logn) + c], d.t_inv_punct[r], P.p, P.cr0, P.cr1);
                    const u64 *pp = d.punct + r * kMaxModuli;
                    // acc += y * (Q / q_r): below 2Q, since acc < Q and y < q_r
                    u64 carry = 0;
#pragma unroll
                    for (int l = 0; l < KMAX; l++)
                        if (l < K)
                        {
                            u64 lo = acc[l], hi = 0;
                            mac128(lo, hi, y, pp[l]);
                            const u64 s = lo + carry;
                            hi += s < lo;
                            acc[l] = s;
                            carry = hi;
                        }
                    // one conditional subtraction of Q (carry is limb K of the sum)
                    bool ge = carry != 0;
                    if (!ge)
                    {
                        ge = true;
                        bool decided = false;
#pragma unroll
                        for (int l = KMAX - 1; l >= 0; l--)
                            if (l < K && !decided && acc[l] != d.q[l])
                            {
                                ge = acc[l] > d.q[l];
                                decided = true;
                            }
                    }
                    if (ge)
                    {
                        u64 borrow = 0;
#pragma unroll
                        for (int l = 0; l < KMAX; l++)
                            if (l < K)
                            {
                                const u64 a = acc[l], b = d.q[l];
                                acc[l] = a - b - borrow;
                                borrow = (a < b) || (a == b && borrow) ? 1 : 0;
                            }
                    }
                }
                // |W| = Q - W if W >= (Q + 1) / 2 (polyarithmod.cpp:27-40)
                bool upper = true, decided = false;
#pragma unroll
                for (int l = KMAX - 1; l >= 0; l--)
                    if (l < K && !decided && acc[l] != d.half[l])
                    {
                        upper = acc[l] > d.half[l];
                        decided = true;
                    }
                if (upper)
                {
                    u64 borrow = 0;
#pragma unroll
                    for (int l = 0; l < KMAX; l++)
                        if (l < K)
                        {
                            const u64 a = d.q[l], b = acc[l];
                            acc[l] = a - b - borrow;
                            borrow = (a < b) || (a == b && borrow) ? 1 : 0;
                        }
                }
                // get_significant_bit_count_uint (uintcore.h:190-207)
                int bits = 0;
#pragma unroll
                for (int l = KMAX - 1; l >= 0; l--)
                    if (l < K && !bits && acc[l])
                        bits = 64 * l + 64 - __clzll(static_cast<long long>(acc[l]));
                local = bits > local ? bits : local;
            }
            // wave64 reduction, then the workgroup's waves through LDS
#pragma unroll
            for (int off = kWave / 2; off > 0; off >>= 1)
            {
                const int other = __shfl_xor(local, off, kWave);
                local = other > local ? other : local;
            }
            __shared__ int wave_max[kThreads / kWave];
            if ((threadIdx.x & (kWave - 1)) == 0)
                wave_max[threadIdx.x / kWave] = local;
            __syncthreads();
            if (threadIdx.x == 0)
            {
                int m = 0;
                for (int w = 0; w < static_cast<int>(blockDim.x / kWave); w++)
                    m = wave_max[w] > m ? wave_max[w] : m;
                if (m)
                    atomicMax(bits_out + item, m);
            }
        }

        template <int KMAX>
        hipError_t launch_bits(const Engine &e, const u64 *v, const NoiseBudgetDev *d, int k, std::size_t count, int *bits_out)
        {
            const std::size_t n = e.n;
            const unsigned blocks_per_item = static_cast<unsigned>(n > kThreads ? n / kThreads : 1);
            // at most 2^22 workgroups per launch: the grid stays far below 2^32 lanes
            const std::size_t per_launch = std::max<std::size_t>(1, (std::size_t(1) << 22) / blocks_per_item);
            for (std::size_t off = 0; off < count; off += per_launch)
            {
                const std::size_t m = std::min(per_launch, count - off);
                noise_bits_kernel<KMAX><<<static_cast<unsigned>(m * blocks_per_item), kThreads, 0, e.lane().stream>>>(
                    v + off * static_cast<std::size_t>(k) * n, d, e.d_primes, e.logn, blocks_per_item, bits_out + off);
                hipError_t err = hipGetLastError();
                if (err != hipSuccess)
                    return err;
            }
            return hipSuccess;
        }
    } // namespace

    hipError_t launch_noise_bits(const Engine &e, const NoiseBudgetDev *d, int k, const u64 *v, std::size_t count,
                                 int *bits_out)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "noise_budget", static_cast<double>(count * static_cast<std::size_t>(k)));
        if (k <= 4)
            return launch_bits<4>(e, v, d, k, count, bits_out);
        if (k <= 8)
            return launch_bits<8>(e, v, d, k, count, bits_out);
        if (k <= 16)
            return launch_bits<16>(e, v, d, k, count, bits_out);
        if (k <= 32)
            return launch_bits<32>(e, v, d, k, count, bits_out);
        return launch_bits<kMaxModuli>(e, v, d, k, count, bits_out);
    }
} // namespace sealhip
