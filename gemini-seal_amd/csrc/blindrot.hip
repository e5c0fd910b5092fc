// blindrot.hip -- blind rotation: the monomial product with an exponent per batch item, read from
// device memory, as the head of every step of the TFHE accumulator loop (Chillotti, Gama, Georgieva, Izabachene, "TFHE",
// J. Cryptology 2020, Alg. 3); the LWE modulus switch from q to 2N that makes those exponents; and the indicator
// polynomials of an LWE secret that the blind-rotation keys encrypt. The fork has no such method.
// All of it is HBM streaming in the style of ringpack.hip: two coefficients per lane, 16-byte coalesced stores, the
// rotation on the load side. No LDS, no MFMA.
#include "engine.hpp"
#include "instance_dispatch.hpp"

namespace sealhip
{
    namespace
    {
        __device__ __forceinline__ u64 neg_if(bool neg, u64 v, u64 p)
        {
            return neg ? neg_mod(v, p) : v;
        }

        // dst[i] = X^(e_i) src[i] - MINUS_ONE * src[i] on both components, e_i = exps[i * exps_stride + step] mod 2N.
        // Item i of src is [2][k][N] at i * src_stride words (0: one operand shared by the batch), of dst at i * dst_stride.
        // One lane per pair of words of one row of one item; global row R = (item, component, r) in 32 bits.
        // FORM 0, coefficient form: with e' = e mod N, word x is +-src[(x - e') mod N], negated when x < e' (the wrap) xor
        //   e >= N (X^N = -1). A pair straddles the wrap when e' is odd: the two loads are scalar.
        // FORM 1, NTT form: position c holds the value at psi^(2 brev(c) + 1), so NTT(X^e)[c] = psi^(e (2 brev(c) + 1) mod 2N).
        //   psi_pow is the natural-order table {psi_r^j, Shoup companion}, j < N, per ciphertext prime; psi^(N + j) = -psi^j.
        template <int FORM, bool MINUS_ONE>
        __global__ __launch_bounds__(kThreads) void monomial_prepare_kernel(const u64 *__restrict__ src, std::size_t src_stride,
                                                                            u64 *__restrict__ dst, std::size_t dst_stride,
                                                                            const std::uint32_t *__restrict__ exps,
                                                                            std::size_t exps_stride, std::size_t step,
                                                                            const PrimeDev *__restrict__ primes,
                                                                            const ulonglong2 *__restrict__ psi_pow, unsigned k,
                                                                            int logn, std::size_t total_pairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total_pairs; i += stride)
            {
                const std::size_t w = 2 * i;
                const std::size_t c = w & nmask;
                const unsigned R = static_cast<unsigned>(w >> logn);
                const unsigned item = R / (2 * k), in_item = R - item * (2 * k);
                const unsigned r = in_item >= k ? in_item - k : in_item;
                const u64 p = primes[r].p;
                const std::size_t e = exps[item * exps_stride + step] & (2 * N - 1);
                const u64 *row = src + item * src_stride + (static_cast<std::size_t>(in_item) << logn);
                u64 o[2];
                if (FORM == 0)
                {
                    const std::size_t s = e & nmask;
                    const bool flip = e >= N;
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t x = c + h;
                        o[h] = neg_if((x < s) != flip, row[(x - s) & nmask], p);
                    }
                    if (MINUS_ONE)
                    {
                        const ulonglong2 own = *reinterpret_cast<const ulonglong2 *>(row + c);
                        o[0] = sub_mod(o[0], own.x, p);
                        o[1] = sub_mod(o[1], own.y, p);
                    }
                }
                else
                {
                    const ulonglong2 own = *reinterpret_cast<const ulonglong2 *>(row + c);
                    const u64 v[2] = { own.x, own.y };
                    const ulonglong2 *tab = psi_pow + (static_cast<std::size_t>(r) << logn);
#pragma unroll
                    for (int h = 0; h < 2; h++)
                    {
                        const std::size_t odd = 2 * static_cast<std::size_t>(__brev(static_cast<unsigned>(c + h)) >> (32 - logn)) + 1;
                        const std::size_t idx = (e * odd) & (2 * N - 1);
                        const ulonglong2 m = tab[idx & nmask];
                        o[h] = neg_if(idx >= N, mulmod_shoup(v[h], m.x, m.y, p), p);
                        if (MINUS_ONE)
                            o[h] = sub_mod(o[h], v[h], p);
                    }
                }
                store_stream2(dst + item * dst_stride + (static_cast<std::size_t>(in_item) << logn) + c, o[0], o[1]);
            }
        }

        // floor((2N x + floor(p / 2)) / p) for x < p, exact: the numerator is below 2^(64 + logn + 1); the quotient estimate is
        // barrett_reduce_128's (floor(2^128 / p) as cr0, cr1), at most two below the quotient, and is corrected by the
        // remainder. The result is in [0, 2N].
        __device__ __forceinline__ std::uint32_t scale_round(u64 x, int logn, const PrimeDev &pr)
        {
            const u64 p = pr.p, half = p >> 1;
            u64 lo = x << (logn + 1), hi = x >> (63 - logn);
            const u64 sum = lo + half;
            hi += sum < lo;
            lo = sum;
            const u64 carry = mulhi(lo, pr.cr0);
            const u64 t_lo = lo * pr.cr1, t_hi = mulhi(lo, pr.cr1);
            const u64 tmp1 = t_lo + carry;
            const u64 tmp3 = t_hi + (tmp1 < t_lo);
            const u64 u_lo = hi * pr.cr0, u_hi = mulhi(hi, pr.cr0);
            const u64 tmp1b = tmp1 + u_lo;
            const u64 carry2 = u_hi + (tmp1b < tmp1);
            u64 q = hi * pr.cr1 + tmp3 + carry2;
            u64 rem = lo - q * p; // (the true remainder is below 3p < 2^64)
#pragma unroll
            for (int it = 0; it < 2; it++)
                if (rem >= p)
                {
                    rem -= p;
                    q++;
                }
            return static_cast<std::uint32_t>(q);
        }

        // exps[i][0] = -(ms(b_i) + b_offset), exps[i][1 + j] = -ms(a_ij) (binary) or exps[i][1 + 2j] = -ms(a_ij),
        // exps[i][2 + 2j] = +ms(a_ij) (ternary), everything mod 2N, with ms(x) = scale_round(x) mod 2N. lwe_a[n][N] and lwe_b[n]
        // are level-1 samples (prime 0). One lane per pair of a words; the lane of pair 0 also writes the sample's exps[i][0].
        __global__ __launch_bounds__(kThreads) void lwe_mod_switch_kernel(const u64 *__restrict__ lwe_a, const u64 *__restrict__ lwe_b,
                                                                          std::uint32_t *__restrict__ exps, bool ternary,
                                                                          std::uint32_t b_offset, const PrimeDev *__restrict__ primes,
                                                                          int logn, std::size_t total_pairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const std::uint32_t m2 = static_cast<std::uint32_t>(2 * N - 1);
            const std::size_t row_words = 1 + (ternary ? 2 * N : N);
            const PrimeDev pr = primes[0];
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total_pairs; i += stride)
            {
                const std::size_t w = 2 * i;
                const std::size_t j = w & nmask, sample = w >> logn;
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(lwe_a + w);
                const std::uint32_t m0 = scale_round(a.x, logn, pr) & m2, m1 = scale_round(a.y, logn, pr) & m2;
                std::uint32_t *out = exps + sample * row_words;
                if (ternary)
                {
                    out[1 + 2 * j] = (0u - m0) & m2;
                    out[2 + 2 * j] = m0;
                    out[3 + 2 * j] = (0u - m1) & m2;
                    out[4 + 2 * j] = m1;
                }
                else
                {
                    out[1 + j] = (0u - m0) & m2;
                    out[2 + j] = (0u - m1) & m2;
                }
                if (j == 0)
                    out[0] = (0u - (scale_round(lwe_b[sample], logn, pr) + b_offset)) & m2;
            }
        }

        // The constant polynomials the blind-rotation keys encrypt: m[t][0] = [s_j == 1] for step t = j (binary) or t = 2j
        // (ternary), [s_j == -1] for t = 2j + 1; every other coefficient 0. One lane per pair of coefficients.
        __global__ __launch_bounds__(kThreads) void lwe_indicator_kernel(const std::int32_t *__restrict__ secret, bool ternary,
                                                                         std::int32_t *__restrict__ m_coeff, int logn,
                                                                         std::size_t total_pairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t nmask = (static_cast<std::size_t>(1) << logn) - 1;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total_pairs; i += stride)
            {
                const std::size_t w = 2 * i;
                const std::size_t t = w >> logn;
                int2 v = make_int2(0, 0);
                if ((w & nmask) == 0)
                {
                    const std::int32_t s = secret[ternary ? t >> 1 : t];
                    v.x = s == ((ternary && (t & 1)) ? -1 : 1) ? 1 : 0;
                }
                *reinterpret_cast<int2 *>(m_coeff + w) = v;
            }
        }
    } // namespace

    hipError_t launch_monomial_prepare(const Engine &e, int k, bool ntt_form, bool minus_one, const u64 *src, std::size_t src_stride,
                                       u64 *dst, std::size_t dst_stride, const std::uint32_t *exps, std::size_t exps_stride,
                                       std::size_t step, const u64 *psi_pow, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        // (the kernel divides the row index with 32-bit arithmetic; the NTT form needs its table)
        if (k < 1 || ((count * 2 * static_cast<std::size_t>(k)) >> 32) || (ntt_form && !psi_pow))
            return hipErrorInvalidValue;
        const std::size_t total = (count * 2 * static_cast<std::size_t>(k) << e.logn) / 2;
        ProfScope prof(e, "monomial_prepare", static_cast<double>(total));
        dispatch_bool(ntt_form, [&](auto ntt) {
            dispatch_bool(minus_one, [&](auto m1) {
                monomial_prepare_kernel<decltype(ntt)::value ? 1 : 0, decltype(m1)::value>
                    <<<grid_for(total), kThreads, 0, e.lane().stream>>>(src, src_stride, dst, dst_stride, exps, exps_stride, step,
                                                                        e.d_primes, reinterpret_cast<const ulonglong2 *>(psi_pow),
                                                                        static_cast<unsigned>(k), e.logn, total);
            });
        });
        return hipGetLastError();
    }

    hipError_t launch_lwe_mod_switch(const Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n_samples, bool ternary,
                                     std::uint32_t b_offset, std::uint32_t *exps)
    {
        if (!n_samples)
            return hipSuccess;
        const std::size_t total = (n_samples << e.logn) / 2;
        ProfScope prof(e, "lwe_mod_switch", static_cast<double>(total));
        lwe_mod_switch_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(
            lwe_a, lwe_b, exps, ternary, b_offset & static_cast<std::uint32_t>(2 * e.n - 1), e.d_primes, e.logn, total);
        return hipGetLastError();
    }

    hipError_t launch_lwe_indicators(const Engine &e, const std::int32_t *secret, std::size_t n_lwe, bool ternary,
                                     std::int32_t *m_coeff)
    {
        const std::size_t total = ((n_lwe * (ternary ? 2 : 1)) << e.logn) / 2;
        if (!total)
            return hipSuccess;
        ProfScope prof(e, "lwe_indicators", static_cast<double>(total));
        lwe_indicator_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(secret, ternary, m_coeff, e.logn, total);
        return hipGetLastError();
    }
} // namespace sealhip
