// encrypt.hip -- the element-wise tail of Encryptor::encrypt / encrypt_symmetric (native/src/seal/encryptor.cpp:106-259,
// util/rlwe.cpp:140-300) after the last transform, one pass per scheme and direction. One lane per (item, polynomial,
// coefficient) walks the rows, as divround_bfv_kernel does; every residue is canonical at every step, so the words equal
// those of the composition of the existing launches (rlwe_stage, divround_bfv / rescale_post, scaling_variant):
//   asym BFV : c_j = divround_{q_k}(P_j + lift(e_j)) [+ Delta m for j = 0]   (P_j = INTT(u (.) pk_j) over k+1 rows)
//   sym  BFV : c_0 = -(c_0 + lift(e)) [+ Delta m]                             (c_0 = INTT(a (.) s), in place)
//   asym CKKS: c_j = (P_j + 4p - T_j) q_k^{-1} [+ plain for j = 0]           (rescale_post into the destination rows)
//   sym  CKKS: c_0 = -(c_0 + a (.) s) [+ plain]                               (c_0 = NTT(lift(e)), in place)
// The pipelines around them are pipeline.cpp op_encrypt / op_encrypt_symmetric.
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        // Delta m_i = floor(q / t) m + fix  (mod q_i), scalingvariant.cpp:31-51, for the lane's coefficient
        __device__ __forceinline__ u64 scaled_plain(const EncryptArgs &a, const PrimeDev &Q, int i, u64 m, u64 fix)
        {
            return mul_add_mod(a.sc.div[i], m, fix, Q.p, Q.cr0, Q.cr1);
        }

        // asymmetric BFV: src = canonical coefficient form of u (.) pk_j over a.rows rows; DIV: a.rows = k + 1 and the
        // sum is divided and rounded by q_k (rns.cpp:731-775) into rows 0..k-1 of ct, else a.rows = k and it is stored.
        template <bool DIV>
        __global__ __launch_bounds__(kThreads) void encrypt_asym_bfv_finish_kernel(EncryptArgs a,
                                                                                   const PrimeDev *__restrict__ primes,
                                                                                   int logn, std::size_t total)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t n = std::size_t(1) << logn;
            const int k = a.k;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t c = i & (n - 1), poly = i >> logn, item = poly >> 1;
                const int j = static_cast<int>(poly & 1);
                const u64 *src = a.src + item * a.src_item_stride + static_cast<std::size_t>(j) * a.rows * n + c;
                u64 *dst = a.ct + item * a.ct_item_stride + static_cast<std::size_t>(j) * k * n + c;
                const int ev = a.e[item * 2 * n + j * n + c];
                const bool add_plain = a.plain && j == 0;
                u64 m = 0, fix = 0;
                if (add_plain)
                {
                    m = a.plain[item * a.plain_item_stride + c];
                    fix = scaling_variant_fix(a.sc, m);
                }
                u64 last = 0, half = 0;
                if (DIV)
                {
                    const PrimeDev &L = primes[k];
                    half = L.p >> 1;
                    const u64 x = add_mod(lift_small(ev, L.p), src[static_cast<std::size_t>(k) << logn], L.p);
                    last = barrett_reduce_63(x + half, L.p, L.cr1);
                }
                for (int r = 0; r < k; r++)
                {
                    const PrimeDev &Q = primes[r];
                    u64 v = add_mod(lift_small(ev, Q.p), src[static_cast<std::size_t>(r) << logn], Q.p);
                    if (DIV)
                    {
                        u64 temp = barrett_reduce_63(last, Q.p, Q.cr1);
                        temp = sub_mod(temp, barrett_reduce_63(half, Q.p, Q.cr1), Q.p);
                        v = mul_mod(sub_mod(v, temp, Q.p), a.inv_q_last[r], Q.p, Q.cr0, Q.cr1);
                    }
                    if (add_plain)
                        v = add_mod(v, scaled_plain(a, Q, r, m, fix), Q.p);
                    dst[static_cast<std::size_t>(r) << logn] = v;
                }
            }
        }

        // symmetric BFV, in place on c_0 = INTT(a (.) s): c_0 = -(c_0 + lift(e)) (rlwe.cpp:286-293) [+ Delta m]
        __global__ __launch_bounds__(kThreads) void encrypt_sym_bfv_finish_kernel(EncryptArgs a,
                                                                                  const PrimeDev *__restrict__ primes,
                                                                                  int logn, std::size_t total)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t n = std::size_t(1) << logn;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t item = i >> logn, c = i & (n - 1);
                u64 *dst = a.ct + item * a.ct_item_stride + c;
                const int ev = a.e[item * n + c];
                u64 m = 0, fix = 0;
                if (a.plain)
                {
                    m = a.plain[item * a.plain_item_stride + c];
                    fix = scaling_variant_fix(a.sc, m);
                }
                for (int r = 0; r < a.k; r++)
                {
                    const PrimeDev &Q = primes[r];
                    u64 v = neg_mod(add_mod(lift_small(ev, Q.p), dst[static_cast<std::size_t>(r) << logn], Q.p), Q.p);
                    if (a.plain)
                        v = add_mod(v, scaled_plain(a, Q, r, m, fix), Q.p);
                    dst[static_cast<std::size_t>(r) << logn] = v;
                }
            }
        }

        // asymmetric CKKS: the part of divide_and_round_q_last_ntt_inplace after the forward transforms (rns.cpp:841-849,
        // rescale_post_kernel's words, lazy temp in [0, 4p)), written into rows 0..k-1 of ct, then c_0 += plain
        // (encryptor.cpp:245-250). src: k+1 rows per polynomial (NTT form), temp: k rows per polynomial.
        __global__ __launch_bounds__(kThreads) void encrypt_asym_ckks_finish_kernel(EncryptArgs a,
                                                                                    const PrimeDev *__restrict__ primes,
                                                                                    int logn, std::size_t total)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t n = std::size_t(1) << logn;
            const int k = a.k;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t c = i & (n - 1), poly = i >> logn, item = poly >> 1;
                const int j = static_cast<int>(poly & 1);
                const u64 *src = a.src + item * a.src_item_stride + static_cast<std::size_t>(j) * a.rows * n + c;
                const u64 *tmp = a.temp + poly * static_cast<std::size_t>(k) * n + c;
                u64 *dst = a.ct + item * a.ct_item_stride + static_cast<std::size_t>(j) * k * n + c;
                const u64 *pl = (a.plain && j == 0) ? a.plain + item * a.plain_item_stride + c : nullptr;
                for (int r = 0; r < k; r++)
                {
                    const PrimeDev &Q = primes[r];
                    const std::size_t off = static_cast<std::size_t>(r) << logn;
                    u64 v = mul_mod(src[off] + (Q.p << 2) - tmp[off], a.inv_q_last[r], Q.p, Q.cr0, Q.cr1);
                    if (pl)
                        v = add_mod(v, pl[off], Q.p);
                    dst[off] = v;
                }
            }
        }

        // symmetric CKKS, in place on c_0 = NTT(lift(e)): c_0 = -(c_0 + c_1 (.) s) (rlwe.cpp:266-284) [+ plain]
        __global__ __launch_bounds__(kThreads) void encrypt_sym_ckks_finish_kernel(EncryptArgs a,
                                                                                   const PrimeDev *__restrict__ primes,
                                                                                   int logn, std::size_t total)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t n = std::size_t(1) << logn;
            const std::size_t poly = static_cast<std::size_t>(a.k) * n;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t item = i >> logn, c = i & (n - 1);
                u64 *dst = a.ct + item * a.ct_item_stride + c;
                const u64 *c1 = dst + poly;
                const u64 *sk = a.src + c;
                const u64 *pl = a.plain ? a.plain + item * a.plain_item_stride + c : nullptr;
                for (int r = 0; r < a.k; r++)
                {
                    const PrimeDev &Q = primes[r];
                    const std::size_t off = static_cast<std::size_t>(r) << logn;
                    u64 v = neg_mod(add_mod(dst[off], mul_mod(c1[off], sk[off], Q.p, Q.cr0, Q.cr1), Q.p), Q.p);
                    if (pl)
                        v = add_mod(v, pl[off], Q.p);
                    dst[off] = v;
                }
            }
        }
    } // namespace

    hipError_t launch_encrypt_finish(const Engine &e, EncryptFinish kind, const EncryptArgs &a, std::size_t count)
    {
        const bool per_poly = kind == EncryptFinish::AsymBfv || kind == EncryptFinish::AsymCkks;
        const std::size_t total = count * (per_poly ? 2 : 1) * e.n;
        if (!total)
            return hipSuccess;
        const unsigned grid = grid_for(total);
        hipStream_t s = e.lane().stream;
        switch (kind)
        {
        case EncryptFinish::AsymBfv: {
            ProfScope prof(e, "encrypt_asym_bfv_finish", static_cast<double>(total));
            if (a.rows == a.k + 1)
                encrypt_asym_bfv_finish_kernel<true><<<grid, kThreads, 0, s>>>(a, e.d_primes, e.logn, total);
            else if (a.rows == a.k)
                encrypt_asym_bfv_finish_kernel<false><<<grid, kThreads, 0, s>>>(a, e.d_primes, e.logn, total);
            else
                return hipErrorInvalidValue;
            break;
        }
        case EncryptFinish::SymBfv: {
            ProfScope prof(e, "encrypt_sym_bfv_finish", static_cast<double>(total));
            encrypt_sym_bfv_finish_kernel<<<grid, kThreads, 0, s>>>(a, e.d_primes, e.logn, total);
            break;
        }
        case EncryptFinish::AsymCkks: {
            if (a.rows != a.k + 1)
                return hipErrorInvalidValue;
            ProfScope prof(e, "encrypt_asym_ckks_finish", static_cast<double>(total));
            encrypt_asym_ckks_finish_kernel<<<grid, kThreads, 0, s>>>(a, e.d_primes, e.logn, total);
            break;
        }
        default: {
            ProfScope prof(e, "encrypt_sym_ckks_finish", static_cast<double>(total));
            encrypt_sym_ckks_finish_kernel<<<grid, kThreads, 0, s>>>(a, e.d_primes, e.logn, total);
            break;
        }
        }
        return hipGetLastError();
    }
} // namespace sealhip
