// keygen.hip -- the last step of KeyGenerator::generate_one_kswitch_key (keygenerator.cpp:325-369) for a batch of keys,
// written into the key buffers themselves. When it runs, c0 of every digit holds NTT(e_j) and c1 holds a_j (pipeline.cpp
// op_generate_kswitch_keys); this kernel finishes encrypt_zero_symmetric (util/rlwe.cpp:266-284) and adds the factored
// new key on the digit's own rows.
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        // reverse_bits(x, bits) of util/common.h for bits in 1..32
        __device__ __forceinline__ std::uint32_t rev_bits(std::uint32_t x, int bits)
        {
            return __brev(x) >> (32 - bits);
        }

        // GaloisTool::generate_table_ntt (galois.cpp:18-47) for one index: apply_galois_ntt reads in[pi(i)] (:188-214).
        // Element 1 is the identity.
        __device__ __forceinline__ std::uint32_t galois_ntt_index(std::uint32_t i, std::uint32_t elt, int logn)
        {
            const std::uint32_t n = 1u << logn;
            const std::uint32_t reversed = rev_bits(n + i, logn + 1);
            const std::uint64_t raw = (static_cast<std::uint64_t>(elt) * reversed) >> 1;
            return rev_bits(static_cast<std::uint32_t>(raw & (n - 1)), logn);
        }

        // One lane per coefficient pair of (key, digit j, key-level row r); row r uses prime id r.
        //   c0 <- -(c0 + c1 (.) s)                                  (rlwe.cpp:266-284, c0 = NTT(e) on entry)
        //   c0 <- c0 + factor_r * s_new[r][pi(i)]   for r in [j*nsp, min((j+1)*nsp, n_ct))   (keygenerator.cpp:350-366)
        __global__ __launch_bounds__(kThreads) void kswitch_keygen_assemble(KeygenArgs a, const PrimeDev *__restrict__ primes,
                                                                            int logn, std::size_t total_pairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t pairs_per_row = std::size_t(1) << (logn - 1);
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total_pairs;
                 i += stride)
            {
                const std::size_t c = (i & (pairs_per_row - 1)) * 2;
                std::size_t rest = i >> (logn - 1);
                const int r = static_cast<int>(rest % a.n_key);
                rest /= a.n_key;
                const int j = static_cast<int>(rest % a.digits);
                const int key = static_cast<int>(rest / a.digits);
                const PrimeDev &P = primes[r];
                u64 *c0 = a.key[key] + ((static_cast<std::size_t>(j) * 2 * a.n_key + r) << logn) + c;
                const u64 *c1 = c0 + (static_cast<std::size_t>(a.n_key) << logn);
                const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(c0);
                const ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(c1);
                const ulonglong2 sv = *reinterpret_cast<const ulonglong2 *>(a.sk + (static_cast<std::size_t>(r) << logn) + c);
                ulonglong2 out;
                out.x = neg_mod(add_mod(e.x, mul_mod(av.x, sv.x, P.p, P.cr0, P.cr1), P.p), P.p);
                out.y = neg_mod(add_mod(e.y, mul_mod(av.y, sv.y, P.p, P.cr0, P.cr1), P.p), P.p);
                const int r0 = j * a.nsp;
                if (r >= r0 && r < r0 + a.nsp && r < a.n_ct)
                {
                    const u64 *sn = a.s_new[key] + (static_cast<std::size_t>(r) << logn);
                    const std::uint32_t elt = a.elt[key];
                    const u64 f = a.factor[r];
                    u64 nx, ny;
                    if (elt == 1)
                    {
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(sn + c);
                        nx = v.x;
                        ny = v.y;
                    }
                    else
                    {
                        nx = sn[galois_ntt_index(static_cast<std::uint32_t>(c), elt, logn)];
                        ny = sn[galois_ntt_index(static_cast<std::uint32_t>(c + 1), elt, logn)];
                    }
                    out.x = add_mod(out.x, mul_mod(nx, f, P.p, P.cr0, P.cr1), P.p);
                    out.y = add_mod(out.y, mul_mod(ny, f, P.p, P.cr0, P.cr1), P.p);
                }
                *reinterpret_cast<ulonglong2 *>(c0) = out;
            }
        }
    } // namespace

    hipError_t launch_keygen_assemble(const Engine &e, const KeygenArgs &a)
    {
        const std::size_t total = static_cast<std::size_t>(a.n_keys) * a.digits * a.n_key * (e.n / 2);
        if (!total)
            return hipSuccess;
        ProfScope prof(e, "kswitch_keygen_assemble", static_cast<double>(total));
        kswitch_keygen_assemble<<<grid_for(total), kThreads, 0, e.lane().stream>>>(a, e.d_primes, e.logn, total);
        return hipGetLastError();
    }
} // namespace sealhip
