// homdft.hip -- kernels of the homomorphic DFT: the generator of a stage's pre-rotated diagonals, and
// the real/imaginary split and merge that go with CoeffToSlot and SlotToCoeff. The generator is a gather (every output word
// is written exactly once: no memset, no atomics); split and merge are pure HBM streaming, 16-byte loads and stores, one pass.
#include "engine.hpp"
#include "homdft_entry.hpp"

namespace sealhip
{
    namespace
    {
        // out[g][b][p] = gain * M[i][i + c h0], i = (p - giant step) mod n, c = c_g n_baby + b: cell [g][b] of the BSGS grid
        // is diagonal c rotated by minus its giant step. One lane per (cell, p); log_baby = log2 n_baby, half_giant the
        // offset of c_g (0 for the folded top stage, n_giant / 2 otherwise).
        __global__ __launch_bounds__(kThreads) void dft_stage_values_kernel(double2 *__restrict__ out,
                                                                            const double *__restrict__ roots,
                                                                            const std::uint32_t *__restrict__ slot_map, int logn,
                                                                            int s0, int r, int inverse, int folded, int log_baby,
                                                                            int half_giant, double gain, std::size_t total)
        {
            const int L = logn - 1;
            const std::uint32_t n = 1u << L;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t idx = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; idx < total; idx += stride)
            {
                const std::uint32_t p = static_cast<std::uint32_t>(idx) & (n - 1);
                const std::uint32_t cell = static_cast<std::uint32_t>(idx >> L);
                const long long b = cell & ((1u << log_baby) - 1), cg = static_cast<long long>(cell >> log_baby) - half_giant;
                const long long c = cg * (1ll << log_baby) + b;
                const std::uint32_t giant = static_cast<std::uint32_t>((cg * (1ll << (log_baby + s0 - 1))) & (n - 1));
                const std::uint32_t i = (p - giant) & (n - 1);
                const long long col_raw = static_cast<long long>(i) + c * (1ll << (s0 - 1));
                const std::uint32_t col = static_cast<std::uint32_t>(col_raw) & (n - 1);
                const bool inside = folded || (col_raw >= 0 && col_raw < static_cast<long long>(n) &&
                                               (col >> (s0 - 1 + r)) == (i >> (s0 - 1 + r)));
                double2 v = make_double2(0.0, 0.0);
                if (inside)
                    dft_stage_entry(roots, slot_map, logn, s0, r, inverse != 0, i, col, gain, v.x, v.y);
                out[idx] = v;
            }
        }

        // CoeffToSlot's tail. a = c', b = sigma_(2N-1)(c'), both count x 2 x k x N in NTT form:
        //     re = a + b,   im = -i (a - b) = X^(N/2) (.) (b - a).
        // NTT(X^(N/2)) at position c of row r is psi_r^(N/2) for c < N/2 and its negative above: the transform's output
        // position c is the evaluation at psi^(2 bitrev(c) + 1), whose parity of bitrev(c) is the top bit of c.
        // psi^(N/2), with its Shoup quotient, is entry 1 of the row's forward twiddle table.
        __global__ __launch_bounds__(kThreads) void dft_conj_split_kernel(const u64 *__restrict__ a, const u64 *__restrict__ b,
                                                                          u64 *__restrict__ re, u64 *__restrict__ im,
                                                                          const PrimeDev *__restrict__ primes, RowMap map, int logn,
                                                                          std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs; i += stride)
            {
                const std::size_t word = 2 * i;
                const PrimeDev &P = primes[map.prime[(word >> logn) % map.rows]];
                const u64 w = P.fwd[2], ws = P.fwd[3];
                const bool upper = (word >> (logn - 1)) & 1;
                const ulonglong2 va = reinterpret_cast<const ulonglong2 *>(a)[i];
                const ulonglong2 vb = reinterpret_cast<const ulonglong2 *>(b)[i];
                // (b - a) in the lower half, (a - b) in the upper one, where the factor is -psi^(N/2)
                const u64 dx = upper ? sub_mod(va.x, vb.x, P.p) : sub_mod(vb.x, va.x, P.p);
                const u64 dy = upper ? sub_mod(va.y, vb.y, P.p) : sub_mod(vb.y, va.y, P.p);
                store_stream2(re + word, add_mod(va.x, vb.x, P.p), add_mod(va.y, vb.y, P.p));
                store_stream2(im + word, mulmod_shoup(dx, w, ws, P.p), mulmod_shoup(dy, w, ws, P.p));
            }
        }

        // SlotToCoeff's head: out = re + X^(N/2) (.) im, the operands count x 2 x k x N in NTT form
        __global__ __launch_bounds__(kThreads) void dft_merge_kernel(const u64 *__restrict__ re, const u64 *__restrict__ im,
                                                                     u64 *__restrict__ out, const PrimeDev *__restrict__ primes,
                                                                     RowMap map, int logn, std::size_t npairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs; i += stride)
            {
                const std::size_t word = 2 * i;
                const PrimeDev &P = primes[map.prime[(word >> logn) % map.rows]];
                const u64 w = P.fwd[2], ws = P.fwd[3];
                const bool upper = (word >> (logn - 1)) & 1;
                const ulonglong2 vr = reinterpret_cast<const ulonglong2 *>(re)[i];
                const ulonglong2 vi = reinterpret_cast<const ulonglong2 *>(im)[i];
                const u64 tx = mulmod_shoup(vi.x, w, ws, P.p), ty = mulmod_shoup(vi.y, w, ws, P.p);
                store_stream2(out + word, upper ? sub_mod(vr.x, tx, P.p) : add_mod(vr.x, tx, P.p),
                              upper ? sub_mod(vr.y, ty, P.p) : add_mod(vr.y, ty, P.p));
            }
        }
    } // namespace

    hipError_t launch_dft_stage_values(const Engine &e, int s0, int r, bool inverse, bool folded, std::uint32_t n_baby,
                                       std::uint32_t n_giant, double gain, double *values)
    {
        int log_baby = 0;
        while ((1u << log_baby) < n_baby)
            log_baby++;
        const std::size_t total = (static_cast<std::size_t>(n_baby) * n_giant) << (e.logn - 1);
        dft_stage_values_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(
            reinterpret_cast<double2 *>(values), e.d_ckks_roots, e.d_ckks_map, e.logn, s0, r, inverse ? 1 : 0, folded ? 1 : 0,
            log_baby, folded ? 0 : static_cast<int>(n_giant / 2), gain, total);
        return hipGetLastError();
    }

    hipError_t launch_dft_conj_split(const Engine &e, const u64 *a, const u64 *b, u64 *re, u64 *im, std::size_t count,
                                     const RowMap &map)
    {
        const std::size_t npairs = (count * 2 * static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (npairs == 0)
            return hipSuccess;
        dft_conj_split_kernel<<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(a, b, re, im, e.d_primes, map, e.logn, npairs);
        return hipGetLastError();
    }

    hipError_t launch_dft_merge(const Engine &e, const u64 *re, const u64 *im, u64 *out, std::size_t count, const RowMap &map)
    {
        const std::size_t npairs = (count * 2 * static_cast<std::size_t>(map.rows) << e.logn) / 2;
        if (npairs == 0)
            return hipSuccess;
        dft_merge_kernel<<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(re, im, out, e.d_primes, map, e.logn, npairs);
        return hipGetLastError();
    }
} // namespace sealhip
