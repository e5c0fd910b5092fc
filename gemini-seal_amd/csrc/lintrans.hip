// lintrans.hip -- kernels of the matrix-vector product from a caller's matrix: the scan that finds
// the diagonals in use, and the gather of the pre-rotated diagonals into the BSGS grid the encoder takes. Both read the
// matrix along its generalised diagonals; every output is written exactly once (no memset, no atomics).
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        // flags[c], one workgroup per diagonal c of the d x d complex matrix: bit 0 = an entry M[i][(i + c) mod d] is
        // non-zero, re or im (-0.0 compares equal to zero; a NaN counts as non-zero), bit 1 = an entry is not finite. The
        // lanes walk the diagonal, so consecutive lanes read (d + 1) * 16 bytes apart: one 16-byte load per line touched,
        // which is what reading along a diagonal of a row-major matrix costs. The votes meet in __syncthreads_or (wave
        // ballots joined through LDS); lane 0 stores the byte, a vector store.
        __global__ __launch_bounds__(kThreads) void lintrans_occupancy_kernel(const double2 *__restrict__ matrix, std::uint32_t d,
                                                                              std::uint8_t *__restrict__ flags)
        {
            const std::uint32_t c = blockIdx.x;
            int nonzero = 0, nonfinite = 0;
            for (std::uint32_t i = threadIdx.x; i < d; i += kThreads)
            {
                const double2 v = matrix[static_cast<std::size_t>(i) * d + ((i + c) & (d - 1))];
                nonzero |= (v.x != 0.0 || v.y != 0.0) ? 1 : 0;
                nonfinite |= (v.x - v.x == 0.0 && v.y - v.y == 0.0) ? 0 : 1; // (x - x is NaN for an infinity and for a NaN)
            }
            const int any_nonzero = __syncthreads_or(nonzero);
            const int any_nonfinite = __syncthreads_or(nonfinite);
            if (threadIdx.x == 0)
                flags[c] = static_cast<std::uint8_t>((any_nonzero ? 1 : 0) | (any_nonfinite ? 2 : 0));
        }

        // out[cell - cell0][p] = {re * gain, im * gain} of M[q mod d][(q + c) mod d], q = (p - g) mod n, for the cells
        // cell0 .. cell0 + total / n - 1 of the grid: cell = gi * n_baby + bi, g = giant[gi], c = g + baby[bi]; zero when
        // diagonal c is not in use. One lane per (cell, p), grid-stride; consecutive lanes store consecutive double2 words
        // and read the matrix (d + 1) * 16 bytes apart (the diagonal's stride), wrapping every d lanes -- a cell re-reads
        // its diagonal n / d times, out of L2. The two products are separate IEEE multiplies with nothing to contract.
        __global__ __launch_bounds__(kThreads) void lintrans_values_kernel(double2 *__restrict__ out,
                                                                           const double2 *__restrict__ matrix,
                                                                           const std::uint8_t *__restrict__ mask,
                                                                           const std::int32_t *__restrict__ baby,
                                                                           const std::int32_t *__restrict__ giant, std::uint32_t n_baby,
                                                                           std::uint32_t d, int log_slots, std::size_t cell0,
                                                                           double gain, std::size_t total)
        {
            const std::uint32_t n = 1u << log_slots;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t idx = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; idx < total; idx += stride)
            {
                const std::uint32_t p = static_cast<std::uint32_t>(idx) & (n - 1);
                const std::uint32_t cell = static_cast<std::uint32_t>(cell0 + (idx >> log_slots));
                const std::uint32_t gi = cell / n_baby, bi = cell - gi * n_baby;
                const std::uint32_t g = static_cast<std::uint32_t>(giant[gi]), c = g + static_cast<std::uint32_t>(baby[bi]);
                double2 v = make_double2(0.0, 0.0);
                if (mask[c])
                {
                    const std::uint32_t q = (p - g) & (n - 1);
                    const double2 m = matrix[static_cast<std::size_t>(q & (d - 1)) * d + ((q + c) & (d - 1))];
                    v = make_double2(m.x * gain, m.y * gain);
                }
                out[idx] = v;
            }
        }
    } // namespace

    hipError_t launch_lintrans_occupancy(const Engine &e, const double *matrix, std::uint32_t d, std::uint8_t *flags)
    {
        ProfScope prof(e, "lintrans_occupancy", static_cast<double>(d) * d);
        lintrans_occupancy_kernel<<<d, kThreads, 0, e.lane().stream>>>(reinterpret_cast<const double2 *>(matrix), d, flags);
        return hipGetLastError();
    }

    hipError_t launch_lintrans_values(const Engine &e, const double *matrix, std::uint32_t d, const std::uint8_t *mask,
                                      const std::int32_t *baby, std::uint32_t n_baby, const std::int32_t *giant, std::size_t cell0,
                                      std::size_t cells, double gain, double *values)
    {
        const std::size_t total = cells << (e.logn - 1);
        if (total == 0)
            return hipSuccess;
        ProfScope prof(e, "lintrans_values", static_cast<double>(total));
        lintrans_values_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(
            reinterpret_cast<double2 *>(values), reinterpret_cast<const double2 *>(matrix), mask, baby, giant, n_baby, d, e.logn - 1,
            cell0, gain, total);
        return hipGetLastError();
    }
} // namespace sealhip
