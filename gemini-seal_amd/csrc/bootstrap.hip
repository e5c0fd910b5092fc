// bootstrap.hip -- the lift of ModRaise: the centred coefficients of polynomials modulo q_0, re-read
// modulo the other primes of a higher level. Pure HBM streaming: one pass, 16-byte loads and stores, every input word read
// once; no LDS, no atomics, no memset.
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        // coef[npolys][N]: canonical residues modulo q_0 = primes[0] in coefficient form. out[npolys][k_out][N]: row i >= 1
        // of every polynomial becomes centre(x) mod q_i, canonical, in coefficient form; row 0 is not touched.
        // centre(x) = x for x <= (q_0 - 1) / 2 and x - q_0 above. q_i may be far smaller than q_0, so |centre(x)| < 2^62
        // takes barrett_reduce_63 (exact below 2^63); a negative value is then q_i minus the residue (0 stays 0).
        // One lane per pair of adjacent coefficients; the primes' constants are uniform loads.
        __global__ __launch_bounds__(kThreads) void mod_raise_lift_kernel(const u64 *__restrict__ coef, u64 *__restrict__ out,
                                                                          const PrimeDev *__restrict__ primes, int k_out, int logn,
                                                                          std::size_t npairs)
        {
            const u64 q0 = primes[0].p, half = (q0 - 1) >> 1;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < npairs; i += stride)
            {
                const std::size_t word = 2 * i;
                const std::size_t poly = word >> logn, off = word & ((static_cast<std::size_t>(1) << logn) - 1);
                const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(coef)[i];
                const bool nx = v.x > half, ny = v.y > half;
                const u64 ax = nx ? q0 - v.x : v.x, ay = ny ? q0 - v.y : v.y;
                u64 *row = out + ((poly * k_out) << logn) + off;
                for (int r = 1; r < k_out; r++)
                {
                    row += static_cast<std::size_t>(1) << logn;
                    const u64 p = primes[r].p, cr1 = primes[r].cr1;
                    const u64 rx = barrett_reduce_63(ax, p, cr1), ry = barrett_reduce_63(ay, p, cr1);
                    store_stream2(row, nx && rx ? p - rx : rx, ny && ry ? p - ry : ry);
                }
            }
        }
    } // namespace

    hipError_t launch_mod_raise_lift(const Engine &e, const u64 *coef, u64 *out, std::size_t npolys, int k_out)
    {
        if (k_out < 2 || k_out > e.k_first)
            return hipErrorInvalidValue;
        const std::size_t npairs = (npolys << e.logn) / 2;
        if (npairs == 0)
            return hipSuccess;
        ProfScope prof(e, "mod_raise_lift", 0);
        mod_raise_lift_kernel<<<grid_for(npairs), kThreads, 0, e.lane().stream>>>(coef, out, e.d_primes, k_out, e.logn, npairs);
        return hipGetLastError();
    }
} // namespace sealhip
