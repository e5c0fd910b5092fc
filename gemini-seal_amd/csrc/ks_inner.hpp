// ks_inner.hpp -- the key switch's inner product, stated once for the kernels of keyswitch.hip and hoist.hip:
//   prod[l][r][c] = ( sum_j D_j[r][.] * K[j][l][row_prime r][c] ) mod p_r          (evaluator.cpp:2315-2349)
// D_j is the target's own NTT-form row when r lies in bundle j (the row's own digit), else row r of the extended digit j;
// the key is laid out [2j + l][n_total][N]. Device only, internal to the library.
#pragma once
#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        // The context's dimensions, read before a kernel splits its lane index (and before its early exit).
        struct MacDims
        {
            int k, nsp, rows, n_total; // ciphertext primes, special primes, k + nsp extended rows, primes of the key
        };
        __device__ __forceinline__ MacDims mac_dims(const KsDev *d) { return {d->k, d->nsp, d->k + d->nsp, d->n_total}; }

        // What a lane needs to know about extended row r of a ring of N. That the offsets are methods (formed at first use), r and
        // N references, and the dimensions and the prime structs of their own is what keeps the kernels' code as it was:
        // profiles/r21/device_code.txt, "What the compiler made of the forms". Compare the assembly before tidying any of it.
        struct MacRow
        {
            int rows, n_total, r, rns_idx, my_digit; // rns_idx = row_prime[r]; my_digit: whose bundle holds row r (-1: a special row)
            std::size_t N;
            // the row in a set of extended rows; between a product's two components; between key slices; the row in a key slice
            __device__ __forceinline__ std::size_t row_off() const { return static_cast<std::size_t>(r) * N; }
            __device__ __forceinline__ std::size_t comp() const { return static_cast<std::size_t>(rows) * N; }
            __device__ __forceinline__ std::size_t key_comp() const { return static_cast<std::size_t>(n_total) * N; }
            __device__ __forceinline__ std::size_t prime_row() const { return static_cast<std::size_t>(rns_idx) * N; }
            // where component l of digit j starts in the key, laid out [2j + l][n_total][N]
            __device__ __forceinline__ std::size_t key_slice(int j, int l) const { return (2 * static_cast<std::size_t>(j) + l) * key_comp(); }
        };
        __device__ __forceinline__ MacRow mac_row(const MacDims &dim, const KsDev *d, const int &r, const std::size_t &N)
        {
            return {dim.rows, dim.n_total, r, static_cast<int>(d->row_prime[r]), r < dim.k ? r / dim.nsp : -1, N};
        }

        // The row's prime, loaded where the kernel calls this: before the key words, after the first digit words or after the loop.
        struct MacMod
        {
            u64 p, two_p, cr0, cr1;
            __device__ __forceinline__ u64 reduce(u64 lo, u64 hi) const { return barrett_reduce_128(lo, hi, p, cr0, cr1); }
        };
        __device__ __forceinline__ MacMod mac_mod(const PrimeDev *__restrict__ primes, const MacRow &m)
        {
            const PrimeDev &P = primes[m.rns_idx];
            return {P.p, P.two_p, P.cr0, P.cr1};
        }

        // The two lane maps; each kernel splits q itself. Flat: lane i of the grid is coefficient c of unit q. Block-uniform: a workgroup
        // lies inside one row (N >= kThreads, the launcher sees to it), so q and all that comes of it are wave-uniform (scalar registers).
        struct MacLane
        {
            std::size_t c, q;
        };
        __device__ __forceinline__ MacLane flat_lane(int logn)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            return {i & ((static_cast<std::size_t>(1) << logn) - 1), i >> logn};
        }
        __device__ __forceinline__ MacLane block_lane(std::size_t N) // (q fits 32 bits: the kernels split it as unsigned)
        {
            const unsigned blocks_per_row = static_cast<unsigned>(N / kThreads);
            return {static_cast<std::size_t>(blockIdx.x % blocks_per_row) * kThreads + threadIdx.x, blockIdx.x / blocks_per_row};
        }

        // One digit word against its two key words: the two 128-bit accumulators of a lane, one per component.
        __device__ __forceinline__ void mac2(u64 x, u64 k0, u64 k1, u64 &lo0, u64 &hi0, u64 &lo1, u64 &hi1)
        {
            mac128(lo0, hi0, x, k0);
            mac128(lo1, hi1, x, k1);
        }

        // Loop form, the key words streamed: digit j of one ciphertext added into the lane's accumulators. pkey is the lane's word
        // of key slice 0, own the row's word of its own digit (the target), pext the row's word of digit 0 of ext.
        __device__ __forceinline__ void digit_mac(const MacRow &m, int j, const u64 *pext, std::size_t ext_digit_stride, const u64 *pkey,
                                                  const u64 *own, u64 &lo0, u64 &hi0, u64 &lo1, u64 &hi1)
        {
            const u64 x = j == m.my_digit ? *own : pext[static_cast<std::size_t>(j) * ext_digit_stride];
            mac2(x, pkey[m.key_slice(j, 0)], pkey[m.key_slice(j, 1)], lo0, hi0, lo1, hi1);
        }

        // The ending: both components leave as streaming stores, after adding what the destination holds when add != 0.
        __device__ __forceinline__ void store2(u64 *po, std::size_t comp, u64 v0, u64 v1)
        {
            store_stream(po, v0);
            store_stream(po + comp, v1);
        }
        __device__ __forceinline__ void add_store2(u64 *po, std::size_t comp, u64 v0, u64 v1, int add, u64 p)
        {
            if (add)
            {
                v0 = add_mod(v0, po[0], p);
                v1 = add_mod(v1, po[comp], p);
            }
            store2(po, comp, v0, v1);
        }
    } // namespace
} // namespace sealhip
