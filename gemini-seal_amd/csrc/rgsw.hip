// rgsw.hip -- the external product RLWE x RGSW: the key switch's inner product (ks_inner.hpp) over the
// 2 nd digits of BOTH components of a ciphertext against the two halves of one RGSW block,
//   prod[l][r][c] = ( sum_{j<nd} D0_j[r][c] K_b[j][l][row_prime r][c] + sum_{j<nd} D1_j[r][c] K_a[j][l][row_prime r][c] ) mod p_r
// with one reduction per output word (two where bounds::ext_mac_sum_fits refuses the whole sum: the same words), and the
// streaming kernel that prepares a CMux: the difference the product decomposes and the copy the mod-down adds into.
// D0_j / D1_j are the digits ks_digits forms for c_0 and c_1: inside bundle j the row's own word (own0 / own1), else row r of
// extended digit j; ext holds the 2 nd digits digit-major, c_0's first. Each half of the block is laid out as a key,
// [2j + l][n_total][N].
#include <algorithm>

#include "engine.hpp"
#include "instance_dispatch.hpp"
#include "ks_inner.hpp"

namespace sealhip
{
    namespace
    {
        // One lane per (item, row, coefficient), the digit count a run-time bound (KsDev::nd).
        __global__ __launch_bounds__(kThreads) void ext_mac_kernel(const KsDev *__restrict__ d, const PrimeDev *__restrict__ primes,
                                                                   const u64 *__restrict__ own0, const u64 *__restrict__ own1,
                                                                   std::size_t own_stride, const u64 *__restrict__ ext,
                                                                   std::size_t ext_stride, std::size_t ext_digit_stride,
                                                                   const u64 *__restrict__ key_b, const u64 *__restrict__ key_a,
                                                                   u64 *__restrict__ prod, std::size_t prod_stride, std::size_t count,
                                                                   int logn, int split)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const int r = static_cast<int>(lane.q % dim.rows);
            const std::size_t item = lane.q / dim.rows;
            if (item >= count)
                return;
            const int nd = d->nd;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t off = m.row_off() + lane.c, key_off = m.prime_row() + lane.c;
            const MacMod mod = mac_mod(primes, m);
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            const u64 *pext = ext + item * ext_stride + off;
            for (int j = 0; j < nd; j++)
                digit_mac(m, j, pext, ext_digit_stride, key_b + key_off, own0 + item * own_stride + off, lo0, hi0, lo1, hi1);
            if (split) // (wave-uniform) the canonical residue of the first half is the second half's first word
            {
                lo0 = mod.reduce(lo0, hi0);
                lo1 = mod.reduce(lo1, hi1);
                hi0 = hi1 = 0;
            }
            pext += static_cast<std::size_t>(nd) * ext_digit_stride;
            for (int j = 0; j < nd; j++)
                digit_mac(m, j, pext, ext_digit_stride, key_a + key_off, own1 + item * own_stride + off, lo0, hi0, lo1, hi1);
            u64 *pp = prod + item * prod_stride + off;
            store2(pp, m.comp(), mod.reduce(lo0, hi0), mod.reduce(lo1, hi1));
        }

        // The same sum with the 2 nd key-word pairs of a lane's (row, coefficient) in registers across `group` consecutive
        // items, the next item's digit words requested before the current one is accumulated (ks_mac_items_kernel's form).
        // ND2 = 2 nd: slot j < nd is digit j of c_0 against K_b, slot nd + j digit j of c_1 against K_a.
        template <int ND2>
        __global__ __launch_bounds__(kThreads) void ext_mac_items_kernel(const KsDev *__restrict__ d, const PrimeDev *__restrict__ primes,
                                                                         const u64 *__restrict__ own0, const u64 *__restrict__ own1,
                                                                         std::size_t own_stride, const u64 *__restrict__ ext,
                                                                         std::size_t ext_stride, std::size_t ext_digit_stride,
                                                                         const u64 *__restrict__ key_b, const u64 *__restrict__ key_a,
                                                                         u64 *__restrict__ prod, std::size_t prod_stride,
                                                                         std::size_t count, int logn, std::size_t group, int split)
        {
            static_assert(ND2 % 2 == 0, "two halves of nd digits");
            constexpr int ND = ND2 / 2;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = block_lane(N); // (N >= kThreads: select_ext_mac) row and item group are wave-uniform
            const int r = static_cast<int>(static_cast<unsigned>(lane.q) % static_cast<unsigned>(dim.rows));
            const std::size_t item0 = (static_cast<unsigned>(lane.q) / static_cast<unsigned>(dim.rows)) * group;
            if (item0 >= count)
                return;
            const std::size_t item1 = item0 + group < count ? item0 + group : count;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t off = m.row_off() + lane.c;
            const u64 *pkb = key_b + m.prime_row() + lane.c, *pka = key_a + m.prime_row() + lane.c;
            u64 k0[ND2], k1[ND2], x[ND2], xn[ND2];
#pragma unroll
            for (int j = 0; j < ND; j++)
            {
                k0[j] = pkb[m.key_slice(j, 0)];
                k1[j] = pkb[m.key_slice(j, 1)];
                k0[ND + j] = pka[m.key_slice(j, 0)];
                k1[ND + j] = pka[m.key_slice(j, 1)];
            }
            auto load_x = [&](u64(&dst)[ND2], std::size_t item) {
#pragma unroll
                for (int j = 0; j < ND; j++)
                {
                    const bool mine = j == m.my_digit;
                    const u64 *pe = ext + item * ext_stride + static_cast<std::size_t>(j) * ext_digit_stride + off;
                    dst[j] = mine ? own0[item * own_stride + off] : pe[0];
                    dst[ND + j] = mine ? own1[item * own_stride + off] : pe[static_cast<std::size_t>(ND) * ext_digit_stride];
                }
            };
            load_x(x, item0);
            const MacMod mod = mac_mod(primes, m);
            for (std::size_t item = item0; item < item1; item++)
            {
                if (item + 1 < item1)
                    load_x(xn, item + 1);
                u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
#pragma unroll
                for (int j = 0; j < ND; j++)
                    mac2(x[j], k0[j], k1[j], lo0, hi0, lo1, hi1);
                if (split)
                {
                    lo0 = mod.reduce(lo0, hi0);
                    lo1 = mod.reduce(lo1, hi1);
                    hi0 = hi1 = 0;
                }
#pragma unroll
                for (int j = ND; j < ND2; j++)
                    mac2(x[j], k0[j], k1[j], lo0, hi0, lo1, hi1);
                store2(prod + item * prod_stride + off, m.comp(), mod.reduce(lo0, hi0), mod.reduce(lo1, hi1));
#pragma unroll
                for (int j = 0; j < ND2; j++)
                    x[j] = xn[j];
            }
        }

        // CMux's head: one lane per pair of words of a ciphertext pair. Global row R = (pair, component, r) in 32 bits.
        __global__ __launch_bounds__(kThreads) void cmux_prepare_kernel(const u64 *__restrict__ ct0, std::size_t stride0,
                                                                        const u64 *__restrict__ ct1, std::size_t stride1,
                                                                        u64 *__restrict__ diff, u64 *__restrict__ base,
                                                                        std::size_t base_stride, const PrimeDev *__restrict__ primes,
                                                                        unsigned k, int logn, std::size_t total_pairs)
        {
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            const std::size_t row_mask = (static_cast<std::size_t>(1) << logn) - 1;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total_pairs; i += stride)
            {
                const std::size_t w = 2 * i;
                const unsigned R = static_cast<unsigned>(w >> logn);
                const unsigned item = R / (2 * k), in_item = R % (2 * k);
                const u64 p = primes[in_item % k].p;
                const std::size_t at = (static_cast<std::size_t>(in_item) << logn) + (w & row_mask);
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(ct0 + item * stride0 + at);
                const ulonglong2 b = *reinterpret_cast<const ulonglong2 *>(ct1 + item * stride1 + at);
                store_stream2(diff + w, sub_mod(b.x, a.x, p), sub_mod(b.y, a.y, p));
                store_stream2(base + item * base_stride + at, a.x, a.y);
            }
        }
    } // namespace

    ExtMacPlan ext_mac_plan(const Engine &e, const KsDev &h, std::size_t count)
    {
        const int rows = h.k + h.nsp;
        u64 pmax = 0;
        for (int r = 0; r < rows; r++)
            pmax = std::max<u64>(pmax, e.key_moduli[h.row_prime[r]]);
        ExtMacPlan plan{ select_ext_mac(e.logn, h.nd, static_cast<std::size_t>(rows), count), false };
        if (!bounds::ext_mac_sum_fits(2 * h.nd, pmax, bounds::kKsDigitRepBits))
        {
            plan.split = true;
            if (!bounds::ext_mac_sum_fits(h.nd, pmax, bounds::kKsDigitRepBits)) // (no context has such a level: nd p < 2^64)
                plan.choice.family = kMacRefused;
        }
        return plan;
    }

    hipError_t launch_ext_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *own0, const u64 *own1,
                              std::size_t own_stride, const u64 *ext, std::size_t ext_stride, std::size_t ext_digit_stride,
                              const u64 *key_b, const u64 *key_a, u64 *prod, std::size_t prod_stride, std::size_t count)
    {
        if (!count)
            return hipSuccess;
        const ExtMacPlan plan = ext_mac_plan(e, h, count);
        const MacChoice &c = plan.choice;
        // (the kernels split the lane's unit index with 32-bit arithmetic)
        if (c.family == kMacRefused || ((count * static_cast<std::size_t>(h.k + h.nsp)) >> 32))
            return hipErrorInvalidValue;
        ProfScope prof(e, "ext_mac", 0);
        const hipStream_t stream = e.lane().stream;
        const int split = plan.split ? 1 : 0;
        bool launched = true;
        if (c.family == kMacItems)
            launched = dispatch_mac_digits(c.nd, [&](auto nd2) {
                constexpr int ND2 = decltype(nd2)::value;
                if constexpr (ND2 % 2 == 0) // (the selector names 2 nd)
                    ext_mac_items_kernel<ND2><<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, own0, own1, own_stride, ext, ext_stride,
                                                                               ext_digit_stride, key_b, key_a, prod, prod_stride,
                                                                               count, e.logn, c.group, split);
            }) && c.nd % 2 == 0;
        else
            ext_mac_kernel<<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, own0, own1, own_stride, ext, ext_stride, ext_digit_stride,
                                                             key_b, key_a, prod, prod_stride, count, e.logn, split);
        return launched ? hipGetLastError() : hipErrorInvalidValue;
    }

    hipError_t launch_cmux_prepare(const Engine &e, int k, const u64 *ct0, std::size_t stride0, const u64 *ct1,
                                   std::size_t stride1, u64 *diff, u64 *base, std::size_t base_stride, std::size_t npairs)
    {
        if (!npairs)
            return hipSuccess;
        if ((npairs * 2 * static_cast<std::size_t>(k)) >> 32) // (the kernel divides the row index with 32-bit arithmetic)
            return hipErrorInvalidValue;
        const std::size_t total = (npairs * 2 * static_cast<std::size_t>(k) << e.logn) / 2;
        ProfScope prof(e, "cmux_prepare", static_cast<double>(total));
        cmux_prepare_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(ct0, stride0, ct1, stride1, diff, base, base_stride,
                                                                              e.d_primes, static_cast<unsigned>(k), e.logn, total);
        return hipGetLastError();
    }
} // namespace sealhip
