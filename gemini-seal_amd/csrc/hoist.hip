// hoist.hip -- kernels of the hoisted rotation: one ciphertext rotated by several Galois
// elements with ONE decomposition of c_1 (Halevi-Shoup). The digits D_j of the key switch (evaluator.cpp:2302-2322) do not
// depend on the element; what does is the inner product against K_g and sigma_g(c_0):
//   prod_g[l][r][c] = ( sum_j D_j[r][T_g[c]] * K_g[j][l][row_prime r][c] ) mod p_r
// with T_g the NTT-form table of the automorphism (galois.cpp:18-47). The gather is folded into the digit loads. T_g maps
// every aligned block of 2^b indices onto an aligned block of 2^b indices (g * e mod 2N on the bit-reversed exponents keeps
// the high bits of the index together), so the 64 words a wave gathers lie in the same four 128-byte lines a straight
// read of one aligned 64-word block would touch: no traffic amplification, no LDS staging.
#include "engine.hpp"
#include "instance_dispatch.hpp"
#include "ks_inner.hpp"

namespace sealhip
{
    namespace
    {
        // One lane per (element, item group, row, coefficient c): the 2 * ND key words of (row, c) stay in registers across
        // the `group` ciphertexts of the lane, two 128-bit accumulators per ciphertext, as ks_mac_items_kernel. The digit
        // words come from column T_g[c] of ext (or of the NTT-form target row when j is the row's own digit); the key
        // words and the stores are coalesced. prod is [element][item][2][rows][N]. Grid order (item group, row, element,
        // coefficient): the elements of one (item group, row) are adjacent, so their re-reads of the digit rows (nd * N * 8
        // bytes per element) come from L2. Measured against the element-major order, where an element's key stays hot
        // instead: 8-16 % faster at 64 ciphertexts, no difference at one (profiles/r06/hoisted_rotate.txt).
        template <int ND>
        __global__ __launch_bounds__(kThreads) void hoist_mac_kernel(const KsDev *__restrict__ d,
                                                                     const PrimeDev *__restrict__ primes,
                                                                     const u64 *__restrict__ target,
                                                                     std::size_t target_stride,
                                                                     const u64 *__restrict__ ext, std::size_t ext_stride,
                                                                     std::size_t ext_digit_stride, HoistElts elts,
                                                                     u64 *__restrict__ prod, std::size_t prod_stride,
                                                                     std::size_t count, int logn, std::size_t group,
                                                                     std::size_t n_groups)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = block_lane(N); // (element, row and item group, so every base address, are wave-uniform)
            const std::size_t c = lane.c;
            unsigned q = static_cast<unsigned>(lane.q);
            const int el = static_cast<int>(q % elts.n);
            q /= elts.n;
            const int r = static_cast<int>(q % dim.rows);
            const std::size_t grp = q / dim.rows;
            if (grp >= n_groups)
                return;
            const std::size_t item0 = grp * group;
            const std::size_t item1 = item0 + group < count ? item0 + group : count;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t src_off = m.row_off() + elts.table[el][c];
            const u64 *pkey = elts.key[el] + m.prime_row() + c;
            u64 k0[ND], k1[ND], x[ND], xn[ND];
#pragma unroll
            for (int j = 0; j < ND; j++)
            {
                k0[j] = pkey[m.key_slice(j, 0)];
                k1[j] = pkey[m.key_slice(j, 1)];
            }
            auto load_x = [&](u64(&dst)[ND], std::size_t item) {
#pragma unroll
                for (int j = 0; j < ND; j++)
                    dst[j] = j == m.my_digit ? target[item * target_stride + src_off]
                                             : ext[item * ext_stride + static_cast<std::size_t>(j) * ext_digit_stride + src_off];
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
                u64 *pp = prod + (static_cast<std::size_t>(el) * count + item) * prod_stride + m.row_off() + c;
                store_stream(pp, mod.reduce(lo0, hi0));
                store_stream(pp + m.comp(), mod.reduce(lo1, hi1));
#pragma unroll
                for (int j = 0; j < ND; j++)
                    x[j] = xn[j];
            }
        }

        // Digit counts without an instance: the same lanes, the key words streamed per ciphertext (as ks_mac_kernel).
        __global__ __launch_bounds__(kThreads) void hoist_mac_loop_kernel(const KsDev *__restrict__ d,
                                                                          const PrimeDev *__restrict__ primes,
                                                                          const u64 *__restrict__ target,
                                                                          std::size_t target_stride,
                                                                          const u64 *__restrict__ ext,
                                                                          std::size_t ext_stride,
                                                                          std::size_t ext_digit_stride, HoistElts elts,
                                                                          u64 *__restrict__ prod, std::size_t prod_stride,
                                                                          std::size_t count, int logn, int nd)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const std::size_t c = lane.c;
            std::size_t q = lane.q;
            const int el = static_cast<int>(q % elts.n);
            q /= elts.n;
            const int r = static_cast<int>(q % dim.rows);
            const std::size_t item = q / dim.rows;
            if (item >= count)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t src_off = m.row_off() + elts.table[el][c];
            const u64 *pkey = elts.key[el] + m.prime_row() + c;
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            for (int j = 0; j < nd; j++)
                digit_mac(m, j, ext + item * ext_stride + src_off, ext_digit_stride, pkey, target + item * target_stride + src_off, lo0, hi0,
                          lo1, hi1);
            const MacMod mod = mac_mod(primes, m);
            store2(prod + (static_cast<std::size_t>(el) * count + item) * prod_stride + m.row_off() + c, m.comp(), mod.reduce(lo0, hi0),
                   mod.reduce(lo1, hi1));
        }

        // sigma_g(c_0) of every (element, item) in one pass: out[element][item][k][N] from component 0 of ct[item]
        // (ct_stride words apart). NTT form: out[c] = in[T_g[c]] (galois.cpp:188-214); coefficient form:
        // out[(c * g) mod N] = +-in[c] (galois.cpp:144-186).
        __global__ __launch_bounds__(kThreads) void hoist_galois_c0_kernel(const u64 *__restrict__ ct, std::size_t ct_stride,
                                                                           u64 *__restrict__ out,
                                                                           const PrimeDev *__restrict__ primes, RowMap map,
                                                                           int logn, std::size_t count, HoistElts elts,
                                                                           int ntt_form)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const int k = map.rows;
            const std::size_t total = (static_cast<std::size_t>(elts.n) * count * k) << logn;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t c = i & nmask;
                std::size_t q = i >> logn;
                const int row = static_cast<int>(q % k);
                q /= k;
                const std::size_t item = q % count;
                const int el = static_cast<int>(q / count);
                const u64 *in = ct + item * ct_stride + static_cast<std::size_t>(row) * N;
                u64 *o = out + ((static_cast<std::size_t>(el) * count + item) * k + row) * N;
                if (ntt_form)
                    o[c] = in[elts.table[el][c]];
                else
                {
                    const u64 p = primes[map.prime[row]].p;
                    const u64 raw = static_cast<u64>(c) * elts.elt[el];
                    u64 v = in[c];
                    if ((raw >> logn) & 1)
                        v = neg_mod(v, p);
                    o[raw & nmask] = v;
                }
            }
        }

        // ---- plaintext-weighted sum of rotations ----
        // acc_s[l][r][c] = sum_i W[s][i][rp(r)][c] * prod_{g_i}[l][r][c]: hoist_mac_kernel's inner product, not stored but
        // multiplied by the plaintext word and summed over the elements of the launch in registers. A lane owns column c of
        // one extended row for 4 / S ciphertexts and S sums: four (ciphertext, sum) slots of two 128-bit accumulators, the
        // same 32 registers whichever way the slots are cut. The element loop is outermost and wave-uniform: the 2 * ND key
        // words of an element are loaded once for the lane's ciphertexts, the two reduced products of a ciphertext once for
        // the lane's sums. At most kHoistMaxElts terms below 2^122 meet in an accumulator, so it is reduced once, at the
        // end; add != 0 adds the words a former launch of a longer element list left in acc.
        template <int ND, int S>
        __global__ __launch_bounds__(kThreads) void hoist_dot_mac_kernel(const KsDev *__restrict__ d,
                                                                         const PrimeDev *__restrict__ primes,
                                                                         const u64 *__restrict__ target,
                                                                         std::size_t target_stride,
                                                                         const u64 *__restrict__ ext, std::size_t ext_stride,
                                                                         std::size_t ext_digit_stride, HoistDotElts elts,
                                                                         std::size_t w_sum_stride, u64 *__restrict__ acc,
                                                                         std::size_t acc_stride, std::size_t count,
                                                                         std::size_t n_sums, int logn, int add)
        {
            constexpr int G = 4 / S;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = block_lane(N); // (row, item group and sum group are wave-uniform)
            const std::size_t c = lane.c;
            unsigned q = static_cast<unsigned>(lane.q);
            const int r = static_cast<int>(q % dim.rows);
            q /= dim.rows;
            const std::size_t sum_groups = (n_sums + S - 1) / S;
            const std::size_t sum0 = static_cast<std::size_t>(q % sum_groups) * S;
            const std::size_t item0 = static_cast<std::size_t>(q / sum_groups) * G;
            if (item0 >= count)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t row_off = m.row_off(), key_comp = m.key_comp(), prime_off = m.prime_row() + c;
            const MacMod mod = mac_mod(primes, m);
            u64 lo[G][S][2], hi[G][S][2];
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int s = 0; s < S; s++)
                    lo[g][s][0] = hi[g][s][0] = lo[g][s][1] = hi[g][s][1] = 0;
            for (int el = 0; el < elts.n; el++)
            {
                // Addresses are walked, not indexed: a lane's pointer advances by the wave-uniform stride from load to load.
                // Indexed, the 2 * ND + G * ND wave-uniform offsets are loop invariants that the compiler holds in scalar
                // registers across the element loop -- more than the 106 there are from ND = 5 on.
                const u64 *pk = elts.key[el] + prime_off;
                const std::size_t src_off = row_off + elts.table[el][c];
                u64 k0[ND], k1[ND], w[S];
#pragma unroll
                for (int j = 0; j < ND; j++)
                {
                    k0[j] = pk[0];
                    k1[j] = pk[key_comp];
                    pk += 2 * key_comp;
                }
#pragma unroll
                for (int s = 0; s < S; s++)
                    w[s] = sum0 + s < n_sums ? elts.w[el][(sum0 + s) * w_sum_stride + prime_off] : 0;
                const u64 *pt = target + item0 * target_stride + src_off, *pe = ext + item0 * ext_stride + src_off;
#pragma unroll
                for (int g = 0; g < G; g++, pt += target_stride, pe += ext_stride)
                {
                    if (item0 + g >= count)
                        break;
                    u64 l0 = 0, h0 = 0, l1 = 0, h1 = 0;
                    const u64 *px = pe;
#pragma unroll
                    for (int j = 0; j < ND; j++, px += ext_digit_stride)
                        mac2(j == m.my_digit ? *pt : *px, k0[j], k1[j], l0, h0, l1, h1);
                    const u64 p0 = mod.reduce(l0, h0), p1 = mod.reduce(l1, h1);
#pragma unroll
                    for (int s = 0; s < S; s++)
                        mac2(w[s], p0, p1, lo[g][s][0], hi[g][s][0], lo[g][s][1], hi[g][s][1]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int s = 0; s < S; s++)
                {
                    if (item0 + g >= count || sum0 + s >= n_sums)
                        continue;
                    u64 *pa = acc + ((sum0 + s) * count + item0 + g) * acc_stride + row_off + c;
                    u64 v0 = mod.reduce(lo[g][s][0], hi[g][s][0]), v1 = mod.reduce(lo[g][s][1], hi[g][s][1]);
                    if (add) // (inline: as add_store2 every instance is scheduled differently, profiles/r21/device_code.txt)
                    {
                        v0 = add_mod(v0, pa[0], mod.p);
                        v1 = add_mod(v1, pa[m.comp()], mod.p);
                    }
                    store2(pa, m.comp(), v0, v1);
                }
        }

        // Digit counts without an instance and rings smaller than a workgroup: one lane per (sum, item, row, c), the key
        // words streamed per element.
        __global__ __launch_bounds__(kThreads) void hoist_dot_mac_loop_kernel(
            const KsDev *__restrict__ d, const PrimeDev *__restrict__ primes, const u64 *__restrict__ target,
            std::size_t target_stride, const u64 *__restrict__ ext, std::size_t ext_stride, std::size_t ext_digit_stride,
            HoistDotElts elts, std::size_t w_sum_stride, u64 *__restrict__ acc, std::size_t acc_stride, std::size_t count,
            std::size_t n_sums, int logn, int nd, int add)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const std::size_t c = lane.c;
            std::size_t q = lane.q;
            const int r = static_cast<int>(q % dim.rows);
            q /= dim.rows;
            const std::size_t item = q % count, sum = q / count;
            if (sum >= n_sums)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t row_off = m.row_off(), prime_off = m.prime_row() + c;
            const MacMod mod = mac_mod(primes, m);
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            for (int el = 0; el < elts.n; el++)
            {
                const u64 *pkey = elts.key[el] + prime_off;
                const std::size_t src_off = row_off + elts.table[el][c];
                u64 l0 = 0, h0 = 0, l1 = 0, h1 = 0;
                for (int j = 0; j < nd; j++)
                    digit_mac(m, j, ext + item * ext_stride + src_off, ext_digit_stride, pkey, target + item * target_stride + src_off, l0, h0,
                              l1, h1);
                const u64 w = elts.w[el][sum * w_sum_stride + prime_off];
                mac128(lo0, hi0, w, mod.reduce(l0, h0));
                mac128(lo1, hi1, w, mod.reduce(l1, h1));
            }
            u64 *pa = acc + (sum * count + item) * acc_stride + row_off + c;
            add_store2(pa, m.comp(), mod.reduce(lo0, hi0), mod.reduce(lo1, hi1), add, mod.p);
        }

        // base_s of section 16: out[sum][item][0][r][c] = sum_i W[s][i][r][c] * C[item][0][r][T_i[c]] over every element of
        // the launch, out[sum][item][1][r][c] = the same over the identity elements (table == null) with C[item][1][r][c].
        // C is in NTT form, item stride 2 k N. The words of C may be any 64-bit representative: the accumulator is folded
        // every fourth term (4 * 2^61 * 2^64 < 2^128).
        __global__ __launch_bounds__(kThreads) void hoist_dot_base_kernel(const u64 *__restrict__ cn, HoistDotElts elts,
                                                                          std::size_t w_sum_stride, u64 *__restrict__ out,
                                                                          std::size_t out_sum_stride,
                                                                          const PrimeDev *__restrict__ primes, int k, int logn,
                                                                          std::size_t count, std::size_t n_sums, int add)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const std::size_t poly = static_cast<std::size_t>(k) << logn;
            const std::size_t total = (n_sums * count * k) << logn;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t c = i & nmask;
                std::size_t q = i >> logn;
                const int row = static_cast<int>(q % k);
                q /= k;
                const std::size_t item = q % count, sum = q / count;
                const PrimeDev &P = primes[row];
                const u64 p = P.p, cr0 = P.cr0, cr1 = P.cr1;
                const std::size_t row_off = static_cast<std::size_t>(row) * N;
                const u64 *in = cn + item * 2 * poly + row_off;
                u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
                for (int el = 0; el < elts.n; el++)
                {
                    const u64 w = elts.w[el][sum * w_sum_stride + row_off + c];
                    const std::uint32_t *tab = elts.table[el];
                    mac128(lo0, hi0, w, in[tab ? tab[c] : c]);
                    if (!tab)
                        mac128(lo1, hi1, w, in[poly + c]);
                    if ((el & 3) == 3)
                    {
                        lo0 = barrett_reduce_128(lo0, hi0, p, cr0, cr1);
                        lo1 = barrett_reduce_128(lo1, hi1, p, cr0, cr1);
                        hi0 = hi1 = 0;
                    }
                }
                u64 *o = out + sum * out_sum_stride + item * 2 * poly + row_off + c;
                u64 v0 = barrett_reduce_128(lo0, hi0, p, cr0, cr1), v1 = barrett_reduce_128(lo1, hi1, p, cr0, cr1);
                if (add)
                {
                    v0 = add_mod(v0, o[0], p);
                    v1 = add_mod(v1, o[poly], p);
                }
                o[0] = v0;
                o[poly] = v1;
            }
        }

        // ---- giant steps in the extended basis ----
        // ACC[l][r][c] += sum over the giants h of the launch of
        //     ( sum_t D_t(d_h)[r][T_h[c]] * K_h[t][l][rp(r)][c] ) mod p_r   (+ acc_h[0][r][T_h[c]] for l = 0),
        // and acc_h[l][r][c] itself for an identity giant (table == null). A lane owns column c of one extended row for four
        // ciphertexts; the giant loop is outermost and wave-uniform, so the 2 * ND key words of a giant are loaded once for the
        // lane's ciphertexts. Every giant has digits of its own (d_h differs from giant to giant): ext[el] / inb[el] are the
        // bases of giant el's first ciphertext, the in-bundle row is read from d_h itself (inb) as my_digit does everywhere.
        // Accumulator bound: one giant's inner product is at most ND <= 16 products below 2^122, below 2^126, and is reduced
        // to its canonical residue at once -- sixteen giants of sixteen digits would be 256 such products, past 2^128. The
        // running sums s[g][l] are kept canonical with add_mod (two or three words below p < 2^61 meet per giant), so any
        // number of giants fits; add != 0 adds the words an earlier launch left in ACC.
        template <int ND>
        __global__ __launch_bounds__(kThreads) void hoist_giant_mac_kernel(const KsDev *__restrict__ d,
                                                                           const PrimeDev *__restrict__ primes,
                                                                           HoistGiantElts elts, std::size_t inb_stride,
                                                                           std::size_t ext_stride, std::size_t ext_digit_stride,
                                                                           std::size_t accj_stride, u64 *__restrict__ acc,
                                                                           std::size_t acc_stride, std::size_t count, int logn,
                                                                           int add)
        {
            constexpr int G = 4;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = block_lane(N); // (row and item group are wave-uniform)
            const std::size_t c = lane.c;
            const unsigned q = static_cast<unsigned>(lane.q);
            const int r = static_cast<int>(q % dim.rows);
            const std::size_t item0 = static_cast<std::size_t>(q / dim.rows) * G;
            if (item0 >= count)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t row_off = m.row_off(), comp = m.comp(), key_comp = m.key_comp(), prime_off = m.prime_row() + c;
            const MacMod mod = mac_mod(primes, m);
            u64 s[G][2];
#pragma unroll
            for (int g = 0; g < G; g++)
                s[g][0] = s[g][1] = 0;
            for (int el = 0; el < elts.n; el++)
            {
                const std::uint32_t *tab = elts.table[el];
                const u64 *pa = elts.accj[el];
                if (!tab) // the identity giant: acc_h as it lies
                {
                    pa += item0 * accj_stride + row_off + c;
#pragma unroll
                    for (int g = 0; g < G; g++, pa += accj_stride)
                    {
                        if (item0 + g >= count)
                            break;
                        s[g][0] = add_mod(s[g][0], pa[0], mod.p);
                        s[g][1] = add_mod(s[g][1], pa[comp], mod.p);
                    }
                    continue;
                }
                // (addresses are walked, not indexed: hoist_dot_mac_kernel records why)
                const u64 *pk = elts.key[el] + prime_off;
                const std::size_t src_off = row_off + tab[c];
                u64 k0[ND], k1[ND];
#pragma unroll
                for (int j = 0; j < ND; j++)
                {
                    k0[j] = pk[0];
                    k1[j] = pk[key_comp];
                    pk += 2 * key_comp;
                }
                const u64 *pt = elts.inb[el] + item0 * inb_stride + src_off, *pe = elts.ext[el] + item0 * ext_stride + src_off;
                if (pa)
                    pa += item0 * accj_stride + src_off;
#pragma unroll
                for (int g = 0; g < G; g++, pt += inb_stride, pe += ext_stride)
                {
                    if (item0 + g >= count)
                        break;
                    u64 l0 = 0, h0 = 0, l1 = 0, h1 = 0;
                    const u64 *px = pe;
#pragma unroll
                    for (int j = 0; j < ND; j++, px += ext_digit_stride)
                        mac2(j == m.my_digit ? *pt : *px, k0[j], k1[j], l0, h0, l1, h1);
                    s[g][0] = add_mod(s[g][0], mod.reduce(l0, h0), mod.p);
                    s[g][1] = add_mod(s[g][1], mod.reduce(l1, h1), mod.p);
                    if (pa)
                    {
                        s[g][0] = add_mod(s[g][0], *pa, mod.p);
                        pa += accj_stride;
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++)
            {
                if (item0 + g >= count)
                    continue;
                u64 *po = acc + (item0 + g) * acc_stride + row_off + c;
                add_store2(po, comp, s[g][0], s[g][1], add, mod.p);
            }
        }

        // Digit counts without an instance and rings smaller than a workgroup: one lane per (item, row, c), the key words
        // streamed per giant. The same sums in the same canonical form.
        __global__ __launch_bounds__(kThreads) void hoist_giant_mac_loop_kernel(
            const KsDev *__restrict__ d, const PrimeDev *__restrict__ primes, HoistGiantElts elts, std::size_t inb_stride,
            std::size_t ext_stride, std::size_t ext_digit_stride, std::size_t accj_stride, u64 *__restrict__ acc,
            std::size_t acc_stride, std::size_t count, int logn, int nd, int add)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const std::size_t c = lane.c;
            const int r = static_cast<int>(lane.q % dim.rows);
            const std::size_t item = lane.q / dim.rows;
            if (item >= count)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t row_off = m.row_off(), comp = m.comp(), prime_off = m.prime_row() + c;
            const MacMod mod = mac_mod(primes, m);
            u64 s0 = 0, s1 = 0;
            for (int el = 0; el < elts.n; el++)
            {
                const std::uint32_t *tab = elts.table[el];
                const u64 *pa = elts.accj[el];
                if (!tab)
                {
                    s0 = add_mod(s0, pa[item * accj_stride + row_off + c], mod.p);
                    s1 = add_mod(s1, pa[item * accj_stride + comp + row_off + c], mod.p);
                    continue;
                }
                const u64 *pkey = elts.key[el] + prime_off;
                const std::size_t src_off = row_off + tab[c];
                u64 l0 = 0, h0 = 0, l1 = 0, h1 = 0;
                for (int j = 0; j < nd; j++)
                    digit_mac(m, j, elts.ext[el] + item * ext_stride + src_off, ext_digit_stride, pkey,
                              elts.inb[el] + item * inb_stride + src_off, l0, h0, l1, h1);
                s0 = add_mod(s0, mod.reduce(l0, h0), mod.p);
                s1 = add_mod(s1, mod.reduce(l1, h1), mod.p);
                if (pa)
                    s0 = add_mod(s0, pa[item * accj_stride + src_off], mod.p);
            }
            add_store2(acc + item * acc_stride + row_off + c, comp, s0, s1, add, mod.p);
        }

        // BASE of section 17, on the k ciphertext rows: out[item][0][r][c] = sum over the giants of the launch of
        // base_h[item][0][r][T_h[c]], out[item][1][r][c] = the sum of base_h[item][1][r][c] over the identity giants
        // (table == null). base_h is canonical (hoist_dot_base_kernel wrote it), item stride 2 k N like out.
        __global__ __launch_bounds__(kThreads) void hoist_giant_base_kernel(HoistGiantBases elts, u64 *__restrict__ out,
                                                                            const PrimeDev *__restrict__ primes, int k, int logn,
                                                                            std::size_t count, int add)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn, nmask = N - 1;
            const std::size_t poly = static_cast<std::size_t>(k) << logn;
            const std::size_t total = (count * k) << logn;
            const std::size_t stride = static_cast<std::size_t>(gridDim.x) * blockDim.x;
            for (std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x; i < total; i += stride)
            {
                const std::size_t c = i & nmask;
                const std::size_t q = i >> logn;
                const int row = static_cast<int>(q % k);
                const std::size_t at = (q / k) * 2 * poly + static_cast<std::size_t>(row) * N;
                const u64 p = primes[row].p;
                u64 v0 = 0, v1 = 0;
                for (int el = 0; el < elts.n; el++)
                {
                    const u64 *in = elts.base[el] + at;
                    const std::uint32_t *tab = elts.table[el];
                    v0 = add_mod(v0, in[tab ? tab[c] : c], p);
                    if (!tab)
                        v1 = add_mod(v1, in[poly + c], p);
                }
                u64 *o = out + at + c;
                if (add)
                {
                    v0 = add_mod(v0, o[0], p);
                    v1 = add_mod(v1, o[poly], p);
                }
                o[0] = v0;
                o[poly] = v1;
            }
        }
    } // namespace

    hipError_t launch_hoist_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                                std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                                std::size_t ext_digit_stride, const HoistElts &elts, u64 *prod, std::size_t prod_stride,
                                std::size_t count)
    {
        if (!count || !elts.n)
            return hipSuccess;
        const MacChoice c = select_hoist_mac(e.logn, h.nd, static_cast<std::size_t>(h.k + h.nsp), elts.n, count);
        if (c.family == kMacRefused)
            return hipErrorInvalidValue;
        ProfScope prof(e, "hoist_mac", 0);
        const hipStream_t stream = e.lane().stream;
        if (!dispatch_mac_digits(c.nd, [&](auto nd) {
                hoist_mac_kernel<decltype(nd)::value><<<c.blocks, kThreads, 0, stream>>>(
                    d, e.d_primes, target, target_stride, ext, ext_stride, ext_digit_stride, elts, prod, prod_stride, count, e.logn,
                    c.group, c.n_groups);
            })) // more than 16 digits, or a ring smaller than a workgroup
            hoist_mac_loop_kernel<<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, target, target_stride, ext, ext_stride,
                                                                    ext_digit_stride, elts, prod, prod_stride, count, e.logn, h.nd);
        return hipGetLastError();
    }

    hipError_t launch_hoist_galois_c0(const Engine &e, const u64 *ct, std::size_t ct_stride, u64 *out, std::size_t count,
                                      const RowMap &map_q, const HoistElts &elts, bool ntt_form)
    {
        const std::size_t total = (static_cast<std::size_t>(elts.n) * count * map_q.rows) << e.logn;
        if (total == 0)
            return hipSuccess;
        ProfScope prof(e, "hoist_galois", 0);
        hoist_galois_c0_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(ct, ct_stride, out, e.d_primes, map_q, e.logn,
                                                                                 count, elts, ntt_form ? 1 : 0);
        return hipGetLastError();
    }

    hipError_t launch_hoist_dot_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                                    std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                                    std::size_t ext_digit_stride, const HoistDotElts &elts, std::size_t w_sum_stride, u64 *acc,
                                    std::size_t acc_stride, std::size_t count, std::size_t n_sums, bool add)
    {
        if (!count || !elts.n || !n_sums)
            return hipSuccess;
        const MacChoice c = select_hoist_dot_mac(e.logn, h.nd, static_cast<std::size_t>(h.k + h.nsp), elts.n, count, n_sums);
        if (c.family == kMacRefused)
            return hipErrorInvalidValue;
        ProfScope prof(e, "hoist_dot_mac", 0);
        const hipStream_t stream = e.lane().stream;
        if (!dispatch_mac_digits(c.nd, [&](auto nd) {
                dispatch_among<1, 2, 4>(c.slots, [&](auto slots) {
                    hoist_dot_mac_kernel<decltype(nd)::value, decltype(slots)::value><<<c.blocks, kThreads, 0, stream>>>(
                        d, e.d_primes, target, target_stride, ext, ext_stride, ext_digit_stride, elts, w_sum_stride, acc, acc_stride,
                        count, n_sums, e.logn, add ? 1 : 0);
                });
            })) // more than 16 digits, or a ring smaller than a workgroup
            hoist_dot_mac_loop_kernel<<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, target, target_stride, ext, ext_stride,
                                                                        ext_digit_stride, elts, w_sum_stride, acc, acc_stride, count,
                                                                        n_sums, e.logn, h.nd, add ? 1 : 0);
        return hipGetLastError();
    }

    hipError_t launch_hoist_dot_base(const Engine &e, const u64 *cn, const HoistDotElts &elts, std::size_t w_sum_stride,
                                     u64 *out, std::size_t out_sum_stride, int k, std::size_t count, std::size_t n_sums,
                                     bool add)
    {
        const std::size_t total = (n_sums * count * static_cast<std::size_t>(k)) << e.logn;
        if (total == 0 || !elts.n)
            return hipSuccess;
        if (elts.n < 0 || elts.n > kHoistMaxElts)
            return hipErrorInvalidValue;
        ProfScope prof(e, "hoist_dot_base", 0);
        hoist_dot_base_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(cn, elts, w_sum_stride, out, out_sum_stride,
                                                                                e.d_primes, k, e.logn, count, n_sums,
                                                                                add ? 1 : 0);
        return hipGetLastError();
    }

    hipError_t launch_hoist_giant_mac(const Engine &e, const KsDev *d, const KsDev &h, const HoistGiantElts &elts,
                                      std::size_t inb_stride, std::size_t ext_stride, std::size_t ext_digit_stride,
                                      std::size_t accj_stride, u64 *acc, std::size_t acc_stride, std::size_t count, bool add)
    {
        if (!count || !elts.n)
            return hipSuccess;
        const MacChoice c = select_hoist_giant_mac(e.logn, h.nd, static_cast<std::size_t>(h.k + h.nsp), elts.n, count);
        if (c.family == kMacRefused)
            return hipErrorInvalidValue;
        ProfScope prof(e, "hoist_giant_mac", 0);
        const hipStream_t stream = e.lane().stream;
        if (!dispatch_mac_digits(c.nd, [&](auto nd) {
                hoist_giant_mac_kernel<decltype(nd)::value><<<c.blocks, kThreads, 0, stream>>>(
                    d, e.d_primes, elts, inb_stride, ext_stride, ext_digit_stride, accj_stride, acc, acc_stride, count, e.logn,
                    add ? 1 : 0);
            })) // more than 16 digits, or a ring smaller than a workgroup
            hoist_giant_mac_loop_kernel<<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, elts, inb_stride, ext_stride,
                                                                          ext_digit_stride, accj_stride, acc, acc_stride, count, e.logn,
                                                                          h.nd, add ? 1 : 0);
        return hipGetLastError();
    }

    hipError_t launch_hoist_giant_base(const Engine &e, const HoistGiantBases &elts, u64 *out, int k, std::size_t count,
                                       bool add)
    {
        const std::size_t total = (count * static_cast<std::size_t>(k)) << e.logn;
        if (total == 0 || !elts.n)
            return hipSuccess;
        if (elts.n < 0 || elts.n > kHoistMaxElts)
            return hipErrorInvalidValue;
        ProfScope prof(e, "hoist_giant_base", 0);
        hoist_giant_base_kernel<<<grid_for(total), kThreads, 0, e.lane().stream>>>(elts, out, e.d_primes, k, e.logn, count,
                                                                                  add ? 1 : 0);
        return hipGetLastError();
    }
} // namespace sealhip
