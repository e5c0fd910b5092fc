// keyswitch.hip -- column-parallel kernels of the hybrid (multi-special-prime) key switch:
// modup_rns / modup_to_single_rns (native/src/seal/multi_special_primes.cpp:80-185), the 128-bit
// inner product against the key (native/src/seal/evaluator.cpp:2315-2357) and
// rescale_special_rns_inplace (multi_special_primes.cpp:237-304).
//
// The reference recomputes the punctured products and inverses on every call
// (multi_special_primes.cpp:110-126, :244-248, :292-299); here they are context constants (KsDev).
// The reference also keeps two (k+nsp) x N arrays of 128-bit accumulators in memory across the digit
// loop; here one lane owns one (row, coefficient) and keeps both accumulators in registers across
// all digits, streaming the key slices.
#include <cstdlib>
#include "engine.hpp"
#include "instance_dispatch.hpp"
#include "ks_inner.hpp"

namespace sealhip
{
    namespace
    {
        // modup constants of digit j: [inv_punch(nsp) | inv_punch_shoup(nsp) | punch[rows][nsp]]
        __device__ __forceinline__ const u64 *modup_block(const KsDev *d, int j)
        {
            const int rows = d->k + d->nsp;
            return d->modup + static_cast<std::size_t>(j) * (2 * d->nsp + rows * d->nsp);
        }

        // For every digit j (or only `only_digit`): read the bundle's coefficient-form rows and write every
        // row outside the bundle of ext[item][j].
        __global__ __launch_bounds__(kThreads) void ks_modup_kernel(const KsDev *__restrict__ d,
                                                                    const PrimeDev *__restrict__ primes,
                                                                    const u64 *__restrict__ coeff,
                                                                    std::size_t coeff_stride, u64 *__restrict__ ext,
                                                                    std::size_t ext_stride,
                                                                    std::size_t ext_digit_stride, std::size_t count,
                                                                    int logn, int only_digit)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t item = i >> logn;
            if (item >= count)
                return;
            const std::size_t c = i & ((static_cast<std::size_t>(1) << logn) - 1);
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const int k = d->k, nsp = d->nsp, rows = k + nsp;
            const u64 *src = coeff + item * coeff_stride + c;
            const int j_begin = only_digit >= 0 ? only_digit : 0;
            const int j_end = only_digit >= 0 ? only_digit + 1 : d->nd;
            for (int j = j_begin; j < j_end; j++)
            {
                const int r0 = j * nsp;
                const int r1 = r0 + nsp < k ? r0 + nsp : k;
                const int bs = r1 - r0;
                u64 *dst = ext + item * ext_stride + static_cast<std::size_t>(j) * ext_digit_stride + c;
                if (bs == 1)
                {
                    // multi_special_primes.cpp:99-108
                    const u64 x = src[r0 * N];
                    const u64 psrc = primes[d->row_prime[r0]].p;
                    for (int r = 0; r < rows; r++)
                    {
                        if (r == r0)
                            continue;
                        const PrimeDev &D = primes[d->row_prime[r]];
                        dst[r * N] = psrc <= D.p ? x : barrett_reduce_63(x, D.p, D.cr1);
                    }
                    continue;
                }
                const u64 *blk = modup_block(d, j);
                u64 y[kMaxModuli > 8 ? 8 : kMaxModuli]; // bundles wider than 8 fall back to recomputation
                const bool cached = bs <= 8;
                if (cached)
                {
#pragma unroll
                    for (int a = 0; a < 8; a++)
                        if (a < bs)
                        {
                            const u64 p = primes[d->row_prime[r0 + a]].p;
                            y[a] = mulmod_shoup(src[(r0 + a) * N], blk[a], blk[nsp + a], p); // :135-139
                        }
                }
                for (int r = 0; r < rows; r++)
                {
                    if (r >= r0 && r < r1)
                        continue;
                    const PrimeDev &D = primes[d->row_prime[r]];
                    const u64 *punch = blk + 2 * nsp + r * nsp;
                    u64 lo = 0, hi = 0;
                    if (cached)
                    {
#pragma unroll
                        for (int a = 0; a < 8; a++)
                            if (a < bs)
                                mac128(lo, hi, y[a], punch[a]);
                    }
                    else
                    {
                        for (int a = 0; a < bs; a++)
                        {
                            const u64 p = primes[d->row_prime[r0 + a]].p;
                            mac128(lo, hi, mulmod_shoup(src[(r0 + a) * N], blk[a], blk[nsp + a], p), punch[a]);
                        }
                    }
                    dst[r * N] = barrett_reduce_128(lo, hi, D.p, D.cr0, D.cr1); // :143-146
                }
            }
        }

        // prod[item][l][r][c] = barrett_reduce_128( sum_j ct_j[r][c] * key[j][l][row_prime[r]][c] )
        // where ct_j = the (NTT-form) target row if r is in bundle j, else ext[j][item][r] (digit-major)
        // (evaluator.cpp:2315-2349). One lane per (item, row, coefficient).
        __global__ __launch_bounds__(kThreads) void ks_mac_kernel(const KsDev *__restrict__ d,
                                                                  const PrimeDev *__restrict__ primes,
                                                                  const u64 *__restrict__ target,
                                                                  std::size_t target_stride,
                                                                  const u64 *__restrict__ ext, std::size_t ext_stride,
                                                                  std::size_t ext_digit_stride,
                                                                  const u64 *__restrict__ key,
                                                                  u64 *__restrict__ prod, std::size_t prod_stride,
                                                                  std::size_t count, int logn, int j0, int j1)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const int r = static_cast<int>(lane.q % dim.rows);
            const std::size_t item = lane.q / dim.rows;
            if (item >= count)
                return;
            const MacRow m = mac_row(dim, d, r, N);
            u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
            const u64 *pext = ext + item * ext_stride + m.row_off() + lane.c, *pkey = key + m.prime_row() + lane.c;
            const u64 *own = target + m.row_off() + lane.c + item * target_stride;
            for (int j = j0; j < j1; j++) // (all digits of the level, or one device's share of them: latency mode)
                digit_mac(m, j, pext, ext_digit_stride, pkey, own, lo0, hi0, lo1, hi1);
            u64 *pp = prod + item * prod_stride + m.row_off() + lane.c;
            const MacMod mod = mac_mod(primes, m);
            pp[0] = barrett_reduce_128(lo0, hi0, mod.p, mod.cr0, mod.cr1); // (not mod.reduce: it reschedules this kernel; plain stores as ever)
            pp[m.comp()] = barrett_reduce_128(lo1, hi1, mod.p, mod.cr0, mod.cr1);
        }

        // The same inner product with the key words of a lane's (row, coefficient) kept in registers across
        // `group` consecutive ciphertexts: the key slice (2 * nd words per lane, 29 MB per pass at cfg3) is read once
        // per group instead of once per ciphertext (it made up two thirds of this kernel's read traffic at group 1, and
        // still 17 % at group 8: config 4 reads 132 digit rows, writes 24 and re-reads 264 / group key rows per
        // ciphertext). The digit words of the next ciphertext are requested before the current one is accumulated, so the
        // group size costs no registers; the launcher picks it from the batch (mac_group).
        template <int ND>
        __global__ __launch_bounds__(kThreads) void ks_mac_items_kernel(const KsDev *__restrict__ d,
                                                                        const PrimeDev *__restrict__ primes,
                                                                        const u64 *__restrict__ target,
                                                                        std::size_t target_stride,
                                                                        const u64 *__restrict__ ext,
                                                                        std::size_t ext_stride,
                                                                        std::size_t ext_digit_stride,
                                                                        const u64 *__restrict__ key,
                                                                        u64 *__restrict__ prod, std::size_t prod_stride,
                                                                        std::size_t count, int logn, std::size_t group)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const MacDims dim = mac_dims(d);
            const MacLane lane = flat_lane(logn);
            const int r = static_cast<int>(lane.q % dim.rows);
            const std::size_t item0 = (lane.q / dim.rows) * group;
            if (item0 >= count)
                return;
            const std::size_t item1 = item0 + group < count ? item0 + group : count;
            const MacRow m = mac_row(dim, d, r, N);
            const std::size_t off = m.row_off() + lane.c;
            const u64 *pkey = key + m.prime_row() + lane.c;
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
                    dst[j] = j == m.my_digit ? target[item * target_stride + off]
                                             : ext[item * ext_stride + static_cast<std::size_t>(j) * ext_digit_stride + off];
            };
            load_x(x, item0);
            const MacMod mod = mac_mod(primes, m);
            for (std::size_t item = item0; item < item1; item++)
            {
                if (item + 1 < item1)
                    load_x(xn, item + 1);
                u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
#pragma unroll
                for (int j = 0; j < ND; j++) // (not mac2: instance 4 would be scheduled differently)
                {
                    mac128(lo0, hi0, x[j], k0[j]);
                    mac128(lo1, hi1, x[j], k1[j]);
                }
                u64 *pp = prod + item * prod_stride + off;
                store_stream(pp, mod.reduce(lo0, hi0));
                store_stream(pp + m.comp(), mod.reduce(lo1, hi1));
#pragma unroll
                for (int j = 0; j < ND; j++)
                    x[j] = xn[j];
            }
        }

        // The pair form of ks_mac_items_kernel, for digit rows whose forward transform stopped before its last layer
        // (kNttSplitLast): row r of ext[j][item] holds E[0..N/2) | O[0..N/2), the transforms of the even- and
        // the odd-indexed coefficients as rings of N/2. One lane per pair index c < N/2 finishes the transform,
        //   X[2c] = E[c] + T,  X[2c+1] = E[c] - T + 2p,  T = O[c] * psi^brev(N/2 + c) as an exact lazy Shoup product (below 2p),
        // with the twiddle pair from the second half of PrimeDev::fwd loaded once and kept across the group like the key words,
        // and accumulates both words into the two components' sums with the key words at 2c, 2c + 1 (16-byte loads; the two
        // canonical residues of a component leave as one 16-byte store). The in-bundle row is the target's whole transform: its
        // pair 2c, 2c + 1 is taken as it is. The words are below 2^64 and nd p < 2^64 (bounds::fwd_split_admits): the 128-bit
        // sums cannot wrap. Workgroups never straddle a row (N/2 >= 2^13 lanes per row): the row's facts are scalars.
        // PF: request the next ciphertext's words before the current one is accumulated (dropped where it would spill).
        // The sums use mac128_wide (devmath.hpp).
        template <int ND, bool PF>
        __global__ __launch_bounds__(kThreads) void ks_mac_pair_kernel(const KsDev *__restrict__ d,
                                                                       const PrimeDev *__restrict__ primes,
                                                                       const u64 *__restrict__ target,
                                                                       std::size_t target_stride,
                                                                       const u64 *__restrict__ ext, std::size_t ext_stride,
                                                                       std::size_t ext_digit_stride,
                                                                       const u64 *__restrict__ key,
                                                                       u64 *__restrict__ prod, std::size_t prod_stride,
                                                                       std::size_t count, int logn, std::size_t group)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn, H = N >> 1;
            const MacDims dim = mac_dims(d);
            const std::size_t lane0 = blockIdx.x * static_cast<std::size_t>(kThreads); // (uniform: H is a multiple of kThreads)
            const std::size_t c0 = lane0 & (H - 1); // the workgroup's first pair; the lane's is c0 + threadIdx.x
            const std::size_t rr = lane0 >> (logn - 1);
            const int r = static_cast<int>(rr % dim.rows);
            const std::size_t item0 = (rr / dim.rows) * group;
            if (item0 >= count)
                return;
            const std::size_t item1 = item0 + group < count ? item0 + group : count;
            const MacRow m = mac_row(dim, d, r, N);
            const int my_digit = m.my_digit;
            const std::size_t row_off = m.row_off();
            const MacMod mod = mac_mod(primes, m);
            const u64 p = mod.p, two_p = mod.two_p, cr0 = mod.cr0, cr1 = mod.cr1;
            // every address is a uniform base (scalar registers) plus the lane's 32-bit byte offset: one offset register for
            // the 8-byte words and one for the 16-byte pairs instead of a 64-bit address per load
            const unsigned off8 = threadIdx.x * 8u, off16 = threadIdx.x * 16u;
            const auto word = [](const u64 *base, unsigned off) {
                return *reinterpret_cast<const u64 *>(reinterpret_cast<const char *>(base) + off);
            };
            const auto pair = [](const u64 *base, unsigned off) {
                return *reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const char *>(base) + off);
            };
            const u64 *key_row = key + m.prime_row() + 2 * c0;
            const std::size_t key_comp = m.key_comp();
            const ulonglong2 w = pair(primes[m.rns_idx].fwd + 2 * (H + c0), off16); // (twiddle, its Shoup quotient) of pair c
            ulonglong2 k0[ND], k1[ND];
#pragma unroll
            for (int j = 0; j < ND; j++)
            {
                k0[j] = pair(key_row + (2 * static_cast<std::size_t>(j)) * key_comp, off16);
                k1[j] = pair(key_row + (2 * static_cast<std::size_t>(j) + 1) * key_comp, off16);
            }
            // where the next ciphertext's words of digit j start for this workgroup (uniform; advanced by every load_x) -- in
            // the bundle: words 2c, 2c + 1 of the target row; else E[c], O[c] of the digit row
            const u64 *src[ND];
#pragma unroll
            for (int j = 0; j < ND; j++)
                src[j] = j == my_digit ? target + item0 * target_stride + row_off + 2 * c0
                                       : ext + item0 * ext_stride + static_cast<std::size_t>(j) * ext_digit_stride + row_off + c0;
            const unsigned off8_o = off8 + (static_cast<unsigned>(H) << 3), off16_o = off16 + 8u;
            const auto load_x = [&](u64(&e)[ND], u64(&o)[ND]) {
#pragma unroll
                for (int j = 0; j < ND; j++)
                {
                    const bool inb = j == my_digit;
                    e[j] = word(src[j], inb ? off16 : off8);
                    o[j] = word(src[j], inb ? off16_o : off8_o);
                    src[j] += inb ? target_stride : ext_stride;
                }
            };
            // one ciphertext: the pair butterflies, the four sums, the two stores
            const auto accumulate = [&](const u64(&e)[ND], const u64(&o)[ND], std::size_t item) {
                u64 lo00 = 0, hi00 = 0, lo01 = 0, hi01 = 0, lo10 = 0, hi10 = 0, lo11 = 0, hi11 = 0;
#pragma unroll
                for (int j = 0; j < ND; j++)
                {
                    u64 x0 = e[j], x1 = o[j];
                    if (j != my_digit)
                    {
                        const u64 t = mulmod_lazy(x1, w.x, w.y, p);
                        x1 = x0 - t + two_p;
                        x0 = x0 + t;
                    }
                    mac128_wide(lo00, hi00, x0, k0[j].x);
                    mac128_wide(lo01, hi01, x1, k0[j].y);
                    mac128_wide(lo10, hi10, x0, k1[j].x);
                    mac128_wide(lo11, hi11, x1, k1[j].y);
                }
                u64 *pp = reinterpret_cast<u64 *>(reinterpret_cast<char *>(prod + item * prod_stride + row_off + 2 * c0) + off16);
                store_stream2(pp, barrett_reduce_128(lo00, hi00, p, cr0, cr1), barrett_reduce_128(lo01, hi01, p, cr0, cr1));
                store_stream2(pp + m.comp(), barrett_reduce_128(lo10, hi10, p, cr0, cr1),
                              barrett_reduce_128(lo11, hi11, p, cr0, cr1));
            };
            u64 xe[ND], xo[ND];
            load_x(xe, xo);
            if constexpr (PF)
            {
                // two ciphertexts per trip, the buffers changing roles: the next one's words are requested before the current
                // one is accumulated, and nothing is copied
                u64 ne[ND], no[ND];
                for (std::size_t item = item0; item < item1; item += 2)
                {
                    if (item + 1 < item1)
                        load_x(ne, no);
                    accumulate(xe, xo, item);
                    if (item + 1 >= item1)
                        break;
                    if (item + 2 < item1)
                        load_x(xe, xo);
                    accumulate(ne, no, item + 1);
                }
            }
            else
                for (std::size_t item = item0; item < item1; item++)
                {
                    accumulate(xe, xo, item);
                    if (item + 1 < item1)
                        load_x(xe, xo);
                }
        }

        // rescale_special_rns_inplace, steps 1-2 (multi_special_primes.cpp:253-282): from the (coefficient
        // form) special rows of one polynomial compute temp_i for every ciphertext prime i.
        __global__ __launch_bounds__(kThreads) void ks_moddown_pre_kernel(const KsDev *__restrict__ d,
                                                                          const PrimeDev *__restrict__ primes,
                                                                          const u64 *__restrict__ prod,
                                                                          std::size_t prod_stride,
                                                                          u64 *__restrict__ temp,
                                                                          std::size_t temp_stride, std::size_t npolys,
                                                                          int logn)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t poly = i >> logn;
            if (poly >= npolys)
                return;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const std::size_t c = i & (N - 1);
            const int k = d->k, nsp = d->nsp;
            const u64 *sp = prod + poly * prod_stride + static_cast<std::size_t>(k) * N + c;
            u64 *pt = temp + poly * temp_stride + c;
            if (nsp == 1)
            {
                const PrimeDev &S = primes[d->row_prime[k]];
                const u64 v = neg_mod(barrett_reduce_63(sp[0], S.p, S.cr1), S.p); // :270-273
                for (int q = 0; q < k; q++)
                {
                    const PrimeDev &Q = primes[d->row_prime[q]];
                    pt[q * N] = barrett_reduce_63(v, Q.p, Q.cr1); // (v < P < 2^61: the one-word Barrett step gives the same canonical residue)
                }
                return;
            }
            for (int q = 0; q < k; q++)
            {
                const PrimeDev &Q = primes[d->row_prime[q]];
                u64 lo = 0, hi = 0;
                for (int j = 0; j < nsp; j++)
                {
                    const u64 pj = primes[d->row_prime[k + j]].p;
                    const u64 y = mulmod_shoup(sp[j * N], d->inv_hat[j], d->inv_hat_shoup[j], pj); // :262-267
                    mac128(lo, hi, y, d->neg_hat[q * nsp + j]);
                }
                pt[q * N] = barrett_reduce_128(lo, hi, Q.p, Q.cr0, Q.cr1);
            }
        }

        // step 4 (multi_special_primes.cpp:291-302) + the final add_poly_coeffmod of evaluator.cpp:2363-2366
        __global__ __launch_bounds__(kThreads) void ks_moddown_post_kernel(const KsDev *__restrict__ d,
                                                                           const PrimeDev *__restrict__ primes,
                                                                           u64 *__restrict__ prod,
                                                                           std::size_t prod_stride,
                                                                           const u64 *__restrict__ temp,
                                                                           std::size_t temp_stride,
                                                                           u64 *__restrict__ ct,
                                                                           std::size_t ct_item_stride,
                                                                           std::size_t npolys, int logn,
                                                                           int add_into_ct, const u64 *__restrict__ c0_src,
                                                                           std::size_t c0_stride, unsigned *__restrict__ tflags)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const int k = d->k;
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t c = i & (N - 1);
            const std::size_t rr = i >> logn;
            const int q = static_cast<int>(rr % k);
            const std::size_t poly = rr / k;
            if (poly >= npolys)
                return;
            const PrimeDev &Q = primes[d->row_prime[q]];
            u64 *pp = prod + poly * prod_stride + static_cast<std::size_t>(q) * N + c;
            const u64 v = mulmod_shoup(*pp + temp[poly * temp_stride + static_cast<std::size_t>(q) * N + c], d->invP[q],
                                       d->invP_shoup[q], Q.p);
            if (add_into_ct)
            {
                // polynomial `poly` is component (poly & 1) of ciphertext (poly >> 1)
                u64 *pc = ct + (poly >> 1) * ct_item_stride + ((poly & 1) * static_cast<std::size_t>(k) + q) * N + c;
                u64 w;
                if (!c0_src)
                    w = add_mod(v, *pc, Q.p);
                else // apply_galois: the ciphertext is (c0_src, 0) and only written here (evaluator.cpp:1903-1935)
                    w = (poly & 1) ? v : add_mod(v, c0_src[(poly >> 1) * c0_stride + static_cast<std::size_t>(q) * N + c], Q.p);
                *pc = w;
                if (poly & 1)
                    note_nonzero(tflags, poly >> 1, w);
            }
            else
                *pp = v;
        }

        // BFV: rescale_special_rns_inplace (multi_special_primes.cpp:237-304) + the final add (evaluator.cpp:2363-2366)
        // in one kernel. In BFV nothing happens between steps 2 and 4 of the rescale (the q rows are simply brought
        // to coefficient form), so temp_q is recomputed per lane from the special rows instead of being written
        // by one kernel and read by the next (2*k row transfers per polynomial), and with DEFER the top inverse-NTT
        // layer of every row read here is applied on load (kNttDeferTop: no ntt_inv_top pass over the 2*(k+nsp) rows).
        // Every value that leaves this kernel is a canonical residue of an exact modular expression, so the
        // representatives chosen for the intermediates do not matter.
        // both coefficients c and c + N/2 of one row: with DEFER the top inverse-NTT layer (BackwardLazyLast,
        // ntt.cpp:274-281) is applied to the pair, else the two words are used as they are
        template <bool DEFER>
        __device__ __forceinline__ void row_pair(const u64 *__restrict__ row, std::size_t c_lo, std::size_t half,
                                                 const PrimeDev &P, u64 &x_lo, u64 &x_hi)
        {
            const u64 u = row[c_lo], v = row[c_lo + half];
            if (!DEFER)
            {
                x_lo = u;
                x_hi = v;
                return;
            }
            u64 tt = u + v;
            tt = tt >= P.two_p ? tt - P.two_p : tt;
            x_lo = mulmod_lazy(tt, P.inv_n, P.inv_n_shoup, P.p);
            x_hi = mulmod_lazy(u - v + P.two_p, P.inv_n_w, P.inv_n_w_shoup, P.p);
        }

        // One lane per (polynomial, coefficient pair c / c + N/2), walking the k ciphertext primes: the special rows (and, with
        // DEFER, their top inverse-NTT layer) are read and reduced ONCE per column pair -- round 3; one lane per (polynomial,
        // prime, pair) had every q lane fetch and transform them again: 6 of 28 row passes per polynomial at config 3 -- every
        // other input word exactly once.
        // ONE: a single special prime (every BASELINE config): its reduced pair lives in two registers across the loop; several
        // special primes re-read their rows per ciphertext prime (the lane's own addresses: L1 hits) as before.
        template <bool DEFER, bool ONE>
        __global__ __launch_bounds__(kThreads) void ks_moddown_bfv_kernel(const KsDev *__restrict__ d,
                                                                          const PrimeDev *__restrict__ primes,
                                                                          const u64 *__restrict__ prod,
                                                                          std::size_t prod_stride, u64 *__restrict__ ct,
                                                                          std::size_t ct_item_stride, std::size_t npolys,
                                                                          int logn, const u64 *__restrict__ c0_src,
                                                                          std::size_t c0_stride, unsigned *__restrict__ tflags)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn, half = N >> 1;
            const int k = d->k, nsp = d->nsp;
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t c = i & (half - 1);
            const std::size_t poly = i >> (logn - 1);
            if (poly >= npolys)
                return;
            const u64 *pp = prod + poly * prod_stride;
            // steps 1-2, the part that does not depend on the ciphertext prime (multi_special_primes.cpp:253-273)
            u64 sred[2] = {0, 0};
            if constexpr (ONE)
            {
                const PrimeDev &S = primes[d->row_prime[k]];
                u64 sv[2];
                row_pair<DEFER>(pp + static_cast<std::size_t>(k) * N, c, half, S, sv[0], sv[1]);
#pragma unroll
                for (int h = 0; h < 2; h++)
                    sred[h] = neg_mod(barrett_reduce_63(sv[h], S.p, S.cr1), S.p); // :270-273
            }
            u64 nz = 0;
            for (int q = 0; q < k; q++)
            {
                const PrimeDev &Q = primes[d->row_prime[q]];
                u64 temp[2];
                if constexpr (ONE)
                {
#pragma unroll
                    for (int h = 0; h < 2; h++)
                        // (sred < P < 2^61 is one word: the one-word Barrett step -- a 64-bit high product, a multiply, a
                        //  conditional subtraction -- gives the canonical residue the two-word form gave with four times the work)
                        temp[h] = barrett_reduce_63(sred[h], Q.p, Q.cr1);
                }
                else
                {
                    u64 lo[2] = {0, 0}, hi[2] = {0, 0};
                    for (int j = 0; j < nsp; j++)
                    {
                        const PrimeDev &S = primes[d->row_prime[k + j]];
                        u64 sv[2];
                        row_pair<DEFER>(pp + static_cast<std::size_t>(k + j) * N, c, half, S, sv[0], sv[1]);
#pragma unroll
                        for (int h = 0; h < 2; h++)
                        {
                            const u64 y = mulmod_shoup(sv[h], d->inv_hat[j], d->inv_hat_shoup[j], S.p); // :262-267
                            mac128(lo[h], hi[h], y, d->neg_hat[q * nsp + j]);
                        }
                    }
                    temp[0] = barrett_reduce_128(lo[0], hi[0], Q.p, Q.cr0, Q.cr1);
                    temp[1] = barrett_reduce_128(lo[1], hi[1], Q.p, Q.cr0, Q.cr1);
                }
                // step 4 (:291-302) and the add into the ciphertext
                u64 pv[2];
                row_pair<DEFER>(pp + static_cast<std::size_t>(q) * N, c, half, Q, pv[0], pv[1]);
                u64 *pc = ct + (poly >> 1) * ct_item_stride + ((poly & 1) * static_cast<std::size_t>(k) + q) * N + c;
#pragma unroll
                for (int h = 0; h < 2; h++)
                {
                    const u64 v = mulmod_shoup(pv[h] + temp[h], d->invP[q], d->invP_shoup[q], Q.p);
                    u64 w;
                    if (!c0_src)
                        w = add_mod(v, pc[h * half], Q.p);
                    else // apply_galois: the ciphertext is (c0_src, 0) and only written here (evaluator.cpp:1903-1935)
                        w = (poly & 1) ? v
                                       : add_mod(v, c0_src[(poly >> 1) * c0_stride + static_cast<std::size_t>(q) * N + c + h * half], Q.p);
                    pc[h * half] = w;
                    nz |= w;
                }
            }
            if (poly & 1) // component 1 of ciphertext poly >> 1: what is_transparent looks at
                note_nonzero(tflags, poly >> 1, nz);
        }

        // ---- the mod-down merged with the CKKS rescale (tests/ks_rescale_ref.py) ----
        // step 1's fold: acc[pl][k-1] += (P mod l) * base[..][k-1], NTT form, canonical. One lane per (polynomial, coefficient).
        __global__ __launch_bounds__(kThreads) void ks_rescale_fold_kernel(const KsRescaleDev *__restrict__ d,
                                                                           const PrimeDev *__restrict__ primes,
                                                                           const u64 *__restrict__ base, std::size_t base_stride,
                                                                           u64 *__restrict__ acc, std::size_t acc_stride,
                                                                           std::size_t npolys, int logn)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t poly = i >> logn;
            if (poly >= npolys)
                return;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const std::size_t c = i & (N - 1);
            const int k = d->k;
            const PrimeDev &L = primes[d->drop_prime[0]];
            const u64 b = base[(poly >> 1) * base_stride + ((poly & 1) * static_cast<std::size_t>(k) + (k - 1)) * N + c];
            u64 *pa = acc + poly * acc_stride + static_cast<std::size_t>(k - 1) * N + c;
            *pa = mul_add_mod(b, d->P_mod_l, *pa, L.p, L.cr0, L.cr1);
        }

        // step 2 for dropped prime a, and step 3's term floor(z * C_d / 2^64) = z * cr1 + mulhi(z, cr0) added into (slo, shi):
        // z < d and C_d = cr1 * 2^64 + cr0 <= 2^128 / d, so z * cr1 < 2^64 and the term fits one word
        __device__ __forceinline__ u64 rescale_z(const KsRescaleDev *__restrict__ d, const PrimeDev *__restrict__ primes, int a,
                                                 u64 y, u64 &slo, u64 &shi)
        {
            const PrimeDev &S = primes[d->drop_prime[a]];
            const u64 z = mulmod_shoup(add_mod(y, d->half_d[a], S.p), d->inv_hat[a], d->inv_hat_shoup[a], S.p);
            const u64 t = z * S.cr1 + mulhi(z, S.cr0);
            const u64 nl = slo + t;
            shi += nl < slo;
            slo = nl;
            return z;
        }

        // steps 2-4 up to the forward transform: one lane per (polynomial, coefficient) computes z_d and the exact quotient v
        // once and walks the k - 1 kept primes. ND1 = |Dset| = nsp + 1 in 2..4 keeps z_d in registers; ND1 = 0 is the loop
        // form for larger sets, which re-reads the dropped rows per kept prime (the lane's own addresses: L1 hits) as
        // ks_moddown_pre_kernel does -- no array indexed by a run-time value.
        // The sum of step 4 is at most (nsp + 1) (2^61)^2 + (nsp + 1) 2^61 + 2^61 < 2^128 for nsp + 1 <= 64 primes of 61 bits
        // (bounds::ks_rescale_sum_fits, executed by tests/ks_rescale_bounds_check.cpp).
        template <int ND1>
        __global__ __launch_bounds__(kThreads) void ks_moddown_rescale_pre_kernel(const KsRescaleDev *__restrict__ d,
                                                                                  const PrimeDev *__restrict__ primes,
                                                                                  const u64 *__restrict__ acc,
                                                                                  std::size_t acc_stride, u64 *__restrict__ temp,
                                                                                  std::size_t npolys, int logn)
        {
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t poly = i >> logn;
            if (poly >= npolys)
                return;
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const std::size_t c = i & (N - 1);
            const int k = d->k, nd1 = d->nsp + 1;
            const u64 *dp = acc + poly * acc_stride + static_cast<std::size_t>(k - 1) * N + c; // dropped row a: dp[a * N]
            u64 *pt = temp + poly * static_cast<std::size_t>(k - 1) * N + c;
            u64 slo = 0, shi = 0;
            if constexpr (ND1 > 0)
            {
                u64 z[ND1];
#pragma unroll
                for (int a = 0; a < ND1; a++)
                    z[a] = rescale_z(d, primes, a, dp[a * N], slo, shi);
                const u64 v = shi; // step 3: the sum's second word
                for (int r = 0; r < k - 1; r++)
                {
                    const PrimeDev &Q = primes[r];
                    const u64 *hat = d->hat + static_cast<std::size_t>(r) * ND1;
                    u64 lo = d->neg_half[r], hi = 0;
#pragma unroll
                    for (int a = 0; a < ND1; a++)
                        mac128(lo, hi, z[a], hat[a]);
                    mac128(lo, hi, v, d->neg_D[r]);
                    pt[r * N] = barrett_reduce_128(lo, hi, Q.p, Q.cr0, Q.cr1);
                }
            }
            else
            {
                for (int a = 0; a < nd1; a++)
                    rescale_z(d, primes, a, dp[a * N], slo, shi);
                const u64 v = shi;
                for (int r = 0; r < k - 1; r++)
                {
                    const PrimeDev &Q = primes[r];
                    const u64 *hat = d->hat + static_cast<std::size_t>(r) * nd1;
                    u64 lo = d->neg_half[r], hi = 0, s0 = 0, s1 = 0;
                    for (int a = 0; a < nd1; a++)
                        mac128(lo, hi, rescale_z(d, primes, a, dp[a * N], s0, s1), hat[a]);
                    mac128(lo, hi, v, d->neg_D[r]);
                    pt[r * N] = barrett_reduce_128(lo, hi, Q.p, Q.cr0, Q.cr1);
                }
            }
        }

        // step 5: out[pl][r] = (acc[pl][r] + (P mod q_r) * base[..][r] - temp[pl][r]) * D^-1 mod q_r; temp is canonical (the
        // forward transform canonicalises). One lane per (polynomial, kept row, coefficient); component 1 notes the flag.
        __global__ __launch_bounds__(kThreads) void ks_moddown_rescale_post_kernel(const KsRescaleDev *__restrict__ d,
                                                                                   const PrimeDev *__restrict__ primes,
                                                                                   const u64 *__restrict__ base,
                                                                                   std::size_t base_stride,
                                                                                   const u64 *__restrict__ acc,
                                                                                   std::size_t acc_stride,
                                                                                   const u64 *__restrict__ temp, u64 *__restrict__ out,
                                                                                   std::size_t npolys, int logn,
                                                                                   unsigned *__restrict__ tflags)
        {
            const std::size_t N = static_cast<std::size_t>(1) << logn;
            const int k = d->k, kk = k - 1;
            const std::size_t i = blockIdx.x * static_cast<std::size_t>(blockDim.x) + threadIdx.x;
            const std::size_t c = i & (N - 1);
            const std::size_t rr = i >> logn;
            const int r = static_cast<int>(rr % kk);
            const std::size_t poly = rr / kk;
            if (poly >= npolys)
                return;
            const PrimeDev &Q = primes[r];
            const std::size_t row = static_cast<std::size_t>(r) * N + c;
            const u64 b = base[(poly >> 1) * base_stride + (poly & 1) * static_cast<std::size_t>(k) * N + row];
            const u64 s = mul_add_mod(b, d->P_mod_q[r], acc[poly * acc_stride + row], Q.p, Q.cr0, Q.cr1);
            const std::size_t o = poly * static_cast<std::size_t>(kk) * N + row;
            const u64 w = mulmod_shoup(sub_mod(s, temp[o], Q.p), d->invD[r], d->invD_shoup[r], Q.p);
            store_stream(out + o, w);
            if (poly & 1)
                note_nonzero(tflags, poly >> 1, w);
        }
    } // namespace

    hipError_t launch_ks_modup(const Engine &e, const KsDev *d, const KsDev &, const u64 *coeff,
                               std::size_t coeff_stride, u64 *ext, std::size_t ext_stride,
                               std::size_t ext_digit_stride, std::size_t count, int only_digit)
    {
        if (!count)
            return hipSuccess;
        ProfScope prof(e, "ks_modup", 0);
        ks_modup_kernel<<<blocks_for(count << e.logn), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, coeff, coeff_stride, ext, ext_stride, ext_digit_stride, count, e.logn, only_digit);
        return hipGetLastError();
    }

    hipError_t launch_ks_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                             std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                             std::size_t ext_digit_stride, const u64 *key, u64 *prod, std::size_t prod_stride,
                             std::size_t count, int j0, int j1, bool pair)
    {
        if (!count)
            return hipSuccess;
        if (j1 < 0)
            j1 = h.nd;
        const MacChoice c = select_ks_mac(e.logn, h.nd, static_cast<std::size_t>(h.k + h.nsp), count, j0, j1, pair);
        if (c.family == kMacRefused)
            return hipErrorInvalidValue;
        ProfScope prof(e, "ks_mac", 0);
        const hipStream_t stream = e.lane().stream;
        bool launched = true;
        if (c.family == kMacPair)
            launched = dispatch_mac_digits(c.nd, [&](auto nd) {
                constexpr int ND = decltype(nd)::value;
                ks_mac_pair_kernel<ND, (ND <= kKsPairPrefetchDigits)><<<c.blocks, kThreads, 0, stream>>>(
                    d, e.d_primes, target, target_stride, ext, ext_stride, ext_digit_stride, key, prod, prod_stride, count, e.logn,
                    c.group);
            });
        else if (c.family == kMacItems)
            launched = dispatch_mac_digits(c.nd, [&](auto nd) {
                ks_mac_items_kernel<decltype(nd)::value><<<c.blocks, kThreads, 0, stream>>>(
                    d, e.d_primes, target, target_stride, ext, ext_stride, ext_digit_stride, key, prod, prod_stride, count, e.logn,
                    c.group);
            });
        else // small batches, a digit range or more than 16 digits: one lane per (ciphertext, row, coefficient)
            ks_mac_kernel<<<c.blocks, kThreads, 0, stream>>>(d, e.d_primes, target, target_stride, ext, ext_stride,
                                                            ext_digit_stride, key, prod, prod_stride, count, e.logn, j0, j1);
        return launched ? hipGetLastError() : hipErrorInvalidValue; // (the selector names no instance outside the range)
    }

    hipError_t launch_ks_moddown_pre(const Engine &e, const KsDev *d, const KsDev &, const u64 *prod,
                                     std::size_t prod_stride, u64 *temp, std::size_t temp_stride, std::size_t npolys)
    {
        if (!npolys)
            return hipSuccess;
        ProfScope prof(e, "ks_moddown_pre", 0);
        ks_moddown_pre_kernel<<<blocks_for(npolys << e.logn), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, prod, prod_stride, temp, temp_stride, npolys, e.logn);
        return hipGetLastError();
    }

    hipError_t launch_ks_moddown_bfv(const Engine &e, const KsDev *d, const KsDev &h, const u64 *prod,
                                     std::size_t prod_stride, u64 *ct, std::size_t ct_item_stride, std::size_t npolys,
                                     bool top_deferred, const u64 *c0_src, std::size_t c0_stride)
    {
        if (!npolys)
            return hipSuccess;
        const std::size_t lanes = npolys << (e.logn - 1); // one lane per (polynomial, coefficient pair)
        ProfScope prof(e, "ks_moddown_bfv", 0);
        dispatch_bool(top_deferred, [&](auto defer) {
            dispatch_bool(h.nsp == 1, [&](auto one) {
                ks_moddown_bfv_kernel<decltype(defer)::value, decltype(one)::value>
                    <<<blocks_for(lanes), kThreads, 0, e.lane().stream>>>(d, e.d_primes, prod, prod_stride, ct, ct_item_stride,
                                                                          npolys, e.logn, c0_src, c0_stride, e.lane().tsink_arm);
            });
        });
        return hipGetLastError();
    }

    hipError_t launch_ks_moddown_post(const Engine &e, const KsDev *d, const KsDev &h, u64 *prod,
                                      std::size_t prod_stride, const u64 *temp, std::size_t temp_stride, u64 *ct,
                                      std::size_t ct_item_stride, std::size_t npolys, int add_into_ct, const u64 *c0_src,
                                      std::size_t c0_stride)
    {
        if (!npolys)
            return hipSuccess;
        const std::size_t lanes = (npolys * static_cast<std::size_t>(h.k)) << e.logn;
        ProfScope prof(e, "ks_moddown_post", 0);
        ks_moddown_post_kernel<<<blocks_for(lanes), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, prod, prod_stride, temp, temp_stride, ct, ct_item_stride, npolys, e.logn, add_into_ct, c0_src, c0_stride,
            add_into_ct ? e.lane().tsink_arm : nullptr);
        return hipGetLastError();
    }

    hipError_t launch_ks_rescale_fold(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &, const u64 *base,
                                      std::size_t base_stride, u64 *acc, std::size_t acc_stride, std::size_t npolys)
    {
        if (!npolys)
            return hipSuccess;
        ProfScope prof(e, "ks_rescale_fold", 0);
        ks_rescale_fold_kernel<<<blocks_for(npolys << e.logn), kThreads, 0, e.lane().stream>>>(d, e.d_primes, base, base_stride, acc,
                                                                                            acc_stride, npolys, e.logn);
        return hipGetLastError();
    }

    hipError_t launch_ks_moddown_rescale_pre(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &h, const u64 *acc,
                                             std::size_t acc_stride, u64 *temp, std::size_t npolys)
    {
        if (!npolys)
            return hipSuccess;
        ProfScope prof(e, "ks_moddown_rescale_pre", 0);
        const auto launch = [&](auto nd1) {
            ks_moddown_rescale_pre_kernel<decltype(nd1)::value><<<blocks_for(npolys << e.logn), kThreads, 0, e.lane().stream>>>(
                d, e.d_primes, acc, acc_stride, temp, npolys, e.logn);
        };
        if (!dispatch_int<2, 4>(h.nsp + 1, launch)) // (larger sets: the loop form)
            launch(std::integral_constant<int, 0>{});
        return hipGetLastError();
    }

    hipError_t launch_ks_moddown_rescale_post(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &h, const u64 *base,
                                              std::size_t base_stride, const u64 *acc, std::size_t acc_stride, const u64 *temp,
                                              u64 *out, std::size_t npolys)
    {
        if (!npolys)
            return hipSuccess;
        const std::size_t lanes = (npolys * static_cast<std::size_t>(h.k - 1)) << e.logn;
        ProfScope prof(e, "ks_moddown_rescale_post", 0);
        ks_moddown_rescale_post_kernel<<<blocks_for(lanes), kThreads, 0, e.lane().stream>>>(
            d, e.d_primes, base, base_stride, acc, acc_stride, temp, out, npolys, e.logn, e.lane().tsink_arm);
        return hipGetLastError();
    }
} // namespace sealhip
