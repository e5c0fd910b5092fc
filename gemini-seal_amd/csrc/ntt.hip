// ntt.hip -- batched negacyclic NTT / inverse NTT for gfx950 (CDNA4).
//
// Replaces util::ntt_negacyclic_harvey{,_lazy} / inverse_ntt_negacyclic_harvey{,_lazy}
// (native/src/seal/util/ntt.cpp:292-404, ntt.h:225-334) for batches of RNS rows.
//
// Shape of the computation: integer, HBM-streaming, ALU-heavy (one Shoup butterfly = one
// 64x64->hi64 and two 64x64->lo64 products built from v_mad_u64_u32); no MFMA.
//
// Decomposition: a row of N = 2^logn coefficients is transformed in ONE launch: for logn <= 13 by the
// tiled kernel in this file (ntt_pass_kernel: the row is a TILE of 2^t coefficients staged HBM -> LDS with 16-byte
// coalesced loads, the threads run register-resident radix-16 rounds -- 16 coefficients = 4 index bits per
// thread, up to 4 butterfly layers per LDS round trip -- and the tile is stored back with 16-byte coalesced
// stores), for logn 14..16 by the single-pass half-row kernels: ntt_half.hpp (what both directions share),
// ntt_fwd.hip and ntt_inv.hip, reached through ntt_fwd_half / ntt_inv_half / ntt_inv_tensor. This file also holds the
// serial kernel of the tiny rings, the planner, the butterfly-rate probe and the public launch_ntt* / ntt_can_* entries.
// (The two-launch "strided columns, then contiguous rows" split of round 1 for logn > 13 was removed in round 4 with its switch.)
// Bit-exactness: every butterfly is exactly the reference's radix-2 lazy butterfly,
// only the schedule differs, so the 64-bit words (including the wrap-around behaviour for 60-bit
// primes) are identical. Twiddle of the butterfly on global bit b whose lower element
// has index j: table entry (N + j) >> (b + 1), in both directions.
//
// LDS image: index l is stored at l + (l >> 4) (one pad word per 16), which makes both the
// stride-1 and the stride-16 access patterns of the rounds bank-conflict free for ds_read_b64.
#include <cstdlib>
#include <stdexcept>

#include "ntt_half.hpp"

namespace sealhip
{
    namespace
    {
        constexpr int kTileBitsMax = 13; // 2^13 coefficients = 64 KiB (+4 KiB pad): two workgroups per CU

        __device__ __forceinline__ int pad_index(int l)
        {
            return l + (l >> 4);
        }

        // DIR 0: forward (Cooley-Tukey, descending bits), DIR 1: inverse (Gentleman-Sande, ascending bits)
        template <int DIR>
        __global__ __launch_bounds__(512, 4) void ntt_pass_kernel(u64 *__restrict__ data,
                                                               const PrimeDev *__restrict__ primes, RowMap map,
                                                               NttPass ps)
        {
            extern __shared__ u64 lds[];
            const int tid = threadIdx.x;
            const int nthreads = blockDim.x;
            const int t = ps.t, c = ps.c, b_lo = ps.b_lo, logn = ps.logn;
            const int tile = blockIdx.x & ((1 << (logn - t)) - 1);
            const size_t row = blockIdx.x >> (logn - t);
            const unsigned short pid = map.prime[row % map.rows];
            if (pid == kSkipRow)
                return; // block-uniform: this row is not part of the transform (e.g. in-bundle rows)
            const PrimeDev P = primes[pid];
            const u64 p = P.p, two_p = P.two_p;
            u64 *rowp = data + (row << logn);
            const int cmask = (1 << c) - 1;
            const int mid_bits = b_lo - c;
            const int base = ((tile >> mid_bits) << (b_lo + t - c)) | ((tile & ((1 << mid_bits) - 1)) << c);
            const u64 *tw = DIR == 0 ? P.fwd : P.inv;
            const int N = 1 << logn;
            const bool strict = (ps.flags & kNttStrict) != 0;

            // ---- stage in: 8 x 16-byte loads per thread, coalesced along the contiguous part of the tile
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
                int l = 2 * (i * nthreads + tid);
                int g = base + ((l >> c) << b_lo) + (l & cmask);
                const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(rowp + g);
                int a = pad_index(l);
                lds[a] = v.x;
                lds[a + 1] = v.y;
            }
            __syncthreads();

            for (int r = 0; r < ps.nrounds; r++)
            {
                const int beta = ps.rounds[r].beta, wlo = ps.rounds[r].wlo, whi = ps.rounds[r].whi;
                const int low = tid & ((1 << beta) - 1);
                const int l0 = ((tid >> beta) << (beta + 4)) | low;
                u64 x[16];
#pragma unroll
                for (int s = 0; s < 16; s++)
                    x[s] = lds[pad_index(l0 + (s << beta))];
                const int j0 = base + ((l0 >> c) << b_lo) + (l0 & cmask);

#pragma unroll
                for (int step = 0; step < 4; step++)
                {
                    const int w = DIR == 0 ? 3 - step : step;
                    if (w < wlo || w > whi)
                        continue; // wave-uniform
                    const int lb = beta + w;
                    const int gb = lb < c ? lb : lb - c + b_lo; // global bit of this layer
                    const int tb = (N + j0) >> (gb + 1);
                    const int bit = 1 << w;
                    if (DIR == 0)
                    {
                        const bool last = (gb == 0) && !strict;
                        // eight butterflies per layer, four at a time in lock step (devmath.hpp: butterflies_fwd_hs)
#pragma unroll
                        for (int c4 = 0; c4 < 8; c4 += 4)
                        {
                            u64 uu[4], yy[4], ww[4], ws[4];
#pragma unroll
                            for (int j = 0; j < 4; j++)
                            {
                                const int s = (((c4 + j) >> w) << (w + 1)) | ((c4 + j) & (bit - 1)); // (c4+j)-th slot with bit w clear
                                const ulonglong2 W = *reinterpret_cast<const ulonglong2 *>(tw + 2 * (tb + (s >> (w + 1))));
                                ww[j] = W.x;
                                ws[j] = W.y;
                                u64 u = x[s];
                                if (strict)
                                    u = u >= two_p ? u - two_p : u;
                                else if (last)
                                    u = barrett_lazy(u, P.rdp, p); // ForwardLazyLast, ntt.cpp:254-261
                                uu[j] = u;
                                yy[j] = x[s | bit];
                            }
                            butterflies_fwd_hs<false, 4>(uu, yy, ww, ws, 0 - p, two_p); // ForwardLazy, ntt.cpp:245-252
#pragma unroll
                            for (int j = 0; j < 4; j++)
                            {
                                const int s = (((c4 + j) >> w) << (w + 1)) | ((c4 + j) & (bit - 1));
                                x[s] = uu[j];
                                x[s | bit] = yy[j];
                            }
                        }
                    }
                    else
                    {
                        // Gentleman-Sande layer, four butterflies in lock step; the top layer (gap N/2) uses the merged
                        // twiddle psi^-1... * n^-1 on the difference side and multiplies the sum side by n^-1 afterwards
                        // (BackwardLazyLast, ntt.cpp:274-281)
                        const bool top = gb == logn - 1;
#pragma unroll
                        for (int c4 = 0; c4 < 8; c4 += 4)
                        {
                            u64 uu[4], yy[4], ww[4], ws[4];
#pragma unroll
                            for (int j = 0; j < 4; j++)
                            {
                                const int s = (((c4 + j) >> w) << (w + 1)) | ((c4 + j) & (bit - 1));
                                ulonglong2 W;
                                if (top)
                                {
                                    W.x = P.inv_n_w;
                                    W.y = P.inv_n_w_shoup;
                                }
                                else
                                    W = *reinterpret_cast<const ulonglong2 *>(tw + 2 * (tb + (s >> (w + 1))));
                                ww[j] = W.x;
                                ws[j] = W.y;
                                uu[j] = x[s];
                                yy[j] = x[s | bit];
                            }
                            butterflies_inv_hs<false, 4>(uu, yy, ww, ws, 0 - p, two_p); // BackwardLazy, ntt.cpp:265-272
#pragma unroll
                            for (int j = 0; j < 4; j++)
                            {
                                const int s = (((c4 + j) >> w) << (w + 1)) | ((c4 + j) & (bit - 1));
                                x[s] = top ? mulmod_lazy(uu[j], P.inv_n, P.inv_n_shoup, p) : uu[j];
                                x[s | bit] = yy[j];
                            }
                        }
                    }
                }
#pragma unroll
                for (int s = 0; s < 16; s++)
                    lds[pad_index(l0 + (s << beta))] = x[s];
                __syncthreads();
            }

            // ---- stage out (optionally with the canonicalising wrapper of ntt.h:236-245 / :328-333)
            const bool canon = (ps.flags & kNttCanonical) != 0;
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
                int l = 2 * (i * nthreads + tid);
                int g = base + ((l >> c) << b_lo) + (l & cmask);
                int a = pad_index(l);
                ulonglong2 v;
                v.x = lds[a];
                v.y = lds[a + 1];
                if (canon)
                {
                    if (DIR == 0)
                    {
                        v.x = v.x >= two_p ? v.x - two_p : v.x;
                        v.y = v.y >= two_p ? v.y - two_p : v.y;
                    }
                    v.x = v.x >= p ? v.x - p : v.x;
                    v.y = v.y >= p ? v.y - p : v.y;
                }
                *reinterpret_cast<ulonglong2 *>(rowp + g) = v;
            }
        }

        // One thread per row: the reference loop nest as written, for tiny rings (logn < 4) where a
        // radix-16 tile does not exist. Only the tests use such sizes.
        template <int DIR>
        __global__ void ntt_serial_kernel(u64 *__restrict__ data, const PrimeDev *__restrict__ primes, RowMap map,
                                          int logn, int flags, size_t nrows)
        {
            const size_t row = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
            if (row >= nrows)
                return;
            const unsigned short pid = map.prime[row % map.rows];
            if (pid == kSkipRow)
                return;
            const PrimeDev P = primes[pid];
            const u64 p = P.p, two_p = P.two_p;
            u64 *x = data + (row << logn);
            const int N = 1 << logn;
            const bool strict = (flags & kNttStrict) != 0;
            for (int step = 0; step < logn; step++)
            {
                const int b = DIR == 0 ? logn - 1 - step : step;
                const int h = 1 << b;
                for (int j = 0; j < N; j++)
                {
                    if (j & h)
                        continue;
                    const int ti = (N + j) >> (b + 1);
                    u64 W = (DIR == 0 ? P.fwd : P.inv)[2 * ti], Ws = (DIR == 0 ? P.fwd : P.inv)[2 * ti + 1];
                    if (DIR == 0)
                    {
                        u64 u = x[j];
                        if (strict)
                            u = u >= two_p ? u - two_p : u;
                        else if (b == 0)
                            u = barrett_lazy(u, P.rdp, p);
                        u64 v = mulmod_lazy(x[j + h], W, Ws, p);
                        x[j] = u + v;
                        x[j + h] = u - v + two_p;
                    }
                    else
                    {
                        const bool top = b == logn - 1;
                        if (top)
                        {
                            W = P.inv_n_w;
                            Ws = P.inv_n_w_shoup;
                        }
                        u64 u = x[j], v = x[j + h];
                        u64 tt = u + v;
                        tt = tt >= two_p ? tt - two_p : tt;
                        if (top)
                            tt = mulmod_lazy(tt, P.inv_n, P.inv_n_shoup, p);
                        x[j] = tt;
                        x[j + h] = mulmod_lazy(u - v + two_p, W, Ws, p);
                    }
                }
            }
            if (flags & kNttCanonical)
                for (int j = 0; j < N; j++)
                {
                    u64 v = x[j];
                    if (DIR == 0)
                        v = v >= two_p ? v - two_p : v;
                    x[j] = v >= p ? v - p : v;
                }
        }

        void make_rounds(NttPass &ps, int lo, int hi, bool inverse)
        {
            const int count = hi - lo + 1;
            const int first = ((count - 1) % 4) + 1;
            ps.nrounds = 0;
            int done = 0;
            while (done < count)
            {
                const int size = done == 0 ? first : 4;
                int r_lo, r_hi;
                if (!inverse)
                {
                    r_hi = hi - done;
                    r_lo = r_hi - size + 1;
                }
                else
                {
                    r_lo = lo + done;
                    r_hi = r_lo + size - 1;
                }
                NttRound &rd = ps.rounds[ps.nrounds++];
                rd.beta = r_lo < ps.t - 4 ? r_lo : ps.t - 4;
                rd.wlo = r_lo - rd.beta;
                rd.whi = r_hi - rd.beta;
                done += size;
            }
        }
    } // namespace

    const NttSwitches &ntt_switches()
    {
        static const NttSwitches sw = { std::getenv("SEALHIP_NTT_NO_FP64") != nullptr, std::getenv("SEALHIP_NTT_EXACT_FWD") != nullptr,
                                        std::getenv("SEALHIP_NTT_EXACT_INV") != nullptr,
                                        std::getenv("SEALHIP_NTT_CANON_EXACT") != nullptr };
        return sw;
    }
    bool fp64_enabled()
    {
        return !ntt_switches().no_fp64;
    }
    bool exact_fwd()
    {
        return ntt_switches().exact_fwd;
    }

    NttPlan plan_ntt(int logn, bool inverse, int flags)
    {
        NttPlan plan{};
        plan.logn = logn;
        plan.serial = logn < 4;
        plan.flags = flags;
        if (plan.serial)
        {
            plan.npass = 0;
            return plan;
        }
        auto init = [&](NttPass &ps, int t, int c, int b_lo, int lo, int hi) {
            ps.logn = logn;
            ps.t = t;
            ps.c = c;
            ps.b_lo = b_lo;
            ps.flags = flags & kNttStrict;
            make_rounds(ps, lo, hi, inverse);
        };
        // (round 4: the two-pass split for logn > 13 -- strided columns, then contiguous rows -- went with its switch
        //  SEALHIP_NTT_TWO_PASS: rings of 2^14 .. 2^16 are served by the single-pass kernels (ntt_fwd.hip, ntt_inv.hip), nothing else reached it)
        // (unreachable: launch_ntt serves rings above 2^13 with the single-pass kernels, the empty batch included, and
        //  refuses them itself before it gets here; this throw must never escape a hipError_t launcher)
        if (logn > kTileBitsMax)
            throw std::logic_error("plan_ntt: rings above 2^13 take the single-pass kernels");
        plan.npass = 1;
        init(plan.pass[0], logn, 0, 0, 0, logn - 1);
        plan.pass[plan.npass - 1].flags |= flags & kNttCanonical; // wrapper fused into the last store
        return plan;
    }

    template <int DIR>
    static hipError_t launch_dir(const Engine &e, u64 *data, size_t nrows, const RowMap &map, const NttPlan &plan)
    {
        if (nrows == 0)
            return hipSuccess;
        if (plan.serial)
        {
            const int threads = 64;
            const unsigned blocks = static_cast<unsigned>((nrows + threads - 1) / threads);
            ntt_serial_kernel<DIR><<<blocks, threads, 0, e.lane().stream>>>(data, e.d_primes, map, plan.logn, plan.flags, nrows);
            return hipGetLastError();
        }
        for (int i = 0; i < plan.npass; i++)
        {
            const NttPass &ps = plan.pass[i];
            const int threads = 1 << (ps.t - 4);
            const size_t lds_bytes = (static_cast<size_t>(1) << ps.t) * 8 + (static_cast<size_t>(1) << (ps.t - 4)) * 8;
            const size_t blocks = nrows << (plan.logn - ps.t);
            if (blocks > 0x7fffffffull)
                return hipErrorInvalidValue;
            hipError_t err;
            {
                ProfScope prof(e, DIR == 0 ? "ntt_fwd_pass" : "ntt_inv_pass", transformed_rows(nrows, map));
                ntt_pass_kernel<DIR><<<static_cast<unsigned>(blocks), threads, lds_bytes, e.lane().stream>>>(data, e.d_primes,
                                                                                                      map, ps);
                err = hipGetLastError();
            }
            if (err != hipSuccess)
                return err;
        }
        return hipSuccess;
    }

    // ---- the arithmetic ceiling of a butterfly sequence, measured on the device it runs on (sealhip_debug_butterfly_rate;
    // bench.py's roofline.valu_ceiling). Nothing but the butterflies of the single-pass kernels' rounds: the same lock-step
    // sequences, 32 values and four per-lane twiddles in registers, no loads, no exchanges, the same launch bounds (two
    // workgroups of 512 lanes per CU). KIND 0: the reference's lazy butterfly (exact Shoup quotient), 1 / 2: the approximate
    // quotients of levels 1 / 2, 3: the FP64 butterfly, 4: the lazy-sum inverse butterfly with the level-2 quotient,
    // 5: the inverse butterfly with the reference's sequence.
    namespace
    {
        template <int KIND>
        __global__ __launch_bounds__(512, 4) void butterfly_rate_kernel(u64 *__restrict__ sink, PrimeDev P, int iters)
        {
            u64 x[16], w[kIL], ws[kIL]; // (16 values: the sequence is what is measured, and nothing may spill)
            const u64 seed = (static_cast<u64>(blockIdx.x) * 512 + threadIdx.x) * 0x9E3779B97F4A7C15ull;
            constexpr bool FP = KIND == 3;
#pragma unroll
            for (int i = 0; i < 16; i++)
            {
                const u64 v = (seed + static_cast<u64>(i) * 0xBF58476D1CE4E5B9ull) % P.p;
                x[i] = FP ? fp_bits(fp_from_u64(v)) : v;
            }
#pragma unroll
            for (int j = 0; j < kIL; j++)
            {
                const u64 wv = (seed ^ (0x94D049BB133111EBull * (j + 1))) % P.p;
                w[j] = FP ? fp_bits(fp_from_u64(wv)) : wv;
                ws[j] = static_cast<u64>((static_cast<unsigned __int128>(wv) << 64) / P.p);
            }
            const u64 neg_p = FP ? fp_bits(P.pinv_d) : 0 - P.p, two_p = FP ? fp_bits(P.p_d) : P.two_p;
            ZeroPairs zp;
            zp.init();
            u64 four_p = two_p << 1; // (opaque like fwd_addend's: one v_lshl_add_u64 per second output)
            asm("" : "+s"(four_p));
            for (int it = 0; it < iters; it++)
            {
#pragma unroll
                for (int W = 3; W >= 0; W--)
                {
#pragma unroll
                    for (int c = 0; c < 8; c += kIL)
                    {
                        u64 u[kIL], y[kIL];
                        const int bit = 1 << W;
#pragma unroll
                        for (int j = 0; j < kIL; j++)
                        {
                            const int sl = (((c + j) >> W) << (W + 1)) | ((c + j) & (bit - 1));
                            u[j] = x[sl];
                            y[j] = x[sl | bit];
                        }
                        if constexpr (KIND == 3)
                        {
#pragma unroll
                            for (int j = 0; j < kIL; j++)
                                fp_butterfly_fwd(u[j], y[j], w[j], fp_of(two_p), fp_of(neg_p));
                        }
                        else if constexpr (KIND == 0)
                            butterflies_fwd_hs<false, kIL, 0>(u, y, w, ws, neg_p, two_p);
                        else if constexpr (KIND == 1)
                            butterflies_fwd_hs<false, kIL, 1>(u, y, w, ws, neg_p, two_p - neg_p);
                        else if constexpr (KIND == 2)
                            butterflies_fwd_apx2<false, kIL>(u, y, w, ws, neg_p, four_p, zp.z);
                        else if constexpr (KIND == 4)
                            butterflies_inv_apx2<false, kIL>(u, y, w, ws, neg_p, four_p, zp.z);
                        else
                            butterflies_inv_hs<false, kIL, 0>(u, y, w, ws, neg_p, two_p);
#pragma unroll
                        for (int j = 0; j < kIL; j++)
                        {
                            const int sl = (((c + j) >> W) << (W + 1)) | ((c + j) & (bit - 1));
                            x[sl] = u[j];
                            x[sl | bit] = y[j];
                        }
                    }
                }
                if constexpr (FP)
                    if ((it & 1) == 1) // (one reduction of every value per eight layers: a little more than the real schedule's)
                    {
#pragma unroll
                        for (int i = 0; i < 16; i++)
                            x[i] = fp_bits(fp_reduce(fp_of(x[i]), fp_of(two_p), fp_of(neg_p)));
                    }
            }
            u64 acc = 0;
#pragma unroll
            for (int i = 0; i < 16; i++)
                acc ^= x[i];
            if (acc == 0x0123456789ABCDEFull) // (never: keeps the arithmetic alive)
                sink[0] = acc;
        }
    } // namespace

    hipError_t ntt_butterfly_rate(const Engine &e, int kind, int prime_id, double *butterflies_per_s)
    {
        if (kind < 0 || kind > 5 || prime_id < 0 || prime_id >= static_cast<int>(e.tables.size()))
            return hipErrorInvalidValue;
        PrimeDev P{};
        hipError_t err = hipMemcpy(&P, e.d_primes + prime_id, sizeof(P), hipMemcpyDeviceToHost);
        if (err != hipSuccess)
            return err;
        if (kind == 3 && P.fwd_d == nullptr)
            return hipErrorInvalidValue; // no FP64 instance for this prime
        u64 *sink = nullptr;
        if ((err = hipMalloc(&sink, 8)) != hipSuccess)
            return err;
        hipStream_t st = e.lane().stream;
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        const unsigned blocks = 256u * 2u * 4u; // four rounds of resident workgroups per CU slot
        const int iters = 800;
        // the transforms' occupancy: their 68 KB of LDS admit two workgroups (four waves per SIMD) per CU; this kernel uses
        // none and fewer registers, so it asks for the same amount to run under the same cap
        const std::size_t lds = static_cast<std::size_t>(hpad(1 << 13)) * 8;
        const void *fns[6] = { reinterpret_cast<const void *>(&butterfly_rate_kernel<0>), reinterpret_cast<const void *>(&butterfly_rate_kernel<1>),
                               reinterpret_cast<const void *>(&butterfly_rate_kernel<2>), reinterpret_cast<const void *>(&butterfly_rate_kernel<3>),
                               reinterpret_cast<const void *>(&butterfly_rate_kernel<4>), reinterpret_cast<const void *>(&butterfly_rate_kernel<5>) };
        if ((err = hipFuncSetAttribute(fns[kind], hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds))) != hipSuccess)
        {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
            (void)hipFree(sink);
            return err;
        }
        const auto launch = [&](int n) {
            switch (kind)
            {
            case 0: butterfly_rate_kernel<0><<<blocks, 512, lds, st>>>(sink, P, n); break;
            case 1: butterfly_rate_kernel<1><<<blocks, 512, lds, st>>>(sink, P, n); break;
            case 2: butterfly_rate_kernel<2><<<blocks, 512, lds, st>>>(sink, P, n); break;
            case 3: butterfly_rate_kernel<3><<<blocks, 512, lds, st>>>(sink, P, n); break;
            case 4: butterfly_rate_kernel<4><<<blocks, 512, lds, st>>>(sink, P, n); break;
            default: butterfly_rate_kernel<5><<<blocks, 512, lds, st>>>(sink, P, n); break;
            }
        };
        launch(iters / 8); // warm-up (clocks, code)
        (void)hipEventRecord(a, st);
        launch(iters);
        launch(iters);
        (void)hipEventRecord(b, st);
        err = hipStreamSynchronize(st);
        float ms = 0;
        if (err == hipSuccess)
            err = hipEventElapsedTime(&ms, a, b);
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        (void)hipFree(sink);
        if (err != hipSuccess)
            return err;
        *butterflies_per_s = 2.0 * blocks * 512.0 * iters * 32.0 / (ms / 1e3);
        return hipGetLastError();
    }

    hipError_t ntt_init_kernels()
    {
        const int max_lds = ((1 << kTileBitsMax) + (1 << (kTileBitsMax - 4))) * 8;
        hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&ntt_pass_kernel<0>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
        if (err != hipSuccess)
            return err;
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&ntt_pass_kernel<1>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
        if (err == hipSuccess)
            err = ntt_fwd_half_init();
        if (err == hipSuccess)
            err = ntt_inv_half_init();
        return err;
    }

    bool ntt_can_defer_top(const Engine &e, int k)
    {
        return e.use_half_kernel && e.logn >= 14 && e.logn <= 16 && k <= 32;
    }

    bool ntt_can_fuse_moddown(const Engine &e, int k, u64 p_special)
    {
        // (the fused store is the floating-point instance's LDS trip, ntt_fwd.hip kStoreExchange: N = 2^15 and 2^16)
        if (!fp64_enabled() || !ntt_can_gather(e) || e.logn < 15 || p_special >= kFpPrimeBound)
            return false;
        for (int r = 0; r < k; r++)
            if (e.key_moduli[r] >= kFpPrimeBound)
                return false;
        return true;
    }

    // STRICT mode: may a producer apply the forward transform's top layer to rows on these primes (kNttTopDone)? Only the
    // dense lazy schedule has an instance that starts below it (ntt_select.hpp select_fwd_half)
    bool ntt_strict_top_done_ok(const Engine &e, const RowMap &map)
    {
        if (!e.use_half_kernel || e.logn < 14 || e.logn > 16 || exact_fwd())
            return false;
        for (int r = 0; r < map.rows; r++)
            if (map.prime[r] != kSkipRow && !bounds::fwd_dense_admits(e.tables[map.prime[r]].p, e.logn))
                return false;
        return true;
    }

    bool ntt_can_gather(const Engine &e)
    {
        return e.use_half_kernel && e.logn >= 14 && e.logn <= 16;
    }

    // May a key switch's digit launch (map, src, flags as launch_ntt_gather will get them) leave its last layer to an inner
    // product of nd digits (kNttSplitLast)? The launch must select an integer instance of that form and
    // every live prime must lie in bounds::fwd_split_admits with nd terms.
    bool ntt_can_split_last(const Engine &e, const RowMap &map, const NttSource &src, int flags, int nd)
    {
        if (!ntt_can_gather(e))
            return false;
        for (int r = 0; r < map.rows; r++)
            if (map.prime[r] != kSkipRow && !bounds::fwd_split_admits(e.tables[map.prime[r]].p, e.logn, nd))
                return false;
        return ntt_fwd_half_splits(e, map, flags | (e.mode_strict ? kNttStrict : 0), src);
    }

    hipError_t launch_ntt_gather(const Engine &e, u64 *data, size_t nrows, const RowMap &map, const NttSource &src,
                                 int flags)
    {
        if (!ntt_can_gather(e))
            return hipErrorInvalidValue;
        if (e.mode_strict)
            flags |= kNttStrict;
        if (nrows == 0)
            return hipSuccess;
        return ntt_fwd_half(e, data, nrows, map, flags, src);
    }

    // inverse NTT of rows read from another buffer (polynomial stride src_poly_stride words), written to data
    hipError_t launch_intt_from(const Engine &e, u64 *data, const u64 *src, std::size_t src_poly_stride, size_t nrows,
                                const RowMap &map, int flags)
    {
        if (!(e.use_half_kernel && e.logn >= 14 && e.logn <= 16))
            return hipErrorInvalidValue;
        if (nrows == 0)
            return hipSuccess;
        return ntt_inv_half(e, data, nrows, map, flags, src, src_poly_stride);
    }

    // inverse NTT of the ciphertext tensor product of two size-2 operands, formed on load from the forward-transformed
    // rows x (item-major: 4 polynomials of kb rows each, item_stride words apart); map has 3 * kb rows (output polynomial
    // I, row r at slot I * kb + r); the stored values carry the Montgomery factor 2^-64 (see ntt_inv.hip DyadicSrc)
    hipError_t launch_intt_tensor(const Engine &e, u64 *data, const u64 *x, std::size_t item_stride, std::size_t poly_stride,
                                  int kb, size_t nrows, const RowMap &map, int flags, bool square)
    {
        if (!(e.use_half_kernel && e.logn >= 14 && e.logn <= 16) || map.rows != 3 * kb)
            return hipErrorInvalidValue;
        if (nrows == 0)
            return hipSuccess;
        return ntt_inv_tensor(e, data, nrows, map, flags, x, item_stride, poly_stride, kb, square);
    }

    hipError_t launch_ntt(const Engine &e, u64 *data, size_t nrows, const RowMap &map, bool inverse, int flags)
    {
        if (nrows == 0)
            return hipSuccess; // the reference's loops over an empty range (every ring size: plan_ntt serves 2^13 and below only)
        if (e.mode_strict)
            flags |= kNttStrict;
        if (e.use_half_kernel && e.logn >= 14 && e.logn <= 16) // single-pass transforms for the large rings
            return inverse ? ntt_inv_half(e, data, nrows, map, flags) : ntt_fwd_half(e, data, nrows, map, flags, NttSource{});
        if (e.logn > kTileBitsMax)
            return hipErrorInvalidValue; // (no single-pass kernel for this ring: never plan_ntt's throw)
        const NttPlan plan = plan_ntt(e.logn, inverse, flags);
        return inverse ? launch_dir<1>(e, data, nrows, map, plan) : launch_dir<0>(e, data, nrows, map, plan);
    }
} // namespace sealhip
