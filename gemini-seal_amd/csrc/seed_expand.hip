// seed_expand.hip -- Ciphertext::expand_seed (ciphertext.cpp:126-133) on the device: the c_1 of a seeded ciphertext or
// key digit re-sampled from its 64-byte seed with BlakePRNG (randomgen.cpp:63-73) and sample_poly_uniform
// (util/rlwe.cpp:101-129), word for word what csrc/blake2xb.cpp computes on the host. DESIGN.md "Seed expansion" states the
// rule in its parallel form:
//   candidate m of a seed = the 64-bit little-endian word at byte 8m of its PRNG stream = output word m & 7 of leaf
//   (m >> 3) & 63 of buffer m >> 9, where buffer c = BLAKE2Xb(4096 bytes, in = c, key = seed) and leaf i = BLAKE2b(H0 of
//   the buffer; node offset i); r = (low32 << 31) | (high32 >> 1); row j takes its N accepted candidates (r < T_j) in
//   stream order, starting after row j-1's last one.
// Phase A generates a provisioned number of candidates per seed fully in parallel (one lane per key block, per buffer root,
// per leaf); phase B walks each seed's rows in one workgroup (flag, block scan, place) and generates in-kernel whatever it
// needs beyond the provision, so the result is exact for every seed, not only for those whose rejections fit the slack.
// The same PRNG also feeds the RLWE samplers (DESIGN.md "RLWE samples on the device from seeds"): phases A.0 and A.1, then
// sample_leaf_kernel maps every raw stream word to one ternary or noise sample (sample_map.hpp) -- fixed consumption, so
// there is no candidate arena and no phase B. The fixed-weight sampler takes the same leaves raw and
// ranks an item's N words against each other (fixed_weight_rank_kernel): the h smallest are the support.
#include "engine.hpp"
#include "sample_map.hpp"

#include <cmath>
#include <cstring>

namespace sealhip
{
    namespace
    {
        // ---------------------------------------------------------------- BLAKE2b (RFC 7693), device form
        constexpr u64 kB2IV[8] = { 0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL,
                                              0xa54ff53a5f1d36f1ULL, 0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL,
                                              0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL };

        // SIGMA (RFC 7693 section 2.7); rounds 10 and 11 repeat rounds 0 and 1. Only called with constant arguments after
        // the rounds are unrolled, so every message index is resolved at compile time.
        __host__ __device__ constexpr int b2_sigma(int r, int i)
        {
            constexpr unsigned char s[10][16] = {
                { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15 }, { 14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3 },
                { 11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4 }, { 7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8 },
                { 9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13 }, { 2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9 },
                { 12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11 }, { 13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10 },
                { 6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5 }, { 10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0 }
            };
            return s[r % 10][i];
        }

        // rotate right by a constant: 32 is a swap of the two halves, 24 / 16 / 63 are two v_alignbit_b32 each
        __host__ __device__ __forceinline__ u64 rotr64(u64 x, int r)
        {
            return (x >> r) | (x << (64 - r));
        }

        // One compression F(h, m, t, last). Every block this file compresses has message words 8..15 zero (the key block is
        // the 64-byte seed padded to 128 bytes, the counter block 8 bytes, a leaf block the 64-byte H0), so only m[0..7]
        // is passed and the zero words fold away.
        template <bool kLast>
        __host__ __device__ __forceinline__ void b2_compress(u64 (&h)[8], const u64 (&m)[8], u64 t0)
        {
            u64 v[16];
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
                v[i] = h[i];
                v[8 + i] = kB2IV[i];
            }
            v[12] ^= t0;
            if (kLast)
                v[14] = ~v[14];
#define SEALHIP_B2_MSG(x) ((x) < 8 ? m[(x) & 7] : u64(0))
#define SEALHIP_B2_G(r, i, a, b, c, d)                                    \
    do                                                                  \
    {                                                                   \
        v[a] = v[a] + v[b] + SEALHIP_B2_MSG(b2_sigma(r, 2 * (i)));       \
        v[d] = rotr64(v[d] ^ v[a], 32);                                 \
        v[c] = v[c] + v[d];                                             \
        v[b] = rotr64(v[b] ^ v[c], 24);                                 \
        v[a] = v[a] + v[b] + SEALHIP_B2_MSG(b2_sigma(r, 2 * (i) + 1));   \
        v[d] = rotr64(v[d] ^ v[a], 16);                                 \
        v[c] = v[c] + v[d];                                             \
        v[b] = rotr64(v[b] ^ v[c], 63);                                 \
    } while (0)
#pragma unroll
            for (int r = 0; r < 12; r++)
            {
                SEALHIP_B2_G(r, 0, 0, 4, 8, 12);
                SEALHIP_B2_G(r, 1, 1, 5, 9, 13);
                SEALHIP_B2_G(r, 2, 2, 6, 10, 14);
                SEALHIP_B2_G(r, 3, 3, 7, 11, 15);
                SEALHIP_B2_G(r, 4, 0, 5, 10, 15);
                SEALHIP_B2_G(r, 5, 1, 6, 11, 12);
                SEALHIP_B2_G(r, 6, 2, 7, 8, 13);
                SEALHIP_B2_G(r, 7, 3, 4, 9, 14);
            }
#undef SEALHIP_B2_G
#undef SEALHIP_B2_MSG
#pragma unroll
            for (int i = 0; i < 8; i++)
                h[i] ^= v[i] ^ v[8 + i];
        }

        constexpr u64 kBufBytes = 4096; // BlakePRNG buffer (randomgen.h:199-222): the BLAKE2Xb output length
        // parameter blocks (BLAKE2 specification 2.5 / BLAKE2X 2), the words that differ from zero:
        // root: digest 64, key 64, fanout 1, depth 1 (word 0); XOF length 4096 (word 1, high half)
        constexpr u64 kRootP0 = 64 | (64 << 8) | (1 << 16) | (1 << 24), kRootP1 = kBufBytes << 32;
        // leaf i: digest 64, fanout 0, depth 0, leaf length 64 (word 0); node offset i, XOF length (word 1); inner length 64
        // (word 2, byte 1)
        constexpr u64 kLeafP0 = 64 | (u64(64) << 32), kLeafP1 = kBufBytes << 32, kLeafP2 = u64(64) << 8;

        // the root state after the key block (t = 128, not last): depends on the seed only
        __host__ __device__ __forceinline__ void key_state(const u64 *seed, u64 (&h)[8])
        {
            u64 m[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
            {
                m[i] = seed[i];
                h[i] = kB2IV[i];
            }
            h[0] ^= kRootP0;
            h[1] ^= kRootP1;
            b2_compress<false>(h, m, 128);
        }

        // H0 of buffer `counter`: the counter block (8 bytes, t = 136, last) on the key state
        __host__ __device__ __forceinline__ void buffer_root(const u64 (&ks)[8], u64 counter, u64 (&h)[8])
        {
            u64 m[8] = { counter, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
            for (int i = 0; i < 8; i++)
                h[i] = ks[i];
            b2_compress<true>(h, m, 136);
        }

        // leaf `leaf` of a buffer (64 bytes, t = 64, last): its 8 output words, the stream words 8 leaf .. 8 leaf + 7 of the
        // buffer
        __host__ __device__ __forceinline__ void leaf_words(const u64 (&h0)[8], unsigned leaf, u64 (&r)[8])
        {
#pragma unroll
            for (int i = 0; i < 8; i++)
                r[i] = kB2IV[i];
            r[0] ^= kLeafP0;
            r[1] ^= kLeafP1 | leaf;
            r[2] ^= kLeafP2;
            b2_compress<true>(r, h0, 64);
        }

        // the same leaf's 8 words as sample_poly_uniform's candidates r
        __host__ __device__ __forceinline__ void leaf_candidates(const u64 (&h0)[8], unsigned leaf, u64 (&r)[8])
        {
            leaf_words(h0, leaf, r);
            // generate() hands out low32(w) first (hi), then high32(w) (lo), and r = (hi << 31) | (lo >> 1) (util/rlwe.cpp:124):
            // the word rotated left by 31 with bit 63 (bit 32 of w) cleared
#pragma unroll
            for (int i = 0; i < 8; i++)
                r[i] = ((r[i] << 31) | (r[i] >> 33)) & 0x7FFFFFFFFFFFFFFFULL;
        }

        constexpr int kGenThreads = 256;

        // phase A.0: the key state of every seed of the chunk (one lane per seed). rec = 9 words per item: seed, dst
        __global__ __launch_bounds__(kGenThreads) void seed_key_state_kernel(const u64 *__restrict__ rec, u64 *__restrict__ ks,
                                                                            unsigned count)
        {
            const unsigned s = blockIdx.x * kGenThreads + threadIdx.x;
            if (s >= count)
                return;
            u64 h[8];
            key_state(rec + static_cast<std::size_t>(s) * 9, h);
#pragma unroll
            for (int i = 0; i < 8; i++)
                ks[static_cast<std::size_t>(s) * 8 + i] = h[i];
        }

        // phase A.1: H0 of every provisioned buffer (one lane per (seed, buffer))
        __global__ __launch_bounds__(kGenThreads) void seed_buffer_root_kernel(const u64 *__restrict__ ks, u64 *__restrict__ h0,
                                                                              unsigned nbuf, unsigned total)
        {
            const unsigned bi = blockIdx.x * kGenThreads + threadIdx.x;
            if (bi >= total)
                return;
            const unsigned s = bi / nbuf, b = bi - s * nbuf;
            u64 k[8], h[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                k[i] = ks[static_cast<std::size_t>(s) * 8 + i];
            buffer_root(k, b, h);
#pragma unroll
            for (int i = 0; i < 8; i++)
                h0[static_cast<std::size_t>(bi) * 8 + i] = h[i];
        }

        // phase A.2: every leaf (one lane per leaf; a wave is one buffer, so H0 is a scalar load). Lane g writes candidates
        // 8g .. 8g+7 of the chunk, which is seed g / (P/8), candidate 8 (g mod P/8) of that seed.
        __global__ __launch_bounds__(kGenThreads) void seed_leaf_kernel(const u64 *__restrict__ h0, u64 *__restrict__ cand,
                                                                       std::size_t total_leaves)
        {
            const std::size_t g = static_cast<std::size_t>(blockIdx.x) * kGenThreads + threadIdx.x;
            if (g >= total_leaves) // (total_leaves is a multiple of 64: whole waves only)
                return;
            const unsigned bi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(g >> 6));
            u64 h[8], r[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                h[i] = h0[static_cast<std::size_t>(bi) * 8 + i];
            leaf_candidates(h, static_cast<unsigned>(g & 63), r);
            ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(cand + g * 8);
#pragma unroll
            for (int i = 0; i < 4; i++)
                dst[i] = make_ulonglong2(r[2 * i], r[2 * i + 1]);
        }

        // ---------------------------------------------------------------- phase B: place
        constexpr int kPlaceThreads = 1024;
        constexpr int kPlaceWaves = kPlaceThreads / 64;
        constexpr unsigned kTile = kPlaceThreads * 8; // candidates per step; a lane owns one leaf (8 aligned candidates)

        struct PlaceArgs
        {
            int rows, logn;
            u64 provisioned; // candidates per seed in the arena (a multiple of 512: whole buffers)
            u64 q[kMaxModuli], cr1[kMaxModuli], T[kMaxModuli];
        };

        // One workgroup per seed. Row j: the tile of 8192 candidates from the row's first one (rounded down to a leaf) is
        // flagged against T_j, block-scanned, and the accepted ones below rank N go to their place; the lane that holds
        // the N-th accepted one tells where the next row starts. Candidates at or past `provisioned` are generated here with
        // the same BLAKE2b code (the continuation).
        __global__ __launch_bounds__(kPlaceThreads) void seed_place_kernel(const u64 *__restrict__ rec, const u64 *__restrict__ ks,
                                                                          const u64 *__restrict__ cand, const PlaceArgs a)
        {
            __shared__ unsigned s_wave[kPlaceWaves];
            __shared__ u64 s_next;
            const unsigned s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
            const std::size_t N = std::size_t(1) << a.logn;
            const u64 *seed_cand = cand + static_cast<std::size_t>(s) * a.provisioned;
            u64 *dst = reinterpret_cast<u64 *>(rec[static_cast<std::size_t>(s) * 9 + 8]);
            u64 pos = 0; // first candidate of the current row
            for (int j = 0; j < a.rows; j++)
            {
                const u64 q = a.q[j], cr1 = a.cr1[j], T = a.T[j];
                u64 *out = dst + static_cast<std::size_t>(j) * N;
                std::size_t produced = 0;
                for (;;)
                {
                    const u64 idx0 = (pos & ~u64(7)) + static_cast<u64>(tid) * 8;
                    u64 r[8];
                    if (idx0 < a.provisioned)
                    {
                        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(seed_cand + idx0);
#pragma unroll
                        for (int i = 0; i < 4; i++)
                        {
                            const ulonglong2 w = src[i];
                            r[2 * i] = w.x;
                            r[2 * i + 1] = w.y;
                        }
                    }
                    else // the continuation: this lane's leaf was not provisioned
                    {
                        u64 k[8], h0[8];
#pragma unroll
                        for (int i = 0; i < 8; i++)
                            k[i] = ks[static_cast<std::size_t>(s) * 8 + i];
                        buffer_root(k, idx0 >> 9, h0);
                        leaf_candidates(h0, static_cast<unsigned>((idx0 >> 3) & 63), r);
                    }
                    unsigned flags = 0;
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        flags |= (idx0 + i >= pos && r[i] < T) ? (1u << i) : 0u;
                    const unsigned cnt = __popc(flags);
                    // block exclusive scan of cnt
                    unsigned incl = cnt;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1)
                    {
                        const unsigned v = __shfl_up(incl, d, 64);
                        if (lane >= static_cast<unsigned>(d))
                            incl += v;
                    }
                    if (lane == 63)
                        s_wave[wid] = incl;
                    __syncthreads();
                    unsigned before = 0, total = 0;
#pragma unroll
                    for (int w = 0; w < kPlaceWaves; w++)
                    {
                        const unsigned t = s_wave[w];
                        before += w < static_cast<int>(wid) ? t : 0u;
                        total += t;
                    }
                    std::size_t rank = produced + before + incl - cnt;
#pragma unroll
                    for (int i = 0; i < 8; i++)
                    {
                        if ((flags >> i) & 1u)
                        {
                            if (rank < N)
                                out[rank] = barrett_reduce_63(r[i], q, cr1);
                            if (rank == N - 1)
                                s_next = idx0 + i + 1;
                            rank++;
                        }
                    }
                    produced += total;
                    __syncthreads(); // s_wave is rewritten by the next step; s_next is visible
                    if (produced >= N)
                    {
                        pos = s_next;
                        break;
                    }
                    pos = (pos & ~u64(7)) + kTile;
                }
                __syncthreads(); // every lane has read s_next before a later row writes it
            }
        }

        // ---------------------------------------------------------------- RLWE samples
        // An item's stream words [pN, (p+1)N) become polynomial p: ternary for p < n_ternary, noise after. `leaves` =
        // (n_ternary + n_noise) N / 8 leaves in `nbuf` buffers per item, the last one partial when N < 512.
        struct SampleArgs
        {
            unsigned logn, n_ternary, leaves, nbuf;
            // item s: its ternary polynomials at out + s * stride, its noise polynomials at out_noise + s * stride_noise
            // (16-byte aligned, strides multiples of 4); one array out[i][p][N] has out_noise = out + n_ternary N
            std::int32_t *out, *out_noise;
            std::size_t stride, stride_noise;
            u64 *raw; // the raw variant: item s's stream words themselves at raw + s N (16-byte aligned)
        };

        // One lane per leaf, one wave per buffer (so H0 is a scalar load): the leaf's 8 words mapped by the kind of its
        // polynomial (N >= 8: a leaf lies in one polynomial) and written with two 16-byte stores. Lanes past the item's
        // last leaf write nothing. kRaw: the words themselves, unmapped, with four 16-byte stores (the fixed-weight sampler
        // ranks them).
        template <bool kRaw>
        __global__ __launch_bounds__(kGenThreads) void sample_leaf_kernel(const u64 *__restrict__ h0, const SampleArgs a,
                                                                         unsigned total_bufs)
        {
            const std::size_t g = static_cast<std::size_t>(blockIdx.x) * kGenThreads + threadIdx.x;
            const unsigned bi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(g >> 6));
            if (bi >= total_bufs)
                return;
            const unsigned s = bi / a.nbuf, lane = static_cast<unsigned>(g & 63), leaf = (bi - s * a.nbuf) * 64 + lane;
            if (leaf >= a.leaves)
                return;
            u64 h[8], w[8];
#pragma unroll
            for (int i = 0; i < 8; i++)
                h[i] = h0[static_cast<std::size_t>(bi) * 8 + i];
            leaf_words(h, lane, w);
            if (kRaw)
            {
                ulonglong2 *raw = reinterpret_cast<ulonglong2 *>(a.raw + (static_cast<std::size_t>(s) << a.logn) +
                                                                 static_cast<std::size_t>(leaf) * 8);
#pragma unroll
                for (int i = 0; i < 4; i++)
                    raw[i] = make_ulonglong2(w[2 * i], w[2 * i + 1]);
                return;
            }
            std::int32_t v[8];
            int4 *dst;
            const unsigned ternary_leaves = a.n_ternary << (a.logn - 3);
            if (leaf >= ternary_leaves) // the kind is public: only the words are secret
            {
#pragma unroll
                for (int i = 0; i < 8; i++)
                    v[i] = sample_noise(w[i]);
                dst = reinterpret_cast<int4 *>(a.out_noise + static_cast<std::size_t>(s) * a.stride_noise +
                                               static_cast<std::size_t>(leaf - ternary_leaves) * 8);
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 8; i++)
                    v[i] = sample_ternary(w[i]);
                dst = reinterpret_cast<int4 *>(a.out + static_cast<std::size_t>(s) * a.stride + static_cast<std::size_t>(leaf) * 8);
            }
            dst[0] = make_int4(v[0], v[1], v[2], v[3]);
            dst[1] = make_int4(v[4], v[5], v[6], v[7]);
        }

        // the kernel's own map functions on caller-supplied words (sealhip_debug_sample_map)
        __global__ __launch_bounds__(kGenThreads) void sample_map_kernel(const u64 *__restrict__ words, std::size_t n, bool noise,
                                                                        std::int32_t *__restrict__ out)
        {
            const std::size_t i = static_cast<std::size_t>(blockIdx.x) * kGenThreads + threadIdx.x;
            if (i < n)
                out[i] = noise ? sample_noise(words[i]) : sample_ternary(words[i]);
        }

        // ---------------------------------------------------------------- fixed-weight polynomials
        // rank_i = #{ j : w_j < w_i, or w_j == w_i and j < i } over a polynomial's N words; coefficient i is 0 when
        // rank_i >= h, else -1 when w_i & 1, else +1. A workgroup owns kRankTile consecutive words, a lane kRankOwn
        // consecutive ones in registers, and walks all N words tile by tile through LDS: every lane reads the same LDS
        // address per step (a broadcast: no bank conflict), and one read feeds kRankOwn 64-bit compares. Constant time in
        // sample_map.hpp's sense: every loop bound, branch, address and LDS index is a function of N, h and the lane's
        // position; a word only ever enters compares whose results are added, and the select at the end is a mask.
        constexpr int kRankThreads = 256, kRankOwn = 4;
        constexpr unsigned kRankTile = kRankThreads * kRankOwn; // words per workgroup = words per LDS tile (8 KiB)

        // kTie: 0 the tile lies before the workgroup's own words (every j < i: count w_j <= w_i), 1 it is the own tile
        // (the full rule), 2 it lies after (every j > i: count w_j < w_i). The tile's position is public.
        template <int kTie>
        __device__ __forceinline__ void rank_tile(const u64 *tile, unsigned len, unsigned j0, unsigned i0, const u64 (&w)[kRankOwn],
                                                  unsigned (&rank)[kRankOwn])
        {
#pragma unroll 8
            for (unsigned jj = 0; jj < len; jj++) // len is a multiple of 8
            {
                const u64 x = tile[jj];
#pragma unroll
                for (int r = 0; r < kRankOwn; r++)
                {
                    if (kTie == 0)
                        rank[r] += static_cast<unsigned>(x <= w[r]);
                    else if (kTie == 2)
                        rank[r] += static_cast<unsigned>(x < w[r]);
                    else
                        rank[r] += static_cast<unsigned>(x < w[r]) |
                                   (static_cast<unsigned>(x == w[r]) & static_cast<unsigned>(j0 + jj < i0 + r));
                }
            }
        }

        // grid (ceil(N / kRankTile), polynomials); words[p][N] -> out + p * stride, N int32 each (16-byte stores). N is a
        // power of two >= 8, so a lane's kRankOwn words lie inside the polynomial or all outside it; lanes outside still
        // stage and synchronise, with zeros for own words, and store nothing.
        __global__ __launch_bounds__(kRankThreads) void fixed_weight_rank_kernel(const u64 *__restrict__ words, unsigned logn,
                                                                                unsigned h, std::int32_t *__restrict__ out,
                                                                                std::size_t stride)
        {
            __shared__ __attribute__((aligned(16))) u64 s_tile[kRankTile];
            const unsigned N = 1u << logn, tid = threadIdx.x, n_tiles = (N + kRankTile - 1) / kRankTile;
            const u64 *poly = words + (static_cast<std::size_t>(blockIdx.y) << logn);
            const unsigned i0 = blockIdx.x * kRankTile + tid * kRankOwn;
            const bool mine = i0 < N;
            u64 w[kRankOwn] = {};
            unsigned rank[kRankOwn] = {};
            if (mine)
            {
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(poly + i0),
                                 b = *reinterpret_cast<const ulonglong2 *>(poly + i0 + 2);
                w[0] = a.x, w[1] = a.y, w[2] = b.x, w[3] = b.y;
            }
            for (unsigned t = 0; t < n_tiles; t++)
            {
                const unsigned j0 = t * kRankTile, len = N - j0 < kRankTile ? N - j0 : kRankTile, mj = tid * kRankOwn;
                if (mj < len)
                {
                    *reinterpret_cast<ulonglong2 *>(s_tile + mj) = *reinterpret_cast<const ulonglong2 *>(poly + j0 + mj);
                    *reinterpret_cast<ulonglong2 *>(s_tile + mj + 2) = *reinterpret_cast<const ulonglong2 *>(poly + j0 + mj + 2);
                }
                __syncthreads();
                if (t < blockIdx.x)
                    rank_tile<0>(s_tile, len, j0, i0, w, rank);
                else if (t == blockIdx.x)
                    rank_tile<1>(s_tile, len, j0, i0, w, rank);
                else
                    rank_tile<2>(s_tile, len, j0, i0, w, rank);
                __syncthreads(); // the next tile overwrites s_tile
            }
            if (mine)
            {
                std::int32_t v[kRankOwn];
#pragma unroll
                for (int r = 0; r < kRankOwn; r++) // +1 or -1 by bit 0, masked to 0 outside the support
                    v[r] = (1 - 2 * static_cast<std::int32_t>(w[r] & 1)) & -static_cast<std::int32_t>(rank[r] < h);
                *reinterpret_cast<int4 *>(out + static_cast<std::size_t>(blockIdx.y) * stride + i0) = make_int4(v[0], v[1], v[2], v[3]);
            }
        }
        static_assert(kRankOwn == 4, "a lane loads its words as two 16-byte pairs and stores one int4");

        // KeyGenerator::generate_sk's lift (keygenerator.cpp:78-84): row j of the key is the ternary polynomial mod q_j
        struct LiftArgs
        {
            int rows, logn;
            u64 q[kMaxModuli];
        };
        __global__ __launch_bounds__(kGenThreads) void ternary_lift_kernel(const std::int32_t *__restrict__ t, u64 *__restrict__ out,
                                                                          const LiftArgs a)
        {
            const std::size_t i = static_cast<std::size_t>(blockIdx.x) * kGenThreads + threadIdx.x;
            if (i >= (static_cast<std::size_t>(a.rows) << a.logn))
                return;
            const std::int32_t v = t[i & ((std::size_t(1) << a.logn) - 1)];
            const u64 q = a.q[i >> a.logn];
            out[i] = v < 0 ? q - static_cast<u64>(-v) : static_cast<u64>(v);
        }

        // candidates a seed needs, as a function of the rows' rejection rates: row j rejects a fraction
        // f_j = (((2^63 - 1) mod q_j) + 2) / 2^63; its rejections before N acceptances are negative-binomial with mean
        // N f/(1-f) and variance N f/(1-f)^2. Slack = mean + 8 standard deviations + 64.
        u64 default_slack(const Engine &e, int rows)
        {
            double mean = 0, var = 0;
            for (int j = 0; j < rows; j++)
            {
                const u64 q = e.key_moduli[j];
                const double f = static_cast<double>((0x7FFFFFFFFFFFFFFFULL % q) + 2) / 9223372036854775808.0;
                mean += static_cast<double>(e.n) * f / (1 - f);
                var += static_cast<double>(e.n) * f / ((1 - f) * (1 - f));
            }
            return static_cast<u64>(std::ceil(mean + 8 * std::sqrt(var))) + 64;
        }
        // The lane's pinned staging for `count` records of 9 words (seed, destination), once its previous copy has left
        // it. The caller fills l.seed_pin, enqueues its copies and records l.seed_pin_done after the last one.
        void stage_records(Lane &l, std::size_t count)
        {
            const std::size_t rec_words = count * 9;
            if (l.seed_pin_done)
                SEALHIP_CHECK(hipEventSynchronize(l.seed_pin_done));
            else
                SEALHIP_CHECK(hipEventCreateWithFlags(&l.seed_pin_done, hipEventDisableTiming));
            if (rec_words > l.seed_pin_words)
            {
                if (l.seed_pin)
                    SEALHIP_CHECK(hipHostFree(l.seed_pin));
                l.seed_pin = nullptr;
                l.seed_pin_words = 0;
                SEALHIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&l.seed_pin), rec_words * 8, hipHostMallocDefault));
                l.seed_pin_words = rec_words;
            }
        }

        // phases A.0 and A.1 for the m staged records from `off`: records to the device, key states, buffer roots
        void roots_of_chunk(Engine &e, std::size_t off, std::size_t m, std::size_t nbuf, u64 *rec, u64 *ks, u64 *h0)
        {
            Lane &l = e.lane();
            SEALHIP_CHECK(hipMemcpyAsync(rec, l.seed_pin + off * 9, m * 9 * 8, hipMemcpyHostToDevice, l.stream));
            {
                ProfScope prof(e, "seed_key_state", static_cast<double>(m));
                seed_key_state_kernel<<<static_cast<unsigned>((m + kGenThreads - 1) / kGenThreads), kGenThreads, 0, l.stream>>>(
                    rec, ks, static_cast<unsigned>(m));
                check(hipGetLastError(), "seed_key_state");
            }
            const std::size_t nroots = m * nbuf;
            {
                ProfScope prof(e, "seed_buffer_root", static_cast<double>(nroots));
                seed_buffer_root_kernel<<<static_cast<unsigned>((nroots + kGenThreads - 1) / kGenThreads), kGenThreads, 0,
                                          l.stream>>>(ks, h0, static_cast<unsigned>(nbuf), static_cast<unsigned>(nroots));
                check(hipGetLastError(), "seed_buffer_root");
            }
        }

        // The sampling steps of one chunk inside a for_chunks body: roots of the m staged seeds from `off`, then every leaf
        // an item needs, mapped. The roots are erased afterwards: a noise seed's roots give its whole stream.
        void sample_chunk(Engine &e, std::size_t off, std::size_t m, SampleArgs a)
        {
            Lane &l = e.lane();
            const std::size_t nroots = m * a.nbuf;
            u64 *h0 = e.ws_alloc(nroots * 8);
            u64 *ks = e.ws_alloc(m * 8);
            u64 *rec = e.ws_alloc(m * 9);
            roots_of_chunk(e, off, m, a.nbuf, rec, ks, h0);
            {
                ProfScope prof(e, "sample_leaf", static_cast<double>(m) * a.leaves);
                const unsigned grid = static_cast<unsigned>((nroots * 64 + kGenThreads - 1) / kGenThreads);
                if (a.raw)
                    sample_leaf_kernel<true><<<grid, kGenThreads, 0, l.stream>>>(h0, a, static_cast<unsigned>(nroots));
                else
                    sample_leaf_kernel<false><<<grid, kGenThreads, 0, l.stream>>>(h0, a, static_cast<unsigned>(nroots));
                check(hipGetLastError(), "sample_leaf");
            }
            SEALHIP_CHECK(hipMemsetAsync(h0, 0, nroots * 64, l.stream));
            SEALHIP_CHECK(hipMemsetAsync(ks, 0, m * 64, l.stream));
            SEALHIP_CHECK(hipMemsetAsync(rec, 0, m * 72, l.stream));
        }
        // bytes of sample_chunk's three temporaries per item
        std::size_t sample_item_bytes(const SampleArgs &a)
        {
            return (static_cast<std::size_t>(a.nbuf) * 8 + 8 + 9) * 8;
        }

        hipError_t launch_fixed_weight_rank(const Engine &e, const u64 *words, std::size_t n_polys, unsigned h, std::int32_t *out,
                                            std::size_t stride)
        {
            // N^2 compares per polynomial
            ProfScope prof(e, "fixed_weight_rank", static_cast<double>(n_polys) * static_cast<double>(e.n) * static_cast<double>(e.n));
            constexpr std::size_t max_polys = 65535; // grid.y
            for (std::size_t p = 0; p < n_polys; p += max_polys)
            {
                const dim3 grid(static_cast<unsigned>((e.n + kRankTile - 1) / kRankTile),
                                static_cast<unsigned>(std::min(max_polys, n_polys - p)));
                fixed_weight_rank_kernel<<<grid, kRankThreads, 0, e.lane().stream>>>(words + p * e.n, static_cast<unsigned>(e.logn),
                                                                                    h, out + p * stride, stride);
            }
            return hipGetLastError();
        }

        // One chunk of fixed-weight polynomials inside a for_chunks body: the m staged seeds' first N stream words raw into
        // arena scratch (sample_chunk's steps with the raw leaf kernel), ranked into out + i * stride; the scratch is erased
        // like the roots. `a` = sample_args(e, 1, 0): the words ternary polynomial 0 would consume.
        void fixed_weight_chunk(Engine &e, std::size_t off, std::size_t m, SampleArgs a, unsigned h, std::int32_t *out,
                                std::size_t stride)
        {
            u64 *words = e.ws_alloc(m * e.n);
            a.raw = words;
            sample_chunk(e, off, m, a);
            check(launch_fixed_weight_rank(e, words, m, h, out, stride), "fixed_weight_rank");
            SEALHIP_CHECK(hipMemsetAsync(words, 0, m * e.n * sizeof(u64), e.lane().stream));
        }
        std::size_t fixed_weight_item_bytes(const Engine &e, const SampleArgs &a)
        {
            return sample_item_bytes(a) + e.n * sizeof(u64);
        }

        SampleArgs sample_args(const Engine &e, unsigned n_ternary, unsigned n_noise)
        {
            if (n_ternary + n_noise == 0 || n_ternary + n_noise > kSampleMaxPolys)
                throw std::invalid_argument("n_ternary + n_noise must be 1 .. 16");
            SampleArgs a{};
            a.logn = static_cast<unsigned>(e.logn);
            a.n_ternary = n_ternary;
            a.leaves = static_cast<unsigned>((static_cast<std::size_t>(n_ternary + n_noise) * e.n) >> 3);
            a.nbuf = (a.leaves + 63) / 64;
            return a;
        }

        // seeds (count x 8 words, host) into the staging; the caller has checked that the lane is not capturing
        void stage_seeds(Lane &l, const std::uint64_t *seeds_host, std::size_t count)
        {
            stage_records(l, count);
            for (std::size_t i = 0; i < count; i++)
            {
                std::memcpy(l.seed_pin + i * 9, seeds_host + i * 8, 64);
                l.seed_pin[i * 9 + 8] = 0;
            }
        }
    } // namespace

    void op_expand_seeds(Engine &e, int rows, const SeedJob *jobs, std::size_t count)
    {
        if (rows < 1 || rows > e.n_key)
            throw std::invalid_argument("level k out of range");
        if (count == 0)
            return;
        Lane &l = e.lane();
        if (l.capturing)
            throw std::logic_error("seed expansion stages its seeds on the host: it cannot be captured in a graph");
        const std::size_t N = e.n;
        const u64 slack = l.seed_slack >= 0 ? static_cast<u64>(l.seed_slack) : default_slack(e, rows);
        const u64 P = (static_cast<u64>(rows) * N + slack + 511) & ~u64(511); // whole PRNG buffers
        const u64 nbuf = P / 512;
        if (nbuf > 0xFFFFFFFFull / 64)
            throw std::invalid_argument("seed expansion: too many candidates per seed");

        PlaceArgs pa{};
        pa.rows = rows;
        pa.logn = e.logn;
        pa.provisioned = P;
        for (int j = 0; j < rows; j++)
        {
            const u64 q = e.key_moduli[j];
            constexpr u64 max_random = 0x7FFFFFFFFFFFFFFFULL; // util/rlwe.cpp:113-117
            pa.q[j] = q;
            pa.T[j] = max_random - (max_random % q) - 1;
            pa.cr1[j] = static_cast<u64>((static_cast<unsigned __int128>(1) << 64) / q); // floor(2^64 / q): barrett_reduce_63
        }

        stage_records(l, count);
        for (std::size_t i = 0; i < count; i++)
        {
            std::memcpy(l.seed_pin + i * 9, jobs[i].seed, 64);
            l.seed_pin[i * 9 + 8] = static_cast<std::uint64_t>(reinterpret_cast<std::uintptr_t>(jobs[i].dst));
        }

        // per item: candidates, buffer roots, key state, record (the padding of each array is in n_buffers)
        const std::size_t per_item = (P + nbuf * 8 + 8 + 9) * 8;
        for_chunks(e, count, per_item, 4, [&](std::size_t off, std::size_t m) {
            u64 *cand = e.ws_alloc(m * P);
            u64 *h0 = e.ws_alloc(m * nbuf * 8);
            u64 *ks = e.ws_alloc(m * 8);
            u64 *rec = e.ws_alloc(m * 9);
            roots_of_chunk(e, off, m, nbuf, rec, ks, h0);
            const std::size_t nroots = m * nbuf;
            const std::size_t leaves = nroots * 64;
            {
                ProfScope prof(e, "seed_leaf", static_cast<double>(leaves));
                seed_leaf_kernel<<<static_cast<unsigned>((leaves + kGenThreads - 1) / kGenThreads), kGenThreads, 0, l.stream>>>(
                    h0, cand, leaves);
                check(hipGetLastError(), "seed_leaf");
            }
            {
                ProfScope prof(e, "seed_place", static_cast<double>(m));
                seed_place_kernel<<<static_cast<unsigned>(m), kPlaceThreads, 0, l.stream>>>(rec, ks, cand, pa);
                check(hipGetLastError(), "seed_place");
            }
        });
        // every record copy has been enqueued before this: once the event completes, the staging may be rewritten
        SEALHIP_CHECK(hipEventRecord(l.seed_pin_done, l.stream));
    }
    void op_sample_polys(Engine &e, const std::uint64_t *seeds_host, std::size_t count, unsigned n_ternary, unsigned n_noise,
                         std::int32_t *out, std::size_t item_stride, std::int32_t *out_noise, std::size_t noise_stride)
    {
        SampleArgs a = sample_args(e, n_ternary, n_noise);
        if (count == 0)
            return;
        if (count > 0xFFFFFFFFull / 64 / a.nbuf)
            throw std::invalid_argument("sampling: too many leaves in one call");
        Lane &l = e.lane();
        if (l.capturing)
            throw std::logic_error("sampling stages its seeds on the host: it cannot be captured in a graph");
        stage_seeds(l, seeds_host, count);
        for_chunks(e, count, sample_item_bytes(a), 3, [&](std::size_t off, std::size_t m) {
            a.out = out + off * item_stride;
            a.stride = item_stride;
            a.out_noise = out_noise + off * noise_stride;
            a.stride_noise = noise_stride;
            sample_chunk(e, off, m, a);
        });
        SEALHIP_CHECK(hipEventRecord(l.seed_pin_done, l.stream));
    }

    void op_debug_sample_map(Engine &e, const u64 *words, std::size_t n, bool noise, std::int32_t *out)
    {
        if (n == 0)
            return;
        sample_map_kernel<<<static_cast<unsigned>((n + kGenThreads - 1) / kGenThreads), kGenThreads, 0, e.lane().stream>>>(
            words, n, noise, out);
        check(hipGetLastError(), "sample_map");
    }

    void op_sample_fixed_weight(Engine &e, const std::uint64_t *seeds_host, std::size_t count, unsigned h, std::int32_t *out,
                                std::size_t item_stride)
    {
        const SampleArgs a = sample_args(e, 1, 0);
        if (count == 0)
            return;
        if (count > 0xFFFFFFFFull / 64 / a.nbuf)
            throw std::invalid_argument("sampling: too many leaves in one call");
        Lane &l = e.lane();
        if (l.capturing)
            throw std::logic_error("sampling stages its seeds on the host: it cannot be captured in a graph");
        stage_seeds(l, seeds_host, count);
        for_chunks(e, count, fixed_weight_item_bytes(e, a), 4, [&](std::size_t off, std::size_t m) {
            fixed_weight_chunk(e, off, m, a, h, out + off * item_stride, item_stride);
        });
        SEALHIP_CHECK(hipEventRecord(l.seed_pin_done, l.stream));
    }

    void op_debug_fixed_weight_map(Engine &e, const u64 *words, std::size_t n_polys, unsigned h, std::int32_t *out)
    {
        if (n_polys == 0)
            return;
        check(launch_fixed_weight_rank(e, words, n_polys, h, out, e.n), "fixed_weight_rank");
    }

    void op_generate_secret_key(Engine &e, const std::uint64_t *seed_host, unsigned h, u64 *sk_ntt)
    {
        SampleArgs a = sample_args(e, 1, 0);
        Lane &l = e.lane();
        if (l.capturing)
            throw std::logic_error("sampling stages its seeds on the host: it cannot be captured in a graph");
        LiftArgs la{};
        la.rows = e.n_key;
        la.logn = e.logn;
        for (int j = 0; j < e.n_key; j++)
            la.q[j] = e.key_moduli[j];
        stage_seeds(l, seed_host, 1);
        const std::size_t t_words = (e.n + 1) / 2, total = static_cast<std::size_t>(e.n_key) * e.n;
        for_chunks(e, 1, (h ? fixed_weight_item_bytes(e, a) : sample_item_bytes(a)) + t_words * 8, h ? 5 : 4,
                   [&](std::size_t off, std::size_t m) {
            std::int32_t *t = reinterpret_cast<std::int32_t *>(e.ws_alloc(t_words));
            a.out = a.out_noise = t;
            a.stride = a.stride_noise = 0;
            if (h)
                fixed_weight_chunk(e, off, m, a, h, t, 0);
            else
                sample_chunk(e, off, m, a);
            ternary_lift_kernel<<<static_cast<unsigned>((total + kGenThreads - 1) / kGenThreads), kGenThreads, 0, l.stream>>>(
                t, sk_ntt, la);
            check(hipGetLastError(), "ternary_lift");
            SEALHIP_CHECK(hipMemsetAsync(t, 0, t_words * 8, l.stream));
        });
        SEALHIP_CHECK(hipEventRecord(l.seed_pin_done, l.stream));
        check(launch_ntt(e, sk_ntt, static_cast<std::size_t>(e.n_key), ct_row_map(e.n_key, 1, -1), false, kNttCanonical), "ntt(sk)");
    }
} // namespace sealhip
