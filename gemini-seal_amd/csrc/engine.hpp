// engine.hpp -- internal interfaces of the sealhip engine (context, device tables, kernel launchers).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <array>
#include <atomic>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <cstdlib>
#include <vector>

#include "devmath.hpp"
#include "ntt_bounds.hpp"
#include "ntt_select.hpp"
#include "mac_select.hpp"
#include "hostmath.hpp"
#include "pool_scratch.hpp"
#include "held_workspace.hpp"
struct sealhip_kswitch_key; // the C ABI's key handle (api.cpp)

namespace sealhip
{
    namespace polyplan { struct Plan; } // poly_plan.hpp
    namespace evalmod { struct Plan; }  // evalmod_plan.hpp
    constexpr int kMaxRows = 136;          // rows of one "polynomial" a launch can describe
    constexpr int kMaxModuli = 64;         // SEAL_COEFF_MOD_COUNT_MAX (util/defines.h:48)
    constexpr unsigned short kSkipRow = 0xFFFF;

    // Which prime each row of a polynomial uses (index into Engine::d_primes); kSkipRow = leave untouched.
    struct RowMap
    {
        int rows;
        unsigned short prime[kMaxRows];
    };

    // Optional gather source of the single-pass forward NTT: destination row r of destination polynomial P reads
    // base[b] + P*poly_stride[b] + src_row*N instead of its own storage (code = b<<15 | reduce<<14 | src_row;
    // kSkipRow = in place). `reduce` applies barrett_reduce_63 w.r.t. the destination prime on load, which is the
    // single-prime mod-up rule of multi_special_primes.cpp:99-108.
    struct NttSource
    {
        const u64 *base[2];
        std::size_t poly_stride[2];
        unsigned short code[kMaxRows];
        // launch-wide treatment of the loaded words (ntt_select.hpp; single-prime mod-up, multi_special_primes.cpp:99-108):
        // kTreatNone, kTreatBarrett: barrett_reduce_63 w.r.t. the row's prime, kTreatCondSub: one conditional subtraction
        // (every source prime is below twice every destination prime, so the canonical residue is x or x - p). Both are
        // no-ops on rows whose source prime does not exceed their own. kTreatNegSpecial: the CKKS mod-down with one special
        // prime (multi_special_primes.cpp:262-273): the
        // word becomes -(x mod aux_p) as the integer aux_p - (x mod aux_p) (0 stays 0), aux_p = the special prime.
        // kTreatNegSpecialTop: the same, on a source row whose inverse transform left its top layer to the consumer (kNttDeferTop): the
        // transform reads the pairs (c, c + N/2) anyway and applies BackwardLazyLast (ntt.cpp:274-281) to them first;
        // aux_top = the special prime's {n^-1, its Shoup quotient, w n^-1, its Shoup quotient}.
        // kTreatModDownStore: that plus the rest of the CKKS mod-down as the transform's store phase (multi_special_primes.cpp:291-302 and the
        // final add, evaluator.cpp:2363-2366): the transformed word t of row (polynomial pl, prime q) is not stored; instead
        // v = (prod[pl][q] + t) * P^-1 mod q goes into the ciphertext -- added to what is there, or, with c0_src set,
        // written as (c0_src + v, v) for components (0, 1). Floating-point instance at log n >= 15 only (ntt_can_fuse_moddown).
        int reduce_mode;
        u64 aux_p, aux_cr1;
        u64 aux_top[4];
        struct ModDownStore
        {
            const u64 *inv_p, *inv_p_shoup; // [k] P^-1 mod q_i and its Shoup quotient (KsDev::invP on the device)
            const u64 *prod;                // [2m polynomials][prod_stride]: rows q of the key-switch products
            std::size_t prod_stride;
            u64 *ct;                        // [m][ct_stride]: component c at c * k rows
            std::size_t ct_stride;
            const u64 *c0_src;              // optional, [m][c0_stride]
            std::size_t c0_stride;
            unsigned *tflags;               // optional transparency sink of the m ciphertexts (devmath.hpp note_nonzero)
        } md;
    };
    constexpr unsigned short kSrcReduce = 0x4000, kSrcSecond = 0x8000; // kSrcReduce: informational (rows that need it)

    // Environment variables the library reads: the resource knobs SEALHIP_WORKSPACE_MB / SEALHIP_HOST_CHUNK /
    // SEALHIP_HOST_THREADS and the switches that run the REFERENCE'S OWN operation sequences instead of the proved shortcuts:
    // SEALHIP_NTT_EXACT_FWD, SEALHIP_NTT_EXACT_INV, SEALHIP_NTT_CANON_EXACT, SEALHIP_NTT_NO_FP64 -- all four read once, by
    // ntt_switches() (ntt.hip), into an NttSwitches (ntt_select.hpp). Nothing else: no variable
    // can re-open a race or switch a proved path off. (The A/B knobs of earlier rounds are gone with their
    // measurement-only build; what they measured is recorded in DESIGN.md and profiles/.)

    // The NTT launch flags (kNttCanonical .. kNttDeferTop), kFpPrimeBound and the names of the single-pass kernels' instance
    // codes: ntt_select.hpp.

    struct NttRound
    {
        int beta, wlo, whi;
    };
    struct NttPass
    {
        int logn, t, c, b_lo, flags, nrounds;
        NttRound rounds[4];
    };
    struct NttPlan
    {
        int logn, npass, flags;
        bool serial;
        NttPass pass[2];
    };
    NttPlan plan_ntt(int logn, bool inverse, int flags);

    // ---- device-resident constants of one BFV level (RNSTool, rns.cpp:539-729) ----
    struct RnsDev
    {
        int k, nB, B;               // |q|, |Bsk|, |B|
        u64 t;                      // plain modulus
        // ---- read by the unit and k > 32 kernels: the reference's constants as they are (the fused lift of both families
        // below reads q_mt_inv, q_to_mt and inv_prod_q_mod_mt too, their sign step inv_prod_B_mod_msk) ----
        // q -> Bsk U {m_tilde}
        u64 q_mt_inv[kMaxModuli];   // m_tilde * (q^_i)^{-1} mod q_i   (fused multiply_poly_scalar + inv_punctured)
        u64 q_inv[kMaxModuli];      // (q^_i)^{-1} mod q_i
        const u64 *q_to_Bsk;        // [nB][k]
        u64 q_to_mt[kMaxModuli];    // [k] mod 2^32
        u64 inv_prod_q_mod_mt;      // mod 2^32
        // per Bsk prime
        u64 prod_q_mod_Bsk[kMaxModuli + 2], inv_prod_q_mod_Bsk[kMaxModuli + 2], inv_mt_mod_Bsk[kMaxModuli + 2];
        // B -> q, B -> m_sk
        u64 B_inv[kMaxModuli + 1];  // (B^_i)^{-1} mod B_i
        const u64 *B_to_q;          // [k][B]
        u64 B_to_msk[kMaxModuli + 1];
        u64 inv_prod_B_mod_msk;
        u64 prod_B_mod_q[kMaxModuli];
        u64 inv_q_last_mod_q[kMaxModuli];
        // ---- read by the run-time-k instance (k <= 32). Of these the exact-k instances read q_p, q_mt_inv_s, b_w1(s),
        // inv_prod_B_mod_msk_s and the m_sk entries b_p[B], b_ninv[B]; everything else reaches them through the rows below ----
        // constant-folded forms of the fused BFV kernels (canonical results are unchanged):
        //   lift : out_j = ( sum_i t_i*L1[j][i] + temp_j*L2[j] ) mod b_j
        //   floor: tb_j  = ( in_j*G1[j] + sum_i t_i*G2[j][i] ) mod b_j,  t_i = in_i*floor_F0[i] mod q_i
        //   L1[j][i] = M_ji * m_tilde^{-1},  L2[j] = prod_q * m_tilde^{-1},  G1[j] = t * g_j,  G2[j][i] = -(M_ji * g_j)  (mod b_j)
        //   with g_j = (prod q)^{-1} [* B^_j^{-1} for j < B]. Engine::level forms them; the device holds their
        //   Montgomery forms only (suffix m: times 2^64 mod the row's prime; s: the Shoup quotient)
        u64 floor_F0[kMaxModuli];     // t * (q^_i)^{-1} mod q_i
        // the same constants with the deferred top inverse-NTT layer's factor folded in (index 0: lower half of a row,
        // n^{-1}; index 1: upper half, w * n^{-1}; ntt.cpp:393-402), so the fused floor kernel multiplies once, not twice
        // Index 2, 3: the same with 2^64 mod the row's prime on top -- the inverse NTT that forms the tensor product on load
        // leaves the Montgomery factor 2^-64 on every word (ntt.hip: DyadicSrc). One array indexed by 2 * mont + half: the
        // kernel selects its table with scalar arithmetic, not with a branch.
        u64 floor_F0_top[4][kMaxModuli], floor_F0_top_s[4][kMaxModuli];
        u64 floor_G1m_top[4][kMaxModuli + 2];
        // per-row prime constants next to the level constants (p, -p^-1 mod 2^64, floor(2^64 / p)): read at compile-time
        // offsets with scalar loads the compiler can batch -- going through PrimeDev[prime id] made every row loop wait for
        // two dependent scalar loads
        u64 q_p[kMaxModuli], q_ninv[kMaxModuli], q_rdp[kMaxModuli];
        u64 b_p[kMaxModuli + 2], b_ninv[kMaxModuli + 2], b_rdp[kMaxModuli + 2];
        u64 b_w1[kMaxModuli + 2], b_w1s[kMaxModuli + 2]; // top-layer forward twiddle of the Bsk rows and its Shoup quotient
        // Montgomery/Shoup companions of the folded constants and of the B -> q, B -> m_sk constants above
        const u64 *lift_L1m, *floor_G2m, *B_to_qm; // [nB][k], [nB][k], [k][B]
        u64 lift_L2m[kMaxModuli + 2], floor_G1m[kMaxModuli + 2];
        u64 q_mt_inv_s[kMaxModuli], floor_F0_s[kMaxModuli];
        u64 B_to_mskm[kMaxModuli + 1];
        u64 inv_prod_B_mod_msk_s;
        u64 pBm[kMaxModuli], nBm[kMaxModuli]; // prod_B_mod_q * 2^64, (q - prod_B_mod_q) * 2^64  (mod q_i)
        // ---- read by the exact-k instances: the same constants, one contiguous row per dot product, every constant split
        // at dot_split (dotacc.hpp dot_pack), followed by the row's prime p and -p^-1 mod 2^64 (not packed) ----
        const u64 *lift_rows;   // [nB][k + 3]     {lift_L2m[j], lift_L1m[j][0..k-1], p, ninv}
        const u64 *floor_rows;  // [5][nB][k + 3]  {G1[j], floor_G2m[j][0..k-1], p, ninv}; G1 = floor_G1m_top[sel] (sel < 4), floor_G1m (4)
        const u64 *q_rows;      // [k][B + 4]      {pBm[i], nBm[i], B_to_qm[i][0..B-1], p, ninv}
        const u64 *floor_first; // [5][k][3]       {F0, its Shoup quotient, q_i}: floor_F0_top(_s)[sel] (sel < 4), floor_F0(_s) (4); plain
        u64 B_to_mskp[kMaxModuli + 1];
        // ---- read by decrypt_scale_and_round (rns.cpp:1070-1126) ---- constants folded where the results are canonical anyway:
        //   y_i = in_i * dsr_scale[i] mod q_i  (|gamma t|_qi times (q^_i)^{-1});  {t, gamma} part = sum_i y_i * dsr_to_t/g[i]
        u64 dsr_scale[kMaxModuli], dsr_scale_s[kMaxModuli], dsr_to_t[kMaxModuli], dsr_to_g[kMaxModuli];
        u64 dsr_neg_inv_q_t, dsr_neg_inv_q_g, dsr_inv_gamma_t, dsr_gamma;
        unsigned gamma_prime; // PrimeDev id of gamma
        int redc_small;                        // every REDC of the fused kernels provably lands below 2p
        int dot_split;                         // 30 or 31: the split the packed rows above carry (bounds::behz_select_split)
        // (32-bit: there are no sub-dword scalar loads; a 16-bit id became a VECTOR load with a vmcnt(0) wait in the middle
        //  of every row loop)
        unsigned q_prime[kMaxModuli];       // prime ids of q rows
        unsigned bsk_prime[kMaxModuli + 2]; // prime ids of Bsk rows (m_sk last)
    };

    // ---- device-resident constants of the hybrid key switch at level k (multi_special_primes.cpp) ----
    struct KsDev
    {
        int k, nsp, nd, n_all, n_total; // ct primes, special primes, digits at this level, first-level k, key primes
        int is_ckks, strict;
        unsigned row_prime[kMaxModuli]; // prime id of ext row r (r < k: r; r >= k: n_all + r - k); 32-bit: scalar loads
        // mod-up: for bundle j, element a (source row j*nsp+a): inv_punch and its shoup; punch[dst row][a]
        const u64 *modup; // layout: [nd][ (2*nsp) + rows*nsp ] see engine.cpp
        // mod-down
        u64 inv_hat[kMaxModuli], inv_hat_shoup[kMaxModuli]; // [nsp]  p^_j^{-1} mod p_j
        const u64 *neg_hat;                                  // [k][nsp]  -p^_j mod q_i
        u64 invP[kMaxModuli], invP_shoup[kMaxModuli];        // [k]  P^{-1} mod q_i
    };

    // ---- the mod-down merged with the CKKS rescale at level k >= 2: the dropped set is
    // Dset = (l = q_{k-1}, p_0 .. p_{nsp-1}), D = P * l, half = floor(D / 2); index a walks Dset, index r the k - 1 kept primes
    struct KsRescaleDev
    {
        int k, nsp;
        unsigned drop_prime[kMaxModuli + 1];                           // prime id of Dset[a]
        u64 inv_hat[kMaxModuli + 1], inv_hat_shoup[kMaxModuli + 1];    // (D / d)^-1 mod d
        u64 half_d[kMaxModuli + 1];                                    // half mod d
        const u64 *hat;                                                // [k - 1][nsp + 1]  (D / d) mod q_r
        u64 neg_D[kMaxModuli], neg_half[kMaxModuli];                   // (-D) mod q_r, (-half) mod q_r
        u64 P_mod_q[kMaxModuli];                                       // P mod q_r (r < k - 1)
        u64 P_mod_l;                                                   // P mod l
        u64 invD[kMaxModuli], invD_shoup[kMaxModuli];                  // D^-1 mod q_r
    };

    // ---- CKKSEncoder::decode constants for the first k primes (RNSBase of the level, rns.cpp:237-290; context.cpp:370-376)
    constexpr int kCkksMaxLimbs = 32;
    struct CkksDecodeDev
    {
        int k;
        u64 q[kCkksMaxLimbs];         // total_coeff_modulus, little-endian limbs
        u64 half[kCkksMaxLimbs];      // upper_half_threshold = (q + 1) >> 1
        u64 inv_punct[kCkksMaxLimbs]; // (q / q_i)^{-1} mod q_i
        u64 punct[kCkksMaxLimbs * kCkksMaxLimbs]; // q / q_i, limbs of row i at i * kCkksMaxLimbs
    };

    // ---- Decryptor::invariant_noise_budget constants for the first k primes (decryptor.cpp:269-325), any level
    struct NoiseBudgetDev
    {
        int k;
        u64 q[kMaxModuli];           // total_coeff_modulus, little-endian limbs
        u64 half[kMaxModuli];        // upper_half_threshold = (q + 1) >> 1 (polyarithmod.cpp:27)
        u64 t_inv_punct[kMaxModuli]; // t * (q / q_i)^{-1} mod q_i: multiply_poly_scalar_coeffmod folded into compose_array
        u64 punct[kMaxModuli * kMaxModuli]; // q / q_i, limbs of row i at i * kMaxModuli
    };

    struct LevelTools
    {
        std::unique_ptr<HostRnsTool> host_rns; // BFV + CKKS (CKKS only uses inv_q_last_mod_q)
        RnsDev *d_rns = nullptr;
        KsDev *d_ks = nullptr;
        KsDev h_ks{};
        KsRescaleDev *d_ksr = nullptr; // built by Engine::level_rescale, at the first *_rescale call of the level
        KsRescaleDev h_ksr{};
        RnsDev h_rns{};
        std::vector<void *> owned; // device allocations to free
        RowMap map_q{}, map_bsk{}, map_key{}, map_qbsk{};
    };

    struct KSwitchKey
    {
        u64 *d_data = nullptr;
        std::uint32_t n_digits = 0;
        std::size_t words = 0;
        // keys made with save_seed (sealhip_generate_*_keys): the seed of c_1 of every digit, 8 words each (host memory);
        // empty otherwise. What the seeded save writes in place of c_1 (ciphertext.cpp:189-208).
        std::vector<std::uint64_t> seeds;
        // sealhip_generate_switching_keys with level < n_ct: the data-prime rows r >= level of every digit and the digits
        // j >= ceil(level / nsp) are zero, so the key serves key switches at levels <= level only. 0: a full key.
        std::uint32_t level = 0;
    };

    // Optional per-launch timing with HIP events on the launch stream (bench.py's roofline line).
    struct ProfRecord
    {
        const char *tag;
        hipEvent_t start, stop;
        double units; // rows (NTT passes) or lanes processed by the launch
    };

    // Per-host-thread execution state of a context: the reference's Evaluator is re-entrant
    // (native/src/seal/evaluator.h:1375-1377: it holds only the context and an immutable map; temporaries come from the
    // MemoryPoolHandle of the call), so every host thread that calls into a context gets its own lane -- HIP stream,
    // temporaries arena, forward-NTT tickets, launch profiler, graph capture state -- and operations of different
    // threads overlap instead of serialising. Tables, level constants and keys are shared and immutable.
    struct HostStage; // pinned staging buffers and copy streams of the *_host batch entries (hostbatch.cpp)
    void free_host_stage(HostStage *s);
    struct Lane
    {
        int device = -1;
        HostStage *stage = nullptr;
        hipStream_t stream = nullptr;
        bool own_stream = false;
        unsigned long long alloc_generation = 0; // bumps when the arena or the ticket buffer is re-allocated
        bool capturing = false; // between sealhip_graph_capture_begin / _end: no allocation, no synchronisation
        bool prof_on = false;
        std::vector<ProfRecord> prof;
        unsigned *d_tickets = nullptr; // per-row tickets of the single-pass forward NTT
        std::size_t tickets_cap = 0;
        // Transparency sink (sealhip_transparency_sink): device flags, one word per ciphertext of the operation's batch.
        // tsink_cur is what the final kernel of the operation in flight writes to (null outside an Evaluator entry that
        // supports it: internal launches of composite operations must not touch the caller's flags)
        unsigned *tsink = nullptr, *tsink_cur = nullptr;
        std::size_t tsink_cap = 0;
        // ... and what the NEXT launch of a sink-capable final kernel writes to (set by pipeline.cpp's SinkArm around exactly
        // that launch: the chunk's first item of tsink_cur)
        unsigned *tsink_arm = nullptr;
        std::size_t tsink_base = 0; // first item of an enclosing chunk loop (op_apply_galois around op_switch_key)
        // Sticky failure flag of this lane's launches (today: the forward NTT's sibling hand-off timing out), one word of
        // host-mapped memory per lane: a time-out in one thread's launch must fail THAT thread's next host-visible point,
        // not be seen and cleared by another thread's
        unsigned *h_fault = nullptr, *d_fault = nullptr;
        void *ws = nullptr; // workspace arena (stream-ordered reuse)
        std::size_t ws_bytes = 0, ws_used = 0;
        std::size_t ws_floor = 0; // bytes at the front of the arena held by an enclosing operation
        std::size_t ws_budget = 0; // cap of this lane's arena, fixed at first use (pipeline.cpp)
        // (batch size, items per arena chunk) of the last operations that walked a batch in chunks (pipeline.cpp for_chunks;
        // sealhip_debug_chunk_log): lets a caller that verifies its results pick the items at the chunk boundaries. The hoisted
        // rotation, when it has to walk its element list in passes, logs (elements, elements per pass) ahead of that pair.
        std::vector<std::pair<std::size_t, std::size_t>> chunk_log;
        // seed expansion (seed_expand.hip): pinned staging of the seed records, reused once the event that follows their
        // copy has completed; seed_slack = candidates provisioned per seed beyond rows x N (< 0: the computed default;
        // sealhip_debug_seed_slack)
        std::uint64_t *seed_pin = nullptr;
        std::size_t seed_pin_words = 0;
        hipEvent_t seed_pin_done = nullptr;
        std::int64_t seed_slack = -1;
        std::recursive_mutex busy; // held for the duration of an operation (a graph may be launched from another thread)
        ~Lane();
    };
    // ---- pooled device memory of a context (pool.cpp; sealhip_pool_* in include/sealhip.h) ----
    constexpr std::size_t kPoolMaxBytes = std::size_t(1) << 46;
    struct PoolBlock
    {
        std::size_t bytes = 0;          // its size class
        Lane *lane = nullptr;           // the lane that took it (held) or released it (cached)
        bool held = false;
        hipEvent_t released = nullptr;  // recorded on that lane's stream at the release; another lane's reuse waits on it
    };
    struct DevicePool
    {
        std::mutex mu;
        std::map<void *, PoolBlock> blocks;                                      // every block the pool holds
        std::map<Lane *, std::map<std::size_t, std::vector<void *>>> free;       // per lane, per size class
        std::uint64_t in_use = 0, cached = 0, mallocs = 0, frees = 0, hits = 0, misses = 0, cross_lane_hits = 0;
    };
    struct Engine;
    std::size_t pool_size_class(std::size_t bytes);
    void *pool_alloc(const Engine &e, std::size_t bytes);
    void pool_check_held(const Engine &e, const void *ptr); // E_INVALIDARG cases, before the device is needed
    void pool_release(const Engine &e, void *ptr);
    void pool_trim(const Engine &e);
    void pool_free_all(Engine &e);
    using Scratch = PoolScratch<Engine>; // an operation's temporaries: pool_alloc / pool_release, scoped (pool_scratch.hpp)

    struct LanePool
    {
        std::mutex mu;
        int device = -1;
        unsigned long long id = 0; // serial number, unique per process
        std::vector<std::unique_ptr<Lane>> all;
        std::vector<Lane *> idle; // lanes whose thread has exited
        Lane *take();
        void give(Lane *lane);
    };

    struct Engine
    {
        // parameters
        int scheme = 0, logn = 0, n_key = 0, nsp = 0, k_first = 0;
        std::size_t n = 0;
        u64 t = 0;
        bool mode_strict = false;
        bool use_half_kernel = true; // single-pass NTT kernels for logn >= 14 (the tiled one-pass kernel serves logn <= 13)
        int device = -1; // -1: host-only
        std::vector<u64> key_moduli, aux_primes;
        std::vector<HostNttTables> tables; // per prime id
        // device
        std::shared_ptr<LanePool> lanes;
        Lane &lane() const; // the calling thread's lane of this context (created on first use)
        std::unique_ptr<DevicePool> pool{ new DevicePool }; // sealhip_pool_* blocks (pool.cpp)
        // Device-side failures are reported through the lane's sticky flag (Lane::h_fault): kernels store to it, every entry
        // point that makes results host-visible reads it after its stream synchronisation (sync_and_check) and fails with
        // E_UNEXPECTED. all_lanes: every lane is synchronised and every lane's flag is read (and cleared).
        void sync_and_check(bool all_lanes = false) const;
        void check_fault() const; // the calling thread's lane alone, after a synchronisation the caller has done itself
        // debug hooks of the NTT hand-off (sealhip_debug_ntt_handoff): spin limit of the sibling wait and
        // suppression of the "finished reading" signal, to drive the failure path in the tests
        unsigned ntt_spin_limit = 1u << 24;
        bool ntt_suppress_signal = false;
        // bumps when a key-switch key is destroyed (graphs embed key pointers); read by other threads' graph launches
        std::atomic<unsigned long long> key_generation{ 0 };
        PrimeDev *d_primes = nullptr;
        std::vector<void *> owned;
        std::map<int, std::unique_ptr<LevelTools>> levels;
        std::map<std::uint32_t, std::uint32_t *> galois_tables; // elt -> device table (galois.cpp:18-47)
        // parms_id of level k (k = n_key: key level), registered by the binding (SEALContext computes them with Blake2,
        // encryptionparams.cpp:132-166); used by the wire-format loader to find a ciphertext's level
        std::map<int, std::array<std::uint64_t, 4>> parms_ids;
        // CKKSEncoder tables (ckks.cpp:37-76): slot map + its inverse (2N words), roots and inverse roots (N complex each)
        std::uint32_t *d_ckks_map = nullptr;
        double *d_ckks_roots = nullptr, *d_ckks_inv_roots = nullptr;
        std::map<int, CkksDecodeDev *> ckks_decode;
        std::map<int, int> total_bits; // significant bits of q_0...q_{k-1} (context.cpp:178)
        void ckks_tables();
        const CkksDecodeDev *ckks_decode_consts(int k);
        std::map<int, NoiseBudgetDev *> noise_budget;
        const NoiseBudgetDev *noise_budget_consts(int k); // BFV
        int total_coeff_modulus_bit_count(int k);
        int plain_prime = -1;                  // prime id of the plain modulus when batching is possible (context.cpp:262-275)
        std::uint32_t *d_batch_map = nullptr;  // BatchEncoder::matrix_reps_index_map_ (batchencoder.cpp:70-94)
        const std::uint32_t *batch_map();
        // ring packing: NTT_r(X^(N / 2^t)) for t = 1 .. logn and every ciphertext prime r, as
        // {word, Shoup companion} pairs: [t - 1][k_first][N][2]
        u64 *d_pack_mono = nullptr;
        const u64 *pack_monomials();
        // oblivious expansion: NTT_r(X^(-2^u)) for u < logn, the same layout: [u][k_first][N][2]
        u64 *d_expand_mono = nullptr;
        const u64 *expand_monomials();
        // blind rotation: psi_r^j for j < N in natural order and every ciphertext prime r, as
        // {word, Shoup companion} pairs: [k_first][N][2]; psi^(N + j) = -psi^j, so the kernel keeps the sign apart
        u64 *d_psi_pow = nullptr;
        const u64 *psi_powers();
        mutable std::mutex mu; // lazily built shared tables (levels, Galois tables, encoder tables, parms_ids)
        // profiler (per lane)
        void prof_begin(const char *tag, double units) const;
        void prof_end() const;
        // per-row tickets of the single-pass forward NTT (zeroed for the launch, stream-ordered), lane-owned
        unsigned *ntt_tickets(std::size_t nrows) const;

        ~Engine();
        int n_primes() const
        {
            return static_cast<int>(tables.size());
        }
        LevelTools &level(int k);       // builds host + device constants on first use
        LevelTools &level_host(int k);  // host constants only
        LevelTools &level_rescale(int k); // level(k) with the merged rescale's constants (CKKS, 2 <= k <= first level)
        const std::uint32_t *galois_table(std::uint32_t elt);
        void ws_reset() const
        {
            Lane &l = lane();
            l.ws_used = l.ws_floor;
        }
        u64 *ws_alloc(std::size_t words) const;
        void ws_reserve(std::size_t bytes) const;
        RowMap map_for(int k, unsigned base);
        int rows_for(int k, unsigned base);
    };

    struct HipError : std::runtime_error
    {
        hipError_t code;
        HipError(hipError_t c, const char *what) : std::runtime_error(what), code(c)
        {}
    };
#define SEALHIP_CHECK(expr)                                                                          \
    do                                                                                               \
    {                                                                                                \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            throw ::sealhip::HipError(_e, (std::string(#expr) + ": " + hipGetErrorString(_e)).c_str()); \
    } while (0)
    // the same for a launcher's return value: `what` names the launch in the message
    inline void check(hipError_t err, const char *what)
    {
        if (err != hipSuccess)
            throw HipError(err, (std::string(what) + ": " + hipGetErrorString(err)).c_str());
    }

    // `words` u64 words in a workspace: their bytes, up to the next 256-byte boundary
    inline std::size_t pad256(std::size_t words)
    {
        return (words * sizeof(u64) + 255) & ~static_cast<std::size_t>(255);
    }
    // a block cut into buffers that each start at a 256-byte step
    struct Carver
    {
        char *base;
        std::size_t at = 0;
        u64 *take(std::size_t words)
        {
            u64 *p = reinterpret_cast<u64 *>(base + at);
            at += pad256(words);
            return p;
        }
    };

    // Launch shape of the elementwise kernels: kThreads lanes per block, one block per kThreads work items up to
    // max_blocks; the kernels grid-stride the rest. (kThreads, and blocks_for -- one lane per work item, no cap -- stand in
    // mac_select.hpp, which a host compiler builds too.)
    inline unsigned grid_for(std::size_t work_items, std::size_t max_blocks = 256u * 16u)
    {
        const std::size_t blocks = (work_items + kThreads - 1) / kThreads;
        return static_cast<unsigned>(blocks < max_blocks ? (blocks ? blocks : 1) : max_blocks);
    }

    struct ProfScope
    {
        const Engine &e;
        ProfScope(const Engine &eng, const char *tag, double units) : e(eng)
        {
            if (e.lane().prof_on)
                e.prof_begin(tag, units);
        }
        ~ProfScope()
        {
            if (e.lane().prof_on)
                e.prof_end();
        }
    };

    // ---- launchers (each enqueues on e.stream) ----
    hipError_t ntt_init_kernels();
    // measured arithmetic ceiling of a butterfly sequence (ntt.hip butterfly_rate_kernel): butterflies per second
    hipError_t ntt_butterfly_rate(const Engine &e, int kind, int prime_id, double *butterflies_per_s);
    hipError_t launch_ntt(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, bool inverse, int flags);
    // forward transform whose input rows are gathered from elsewhere (only when ntt_can_gather(e))
    bool ntt_can_gather(const Engine &e);
    bool ntt_strict_top_done_ok(const Engine &e, const RowMap &map); // STRICT: kNttTopDone needs the dense forward schedule
    hipError_t launch_ntt_gather(const Engine &e, u64 *data, std::size_t nrows, const RowMap &map, const NttSource &src,
                                 int flags);
    // may this gathered launch leave the transform's last layer to an inner product of nd digits (kNttSplitLast)?
    bool ntt_can_split_last(const Engine &e, const RowMap &map, const NttSource &src, int flags, int nd);

    enum class PolyOp
    {
        Dyadic,
        Add,
        Sub,
        Negate,
        Scalar,
        Mod63 // modulo_poly_coeffs_63, polyarithsmallmod.h:98-120
    };
    hipError_t launch_poly_op(const Engine &e, PolyOp op, const u64 *a, const u64 *b, u64 scalar, u64 *r,
                              std::size_t nrows, const RowMap &map);
    // out[I] = sum_{i1+i2=I} a[i1] (.) b[i2]  over rows of `map` (evaluator.cpp:376-420 / 493-520)
    hipError_t launch_tensor_product(const Engine &e, const u64 *a, int sa, std::size_t a_stride, const u64 *b, int sb,
                                     std::size_t b_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                     const RowMap &map, bool square = false);
    hipError_t launch_fill_rows(const Engine &e, u64 *dst, const u64 *row_values, int rows, std::size_t count);
    // Sum of the (2,2) tensor products of a group of terms (poly.hip tensor_dot_kernel). Term t reads a[t] and b[t]: items
    // a_stride / b_stride words apart, two polynomials of map.rows rows each. c_0, c_1 go to out01 (one polynomial apart), c_2
    // to out2. reduce_on_load: the operands may be any 64-bit words (lazy forward transforms); otherwise they are canonical.
    // add_partial: the canonical sums already at out01 / out2 are added in. The transparency sink, when armed, gets
    // c_1 | c_2 of every item.
    constexpr int kDotGroup = bounds::kDotGroupTerms;
    struct DotTerms
    {
        const u64 *a[kDotGroup];
        const u64 *b[kDotGroup];
        int n;
    };
    hipError_t launch_tensor_dot(const Engine &e, const DotTerms &terms, std::size_t a_stride, std::size_t b_stride, u64 *out01,
                                 std::size_t out01_stride, u64 *out2, std::size_t out2_stride, std::size_t count,
                                 const RowMap &map, bool reduce_on_load, bool add_partial);
    // Linear combinations of ciphertexts with per-prime scalar weights (poly.hip lincomb_kernel):
    // out[s] = sum_t w[s][t] * x[t] (+ constant[s] on polynomial 0) for s < n_sums <= kLinTile over a group of up to kLinGroup
    // terms. x[t]: items x_stride words apart, `size` polynomials of map.rows rows each. w points at the weight of (sum 0,
    // term 0, row 0): rows are adjacent, terms map.rows words apart, sums w_sum_stride words apart. constant (or null):
    // n_sums x map.rows words; const_mode 1 adds it at coefficient 0 (coefficient form), 2 at every coefficient (NTT form).
    // out: sums out_sum_stride words apart, items x_stride words apart. add_partial: the canonical sums already in out are
    // added in. The transparency sink, when armed, gets polynomials 1.. of (sum s, item c) at flag s * flag_sum_stride + c.
    constexpr int kLinGroup = bounds::kLinGroupTerms, kLinTile = bounds::kLinTileSums;
    struct LinTerms
    {
        const u64 *x[kLinGroup];
        int n;
    };
    hipError_t launch_lincomb(const Engine &e, const LinTerms &terms, int size, std::size_t x_stride, const u64 *w,
                              std::size_t w_sum_stride, const u64 *constant, int const_mode, u64 *out, std::size_t out_sum_stride,
                              int n_sums, std::size_t count, const RowMap &map, bool add_partial, std::size_t flag_sum_stride);
    // Sums of ciphertexts against rows of plaintexts, all in NTT form (poly.hip dot_plain_kernel):
    // out[s] = sum_t x[t] (.) plain[s][t] for s < n_sums <= kLinTile over a group of n_terms <= kLinGroup terms. x points at
    // term 0 of item 0: terms are size * map.rows * N words apart, items item_stride words. plain points at plaintext (sum 0,
    // term 0): terms map.rows * N words apart, sums plain_sum_stride words. out, add_partial and the flags are those of
    // launch_lincomb, out's items size * map.rows * N words apart.
    hipError_t launch_dot_plain(const Engine &e, const u64 *x, int size, std::size_t item_stride, int n_terms, const u64 *plain,
                                std::size_t plain_sum_stride, u64 *out, std::size_t out_sum_stride, int n_sums, std::size_t count,
                                const RowMap &map, bool add_partial, std::size_t flag_sum_stride);
    // The same sums over terms that keep their own level and size (poly.hip lincomb_levels_kernel): a
    // CKKS ciphertext at a higher level holds the rows of a lower one at its own row stride, so term t is read in place as
    // items size[t] * rows[t] * N words apart, polynomials rows[t] * N words apart, rows r < map.rows of polynomials
    // j < size[t]; polynomials j >= size[t] are zero. rows[t] >= map.rows and 1 <= size[t] <= size. Weights, constant, out,
    // add_partial and the flags are those of launch_lincomb; out's items are out_stride = size * map.rows * N words apart.
    constexpr int kLinLevelsTile = bounds::kLinLevelsTileSums;
    struct LinLevelTerms
    {
        const u64 *x[kLinGroup];
        unsigned char rows[kLinGroup]; // (kMaxModuli and the size bound 16 fit a byte)
        unsigned char size[kLinGroup];
        int n;
    };
    hipError_t launch_lincomb_levels(const Engine &e, const LinLevelTerms &terms, int size, std::size_t out_stride, const u64 *w,
                                     std::size_t w_sum_stride, const u64 *constant, int const_mode, u64 *out,
                                     std::size_t out_sum_stride, int n_sums, std::size_t count, const RowMap &map,
                                     bool add_partial, std::size_t flag_sum_stride);
    // The weight and constant tables of a polynomial's inner sums (sealhip_evaluator_evaluate_polynomial): coefficient
    // e = j * ms + i (j < n_sums, i < ms) of the zero-padded list becomes constant[j][r] = the word
    // multiply_add_plain_with_scaling_variant adds at coefficient 0 for the one-coefficient plaintext c_e (i == 0), or
    // w[j][i - 1][r] = (c_e - t [c_e >= (t + 1) / 2]) mod q_r (i >= 1). The coefficients travel in kernel arguments.
    hipError_t launch_poly_tables(const Engine &e, int k, const u64 *coeffs, std::size_t n_coeffs, std::size_t ms, u64 *w,
                                  u64 *constant);
    // dst[0 .. n) = words (host memory), carried in kernel arguments kPutWords at a time: no staging buffer whose lifetime a
    // stream would have to respect (the planned tables of sealhip_evaluator_evaluate_polynomial_ckks)
    constexpr int kPutWords = 256;
    hipError_t launch_put_words(const Engine &e, u64 *dst, const u64 *words, std::size_t n);
    hipError_t launch_copy_rows(const Engine &e, const u64 *src, std::size_t src_poly_stride, u64 *dst,
                                std::size_t dst_poly_stride, std::size_t npolys, int rows);

    // RNSTool kernels; item strides are in words
    hipError_t launch_fastbconv_m_tilde(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                        std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count);
    hipError_t launch_sm_mrq(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in, std::size_t in_stride,
                             u64 *out, std::size_t out_stride, std::size_t count);
    // The dispatch of one BFV multiply / square at level k (op_bfv_multiply): the pipeline forks and the instances of the
    // two fused BEHZ kernels. op_bfv_multiply and the two launchers below consume it; sealhip_debug_bfv_multiply_plan
    // reports it (host constants only: it works on host-only contexts).
    constexpr int kBehzGeneric = 32; // instance codes: 1..bounds::kBehzExactMaxK exact k, 32 the run-time-k one (k <= 32),
    constexpr int kBehzStepwise = 64; // 64 the step-by-step kernels (k > 32)
    struct BfvMulPlan
    {
        int k, B, nB;       // level, |B|, |Bsk| = |B| + 1
        bool square;        // the square path (size-2 operand, b == nullptr)
        bool redc_small;    // bounds::behz_redc_small: every REDC of the fused kernels lands below 2p
        bool gather;        // q rows gathered from the operands by the forward NTT
        bool defer;         // inverse NTT leaves its top layer to the floor kernel
        bool fused_tensor;  // tensor product formed by the inverse NTT on load (launch_intt_tensor)
        bool tensor_apx;    // ... with the approximate-quotient forward transform
        bool lift_top;      // lift applies the forward NTT's top layer (kNttTopDone)
        int lift_kernel;    // instance code of the lift (above)
        int floor_kernel;   // instance code of the floor
        int deferred_top;   // floor input: 0 canonical, 1 top layer deferred, 2 and Montgomery-scaled (fused tensor)
    };
    BfvMulPlan plan_bfv_multiply(Engine &e, int k, int sa, int sb, bool square);
    bool ks_split_last_plan(Engine &e, int k, std::size_t count); // (sealhip_debug_ks_split_last)

    // fused fastbconv_m_tilde + sm_mrq: in k rows -> out |Bsk| rows, instance plan.lift_kernel
    // plan.lift_top: also apply the forward NTT's top layer to the rows written (exact-k instances only; the caller then
    // transforms them with kNttTopDone). -> bfv_lift_can_apply_top tells whether this level has such an instance.
    bool bfv_lift_can_apply_top(const Engine &e, int k, bool redc_small);
    hipError_t launch_bfv_lift(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in, std::size_t in_stride,
                               u64 *out, std::size_t out_stride, std::size_t count, const BfvMulPlan &plan);
    hipError_t launch_fast_floor(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                 std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                 int mul_t);
    hipError_t launch_fastbconv_sk(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count);
    // fused (x t) + fast_floor + fastbconv_sk: in (k+|Bsk|) rows -> out k rows, instance plan.floor_kernel
    // plan.deferred_top != 0: `in` holds the output of the single-pass inverse kernel WITHOUT its top layer; the kernel
    // applies that layer and the canonicalising subtraction while loading (needs ntt_can_defer_top(e))
    // plan.deferred_top == 2: as 1, and every input word carries the Montgomery factor 2^-64 (launch_intt_tensor)
    hipError_t launch_bfv_floor_sk(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                   const BfvMulPlan &plan);
    bool ntt_can_defer_top(const Engine &e, int k);
    // reduce mode 7 available for a gathered launch over the first k ciphertext primes with this special prime?
    bool ntt_can_fuse_moddown(const Engine &e, int k, u64 p_special);
    // inverse NTT whose input rows come from another buffer (single-pass kernels only: ntt_can_gather(e))
    hipError_t launch_intt_from(const Engine &e, u64 *data, const u64 *src, std::size_t src_poly_stride, std::size_t nrows,
                                const RowMap &map, int flags);
    // inverse NTT that forms the (2,2) ciphertext tensor product on load (needs ntt_can_gather(e)); see ntt.hip
    hipError_t launch_intt_tensor(const Engine &e, u64 *data, const u64 *x, std::size_t item_stride, std::size_t poly_stride,
                                  int kb, std::size_t nrows, const RowMap &map, int flags, bool square = false);
    hipError_t launch_divround_bfv(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, u64 *out, std::size_t out_stride, std::size_t count,
                                   int out_rows);
    // `last` points at the (inverse-transformed) last row of item 0; items are last_stride words apart
    hipError_t launch_rescale_pre(const Engine &e, const RnsDev *d, const RnsDev &h, u64 *last,
                                  std::size_t last_stride, u64 *temp, std::size_t temp_stride, std::size_t count);
    hipError_t launch_rescale_post(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in,
                                   std::size_t in_stride, const u64 *temp, std::size_t temp_stride, u64 *out,
                                   std::size_t out_stride, std::size_t count);

    // Galois
    enum class CtLinearOp
    {
        Add,
        Sub,
        Negate,
        MulPlain
    };
    // batches of ciphertexts [count][size][k][N]; b_item_stride only for MulPlain (0 = one plaintext for all)
    hipError_t launch_ct_linear(const Engine &e, CtLinearOp op, const u64 *a, int sa, const u64 *b, int sb,
                                std::size_t b_item_stride, u64 *out, std::size_t count, const RowMap &map);
    hipError_t launch_nonzero_words(const Engine &e, const u64 *data, std::size_t item_stride, std::size_t words,
                                    std::size_t count, unsigned *flags);
    hipError_t launch_nonzero_tail(const Engine &e, const u64 *ct, std::size_t item_words, std::size_t skip_words,
                                   std::size_t count, unsigned *flags);
    // Transparency as a flag output (sealhip_transparency_sink): an Evaluator entry clears the flags of its batch, then either
    // lets the final kernel of the operation write them (fused: multiply, square, relinearize, apply_galois) or runs the
    // read pass over its result (the remaining entries).
    // Order of effects: the constructor VALIDATES the capacity and nothing else, so an entry can build its
    // scope before its first launch and a call rejected for any reason leaves both the data and the caller's flags as they
    // were. The flags are cleared where they start to be written: by begin() (fused entries call it after their argument
    // checks, right before the operation), by arm() (relinearize: before its last key switch) or by read_pass().
    struct SinkScope
    {
        Engine &e;
        Lane &l;
        bool on;
        size_t count;
        bool cleared = false;
        SinkScope(Engine &eng, size_t n) : e(eng), l(eng.lane()), on(l.tsink != nullptr), count(n)
        {
            if (on && count > l.tsink_cap)
                throw std::invalid_argument("the transparency sink is smaller than this batch");
        }
        void clear()
        {
            if (on && !cleared && count)
                SEALHIP_CHECK(hipMemsetAsync(l.tsink, 0, count * sizeof(unsigned), l.stream));
            cleared = true;
            l.tsink_base = 0;
        }
        void begin() // fused entries (multiply, square, apply_galois): the operation's last kernel writes the flags
        {
            clear();
            if (on)
                l.tsink_cur = l.tsink;
        }
        void arm() // (relinearize: only its last key switch stores the final polynomial 1)
        {
            begin();
        }
        void read_pass(const u64 *result, uint32_t size, size_t poly_words, size_t n)
        {
            clear();
            if (on && size >= 2 && n)
                check(launch_nonzero_tail(e, result, poly_words * size, poly_words, n, l.tsink), "transparency");
        }
        ~SinkScope()
        {
            l.tsink_cur = l.tsink_arm = nullptr;
            l.tsink_base = 0;
        }
    };
    hipError_t launch_out_of_range(const Engine &e, const u64 *ct, std::size_t item_words, std::size_t count,
                                   const RowMap &map, unsigned *flags);
    hipError_t launch_plain_lift(const Engine &e, const u64 *plain, std::size_t plain_stride, u64 *out, std::size_t nplains,
                                 const RowMap &map, u64 t);
    // transform_to_ntt(Plaintext)'s lift (both reference branches, one formula: poly.hip): out[nplains][map.rows][N]
    hipError_t launch_plain_lift_centered(const Engine &e, const u64 *plain, std::size_t coeff_count, std::size_t plain_stride,
                                          u64 *out, std::size_t nplains, const RowMap &map, u64 t);
    hipError_t launch_galois(const Engine &e, const u64 *in, u64 *out, std::size_t nrows, const RowMap &map,
                             std::uint32_t elt, const std::uint32_t *table /* null: coefficient form */);

    // ring packing (ringpack.hip). map_q: the level's k ciphertext rows.
    // lwe_a[count][n_idx][k][N], lwe_b[count][n_idx][k] = the LWE samples of the coefficients idx[.] (device, each < N) of
    // the coefficient-form size-2 ciphertexts ct (ct_stride words per item)
    hipError_t launch_lwe_extract(const Engine &e, const u64 *ct, std::size_t ct_stride, std::size_t count,
                                  const std::uint32_t *idx, std::size_t n_idx, u64 *lwe_a, u64 *lwe_b, const RowMap &map_q);
    // out[jj][item][2][k][N], jj < n_out = the embedding of sample (item, j) of lwe_a[items][n][k][N] times w[r] (w_shoup: its
    // Shoup companions; host arrays of k words); c_1 in coefficient form, c_0 in coefficient form or (ntt_c0) as its
    // transform. n_out = c: j = j0 + jj. n_out = 2 c: then also j = n / 2 + j0 + (jj - c), the other operands of c merges.
    hipError_t launch_lwe_embed(const Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n, std::size_t items,
                                std::size_t j0, std::size_t c, std::size_t n_out, u64 *out, const RowMap &map_q, const u64 *w,
                                const u64 *w_shoup, bool ntt_c0);
    // out[x] = ((E_0 + O_0) + sigma_g(E_0 - O_0), E_1 + O_1), target[x] = sigma_g(E_1 - O_1) for ncts ciphertexts, O = X^shift B
    // (B null: O absent, the trace step). table null: coefficient form with ginv = g^{-1} mod 2N; else NTT form with
    // table = T_g and mono = the step's rows of Engine::pack_monomials. out and target overlap neither E nor B.
    hipError_t launch_pack_merge(const Engine &e, const u64 *E, const u64 *B, u64 *out, u64 *target, std::size_t ncts,
                                 const RowMap &map_q, std::uint32_t shift, std::uint32_t ginv, const std::uint32_t *table,
                                 const u64 *mono);

    // One step of the oblivious expansion without its key switch (ringpack.hip): for nsrc sources E
    // (src_stride words apart) and O = X^(-shift) E: out_even = (E_0 + sigma_g(E_0), E_1), target_even = sigma_g(E_1) and
    // the same of O. Source x = item * 2^log_grp + j: its even result is ciphertext item * out_item + j of out, its odd one
    // out_odd ciphertexts behind; the targets likewise with tgt_item and tgt_odd. table null: coefficient form with
    // ginv = g^{-1} mod 2N; else NTT form with table = T_g and mono = the step's rows of Engine::expand_monomials. w (or null)
    // and w_shoup: host arrays of map_q.rows words, the factor every loaded word gets. out and target do not overlap E.
    hipError_t launch_expand_step(const Engine &e, const u64 *E, std::size_t src_stride, std::size_t nsrc, int log_grp, u64 *out,
                                  std::size_t out_item, std::size_t out_odd, u64 *target, std::size_t tgt_item, std::size_t tgt_odd,
                                  const RowMap &map_q, std::uint32_t shift, std::uint32_t ginv, const std::uint32_t *table,
                                  const u64 *mono, const u64 *w, const u64 *w_shoup);

    // key switch
    // ext is digit-major: ext + j*ext_digit_stride + item*ext_stride + r*N
    hipError_t launch_ks_modup(const Engine &e, const KsDev *d, const KsDev &h, const u64 *coeff,
                               std::size_t coeff_stride, u64 *ext, std::size_t ext_stride,
                               std::size_t ext_digit_stride, std::size_t count, int only_digit);
    hipError_t launch_ks_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                             std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                             std::size_t ext_digit_stride, const u64 *key, u64 *prod, std::size_t prod_stride,
                             std::size_t count, int j0 = 0, int j1 = -1, // digits [j0, j1) (default: all of the level)
                             bool pair = false); // the digit rows lack their last layer (kNttSplitLast): the pair form
    inline bool ks_mac_has_pair_form(const Engine &e, const KsDev &h, std::size_t count, int j0, int j1) // (mac_select.hpp)
    {
        return ks_mac_has_pair_form(e.logn, h.nd, count, j0, j1);
    }
    hipError_t launch_ks_moddown_pre(const Engine &e, const KsDev *d, const KsDev &h, const u64 *prod,
                                     std::size_t prod_stride, u64 *temp, std::size_t temp_stride, std::size_t npolys);
    // BFV only: steps 1-4 of the rescale + the add into the ciphertext in one kernel; top_deferred = the rows of prod
    // come from an inverse NTT launched with kNttDeferTop. c0_src (both mod-down launchers): when set, the ciphertext is
    // not read: component 0 becomes c0_src + result, component 1 the result (apply_galois: the ciphertext the key switch
    // adds into is (galois(c0), 0), evaluator.cpp:1903-1935 -- no copy of c0, no zero fill of c1).
    hipError_t launch_ks_moddown_bfv(const Engine &e, const KsDev *d, const KsDev &h, const u64 *prod,
                                     std::size_t prod_stride, u64 *ct, std::size_t ct_item_stride, std::size_t npolys,
                                     bool top_deferred, const u64 *c0_src = nullptr, std::size_t c0_stride = 0);
    hipError_t launch_ks_moddown_post(const Engine &e, const KsDev *d, const KsDev &h, u64 *prod,
                                      std::size_t prod_stride, const u64 *temp, std::size_t temp_stride, u64 *ct,
                                      std::size_t ct_item_stride, std::size_t npolys, int add_into_ct,
                                      const u64 *c0_src = nullptr, std::size_t c0_stride = 0);
    // The mod-down merged with the CKKS rescale (tests/ks_rescale_ref.py). Polynomial pl is component
    // pl & 1 of item pl >> 1: base[item][comp][k][N] at base_stride words per item, acc[pl][k + nsp][N] at acc_stride words
    // per polynomial. fold: acc[pl][k-1] += (P mod l) * base[..][k-1] (step 1, NTT form). pre: steps 2-4 from the
    // coefficient-form dropped rows k-1 .. k+nsp-1 of acc into temp[pl][k-1][N]. post: step 5 into out[pl][k-1][N].
    hipError_t launch_ks_rescale_fold(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &h, const u64 *base,
                                      std::size_t base_stride, u64 *acc, std::size_t acc_stride, std::size_t npolys);
    hipError_t launch_ks_moddown_rescale_pre(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &h, const u64 *acc,
                                             std::size_t acc_stride, u64 *temp, std::size_t npolys);
    hipError_t launch_ks_moddown_rescale_post(const Engine &e, const KsRescaleDev *d, const KsRescaleDev &h, const u64 *base,
                                              std::size_t base_stride, const u64 *acc, std::size_t acc_stride, const u64 *temp,
                                              u64 *out, std::size_t npolys);

    // hoisted rotation (hoist.hip): the Galois elements of one launch, by value in the kernel arguments (nothing to upload,
    // so the launch is capturable): the NTT-form table T_g (Engine::galois_table), the key K_g, the element itself
    // (at most kHoistMaxElts of them: mac_select.hpp)
    struct HoistElts
    {
        int n;
        std::uint32_t elt[kHoistMaxElts];
        const std::uint32_t *table[kHoistMaxElts];
        const u64 *key[kHoistMaxElts];
    };
    // prod[element][item][2][k + nsp][N] = the inner product of the digits, read at column T_g[c], with K_g; target / ext as
    // for launch_ks_mac
    hipError_t launch_hoist_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                                std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                                std::size_t ext_digit_stride, const HoistElts &elts, u64 *prod, std::size_t prod_stride,
                                std::size_t count);
    // out[element][item][k][N] = sigma_g of component 0 of ct[item] (NTT form through T_g, else coefficient form)
    hipError_t launch_hoist_galois_c0(const Engine &e, const u64 *ct, std::size_t ct_stride, u64 *out, std::size_t count,
                                      const RowMap &map_q, const HoistElts &elts, bool ntt_form);
    // plaintext-weighted sum of rotations: the elements of one launch with their plaintexts.
    // w[i] = W[0][i] in key-level NTT form (n_key x N); sum s lies w_sum_stride words further. table[i] == null is the
    // identity (the base kernel only; the inner product is never launched with one).
    struct HoistDotElts
    {
        int n;
        const std::uint32_t *table[kHoistMaxElts];
        const u64 *key[kHoistMaxElts];
        const u64 *w[kHoistMaxElts];
    };
    // acc[sum][item][2][k + nsp][N] (item stride acc_stride) = sum over the launch's elements of W[sum][i] (.) prod_{g_i},
    // canonical; add: plus what acc holds
    hipError_t launch_hoist_dot_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *target,
                                    std::size_t target_stride, const u64 *ext, std::size_t ext_stride,
                                    std::size_t ext_digit_stride, const HoistDotElts &elts, std::size_t w_sum_stride, u64 *acc,
                                    std::size_t acc_stride, std::size_t count, std::size_t n_sums, bool add);
    // out[sum * out_sum_stride + item * 2kN] = (sum_i W[sum][i] (.) sigma_i(C_0), sum_{i identity} W[sum][i] (.) C_1) on the
    // k ciphertext rows, cn = C in NTT form (item stride 2kN); add: plus what out holds
    hipError_t launch_hoist_dot_base(const Engine &e, const u64 *cn, const HoistDotElts &elts, std::size_t w_sum_stride,
                                     u64 *out, std::size_t out_sum_stride, int k, std::size_t count, std::size_t n_sums,
                                     bool add);

    // giant steps in the extended basis: the giants of one launch. table[i] == null is the identity
    // giant, which only adds accj[i]; else inb[i] / ext[i] are the in-bundle rows and the digits of d_i for giant i's first
    // ciphertext (item strides inb_stride / ext_stride), key[i] its key, accj[i] its inner sum's acc (null: none was formed).
    struct HoistGiantElts
    {
        int n;
        const std::uint32_t *table[kHoistMaxElts];
        const u64 *key[kHoistMaxElts];
        const u64 *inb[kHoistMaxElts];
        const u64 *ext[kHoistMaxElts];
        const u64 *accj[kHoistMaxElts];
    };
    // acc[item][2][k + nsp][N] (item stride acc_stride) = the sum over the giants of their permuted inner products with
    // their keys, plus the permuted accj[.][0] (both components of accj straight for an identity giant); add: plus what
    // acc holds
    hipError_t launch_hoist_giant_mac(const Engine &e, const KsDev *d, const KsDev &h, const HoistGiantElts &elts,
                                      std::size_t inb_stride, std::size_t ext_stride, std::size_t ext_digit_stride,
                                      std::size_t accj_stride, u64 *acc, std::size_t acc_stride, std::size_t count, bool add);
    struct HoistGiantBases
    {
        int n;
        const std::uint32_t *table[kHoistMaxElts];
        const u64 *base[kHoistMaxElts]; // base_i of the first ciphertext, [item][2][k][N]
    };
    // out[item][2][k][N] = (sum_i sigma_i(base_i[0]), sum_{i identity} base_i[1]) in NTT form; add: plus what out holds
    hipError_t launch_hoist_giant_base(const Engine &e, const HoistGiantBases &elts, u64 *out, int k, std::size_t count,
                                       bool add);

    // ---- batches of separately allocated host ciphertexts (hostbatch.cpp) ----
    struct HostBatchIO
    {
        struct In
        {
            const u64 *const *ptrs; // one host pointer per item
            std::size_t words;      // words per item
        };
        struct Out
        {
            u64 *const *ptrs;
            std::size_t words;
        };
        std::vector<In> in;
        std::vector<Out> out;
        std::size_t tmp_words = 0; // device scratch per item for the chunk function
    };
    // enqueues the operation for m items on the calling thread's lane: d_in[a] / d_out[a] hold the items of array a back to back
    using HostChunkFn = std::function<void(Engine &, const std::vector<u64 *> &d_in, const std::vector<u64 *> &d_out, u64 *d_tmp,
                                           std::size_t m)>;
    void run_host_batch(Engine &e, const HostBatchIO &io, std::size_t count, const HostChunkFn &fn);
    // pins [ptr, ptr + bytes) in place (hipHostRegister) and remembers the range: run_host_batch copies arrays whose items lie
    // in registered ranges straight between the caller's buffers and the device (no staging copy)
    void host_register(const Engine &e, void *ptr, std::size_t bytes);
    void host_unregister(const Engine &e, void *ptr);

    // ---- composed operations (pipeline.cpp) ----
    // c0_src: see launch_ks_moddown_bfv -- the ciphertext is then write-only: (c0_src + result_0, result_1)
    // SURVEY 8(e) latency mode: the digits of ONE key switch split across devices. partial_out: only the inner product over
    // the digits [j0, j1) is formed, reduced to canonical residues and written there (count x 2 x (k + nsp) x N; ct unused).
    // partial_sum: the element-wise sum of every device's partials (words below ranks * p < 2^63; clobbered): reduced, then
    // the key switch continues from there (target, key unused). Modular sums are associative, so every later word is the one
    // the unsplit operation produces.
    struct KsSplit
    {
        int j0 = 0, j1 = 0;
        u64 *partial_out = nullptr;
        u64 *partial_sum = nullptr;
    };
    void op_switch_key(Engine &e, int k, u64 *ct, std::size_t ct_stride, const u64 *target, std::size_t target_stride,
                       std::size_t count, const KSwitchKey &key, const u64 *c0_src = nullptr, std::size_t c0_stride = 0,
                       const KsSplit *split = nullptr);
    // CKKS: out[count][2][k-1][N] = the merged mod-down and rescale of base + key switch of target;
    // base[item] = two polynomials of k rows at base_stride words per item; nothing but out is written
    void op_switch_key_rescale(Engine &e, int k, const u64 *base, std::size_t base_stride, const u64 *target,
                               std::size_t target_stride, std::size_t count, const KSwitchKey &key, u64 *out);
    void op_modup(Engine &e, int k, int bundle, u64 *ext, std::size_t count);
    void op_bfv_multiply(Engine &e, int k, const u64 *a, int sa, const u64 *b, int sb, std::size_t count, u64 *out);
    void op_ckks_multiply(Engine &e, int k, const u64 *a, int sa, const u64 *b, int sb, std::size_t count, u64 *out);
    // Ciphertext inner product: sum_i a[i] * b[i] over n_terms pairs of size-2 batches
    // [count][2][k][N], the tensor products summed in NTT form -- for BFV (STRICT) in the extended base, so that the sum
    // takes ONE inverse transform and ONE floor. key == nullptr: out[count][3][k][N]; else the sum is relinearized once and
    // out is [count][2][k][N]. The operands are only read.
    void op_dot_product(Engine &e, int k, const u64 *const *a, const u64 *const *b, std::size_t n_terms, std::size_t count,
                        const KSwitchKey *key, u64 *out, bool rescale = false);
    // terms a level admits (BFV: while the floor's Shenoy-Kumaresan conversion stays exact; CKKS: 2^32 - 1); host constants only
    std::uint64_t dot_product_max_terms(Engine &e, int k);
    // out[s][count][size][k][N] = sum_i weights[s][i][r] * terms[i] (+ constant[s][r] on polynomial 0: at coefficient 0 for BFV,
    // at every coefficient for CKKS), DESIGN.md section 20. terms[i]: [count][size][k][N], only read; weights
    // [n_sums][n_terms][k] and constant [n_sums][k] (or null) are device memory.
    void op_linear_combination(Engine &e, int k, const u64 *const *terms, std::size_t n_terms, int size, std::size_t count,
                               const u64 *weights, const u64 *constant, std::size_t n_sums, u64 *out);
    // the same over CKKS terms at their own level and size: terms[i] is [count][sizes[i]][levels[i]][N],
    // levels[i] >= k, sizes[i] <= size; levels and sizes are host arrays
    void op_linear_combination_levels(Engine &e, int k, const u64 *const *terms, const std::uint32_t *levels,
                                      const std::uint32_t *sizes, std::size_t n_terms, int size, std::size_t count,
                                      const u64 *weights, const u64 *constant, std::size_t n_sums, u64 *out);
    // ---- polynomial evaluation (poly_eval.cpp; DESIGN.md sections 20 and 21) ----
    // a * b relinearized to size 2 (api.cpp: multiply, relinearize, copy): wide [count][3][k][N] is scratch, the result is narrow
    const u64 *relin_product(Engine &e, std::uint32_t k, const u64 *a, const u64 *b, std::size_t count,
                             const sealhip_kswitch_key *const *relin_keys, std::uint32_t n_relin_keys, u64 *wide, u64 *narrow);
    // BFV: the host-only plan of sum_c coeffs[c] x^c (its refusals are E_INVALIDARG; polyplan::make_plan is the CKKS one)
    struct BfvPolyPlan
    {
        std::size_t d, m, g, n_terms, ms; // degree (trailing zeros trimmed), baby and giant steps, an inner sum's terms (+ 1)
        std::vector<u64> padded;        // [g][ms] coefficients
        std::vector<std::size_t> outer; // the giant steps j >= 1 whose inner sum survives
    };
    BfvPolyPlan bfv_poly_plan(Engine &h, std::uint32_t k, const u64 *coeffs, std::size_t degree, std::size_t n_baby);
    // out[count][2][k][N] = p(x) (CKKS: [p.out_level] rows, p made with its tables); key: relin_keys' first, null only when
    // d = 1; sink: the entry's scope
    void op_evaluate_polynomial(Engine &e, const BfvPolyPlan &plan, std::uint32_t k, const u64 *x, std::size_t count,
                                const KSwitchKey *key, const sealhip_kswitch_key *const *relin_keys, std::uint32_t n_relin_keys,
                                u64 *out, SinkScope &sink);
    void op_evaluate_polynomial_ckks(Engine &e, const polyplan::Plan &p, std::uint32_t k, const u64 *x, std::size_t count,
                                     const KSwitchKey *key, u64 *out, SinkScope &sink);
    std::size_t ckks_poly_temp_words(const polyplan::Plan &p, std::size_t N); // per item, what that call takes from the pool
    // Evaluator::square as its own path (evaluator.cpp:560-770): the operand is lifted / transformed once
    void op_bfv_square(Engine &e, int k, const u64 *a, int sa, std::size_t count, u64 *out);
    void op_ckks_square(Engine &e, int k, const u64 *a, int sa, std::size_t count, u64 *out);
    void op_mod_switch_scale(Engine &e, int k, const u64 *ct, int size, std::size_t count, u64 *out,
                             std::size_t in_item_stride = 0);
    void op_divround_ntt_inplace(Engine &e, int k, u64 *data, std::size_t count);
    void op_rescale_special_inplace(Engine &e, int k, u64 *poly, std::size_t count);
    void op_apply_galois(Engine &e, int k, u64 *ct, std::size_t count, std::uint32_t elt, const KSwitchKey &key);
    // Ring packing. extract: the samples of the coefficients idx (device) of ct[count][2][k][N] in the
    // scheme's form; ct is only read. pack: out[count][2][k][N] = the pack of the n = 2^l samples of every item, then (trace)
    // the field trace (n is passed as l); keys[t] is the key of 2^t + 1 for the steps t that run (1 .. l, and l + 1 .. logn with trace).
    void op_extract_lwe(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *idx, std::size_t n_idx,
                        u64 *lwe_a, u64 *lwe_b);
    void op_pack_lwes(Engine &e, int k, const u64 *lwe_a, const u64 *lwe_b, int l, std::size_t count,
                      const KSwitchKey *const *keys, bool trace, bool normalize, u64 *out, SinkScope &sink);
    // Oblivious expansion: out[count][n][2][k][N], n = 2^l, from ct[count][2][k][N] (only read) in the
    // scheme's form; keys[t] is the key of N / 2^(t-1) + 1 for the steps t = 1 .. l. sink: count * n flags.
    void op_expand(Engine &e, int k, const u64 *ct, int l, std::size_t count, const KSwitchKey *const *keys, bool normalize,
                   u64 *out, SinkScope &sink);
    // Sums against plaintext rows: out[n_sums][count][size][k][N] = sum_i cts[count][n_terms][size][k][N]
    // (.) plain[n_sums][n_terms][k][N], everything in NTT form
    void op_dot_plain(Engine &e, int k, const u64 *cts, std::size_t n_terms, int size, std::size_t count, const u64 *plain,
                      std::size_t n_sums, u64 *out);
    // RGSW. An RGSW encryption of a small m is two key-switch keys in one block,
    // [half][digit][component][n_key][N]: half 0 (K_b) made with new_key = m, half 1 (K_a) with new_key = m s.
    struct RgswKey
    {
        u64 *d_data = nullptr;
        std::uint32_t n_digits = 0;
        std::size_t half_words = 0; // n_digits * 2 * n_key * N
        std::uint32_t level = 0;    // as KSwitchKey::level
        const u64 *half(int h) const { return d_data + static_cast<std::size_t>(h) * half_words; }
    };
    // what launch_ext_mac would run for a chunk of `count` items at level k, with no launch (sealhip_debug_ext_mac_plan)
    struct ExtMacPlan
    {
        MacChoice choice;
        bool split; // the sum is reduced between its halves (bounds::ext_mac_sum_fits fails for 2 nd terms)
    };
    ExtMacPlan ext_mac_plan(const Engine &e, const KsDev &h, std::size_t count);
    // prod[item][l][r][c] = ( sum_j D0_j K_b[j][l] + sum_j D1_j K_a[j][l] ) mod p_r: ext holds the 2 nd digits digit-major
    // (those of c_0 first), own0 / own1 the rows the sum reads inside a bundle, own_stride words from item to item
    hipError_t launch_ext_mac(const Engine &e, const KsDev *d, const KsDev &h, const u64 *own0, const u64 *own1,
                              std::size_t own_stride, const u64 *ext, std::size_t ext_stride, std::size_t ext_digit_stride,
                              const u64 *key_b, const u64 *key_a, u64 *prod, std::size_t prod_stride, std::size_t count);
    // blind rotation (blindrot.hip).
    // dst[i] = X^(e_i) src[i] - minus_one * src[i] for count size-2 ciphertexts at level k, e_i = exps[i * exps_stride + step]
    // mod 2N (device); src_stride 0 shares one operand. ntt_form: psi_pow = Engine::psi_powers. dst does not overlap src.
    hipError_t launch_monomial_prepare(const Engine &e, int k, bool ntt_form, bool minus_one, const u64 *src, std::size_t src_stride,
                                       u64 *dst, std::size_t dst_stride, const std::uint32_t *exps, std::size_t exps_stride,
                                       std::size_t step, const u64 *psi_pow, std::size_t count);
    // exps[n_samples][1 + (ternary ? 2N : N)] from the level-1 samples lwe_a[n_samples][N], lwe_b[n_samples]
    hipError_t launch_lwe_mod_switch(const Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n_samples, bool ternary,
                                     std::uint32_t b_offset, std::uint32_t *exps);
    // m_coeff[n_lwe * (ternary ? 2 : 1)][N]: the constant polynomials [s_j = 1] (and [s_j = -1]) of secret[n_lwe] (device)
    hipError_t launch_lwe_indicators(const Engine &e, const std::int32_t *secret, std::size_t n_lwe, bool ternary,
                                     std::int32_t *m_coeff);
    // out[i] = X^(e_i) ct[i] - minus_one * ct[i], e_i = exps[i * exps_stride] (ct_stride 0: one ct shared by the batch)
    void op_multiply_monomial(Engine &e, int k, const u64 *ct, std::size_t ct_stride, std::size_t count, const std::uint32_t *exps,
                              std::size_t exps_stride, bool minus_one, u64 *out);
    // acc_0 = X^(exps[i][0]) tv[i]; acc_t = acc_(t-1) + ((X^(exps[i][t]) - 1) acc_(t-1)) (x) rgsw[t-1]; out = acc_(n_steps).
    // exps: count x (1 + n_steps) words (device). The accumulator lives in out from step 0 on.
    void op_blind_rotate(Engine &e, int k, const u64 *tv, std::size_t tv_stride, std::size_t count, const std::uint32_t *exps,
                         std::size_t n_steps, const RgswKey *const *rgsw, u64 *out, SinkScope &sink);
    void op_lwe_mod_switch(Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n_samples, bool ternary,
                           std::uint32_t b_offset, std::uint32_t *exps);
    // diff[i] = ct1[i] - ct0[i] (2 k N words per item, back to back) and base[i] = ct0[i], for npairs ciphertext pairs whose
    // operands lie stride0 / stride1 words apart; everything 16-byte aligned
    hipError_t launch_cmux_prepare(const Engine &e, int k, const u64 *ct0, std::size_t stride0, const u64 *ct1,
                                   std::size_t stride1, u64 *diff, u64 *base, std::size_t base_stride, std::size_t npairs);
    // n blocks (rgsw[i]: 2 x digits x 2 x n_key x N words) from m_coeff[n][N]; seeds_host n x 2 x digits x 8, noise n x 2 x digits x N
    void op_generate_rgsw(Engine &e, const u64 *sk_ntt, const std::int32_t *m_coeff, std::size_t n, int level,
                          const std::uint64_t *seeds_host, const std::int32_t *noise, u64 *scratch, u64 *const *rgsw);
    // out[count][2][k][N] += ct (x) rgsw: out holds the base on entry (ct_stride words between the items of ct)
    void op_external_product(Engine &e, int k, const u64 *ct, std::size_t ct_stride, std::size_t count, const RgswKey &g, u64 *out);
    // out = ct0 + (ct1 - ct0) (x) rgsw
    void op_cmux(Engine &e, int k, const u64 *ct0, std::size_t stride0, const u64 *ct1, std::size_t stride1, std::size_t count,
                 const RgswKey &g, u64 *out);
    // out[count] = cts[count][index], the index's bit t encrypted in bits[t] (least significant first): l levels of CMux
    void op_select(Engine &e, int k, const u64 *cts, std::size_t count, int l, const RgswKey *const *bits, u64 *out,
                   SinkScope &sink);
    // One decomposition of c_1, n_elts rotations: out[n_elts][count][2][k][N], ct is only read.
    // Not the words of n_elts calls of op_apply_galois (the automorphism does not commute with the mod-up).
    void op_apply_galois_many(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *elts,
                              const KSwitchKey *const *keys, std::size_t n_elts, u64 *out,
                              const std::uint32_t *slots = nullptr); // slots[i]: output slot of element i (null: i)
    // sum_i W[s][i] * sigma_{g_i}(ct) with one decomposition and one mod-down per sum:
    // out[n_sums][count][2][k][N]; plain_ntt[n_sums][n_elts][n_key][N]; keys[i] may be null where elts[i] == 1.
    void op_apply_galois_dot_plain(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *elts,
                                   const KSwitchKey *const *keys, std::size_t n_elts, const u64 *plain_ntt,
                                   std::size_t n_sums, u64 *out, bool rescale = false);
    // sum_j sigma_{h_j}( sum_i W[j][i] * sigma_{g_i}(ct) ) with the giant steps accumulated in the extended basis and one
    // full mod-down: out[count][2][k][N]; plain_ntt[n_giant][n_baby][n_key][N]; a key may be null
    // where its element is 1.
    void op_apply_galois_bsgs_plain(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *baby_elts,
                                    const KSwitchKey *const *baby_keys, std::size_t n_baby, const std::uint32_t *giant_elts,
                                    const KSwitchKey *const *giant_keys, std::size_t n_giant, const u64 *plain_ntt, u64 *out,
                                    bool rescale = false);
    void op_multiply_plain(Engine &e, int k, u64 *ct, int size, std::size_t count, const u64 *plain,
                           std::size_t plain_stride);
    // Evaluator::transform_to_ntt(Plaintext) (evaluator.cpp:1648-1744), BFV: plain_ntt[count][k][N]
    void op_transform_plain_to_ntt(Engine &e, int k, const u64 *plain, std::size_t coeff_count, std::size_t plain_stride,
                                   std::size_t count, u64 *plain_ntt);
    // Decryptor::dot_product_ct_sk_array (decryptor.cpp:218-265) and RNSTool::decrypt_scale_and_round
    void op_dot_product_ct_sk(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers,
                              bool is_ntt_form, u64 *out);
    hipError_t launch_dot_sk(const Engine &e, const u64 *ct, int size, std::size_t ct_item_stride, const u64 *sk_powers,
                             std::size_t sk_power_stride, u64 *out, std::size_t count, const RowMap &map, int add_c0);
    hipError_t launch_decrypt_scale_and_round(const Engine &e, const RnsDev *d, const RnsDev &h, const u64 *in, u64 *out,
                                              std::size_t count);

    // ---- encrypt-side arithmetic, scaling variant, BatchEncoder (rlwe.hip) ----
    struct RlweArgs
    {
        u64 *ct;
        std::size_t ct_item_stride, ct_poly_stride; // words
        int polys, rows;                            // polynomials written per item; rows (prime ids 0..rows-1)
        const u64 *x;                               // per-item multiplicand
        std::size_t x_item_stride, x_poly_stride;
        const u64 *y; // multiplicand shared by all items (secret key / public key, NTT form)
        std::size_t y_poly_stride;
        const std::int32_t *e; // small signed samples, N per polynomial
        std::size_t e_item_stride, e_poly_stride;
        int negate;
    };
    struct ScalingArgs
    {
        const u64 *plain;
        std::size_t plain_item_stride;
        u64 *c0;
        std::size_t c0_item_stride;
        int k, sub;
        u64 t, t_cr0, t_cr1, q_mod_t, threshold;
        u64 div[kMaxModuli]; // floor(q / t) mod q_j  (context.cpp:303-321)
    };
    // scalingvariant.cpp:31-51: fix = floor((m * (q mod t) + upper_half_increment) / t) for one plaintext coefficient m;
    // the quotient of barrett_reduce_128 (uintarithsmallmod.h:140-178) kept instead of thrown away, one correction
    // (numerator < t^2 + t < 2^123, quotient <= t). Shared by scaling_variant_kernel and the fused encrypt kernels.
    __device__ __forceinline__ u64 scaling_variant_fix(const ScalingArgs &a, u64 m)
    {
        u64 lo = 0, hi = 0;
        mac128(lo, hi, m, a.q_mod_t);
        const u64 lo2 = lo + a.threshold;
        hi += lo2 < lo;
        lo = lo2;
        const u64 carry0 = mulhi(lo, a.t_cr0);
        const u64 t1lo = lo * a.t_cr1, t1hi = mulhi(lo, a.t_cr1);
        const u64 tmp1 = t1lo + carry0;
        const u64 tmp3 = t1hi + (tmp1 < t1lo);
        const u64 ulo = hi * a.t_cr0, uhi = mulhi(hi, a.t_cr0);
        const u64 tmp1b = tmp1 + ulo;
        const u64 carry1 = uhi + (tmp1b < tmp1);
        u64 fix = hi * a.t_cr1 + tmp3 + carry1;
        const u64 rem = lo - fix * a.t;
        fix += rem >= a.t;
        return fix;
    }
    // the scaling constants of level k (floor(q / t) mod q_j, q mod t, t's Barrett constants; context.cpp:303-321)
    void fill_scaling_args(const Engine &e, int k, ScalingArgs &a);
    hipError_t launch_rlwe_stage(const Engine &e, int stage, const RlweArgs &a, std::size_t count);
    hipError_t launch_scaling_variant(const Engine &e, const ScalingArgs &a, std::size_t count);
    hipError_t launch_batch_permute(const Engine &e, bool encode, const u64 *in, std::size_t in_item_stride,
                                    std::size_t nvalues, u64 *out, const std::uint32_t *map, std::size_t count,
                                    u64 signed_t = 0);
    // util/rlwe.cpp:204-300: ct[item] = ([-(a*s + e)]_q, a) over key primes 0..rows-1; a_ntt = count x rows x N
    // uniform words in NTT form, e = count x N, sk_ntt = rows x N (row stride N)
    void op_encrypt_zero_symmetric(Engine &e, int rows, bool is_ntt_form, const u64 *a_ntt, const std::int32_t *noise,
                                   const u64 *sk_ntt, std::size_t count, u64 *ct);
    // util/rlwe.cpp:140-202: ct[item][j] = pk[j]*u + e[j]; pk = 2 x rows x N (NTT form), u = count x N, e = count x 2 x N
    void op_encrypt_zero_asymmetric(Engine &e, int rows, bool is_ntt_form, const u64 *pk, const std::int32_t *u,
                                    const std::int32_t *noise, std::size_t count, u64 *ct);
    // util/scalingvariant.cpp:15-92 on the c0 of every item (ct_item_stride words apart)
    void op_scaling_variant(Engine &e, int k, const u64 *plain, std::size_t plain_item_stride, u64 *ct,
                            std::size_t ct_item_stride, std::size_t count, bool sub);

    // ---- Encryptor (encrypt.hip, pipeline.cpp) ----
    enum class EncryptFinish
    {
        AsymBfv,
        SymBfv,
        AsymCkks,
        SymCkks
    };
    struct EncryptArgs
    {
        u64 *ct; // [item][2][k][N]; the symmetric kernels work in place on c_0
        std::size_t ct_item_stride;
        int k, rows;                 // ciphertext level; rows of src per polynomial (asymmetric: k + 1 divides by q_k)
        const u64 *src;              // asymmetric: [item][2][rows][N] (src_item_stride); symmetric CKKS: the secret key
        std::size_t src_item_stride;
        const u64 *temp;             // asymmetric CKKS: lazy NTT of the rescale_pre output, [item][2][k][N]
        const std::int32_t *e;       // BFV: small signed noise, [item][2][N] (asymmetric) or [item][N] (symmetric)
        const u64 *plain;            // nullptr: encrypt_zero. BFV: [item][N] < t; CKKS: [item][k][N] NTT form
        std::size_t plain_item_stride;
        u64 inv_q_last[kMaxModuli];  // q_k^{-1} mod q_i of level k + 1 (inv_q_last_mod_q, rns.cpp:719-728)
        ScalingArgs sc;              // BFV: the scaling constants of level k (only the constant fields are read)
    };
    hipError_t launch_encrypt_finish(const Engine &e, EncryptFinish kind, const EncryptArgs &a, std::size_t count);
    // Encryptor::encrypt / encrypt_zero with a public key (encryptor.cpp:141-176, :205-253) at level k: encrypt_zero_asymmetric
    // over the k + 1 rows of the previous level (k = n_key: k rows), divide_and_round_q_last(_ntt) and, with plain, the
    // plaintext step. pk = 2 x n_key x N (NTT form), u = count x N, noise = count x 2 x N; ct = count x 2 x k x N.
    void op_encrypt(Engine &e, int k, const u64 *pk, const u64 *plain, std::size_t plain_item_stride, const std::int32_t *u,
                    const std::int32_t *noise, std::size_t count, u64 *ct);
    // Encryptor::encrypt_symmetric / encrypt_zero_symmetric (rlwe.cpp:204-300) at level k: c_1 expanded from seeds_host
    // (count x 8 words), sk = n_key x N (NTT form), noise = count x N. seeded: the BFV save_seed branch (a sampled in
    // coefficient form); the caller has already dropped it where k x N < 9.
    void op_encrypt_symmetric(Engine &e, int k, const u64 *sk, const u64 *plain, std::size_t plain_item_stride,
                              const std::uint64_t *seeds_host, const std::int32_t *noise, bool seeded, std::size_t count,
                              u64 *ct);
    // batchencoder.cpp:113-154 / :339-376 (needs a prime plain modulus = 1 mod 2N: Engine::plain_prime >= 0)
    void op_batch_encode(Engine &e, const u64 *values, std::size_t nvalues, std::size_t count, u64 *plain, bool is_signed = false);
    void op_batch_decode(Engine &e, const u64 *plain, std::size_t count, u64 *values, bool is_signed = false);

    // CKKSEncoder (ckks_encoder.hip)
    hipError_t launch_ckks_encode_front(const Engine &e, const double *values, std::size_t n_values, std::size_t count,
                                        double n_inv_scale, double *cv, u64 *out, int rows, const std::uint32_t *map,
                                        const double *inv_roots, unsigned long long *max_abs);
    hipError_t launch_ckks_decode_back(const Engine &e, const u64 *coeff, const CkksDecodeDev *d, int k, std::size_t count,
                                       double inv_scale, double *res, double *values, const std::uint32_t *map,
                                       const double *roots);
    // values: count x n_values complex doubles (device); plain: count x k x N, NTT form
    void op_ckks_encode(Engine &e, int k, const double *values, std::size_t n_values, std::size_t count, double scale,
                        u64 *plain);
    // values out: count x N/2 complex doubles
    void op_ckks_decode(Engine &e, int k, const u64 *plain, std::size_t count, double scale, double *values);

    // ---- homomorphic DFT: CoeffToSlot / SlotToCoeff (homdft.hip, homdft.cpp, homdft_plan.hpp) ----
    namespace dftplan
    {
        struct Plan;
    }
    // values[n_giant][n_baby][N/2] complex doubles (device): gain * the stage's diagonals, pre-rotated for BSGS; the encoder's
    // tables must be resident (Engine::ckks_tables)
    hipError_t launch_dft_stage_values(const Engine &e, int s0, int r, bool inverse, bool folded, std::uint32_t n_baby,
                                       std::uint32_t n_giant, double gain, double *values);
    // a, b = count x 2 x map.rows x N in NTT form: re = a + b, im = -i (a - b) / out = re + i im
    hipError_t launch_dft_conj_split(const Engine &e, const u64 *a, const u64 *b, u64 *re, u64 *im, std::size_t count,
                                     const RowMap &map);
    hipError_t launch_dft_merge(const Engine &e, const u64 *re, const u64 *im, u64 *out, std::size_t count, const RowMap &map);
    // the real factor of a stage's values: `gain` on the last CoeffToSlot / first SlotToCoeff stage, 1/2 more on the last
    // CoeffToSlot stage (the split adds a value to its conjugate), 2^-r on every CoeffToSlot stage (inverse layers)
    double dft_stage_gain(const dftplan::Plan &p, std::size_t stage, double gain);
    void dft_stage_values_host(const Engine &h, const dftplan::Plan &p, std::size_t stage, double gain, double *values);
    void op_dft_stage_values(Engine &e, const dftplan::Plan &p, std::size_t stage, double gain, double *values);
    // The end of tables that hold a workspace (held_workspace.hpp) next to `engine` and `device`: refused during a graph
    // capture with the owner's text; else the blocks go back to the pool on the calling thread's lane, `rest` frees what
    // else the tables own and the tables themselves, and the caller's current device is left as it was.
    template <class Tables, class Rest>
    void destroy_held_tables(Tables *t, const char *refusal, Rest rest)
    {
        const Engine &e = *t->engine;
        if (e.lane().capturing)
            throw std::logic_error(refusal);
        int current = -1;
        (void)hipGetDevice(&current);
        SEALHIP_CHECK(hipSetDevice(t->device));
        t->held.release_all(e);
        rest();
        if (current >= 0 && current != e.device)
            (void)hipSetDevice(current);
    }
    struct DftTables; // the plan and, per stage, plain_ntt[n_giant][n_baby][n_key][N] in device memory
    DftTables *dft_tables_create(Engine &e, const dftplan::Plan &p, double gain);
    void dft_tables_destroy(DftTables *t);
    const dftplan::Plan &dft_tables_plan(const DftTables &t);
    const Engine *dft_tables_engine(const DftTables &t); // the context they were made on
    const u64 *dft_tables_stage(const DftTables &t, std::size_t stage);
    struct DftStageKeys // a stage's Galois elements (1 = the identity) and keys (null there), as op_apply_galois_bsgs_plain takes them
    {
        std::vector<std::uint32_t> baby, giant;
        std::vector<const KSwitchKey *> baby_keys, giant_keys;
    };
    // ct[count][2][k][N] -> out_re, out_im[count][2][k - n_stages][N]; conj_key: the key of element 2N - 1
    void op_coeffs_to_slots(Engine &e, const DftTables &t, const u64 *ct, std::size_t count, const std::vector<DftStageKeys> &keys,
                            const KSwitchKey &conj_key, u64 *out_re, u64 *out_im);
    // ct_re, ct_im[count][2][k][N] -> out[count][2][k - n_stages][N]
    void op_slots_to_coeffs(Engine &e, const DftTables &t, const u64 *ct_re, const u64 *ct_im, std::size_t count,
                            const std::vector<DftStageKeys> &keys, u64 *out);

    // ---- towards CKKS bootstrapping: ModRaise and the double-angle step (bootstrap.hip, poly.hip) ----
    // coef[npolys][N] (coefficient form, canonical modulo q_0) -> rows 1 .. k_out-1 of out[npolys][k_out][N]: the centred
    // coefficients modulo each row's prime, canonical, in coefficient form. Row 0 is left alone.
    hipError_t launch_mod_raise_lift(const Engine &e, const u64 *coef, u64 *out, std::size_t npolys, int k_out);
    // ct[count][2][k_in][N] -> out[count][2][k_out][N] (CKKS, NTT form): row 0 is the input's, row i >= 1 the forward
    // transform of centre(INTT_0(row 0)) mod q_i. Only the q_0 rows of ct are read.
    void op_mod_raise(Engine &e, int k_in, const u64 *ct, std::size_t count, int k_out, u64 *out);
    // out[count][3][map.rows][N] = (2 a_0^2 + constant[r], 4 a_0 a_1, 2 a_1^2) of a[count][2][map.rows][N], canonical;
    // constant: map.rows words of host memory (they travel in the kernel's arguments)
    hipError_t launch_square_affine(const Engine &e, const u64 *a, u64 *out, std::size_t count, const RowMap &map,
                                    const u64 *constant);
    // CKKS: out[count][2][k-1][N] = the merged key switch and rescale of 2 ct^2 + constant (host, k words)
    void op_double_angle(Engine &e, int k, const u64 *ct, std::size_t count, const u64 *constant, const KSwitchKey &key,
                         u64 *out);
    // EvalMod (poly_eval.cpp over evalmod_plan.hpp): out[count][2][p.out_level][N] = the planned Chebyshev polynomial of x
    // followed by p.r double-angle steps; key: relin_keys' first; sink: the entry's scope. Temporaries are pool blocks.
    void op_eval_mod(Engine &e, const evalmod::Plan &p, std::uint32_t k, const u64 *x, std::size_t count, const KSwitchKey *key,
                     u64 *out, SinkScope &sink);
    std::size_t evalmod_temp_words(const evalmod::Plan &p, std::size_t N); // per item, what that call takes from the pool
    // The bootstrap (bootstrap.cpp): two DFT tables (CoeffToSlot with gain 1, SlotToCoeff with the plan's gain), the EvalMod
    // plan, and one pool block per lane for the intermediates
    struct BootstrapTables;
    BootstrapTables *bootstrap_tables_create(Engine &e, std::uint32_t k_top, const dftplan::Plan &c2s, const evalmod::Plan &em,
                                             const dftplan::Plan &s2c, double s2c_gain);
    void bootstrap_tables_destroy(BootstrapTables *t);
    const Engine *bootstrap_tables_engine(const BootstrapTables &t);
    const DftTables &bootstrap_tables_c2s(const BootstrapTables &t);
    const DftTables &bootstrap_tables_s2c(const BootstrapTables &t);
    std::size_t bootstrap_temp_words(std::uint32_t k_top, const dftplan::Plan &c2s, const evalmod::Plan &em, std::size_t N);
    // ct[count][2][k_in][N] -> out[count][2][s2c out level][N]: mod_raise to k_top, coeffs_to_slots, eval_mod ONCE over the
    // 2 count real and imaginary halves, slots_to_coeffs. With to_sparse and to_dense (both or neither; DESIGN.md section
    // 25) only the raise runs under the sparse secret: the q_0 rows are switched with to_sparse at level 1, raised, and
    // switched back with to_dense at k_top; the rest is the same code.
    void op_bootstrap(Engine &e, const BootstrapTables &t, int k_in, const u64 *ct, std::size_t count,
                      const std::vector<DftStageKeys> &c2s_keys, const KSwitchKey &conj_key,
                      const std::vector<DftStageKeys> &s2c_keys, const KSwitchKey &relin_key, u64 *out,
                      const KSwitchKey *to_sparse = nullptr, const KSwitchKey *to_dense = nullptr);
    // out[count][2][k][N] = (c_0, 0) + switch_key(c_1): a ciphertext under the key's source secret becomes one under its
    // target secret. c0 and c1 are k rows each (NTT form for CKKS, coefficient form for BFV, as op_switch_key's target),
    // `stride` words from one item to the next; out must not overlap them.
    void op_switch_secret(Engine &e, int k, const u64 *c0, const u64 *c1, std::size_t stride, std::size_t count,
                          const KSwitchKey &key, u64 *out);

    // ---- Decryptor (decrypt.hip, pipeline.cpp) ----
    // bits_out[i] = max(bits_out[i], bits of the largest centred |t v| of item i), v = count x k x N dot products
    hipError_t launch_noise_bits(const Engine &e, const NoiseBudgetDev *d, int k, const u64 *v, std::size_t count,
                                 int *bits_out);
    // Decryptor::invariant_noise_budget (decryptor.cpp:269-325), BFV, ct[count][size][k][N] in coefficient form; budgets in host
    // memory; synchronises once
    void op_invariant_noise_budget(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers,
                                   std::int32_t *budgets);
    // Decryptor::decrypt (decryptor.cpp:51-150): BFV plain[count][N] mod t from coefficient form, CKKS plain[count][k][N] in
    // NTT form; stream-ordered
    void op_decrypt(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers, u64 *plain);

    // ---- Ciphertext::expand_seed on the device (seed_expand.hip) ----
    // dst of job i receives the rows x N words of c_1 re-sampled from the 64-byte seed (8 words, random_seed_type) of job i:
    // sample_poly_uniform(BlakePrng(seed), first `rows` key primes), word for word. Stream-ordered on the calling thread's
    // lane; the seeds are staged, so the caller's seed memory may go away when this returns.
    struct SeedJob
    {
        const void *seed; // host, 64 bytes (any alignment: seeds inside a byte stream are not word-aligned)
        u64 *dst;                  // device
    };
    void op_expand_seeds(Engine &e, int rows, const SeedJob *jobs, std::size_t count);

    // ---- RLWE samples from seeds (seed_expand.hip, sample_map.hpp) ----
    constexpr unsigned kSampleMaxPolys = 16; // polynomials per item
    // Item i: n_ternary ternary polynomials at out + i * item_stride, n_noise noise polynomials at out_noise + i *
    // noise_stride (int32, N values each), from the BlakePRNG stream of seed i (seeds_host: count x 8 words): word pN + j of
    // the stream gives coefficient j of polynomial p, ternary ones first. One array out[i][p][N] is out_noise = out +
    // n_ternary N with equal strides. Pointers are 16-byte aligned and strides multiples of 4. Stream-ordered on the calling
    // thread's lane; the seeds are staged (not capturable), and the roots derived from them are erased from the arena.
    void op_sample_polys(Engine &e, const std::uint64_t *seeds_host, std::size_t count, unsigned n_ternary, unsigned n_noise,
                         std::int32_t *out, std::size_t item_stride, std::int32_t *out_noise, std::size_t noise_stride);
    // the kernels' map functions on n caller-supplied words (device)
    void op_debug_sample_map(Engine &e, const u64 *words, std::size_t n, bool noise, std::int32_t *out);
    // KeyGenerator::generate_sk (keygenerator.cpp:66-103): one ternary polynomial from the seed, lifted over the n_key key
    // primes and transformed; sk_ntt = n_key x N words. The coefficient-form scratch is erased. h > 0: the fixed-weight
    // polynomial of weight h in place of the ternary one.
    void op_generate_secret_key(Engine &e, const std::uint64_t *seed_host, unsigned h, u64 *sk_ntt);
    // Fixed-weight polynomials: out + i * item_stride receives the N int32 coefficients of weight
    // h (1 .. N) for seed i, from the first N stream words of BlakePRNG(seed i) -- the h smallest words are the support, bit 0
    // the sign. Pointer and stride rules, staging and erasure as op_sample_polys; the raw-word scratch is erased too.
    void op_sample_fixed_weight(Engine &e, const std::uint64_t *seeds_host, std::size_t count, unsigned h, std::int32_t *out,
                                std::size_t item_stride);
    // the rank kernel itself on caller-supplied words[n_polys][N] (device) -> out[n_polys][N]
    void op_debug_fixed_weight_map(Engine &e, const u64 *words, std::size_t n_polys, unsigned h, std::int32_t *out);

    // ---- KeyGenerator::generate_one_kswitch_key for a batch of keys (keygen.hip, composition in pipeline.cpp) ----
    constexpr int kKeygenMaxKeys = 32; // keys per assemble launch (kernel-argument table)
    struct KeygenArgs
    {
        u64 *key[kKeygenMaxKeys];         // digits x 2 x n_key x N each
        const u64 *s_new[kKeygenMaxKeys]; // new key source, n_key rows of N (NTT form): sk (Galois) or a power of sk (relin)
        std::uint32_t elt[kKeygenMaxKeys]; // s_new is read through the NTT-form Galois permutation of elt (1: identity)
        const u64 *sk;                     // n_key x N, NTT form
        u64 factor[kMaxModuli];            // prod of the special primes mod q_r, r < n_ct (keygenerator.cpp:355-359)
        int n_keys, digits, n_key, nsp, n_ct;
    };
    hipError_t launch_keygen_assemble(const Engine &e, const KeygenArgs &a);
    // Key i (key_data[i]: digits x 2 x n_key x N words of device memory) for the new key apply_galois_ntt(sk, elts[i]), or,
    // with elts == nullptr, sk^(i+2) (relin_keys, keygenerator.cpp:146-175). seeds_host: n_keys x digits x 8 words (the
    // seeds of c_1), noise: n_keys x digits x N small signed samples (device). Stream-ordered on the calling thread's lane.
    // s_from (n_keys x n_key x N, NTT form, with elts == nullptr): the new key of key i handed in -- a switching key from
    // that secret to sk_ntt's; then `level` < n_ct zero-fills, in both components, the data-prime rows r >= level of every
    // digit and every digit j >= ceil(level / nsp) once the keys are assembled.
    void op_generate_kswitch_keys(Engine &e, const u64 *sk_ntt, const std::uint32_t *elts, std::size_t n_keys,
                                  const std::uint64_t *seeds_host, const std::int32_t *noise, u64 *const *key_data,
                                  const u64 *s_from = nullptr, int level = 0);
    // The chunk loop of every operation that needs arena temporaries per item (pipeline.cpp): as many items per chunk as
    // the lane's arena holds at `bytes_per_item` (the padded sum over the item's `n_buffers` temporaries), one
    // (count, chunk) entry in Lane::chunk_log, then body(off, m) for the m items from item `off` with the arena reset.
    void for_chunks(Engine &e, std::size_t count, std::size_t bytes_per_item, int n_buffers,
                    const std::function<void(std::size_t off, std::size_t m)> &body);
    // The same division for an operation that walks its items itself: how many of `count` items the lane's arena cap holds
    // at `bytes_per_item` (at least one), logged as (count, chunk) in Lane::chunk_log. Reserves nothing.
    std::size_t arena_chunk_items(Engine &e, std::size_t count, std::size_t bytes_per_item);
    // rows 0..rows-1 of the key primes for each of `polys` polynomials of an item; `only` >= 0 keeps that polynomial
    RowMap ct_row_map(int rows, int polys, int only);

    // ---- matrix-vector products from a caller's matrix (lintrans.hip, lintrans.cpp, lintrans_plan.hpp) ----
    namespace ltplan
    {
        struct Plan;
    }
    // flags[c], c < d (device): bit 0 = diagonal c of the d x d complex matrix has a non-zero entry, bit 1 = a non-finite one
    hipError_t launch_lintrans_occupancy(const Engine &e, const double *matrix, std::uint32_t d, std::uint8_t *flags);
    // values: `cells` cells of N/2 complex doubles (device), the grid's cells cell0 .. cell0 + cells - 1 in [gi][bi] order;
    // mask (d bytes), baby and giant (the plan's steps) in device memory
    hipError_t launch_lintrans_values(const Engine &e, const double *matrix, std::uint32_t d, const std::uint8_t *mask,
                                      const std::int32_t *baby, std::uint32_t n_baby, const std::int32_t *giant, std::size_t cell0,
                                      std::size_t cells, double gain, double *values);
    // occupied: d bytes on the host, 0 or 1; returns whether every entry is finite. Synchronises.
    bool op_lintrans_occupancy(Engine &e, const double *matrix, std::uint32_t d, std::uint8_t *occupied);
    // the whole grid, n_giant x n_baby x N/2 complex doubles (device). Stages the plan's steps from the host and synchronises.
    void op_lintrans_values(Engine &e, const ltplan::Plan &p, const double *matrix, double gain, double *values);
    struct LinearTransform; // the plan and plain_ntt[n_giant][n_baby][n_key][N] in device memory
    LinearTransform *lintrans_create(Engine &e, const double *matrix, std::uint32_t d, std::uint32_t n1, double scale, double gain);
    void lintrans_destroy(LinearTransform *t);
    const Engine *lintrans_engine(const LinearTransform &t); // the context they were made on
    const ltplan::Plan &lintrans_plan(const LinearTransform &t);
    const u64 *lintrans_plain(const LinearTransform &t);
    double lintrans_scale(const LinearTransform &t);

    std::unique_ptr<Engine> make_engine(int scheme, int logn, const u64 *key_moduli, int n_key, int nsp, u64 t,
                                        bool strict, int device);
} // namespace sealhip
