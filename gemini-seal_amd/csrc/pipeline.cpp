// pipeline.cpp -- the Evaluator-level operations composed from the kernels: BFV/CKKS multiply
// (native/src/seal/evaluator.cpp:274-527), hybrid key switch (:2259-2368), modulus switch / rescale
// (:829-957) and apply_galois (:1841-1943), batched over independent ciphertexts. Large batches are
// processed in chunks sized to the workspace arena; every chunk is a fixed sequence of launches on
// one stream, so temporaries are reused in stream order without host synchronisation.
//
// What the composite operations share (anonymous namespaces, each ahead of its first user):
//   arena     plan_chunk / for_chunks (items per chunk), plan_pass (a list walked in passes next to one item), KsArena /
//             switch_key_arena (a key switch's item, also for the operations that nest one), FloorRestore (scratch parked
//             under a raised floor, and the sink's first item, around a nested chunk loop)
//   key switch  ks_digits + ks_products (front half), ks_finish / ks_finish_rescale (back half)
//   BFV in q u Bsk  split_q_bsk, bfv_lift_and_transform (steps 1-3), bfv_inverse_and_floors / bfv_floors (steps 5-8)
//   Galois lists  check_galois_elt, check_axis + load_tables (GaloisAxis)
//   weighted sums  check_weighted_form, components_ntt, hoist_dot_sums, finish_sum
#include "engine.hpp"

#include <cmath>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace sealhip
{
    namespace
    {
        std::size_t workspace_budget_bytes(const Engine &e)
        {
            // cap of a lane's temporaries arena (it grows on demand up to this): SEALHIP_WORKSPACE_MB, else a sixth of the
            // memory free on the device when the lane first needs it, between 2 and 48 GiB -- sized for 288 GB of HBM,
            // where larger chunks mean larger launches (bench: +3 % from 8 to 48 GiB). Fixed per lane (an operation that
            // parks scratch at the front of the arena relies on the nested operation seeing the same cap); a lane created
            // later sees what the earlier ones left, so the caps of all threads' lanes cannot add up to more than the device.
            // An operation that parks scratch plans the nested one with the whole cap: the arena then exceeds it by the
            // parked bytes (op_apply_galois: at most 1 GiB; op_pack_lwes, op_expand and op_select: at most half of the cap, 1.5 times
            // in all).
            Lane &l = e.lane();
            if (l.ws_budget)
                return l.ws_budget;
            static const std::size_t env_budget = [] {
                if (const char *env = std::getenv("SEALHIP_WORKSPACE_MB"))
                {
                    std::size_t mb = static_cast<std::size_t>(std::strtoull(env, nullptr, 10));
                    return (mb < 64 ? std::size_t(64) : mb) << 20;
                }
                return std::size_t(0);
            }();
            if (env_budget)
                return l.ws_budget = env_budget;
            std::size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
                return l.ws_budget = std::size_t(8192) << 20;
            const std::size_t lo = std::size_t(2) << 30, hi = std::size_t(48) << 30;
            return l.ws_budget = std::min(hi, std::max(lo, (free_b + l.ws_bytes) / 6));
        }

        // one (length, entries per pass) pair of Lane::chunk_log, the oldest of 64 dropped
        void log_chunk(Engine &e, std::size_t length, std::size_t per_pass)
        {
            auto &log = e.lane().chunk_log;
            if (log.size() >= 64)
                log.erase(log.begin());
            log.emplace_back(length, per_pass);
        }

        // how many items fit the arena, given the padded byte need of one item (sum over its buffers). log = false: an
        // operation that parks scratch under a raised floor asks, before the scratch goes live, for what the nested
        // operation's chunk loop will ask for -- the arena then cannot move while the scratch is live
        std::size_t plan_chunk(Engine &e, std::size_t count, std::size_t bytes_per_item, int n_buffers, bool log = true)
        {
            const std::size_t budget = workspace_budget_bytes(e);
            std::size_t chunk = budget / (bytes_per_item ? bytes_per_item : 1);
            chunk = std::max<std::size_t>(1, std::min(chunk, count));
            if (log)
                log_chunk(e, count, chunk);
            e.ws_reserve(e.lane().ws_floor + chunk * bytes_per_item + static_cast<std::size_t>(n_buffers) * 256);
            return chunk;
        }

        // "The list does not fit: walk it in passes". Next to fixed_bytes per item, how many of a list's n units of
        // unit_bytes the arena takes at once: all of them, else what fits (at least one) -- and then the split is logged as
        // (logged_n or n, pass), ahead of the operation's item chunks (sealhip_debug_chunk_log).
        std::size_t plan_pass(Engine &e, std::size_t fixed_bytes, std::size_t unit_bytes, std::size_t n, std::size_t logged_n = 0)
        {
            const std::size_t budget = workspace_budget_bytes(e);
            if (fixed_bytes + n * unit_bytes <= budget)
                return n;
            const std::size_t fit = budget > fixed_bytes ? (budget - fixed_bytes) / unit_bytes : 0;
            const std::size_t pass = std::max<std::size_t>(1, std::min(fit, n));
            log_chunk(e, logged_n ? logged_n : n, pass);
            return pass;
        }

        RowMap skip_map(const RowMap &base, int keep_lo, int keep_hi)
        {
            RowMap m = base;
            for (int r = 0; r < m.rows; r++)
                if (r < keep_lo || r >= keep_hi)
                    m.prime[r] = kSkipRow;
            return m;
        }

        // Two maps over disjoint rows of `polys` polynomials in the extended base (qbsk = a level's map_qbsk, k of its
        // rows the ciphertext primes): the q rows and the Bsk rows, for the launch pairs that treat them differently
        struct QBskMaps
        {
            RowMap q, bsk;
        };
        QBskMaps split_q_bsk(const RowMap &qbsk, int k, int polys)
        {
            QBskMaps s{};
            s.q.rows = s.bsk.rows = polys * qbsk.rows;
            for (int p = 0; p < polys; p++)
                for (int r = 0; r < qbsk.rows; r++)
                {
                    s.q.prime[p * qbsk.rows + r] = r < k ? qbsk.prime[r] : kSkipRow;
                    s.bsk.prime[p * qbsk.rows + r] = r < k ? kSkipRow : qbsk.prime[r];
                }
            return s;
        }
    } // namespace

    void for_chunks(Engine &e, std::size_t count, std::size_t bytes_per_item, int n_buffers,
                    const std::function<void(std::size_t off, std::size_t m)> &body)
    {
        const std::size_t chunk = plan_chunk(e, count, bytes_per_item, n_buffers);
        for (std::size_t off = 0; off < count; off += chunk)
        {
            e.ws_reset();
            body(off, std::min(chunk, count - off));
        }
    }

    std::size_t arena_chunk_items(Engine &e, std::size_t count, std::size_t bytes_per_item)
    {
        const std::size_t fit = workspace_budget_bytes(e) / (bytes_per_item ? bytes_per_item : 1);
        const std::size_t chunk = std::max<std::size_t>(1, std::min(fit, count));
        log_chunk(e, count, chunk);
        return chunk;
    }

    RowMap ct_row_map(int rows, int polys, int only)
    {
        if (rows * polys > kMaxRows)
            throw std::invalid_argument("too many rows");
        RowMap m{};
        m.rows = rows * polys;
        for (int j = 0; j < polys; j++)
            for (int r = 0; r < rows; r++)
                m.prime[j * rows + r] = (only < 0 || only == j) ? static_cast<unsigned short>(r) : kSkipRow;
        return m;
    }

    namespace
    {
        // The arena of one item of a key switch, in words: what its chunk loop plans with and carves, and what an
        // operation that nests it (op_apply_galois, op_dot_product) sizes the arena by
        struct KsArena
        {
            std::size_t w_coeff, w_ext, w_prod, w_temp;
            static constexpr int n_buffers = 4; // (coeff counts whether or not an item has one: 256 bytes of slack)
            std::size_t item_bytes() const
            {
                return (w_coeff + w_ext + w_prod + w_temp) * sizeof(u64);
            }
        };
        // op_switch_key: the target's k rows in the other form (CKKS, STRICT BFV), the digits, the products, the
        // mod-down's temporaries. op_switch_key_rescale (rescale; CKKS): the temporaries are at the level below.
        KsArena switch_key_arena(Engine &e, int k, bool rescale = false)
        {
            const std::size_t N = e.n, rows = static_cast<std::size_t>(k + e.nsp);
            const std::size_t nd = static_cast<std::size_t>(e.level(k).h_ks.nd);
            const bool has_coeff = e.scheme == 2 || e.mode_strict;
            return KsArena{ has_coeff ? static_cast<std::size_t>(k) * N : 0, nd * rows * N, 2 * rows * N,
                            2 * static_cast<std::size_t>(rescale ? k - 1 : k) * N };
        }

        // Transparency sink (devmath.hpp note_nonzero): the sink of the operation in flight, shifted to a chunk's first
        // item, and the scope around the ONE launch that stores the result's polynomials 1..
        unsigned *sink_at(Engine &e, std::size_t off)
        {
            Lane &l = e.lane();
            return l.tsink_cur ? l.tsink_cur + l.tsink_base + off : nullptr;
        }
        struct SinkArm
        {
            Lane &l;
            SinkArm(Engine &e, unsigned *flags) : l(e.lane())
            {
                l.tsink_arm = flags;
            }
            ~SinkArm()
            {
                l.tsink_arm = nullptr;
            }
        };
        // Restores the arena floor an operation raised over buffers at the front of the arena that must survive a nested
        // operation's chunk loop (which resets the arena to the floor), and the sink's first item, which such an operation
        // shifts to its own chunk for the nested loop (sink_at). Both go back to what they were, also after a throw.
        struct FloorRestore
        {
            Lane &l;
            const std::size_t floor, base;
            explicit FloorRestore(Engine &e) : l(e.lane()), floor(l.ws_floor), base(l.tsink_base)
            {}
            ~FloorRestore()
            {
                l.ws_floor = floor;
                l.tsink_base = base;
            }
            void raise(std::size_t bytes) // over the saved floor: what lies there is parked
            {
                l.ws_floor = floor + bytes;
            }
            void *parked() const // (ask after whatever may still move the arena)
            {
                return static_cast<char *>(l.ws) + floor;
            }
        };

        // The part of the key switch that does not depend on the key (evaluator.cpp:2302-2322): the digits [dj0, dj1) of m
        // targets, extended to every row outside their bundle and transformed, into ext (digit-major); returns the rows the
        // inner product reads inside a bundle (the targets themselves, or their transform in coeff for STRICT BFV).
        // split_last (only ks_products asks for it, the other consumers need whole rows): the digit rows
        // are stored without the transform's last layer, as E | O, where every digit launch can take that form and the inner
        // product has its pair form for the batch -- KsRows::split_last says whether they were.
        struct KsRows
        {
            const u64 *inb;
            std::size_t inb_stride;
            bool split_last;
        };
        KsRows ks_digits(Engine &e, LevelTools &lt, int k, const u64 *tg, std::size_t target_stride, std::size_t m, u64 *coeff,
                         u64 *ext, int dj0, int dj1, bool split_last = false, bool plan_only = false)
        {
            const KsDev &h = lt.h_ks;
            const std::size_t N = e.n;
            const int rows = k + e.nsp;
            const bool ckks = e.scheme == 2;
            const bool strict_bfv = e.mode_strict && !ckks;
            const RowMap map_q = lt.map_q;
            const RowMap map_rows = lt.map_key;
            const std::size_t ext_item = static_cast<std::size_t>(rows) * N;
            const std::size_t ext_digit = ext_item * m; // digit-major
            // Step 1 (:2302-2307): CKKS bundles go back to coefficient form (canonical inverse NTT)
            const u64 *src = tg;
            std::size_t src_stride = target_stride;
            if (ckks && !plan_only) // (plan_only: no launch, only KsRows::split_last is computed; no pointer is followed)
            {
                // (valid ciphertext rows are below p and the canonicalising top kernel follows: any representative will do)
                if (ntt_can_gather(e)) // the inverse kernel reads the target rows where they are
                    check(launch_intt_from(e, coeff, tg, target_stride, m * k, map_q, kNttCanonical | kNttAnyRep),
                          "intt(target)");
                else
                {
                    check(launch_copy_rows(e, tg, target_stride, coeff, static_cast<std::size_t>(k) * N, m, k), "copy");
                    check(launch_ntt(e, coeff, m * k, map_q, true, kNttCanonical), "intt(target)");
                }
                src = coeff;
                src_stride = static_cast<std::size_t>(k) * N;
            }
            // Step 2 (:2310) + 3a (:2322): mod-up of every bundle, then the lazy forward NTT of every row outside
            // the bundle. With one special prime the mod-up of a row is a copy or a Barrett-63 reduction of the
            // bundle's single row (multi_special_primes.cpp:99-108): the NTT kernel gathers and reduces it on load,
            // so the extended polynomial is never written in coefficient form.
            const bool gather = e.nsp == 1 && ntt_can_gather(e);
            // launch-wide reduction of the gathered words: none when no source prime exceeds a destination prime, one
            // conditional subtraction when every source prime is below twice every destination prime, else Barrett-63
            bool need_any = false, need_barrett = false;
            for (int a = 0; a < k; a++)
                for (int b = 0; b < rows; b++)
                {
                    const u64 ps = e.key_moduli[h.row_prime[a]], pd = e.key_moduli[h.row_prime[b]];
                    need_any = need_any || (a != b && ps > pd);
                    need_barrett = need_barrett || (a != b && ps >= 2 * pd);
                }
            int modup_mode = need_barrett ? kTreatBarrett : (need_any ? kTreatCondSub : kTreatNone);
            if (modup_mode == kTreatCondSub)
            {
                // A gathered word is then below 2p of its destination prime. The lazy forward transform takes such an input
                // as it is (the first operand of a butterfly is never reduced before the last layer, the second goes through
                // mulmodLazy, ntt.cpp:245-261): with p < 2^58 nothing can wrap (2p(log n + 1) < 2^64), the extended
                // polynomial never leaves this function, and the inner product reduces to the canonical residue either
                // way -- so the conditional subtraction of all loaded words (6 % of the kernel's vector instructions, and
                // the kernel runs at the package power cap) is dropped. Larger primes keep it.
                u64 pmax = 0;
                for (int r = 0; r < rows; r++)
                    pmax = std::max(pmax, e.key_moduli[h.row_prime[r]]);
                if (bounds::fwd_lazy_admits(pmax, e.logn)) // (inputs below 2p: the case the recurrence in ntt_bounds.hpp walks)
                    modup_mode = kTreatNone;
            }
            if (!gather && !plan_only)
                check(launch_ks_modup(e, lt.d_ks, h, src, src_stride, ext, ext_item, ext_digit, m, -1), "modup");
            // digit j's launch: every row but the bundle's, each gathered from the bundle's single row
            const auto digit_map = [&](int j) {
                RowMap mj = map_rows;
                const int r0 = j * e.nsp, r1 = std::min(r0 + e.nsp, k);
                for (int r = r0; r < r1; r++)
                    mj.prime[r] = kSkipRow;
                return mj;
            };
            const auto digit_source = [&](int j) {
                NttSource ns{};
                ns.base[0] = src;
                ns.poly_stride[0] = src_stride;
                ns.reduce_mode = modup_mode;
                const u64 p_src = e.key_moduli[h.row_prime[j]];
                for (int r = 0; r < rows; r++)
                {
                    if (r == j)
                    {
                        ns.code[r] = kSkipRow;
                        continue;
                    }
                    const u64 p_dst = e.key_moduli[h.row_prime[r]];
                    ns.code[r] = static_cast<unsigned short>(j | (p_src <= p_dst ? 0 : kSrcReduce));
                }
                return ns;
            };
            // (the inner product reduces canonically: any representative of the transformed rows will do)
            const int digit_flags = kNttAnyRep | kNttApprox;
            split_last = split_last && gather && ks_mac_has_pair_form(e, h, m, dj0, dj1);
            for (int j = dj0; split_last && j < dj1; j++)
                split_last = ntt_can_split_last(e, digit_map(j), digit_source(j), digit_flags, h.nd);
            if (plan_only)
                return KsRows{ nullptr, 0, split_last };
            for (int j = dj0; j < dj1; j++)
            {
                const RowMap mj = digit_map(j);
                if (gather)
                    check(launch_ntt_gather(e, ext + j * ext_digit, m * rows, mj, digit_source(j), digit_flags | (split_last ? kNttSplitLast : 0)),
                          "ntt(ext, gathered)");
                else
                    check(launch_ntt(e, ext + j * ext_digit, m * rows, mj, false, kNttAnyRep), "ntt(ext)"); // (as above)
            }
            // in-bundle rows: the reference multiplies the target rows as they are (:2319-2320);
            // STRICT transforms the coefficient-form BFV rows first
            const u64 *inb = tg;
            std::size_t inb_stride = target_stride;
            if (strict_bfv)
            {
                if (ntt_can_gather(e))
                {
                    // the transform reads the target rows where they are (no copy pass); the inner product reduces canonically,
                    // so any representative of the transformed rows will do, as for the digit rows above
                    NttSource ns{};
                    ns.base[0] = tg;
                    ns.poly_stride[0] = target_stride;
                    for (int r = 0; r < k; r++)
                        ns.code[r] = static_cast<unsigned short>(r);
                    check(launch_ntt_gather(e, coeff, m * k, map_q, ns, kNttAnyRep | kNttApprox), "ntt(target, gathered)");
                }
                else
                {
                    check(launch_copy_rows(e, tg, target_stride, coeff, static_cast<std::size_t>(k) * N, m, k), "copy");
                    check(launch_ntt(e, coeff, m * k, map_q, false, 0), "ntt(target)");
                }
                inb = coeff;
                inb_stride = static_cast<std::size_t>(k) * N;
            }
            return KsRows{ inb, inb_stride, split_last };
        }

        // The front half of a key switch: ks_digits, then Step 3b + 4 (:2326-2349), the 128-bit inner product of the digits
        // [dj0, dj1) with the key, reduced, into prod[m][2][k + nsp][N]
        void ks_products(Engine &e, LevelTools &lt, int k, const u64 *tg, std::size_t target_stride, std::size_t m, u64 *coeff,
                         u64 *ext, const KSwitchKey &key, u64 *prod, int dj0, int dj1)
        {
            const std::size_t ext_item = static_cast<std::size_t>(k + e.nsp) * e.n;
            const KsRows in_bundle = ks_digits(e, lt, k, tg, target_stride, m, coeff, ext, dj0, dj1, true);
            check(launch_ks_mac(e, lt.d_ks, lt.h_ks, in_bundle.inb, in_bundle.inb_stride, ext, ext_item, ext_item * m /* digit-major */,
                                key.d_data, prod, 2 * ext_item, m, dj0, dj1, in_bundle.split_last),
                  "mac");
        }

        // The part after the inner product (evaluator.cpp:2351-2366): the m x 2 reduced products go through
        // rescale_special_rns_inplace and are added into the ciphertexts (or, with c0p, stored as (c0p + r0, r1)).
        // sink: the transparency flags of these m ciphertexts (null: none).
        // one_component: the same launches at polynomial granularity. prod is then component 1 of the
        // first of m products that lie 2 (k + nsp) N words apart (their components 0 are neither read nor written), ctp is
        // m polynomials of k rows back to back (ct_stride = 2 k N: the kernels' polynomial `pl` of ciphertext `pl >> 1`
        // lands on polynomial `pl`), temp holds m polynomials, and there is no c0p and no sink.
        void ks_finish(Engine &e, LevelTools &lt, int k, u64 *prod, u64 *temp, u64 *ctp, std::size_t ct_stride, const u64 *c0p,
                       std::size_t c0_stride, std::size_t m, unsigned *sink, bool one_component = false)
        {
            const KsDev &h = lt.h_ks;
            const std::size_t N = e.n;
            const int rows = k + e.nsp;
            const bool ckks = e.scheme == 2;
            const RowMap map_q = lt.map_q;
            const std::size_t ext_item = static_cast<std::size_t>(rows) * N;
            // what the transforms of prod walk: m x 2 polynomials of `rows` rows from prod on -- or, for one component, the
            // same rows from the skipped component 0 on, under a map of 2 * rows rows that leaves the first half alone
            RowMap map_rows = lt.map_key;
            u64 *const prod_rows = one_component ? prod - ext_item : prod;
            const std::size_t npolys = one_component ? m : 2 * m, prod_stride = one_component ? 2 * ext_item : ext_item;
            const int lead = one_component ? rows : 0; // rows of map_rows ahead of the polynomial's own
            if (one_component)
            {
                if (c0p || sink || ct_stride != 2 * static_cast<std::size_t>(k) * N || 2 * rows > kMaxRows)
                    throw std::logic_error("internal: one-component mod-down misused");
                map_rows.rows = 2 * rows;
                for (int r = 0; r < rows; r++)
                {
                    map_rows.prime[rows + r] = map_rows.prime[r];
                    map_rows.prime[r] = kSkipRow;
                }
            }
            if (!ckks)
            {
                // BFV: every row of both products goes back to coefficient form in one launch (the reference does the
                // special rows first, :2351-2355, and the others inside rescale_special_rns_inplace, :286-289 -- the
                // order of independent row transforms does not matter), then one fused mod-down kernel
                const bool defer = ntt_can_defer_top(e, k);
                // (ks_moddown_bfv reduces what it reads canonically: any representative below 2p will do)
                check(launch_ntt(e, prod_rows, m * 2 * rows, map_rows, true, (defer ? kNttDeferTop : 0) | kNttAnyRep), "intt(prod)");
                SinkArm arm(e, sink); // (component 1 of the m ciphertexts of this chunk)
                check(launch_ks_moddown_bfv(e, lt.d_ks, h, prod, prod_stride, ctp, ct_stride, npolys, defer, c0p, c0_stride),
                      "moddown_bfv");
                return;
            }
            const u64 p_special = (ckks && e.nsp == 1) ? e.key_moduli[h.row_prime[k]] : 0;
            // The gathered transform is handed the integer P - r < P instead of the residue (-(s mod P)) mod q_i: the same
            // word wherever P <= q_i; where q_i < P < 2 q_i it is an unreduced input below 2 q_i, which the lazy forward
            // transform takes as it is only while nothing can wrap (ntt_bounds.hpp section 2, inputs below 2p).
            bool fold_ok = ckks && e.nsp == 1 && ntt_can_gather(e);
            for (int r = 0; fold_ok && r < k; r++)
            {
                const u64 q = e.key_moduli[h.row_prime[r]];
                fold_ok = p_special <= q || (p_special < 2 * q && bounds::fwd_lazy_admits(q, e.logn));
            }
            const bool fold_pre = fold_ok;
            // the gathered transform below reads the special row as pairs (c, c + N/2): it can apply the top inverse layer
            const bool fold_top = fold_pre && ntt_can_defer_top(e, k);
            // ... and, in its floating-point form, finish the mod-down as it stores (kTreatModDownStore): temp is never written
            const bool fold_store = fold_top && ntt_can_fuse_moddown(e, k, p_special);
            // (:2351-2355) special rows back to coefficient form (lazy)
            // (the mod-down reduces the special rows with barrett_reduce_63 / a Shoup product: canonical either way)
            check(launch_ntt(e, prod_rows, m * 2 * rows, skip_map(map_rows, lead + k, lead + rows), true,
                             kNttAnyRep | (fold_top ? kNttDeferTop : 0)),
                  "intt(special)");
            // Step 5 (:2361): rescale_special_rns_inplace, then add into the ciphertext (:2363-2366)
            // Step 5 for CKKS with one special prime P: temp_i = (-(special mod P)) mod q_i, then its forward transform
            // (multi_special_primes.cpp:262-289). With the single-pass kernel the transform gathers the special row and forms
            // temp_i while it loads (kTreatNegSpecial): no pass that writes the k rows of temp, none that reads them back.
            if (fold_pre)
            {
                NttSource ns{};
                ns.base[0] = prod;
                ns.poly_stride[0] = prod_stride;
                ns.reduce_mode = fold_store ? kTreatModDownStore : (fold_top ? kTreatNegSpecialTop : kTreatNegSpecial);
                if (fold_store)
                {
                    ns.md.inv_p = lt.d_ks->invP; // (addresses inside the device copy of KsDev; not dereferenced here)
                    ns.md.inv_p_shoup = lt.d_ks->invP_shoup;
                    ns.md.prod = prod;
                    ns.md.prod_stride = prod_stride;
                    ns.md.ct = ctp;
                    ns.md.ct_stride = ct_stride;
                    ns.md.c0_src = c0p;
                    ns.md.c0_stride = c0_stride;
                    ns.md.tflags = sink;
                }
                ns.aux_p = p_special;
                ns.aux_cr1 = HostModulus(p_special).cr1;
                {
                    const HostNttTables &tb = e.tables[h.row_prime[k]];
                    ns.aux_top[0] = tb.inv_n;
                    ns.aux_top[1] = tb.inv_n_shoup;
                    ns.aux_top[2] = tb.inv_n_w;
                    ns.aux_top[3] = tb.inv_n_w_shoup;
                }
                for (int r = 0; r < k; r++)
                    ns.code[r] = static_cast<unsigned short>(k); // every row of temp reads the special row of its polynomial
                // (ks_moddown_post adds these rows to the q rows and reduces the sum canonically: any representative will do)
                check(launch_ntt_gather(e, temp, npolys * k, map_q, ns, kNttAnyRep), "ntt(temp, gathered from the special row)");
            }
            else
            {
                check(launch_ks_moddown_pre(e, lt.d_ks, h, prod, prod_stride, temp, static_cast<std::size_t>(k) * N, npolys),
                      "moddown_pre");
                if (ckks)
                    check(launch_ntt(e, temp, npolys * k, map_q, false, kNttAnyRep), "ntt(temp)"); // (moddown_post reduces the sum)
                else
                    check(launch_ntt(e, prod_rows, m * 2 * rows, skip_map(map_rows, lead, lead + k), true, kNttAnyRep), "intt(prod)");
            }
            if (!fold_store)
            {
                SinkArm arm(e, sink);
                check(launch_ks_moddown_post(e, lt.d_ks, h, prod, prod_stride, temp, static_cast<std::size_t>(k) * N, ctp,
                                             ct_stride, npolys, 1, c0p, c0_stride),
                      "moddown_post");
            }
        }

        // ks_finish merged with rescale_to_next (the words are those of tests/ks_rescale_ref.py):
        // out[m][2][k-1][N] = floor((P * base + acc + half) / (P * q_{k-1})), CKKS only. base: m items of two polynomials of k
        // rows (NTT form, canonical), base_stride words apart, read only. acc: the m x 2 reduced products, 2 (k + nsp) N
        // words per item; their dropped rows are overwritten. temp: 2 (k - 1) N words per item. The nsp + 1 dropped rows go
        // back to coefficient form in one launch, one kernel converts them to the k - 1 kept rows with the exact quotient,
        // those go forward, one kernel finishes: 2 (nsp + k) row transforms, and the level-k result is never formed.
        void ks_finish_rescale(Engine &e, LevelTools &lt, int k, const u64 *base, std::size_t base_stride, u64 *acc, u64 *temp,
                               u64 *out, std::size_t m, unsigned *sink)
        {
            if (e.scheme != 2 || k < 2 || !lt.d_ksr)
                throw std::logic_error("internal: merged rescale misused");
            const KsRescaleDev &h = lt.h_ksr;
            const std::size_t N = e.n;
            const int rows = k + e.nsp;
            const std::size_t ext_item = static_cast<std::size_t>(rows) * N;
            check(launch_ks_rescale_fold(e, lt.d_ksr, h, base, base_stride, acc, ext_item, 2 * m), "rescale_fold");
            // (the conversion adds half to canonical residues: the canonicalising inverse)
            check(launch_ntt(e, acc, m * 2 * rows, skip_map(lt.map_key, k - 1, rows), true, kNttCanonical), "intt(dropped)");
            check(launch_ks_moddown_rescale_pre(e, lt.d_ksr, h, acc, ext_item, temp, 2 * m), "moddown_rescale_pre");
            // the exact transform in both modes (PARITY's uncorrected butterflies may wrap on 60- and 61-bit primes, SURVEY
            // B.6, and there is no reference behaviour to reproduce for an operation the fork does not have); canonical,
            // because the post kernel subtracts these words from canonical residues
            check(launch_ntt(e, temp, m * 2 * (k - 1), e.level_host(k - 1).map_q, false, kNttCanonical | kNttStrict), "ntt(temp)");
            SinkArm arm(e, sink);
            check(launch_ks_moddown_rescale_post(e, lt.d_ksr, h, base, base_stride, acc, ext_item, temp, out, 2 * m),
                  "moddown_rescale_post");
        }
    } // namespace

    // sealhip_debug_ks_split_last: would ks_products store the digit rows of a chunk of `count` items at level k without the
    // transform's last layer? The decision ks_digits makes, with no launch.
    bool ks_split_last_plan(Engine &e, int k, std::size_t count)
    {
        LevelTools &lt = e.level(k);
        const u64 *const rows_not_read = reinterpret_cast<const u64 *>(&lt); // (a source is "gathered" by being non-null)
        return ks_digits(e, lt, k, rows_not_read, 0, count, const_cast<u64 *>(rows_not_read), nullptr, 0, lt.h_ks.nd, true, true).split_last;
    }

    // ------------------------------------------------------------------------------------------
    // switch_key_inplace (evaluator.cpp:2259-2368)
    // ------------------------------------------------------------------------------------------
    void op_switch_key(Engine &e, int k, u64 *ct, std::size_t ct_stride, const u64 *target, std::size_t target_stride,
                       std::size_t count, const KSwitchKey &key, const u64 *c0_src, std::size_t c0_stride, const KsSplit *split)
    {
        if (k > e.k_first)
            throw std::invalid_argument("key switching needs a ciphertext level");
        LevelTools &lt = e.level(k);
        const KsDev &h = lt.h_ks;
        const bool finish = split && split->partial_sum;   // latency mode, after the all-reduce
        const bool partial = split && split->partial_out;  // latency mode, before it
        if (!finish && (static_cast<int>(key.n_digits) < h.nd || (key.level && k > static_cast<int>(key.level))))
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
        const int dj0 = partial ? split->j0 : 0, dj1 = partial ? split->j1 : h.nd;
        if (dj0 < 0 || dj0 > dj1 || dj1 > h.nd)
            throw std::invalid_argument("digit range out of bounds");
        const int rows = k + e.nsp;
        const KsArena ar = switch_key_arena(e, k);
        const RowMap map_rows = lt.map_key;
        for_chunks(e, count, ar.item_bytes(), KsArena::n_buffers, [&](std::size_t off, std::size_t m) {
            u64 *coeff = ar.w_coeff ? e.ws_alloc(ar.w_coeff * m) : nullptr;
            u64 *ext = e.ws_alloc(ar.w_ext * m);
            u64 *prod = e.ws_alloc(ar.w_prod * m);
            u64 *temp = e.ws_alloc(ar.w_temp * m);
            if (partial)
                prod = split->partial_out + off * ar.w_prod;
            if (finish)
                prod = split->partial_sum + off * ar.w_prod;
            u64 *ctp = partial ? nullptr : ct + off * ct_stride;
            const u64 *c0p = c0_src ? c0_src + off * c0_stride : nullptr;

            if (finish)
                // the summed canonical partials (below ranks * p < 2^63) back to canonical residues: from here on every word
                // is what the unsplit inner product (:2341-2349) leaves
                check(launch_poly_op(e, PolyOp::Mod63, prod, nullptr, 0, prod, m * 2 * rows, map_rows), "mod(partial sum)");
            else
                ks_products(e, lt, k, target + off * target_stride, target_stride, m, coeff, ext, key, prod, dj0, dj1);
            if (partial)
                return; // the reduced partial products leave here (all-reduce, then op_switch_key with partial_sum)
            ks_finish(e, lt, k, prod, temp, ctp, ct_stride, c0p, c0_stride, m, sink_at(e, off));
        });
    }

    // The plain re-encryption under another secret: as op_apply_galois without the automorphism, the
    // key switch's last kernel writes (c_0 + r_0, r_1) straight into `out`.
    void op_switch_secret(Engine &e, int k, const u64 *c0, const u64 *c1, std::size_t stride, std::size_t count,
                          const KSwitchKey &key, u64 *out)
    {
        op_switch_key(e, k, out, 2 * static_cast<std::size_t>(k) * e.n, c1, stride, count, key, c0, stride);
    }

    // relinearize + rescale_to_next in one call: op_switch_key's front half, then the merged finish
    void op_switch_key_rescale(Engine &e, int k, const u64 *base, std::size_t base_stride, const u64 *target,
                               std::size_t target_stride, std::size_t count, const KSwitchKey &key, u64 *out)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("the merged rescale is a CKKS operation");
        if (k > e.k_first)
            throw std::invalid_argument("key switching needs a ciphertext level");
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached"); // evaluator.cpp:1005-1008
        LevelTools &lt = e.level_rescale(k);
        const KsDev &h = lt.h_ks;
        if (static_cast<int>(key.n_digits) < h.nd)
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
        const KsArena ar = switch_key_arena(e, k, true);
        for_chunks(e, count, ar.item_bytes(), KsArena::n_buffers, [&](std::size_t off, std::size_t m) {
            u64 *coeff = e.ws_alloc(ar.w_coeff * m);
            u64 *ext = e.ws_alloc(ar.w_ext * m);
            u64 *prod = e.ws_alloc(ar.w_prod * m);
            u64 *temp = e.ws_alloc(ar.w_temp * m);
            ks_products(e, lt, k, target + off * target_stride, target_stride, m, coeff, ext, key, prod, 0, h.nd);
            ks_finish_rescale(e, lt, k, base + off * base_stride, base_stride, prod, temp, out + off * ar.w_temp, m,
                              sink_at(e, off));
        });
    }

    // The double-angle step 2 x^2 - 1 of EvalMod: square_affine_kernel writes the size-3 ciphertext
    // 2 ct^2 + constant into the arena in one pass, and the merged key switch and rescale brings it to level k - 1. The wide
    // ciphertext is parked under a raised floor while the nested chunk loop runs, as op_dot_product parks its sum.
    void op_double_angle(Engine &e, int k, const u64 *ct, std::size_t count, const u64 *constant, const KSwitchKey &key, u64 *out)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("the merged rescale is a CKKS operation");
        if (k > e.k_first)
            throw std::invalid_argument("key switching needs a ciphertext level");
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached"); // evaluator.cpp:1005-1008
        LevelTools &lt = e.level_rescale(k);
        if (static_cast<int>(key.n_digits) < lt.h_ks.nd)
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
        const std::size_t N = e.n, poly_q = static_cast<std::size_t>(k) * N, w_wide = 3 * poly_q;
        const std::size_t ks_bytes = switch_key_arena(e, k, true).item_bytes();
        for_chunks(e, count, w_wide * sizeof(u64) + ks_bytes, 2 + KsArena::n_buffers, [&](std::size_t off, std::size_t m) {
            u64 *wide = e.ws_alloc(w_wide * m);
            FloorRestore guard(e);
            check(launch_square_affine(e, ct + off * 2 * poly_q, wide, m, lt.map_q, constant), "square_affine");
            guard.raise(pad256(w_wide * m));
            e.lane().tsink_base = guard.base + off; // (the nested chunk loop counts its items from this chunk's first ciphertext)
            op_switch_key_rescale(e, k, wide, w_wide, wide + 2 * poly_q, w_wide, m, key, out + off * 2 * (poly_q - N));
        });
    }

    // ModRaise: the q_0 rows of the batch go to coefficient form in the arena, the lift re-reads their
    // centred coefficients modulo q_1 .. q_(k_out-1) into the output's rows, which are then transformed in place; row 0 of
    // the output is the input's row 0, copied.
    void op_mod_raise(Engine &e, int k_in, const u64 *ct, std::size_t count, int k_out, u64 *out)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("ModRaise is a CKKS operation");
        if (k_in < 1 || k_in > e.k_first || k_out < 2 || k_out > e.k_first)
            throw std::invalid_argument("level k out of range");
        const std::size_t N = e.n, in_poly = static_cast<std::size_t>(k_in) * N, out_poly = static_cast<std::size_t>(k_out) * N;
        RowMap first{};
        first.rows = 1;
        first.prime[0] = 0;
        const RowMap raised = skip_map(e.level_host(k_out).map_q, 1, k_out);
        for_chunks(e, count, 2 * N * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *coef = e.ws_alloc(2 * N * m);
            const u64 *in = ct + off * 2 * in_poly;
            u64 *o = out + off * 2 * out_poly;
            check(launch_copy_rows(e, in, in_poly, coef, N, 2 * m, 1), "copy(q_0 rows)");
            check(launch_ntt(e, coef, 2 * m, first, true, kNttCanonical), "intt(q_0 rows)");
            check(launch_mod_raise_lift(e, coef, o, 2 * m, k_out), "mod_raise_lift");
            check(launch_ntt(e, o, 2 * m * k_out, raised, false, kNttCanonical), "ntt(raised rows)");
            check(launch_copy_rows(e, in, in_poly, o, out_poly, 2 * m, 1), "copy(row 0)");
        });
    }

    // modup_rns as a standalone operation (multi_special_primes.cpp:151-185)
    void op_modup(Engine &e, int k, int bundle, u64 *ext, std::size_t count)
    {
        LevelTools &lt = e.level(k);
        if (k > e.k_first || bundle < 0 || bundle >= lt.h_ks.nd)
            throw std::invalid_argument("modup_rns: src_bundle_index out of bound");
        const std::size_t stride = static_cast<std::size_t>(k + e.nsp) * e.n;
        check(launch_ks_modup(e, lt.d_ks, lt.h_ks, ext, stride, ext, stride, 0, count, bundle), "modup");
    }

    // rescale_special_rns_inplace as a standalone operation (multi_special_primes.cpp:237-304)
    void op_rescale_special_inplace(Engine &e, int k, u64 *poly, std::size_t count)
    {
        if (k > e.k_first)
            throw std::invalid_argument("rescale_special needs a ciphertext level");
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n;
        const int rows = k + e.nsp;
        const std::size_t per_item = static_cast<std::size_t>(k) * N * sizeof(u64);
        for_chunks(e, count, per_item, 1, [&](std::size_t off, std::size_t m) {
            u64 *temp = e.ws_alloc(static_cast<std::size_t>(k) * N * m);
            u64 *p = poly + off * rows * N;
            check(launch_ks_moddown_pre(e, lt.d_ks, lt.h_ks, p, static_cast<std::size_t>(rows) * N, temp,
                                        static_cast<std::size_t>(k) * N, m),
                  "moddown_pre");
            if (e.scheme == 2)
                check(launch_ntt(e, temp, m * k, lt.map_q, false, 0), "ntt(temp)");
            else
                check(launch_ntt(e, p, m * rows, skip_map(lt.map_key, 0, k), true, 0), "intt(poly)");
            check(launch_ks_moddown_post(e, lt.d_ks, lt.h_ks, p, static_cast<std::size_t>(rows) * N, temp,
                                         static_cast<std::size_t>(k) * N, nullptr, 0, m, 0),
                  "moddown_post");
        });
    }

    // ------------------------------------------------------------------------------------------
    // bfv_multiply (evaluator.cpp:274-445)
    // ------------------------------------------------------------------------------------------
    // b == nullptr: bfv_square of a size-2 ciphertext (evaluator.cpp:560-702) -- the two polynomials of `a` are lifted and
    // transformed once (:604-634) and the tensor product is c_0 = x_0^2, c_1 = x_0 x_1 added to itself, c_2 = x_1^2
    // (:644-657); everything after it is bfv_multiply's tail.
    BfvMulPlan plan_bfv_multiply(Engine &e, int k, int sa, int sb, bool square)
    {
        if (e.scheme != 1)
            throw std::invalid_argument("plan_bfv_multiply: BFV contexts only");
        if (sa < 2 || sb < 2 || (square && (sa != 2 || sb != 2)))
            throw std::invalid_argument("plan_bfv_multiply: operand sizes (the square path takes size-2 operands)");
        LevelTools &lt = e.level_host(k);
        const HostRnsTool &hr = *lt.host_rns;
        BfvMulPlan p{};
        p.k = k;
        p.B = static_cast<int>(hr.B_size);
        p.nB = static_cast<int>(hr.Bsk.size());
        p.square = square;
        u64 max_q = 0, max_b = 0;
        for (int i = 0; i < k; i++)
            max_q = std::max(max_q, hr.q[i]);
        for (int j = 0; j < p.nB; j++)
            max_b = std::max(max_b, hr.Bsk[j]);
        p.redc_small = bounds::behz_redc_small(k, p.B, max_q, max_b);
        const int kb = k + p.nB, sin = square ? sa : sa + sb, dest = sa + sb - 1;
        // steps (1)-(3) (:335-353): the q rows are gathered straight from the operands by the forward NTT (no set_poly copy)
        // when the single-pass kernel is available and one launch can describe all sin * (k + |Bsk|) rows of an item
        p.gather = ntt_can_gather(e) && sin * kb <= kMaxRows;
        // the single-pass inverse leaves its top layer (and the canonicalisation) to bfv_floor_sk, which applies it on load
        p.defer = ntt_can_defer_top(e, k);
        // with two size-2 operands the tensor product (step 4) is formed by the inverse NTT while it loads its rows (no
        // separate pass over 7 rows per prime; launch_intt_tensor). Its Montgomery reduction lands below 2p on operands below
        // 4p for ciphertext primes under 2^59 (the exact forward sequence), on operands below (2 + g) p -- what an
        // approximate-quotient launch without kNttAnyRep stores -- for primes under 2^57 (ntt_bounds.hpp section 3:
        // tensor_admits_apx); the Bsk rows are stored below 2p
        p.fused_tensor = p.gather && p.defer && sa == 2 && sb == 2 && dest * kb <= kMaxRows;
        p.tensor_apx = true;
        for (int r = 0; r < k; r++)
        {
            p.fused_tensor = p.fused_tensor && bounds::tensor_admits_4p(e.key_moduli[r]);
            p.tensor_apx = p.tensor_apx && bounds::tensor_admits_apx(e.key_moduli[r]);
        }
        for (int j = 0; j < p.nB; j++)
            p.fused_tensor = p.fused_tensor && bounds::tensor_admits_2p(e.tables[lt.map_qbsk.prime[k + j]].p);
        // the lift applies the forward transform's top layer to the Bsk rows it writes (kNttTopDone)
        p.lift_top = p.fused_tensor && bfv_lift_can_apply_top(e, k, p.redc_small);
        if (p.lift_top && e.mode_strict)
        {
            RowMap bsk{};
            bsk.rows = p.nB;
            for (int j = 0; j < p.nB; j++)
                bsk.prime[j] = lt.map_qbsk.prime[k + j];
            p.lift_top = ntt_strict_top_done_ok(e, bsk);
        }
        // the fused kernels: an exact-k instance where every REDC provably lands below 2p, else the run-time-k one; past
        // k = 32 the step-by-step kernels (rns.hip launch_bfv_lift / launch_bfv_floor_sk)
        const int code = k > 32 ? kBehzStepwise : p.redc_small && k <= bounds::kBehzExactMaxK ? k : kBehzGeneric;
        p.lift_kernel = p.floor_kernel = code;
        p.deferred_top = p.fused_tensor ? 2 : p.defer ? 1 : 0;
        return p;
    }

    namespace
    {
        // bfv_multiply's steps (1)-(3) (:335-353) for m items: the sa polynomials of a, then the sb of b (null: none, the
        // square), are lifted to Bsk (fastbconv_m_tilde + sm_mrq) and all rows go to NTT form (lazy), into
        // X[m][sin][k + |Bsk|][N]. a, b: the first item's polynomials of k rows, items back to back.
        void bfv_lift_and_transform(Engine &e, LevelTools &lt, const BfvMulPlan &plan, const u64 *a, int sa, const u64 *b, int sb,
                                    u64 *X, std::size_t m)
        {
            const RnsDev &h = lt.h_rns;
            const int k = plan.k, kb = k + plan.nB, sin = b ? sa + sb : sa;
            const std::size_t poly_q = static_cast<std::size_t>(k) * e.n, poly_x = static_cast<std::size_t>(kb) * e.n;
            const std::size_t w_x = sin * poly_x;
            for (int s = 0; s < sin; s++)
            {
                const bool first = s < sa;
                const u64 *src = first ? a + s * poly_q : b + (s - sa) * poly_q;
                const std::size_t src_stride = (first ? sa : sb) * poly_q;
                u64 *dst = X + s * poly_x;
                if (!plan.gather)
                    check(launch_copy_rows(e, src, src_stride, dst, w_x, m, k), "copy");
                check(launch_bfv_lift(e, lt.d_rns, h, src, src_stride, dst + poly_q, w_x, m, plan), "bfv_lift");
            }
            if (!plan.gather)
            {
                // (the tensor product reduces whatever it reads, polyarithsmallmod.cpp:63-117; the 60-bit Bsk rows keep the
                //  reference's wrapped words either way: launch_half / the pass kernels only use the freedom on small primes)
                check(launch_ntt(e, X, m * sin * kb, lt.map_qbsk, false, kNttAnyRep), "ntt(X)");
                return;
            }
            // one "polynomial" of the launch = all sin*(k+|Bsk|) rows of an item; the q rows are gathered from the operands
            NttSource ns{};
            ns.base[0] = a;
            ns.base[1] = b;
            ns.poly_stride[0] = sa * poly_q;
            ns.poly_stride[1] = sb * poly_q;
            for (int s = 0; s < sin; s++)
                for (int r = 0; r < kb; r++)
                {
                    unsigned short code = kSkipRow; // Bsk rows: in place (written by bfv_lift)
                    if (r < k)
                        code = static_cast<unsigned short>((s < sa ? 0 : kSrcSecond) | ((s < sa ? s : s - sa) * k + r));
                    ns.code[s * kb + r] = code;
                }
            // two launches over disjoint rows: the q rows only feed the tensor product, which reduces canonically, so
            // their last layer may skip its Barrett step (kNttAnyRep); the 60-bit Bsk rows wrap in the reference (F2)
            // and keep its exact sequence. (The fused tensor product multiplies the q rows without reducing them first
            // and needs them below 5p: there the last layer keeps its Barrett step.) kNttApprox: the approximate Shoup
            // quotient where every prime is below 2^58 (one multiplier instruction less per butterfly).
            const QBskMaps maps = split_q_bsk(lt.map_qbsk, k, sin);
            check(launch_ntt_gather(e, X, m * sin * kb, maps.q, ns,
                                    plan.fused_tensor ? (plan.tensor_apx ? kNttApprox : 0) : (kNttAnyRep | kNttApprox)),
                  "ntt(X, gathered q rows)");
            // (fused tensor product: the wrapped Bsk words are brought below 2p as they are stored -- the residue class
            //  is all the dyadic product depends on)
            // (kNttAnyRep next to kNttReduceOut: "any representative below 2p will do". PARITY launches drop it on these
            //  60-bit primes and keep the reference's words; STRICT launches take the dense lazy schedule with it, launch_half)
            check(launch_ntt(e, X, m * sin * kb, maps.bsk, false,
                             plan.fused_tensor ? (kNttReduceOut | kNttAnyRep | (plan.lift_top ? kNttTopDone : 0)) : 0),
                  "ntt(X, Bsk rows)");
        }

        // where one polynomial of the product goes: items `stride` words apart, and its items' transparency flags (null:
        // not a polynomial 1.. of the result)
        struct BfvFloorDst
        {
            u64 *dst;
            std::size_t stride;
            unsigned *sink;
        };
        // steps (6)-(8) (:427-444): one floor per polynomial of D[m][dest][k + |Bsk|][N]
        void bfv_floors(Engine &e, LevelTools &lt, const BfvMulPlan &plan, u64 *D, int dest, std::size_t m, const BfvFloorDst *to)
        {
            const std::size_t poly_x = static_cast<std::size_t>(plan.k + plan.nB) * e.n;
            for (int I = 0; I < dest; I++)
            {
                SinkArm arm(e, to[I].sink);
                check(launch_bfv_floor_sk(e, lt.d_rns, lt.h_rns, D + I * poly_x, dest * poly_x, to[I].dst, to[I].stride, m, plan),
                      "floor_sk");
            }
        }
        // the unfused path's step (5) (:423-424), then the floors; with the single-pass kernels the top inverse layer and
        // the canonicalisation are applied by the consumer while it loads (saves one read+write pass over D)
        void bfv_inverse_and_floors(Engine &e, LevelTools &lt, const BfvMulPlan &plan, u64 *D, int dest, std::size_t m,
                                    const BfvFloorDst *to)
        {
            const int kb = plan.k + plan.nB;
            if (plan.defer)
            {
                // two launches over disjoint rows: the q rows may store any representative (bfv_floor_sk canonicalises
                // while it applies the deferred top layer), which lets the kernel drop most conditional subtractions
                // (sparse lazy schedule); so may the 60-bit Bsk rows, which take the dense schedule (round 4)
                const QBskMaps maps = split_q_bsk(lt.map_qbsk, plan.k, 1);
                check(launch_ntt(e, D, m * dest * kb, maps.q, true, kNttDeferTop | kNttAnyRep), "intt(D, q rows)");
                check(launch_ntt(e, D, m * dest * kb, maps.bsk, true, kNttDeferTop | kNttAnyRep), "intt(D, Bsk rows)");
            }
            else
                check(launch_ntt(e, D, m * dest * kb, lt.map_qbsk, true, kNttCanonical), "intt(D)");
            bfv_floors(e, lt, plan, D, dest, m, to);
        }
    } // namespace

    void op_bfv_multiply(Engine &e, int k, const u64 *a, int sa, const u64 *b, int sb, std::size_t count, u64 *out)
    {
        LevelTools &lt = e.level(k);
        const RnsDev &h = lt.h_rns;
        const std::size_t N = e.n;
        const bool sq = b == nullptr;
        if (sq && (sa != 2 || sb != 2))
            throw std::logic_error("op_bfv_multiply: the square path takes size-2 operands");
        const BfvMulPlan plan = plan_bfv_multiply(e, k, sa, sb, sq);
        if (plan.nB != h.nB || plan.redc_small != (h.redc_small != 0))
            throw std::logic_error("op_bfv_multiply: the plan and the level's device constants disagree");
        const int nB = h.nB, kb = k + nB, sin = sq ? sa : sa + sb, dest = sa + sb - 1;
        const std::size_t w_x = static_cast<std::size_t>(sin) * kb * N;
        const std::size_t w_d = static_cast<std::size_t>(dest) * kb * N;
        const std::size_t poly_q = static_cast<std::size_t>(k) * N, poly_x = static_cast<std::size_t>(kb) * N;
        std::vector<BfvFloorDst> to(dest);
        for_chunks(e, count, (w_x + w_d) * sizeof(u64), 2, [&](std::size_t off, std::size_t m) {
            u64 *X = e.ws_alloc(w_x * m);
            u64 *D = e.ws_alloc(w_d * m);
            bfv_lift_and_transform(e, lt, plan, a + off * sa * poly_q, sa, sq ? nullptr : b + off * sb * poly_q, sb, X, m);
            for (int I = 0; I < dest; I++) // (the sink: polynomials 1.. of the product)
                to[I] = BfvFloorDst{ out + off * dest * poly_q + I * poly_q, dest * poly_q, I >= 1 ? sink_at(e, off) : nullptr };
            if (plan.fused_tensor)
            {
                // steps (4) + (5) (:376-424): D[I] = inverse NTT of sum_{i1+i2=I} X[i1] (.) X[2+i2], top layer deferred, every
                // word with the Montgomery factor 2^-64 that bfv_floor_sk's constants undo. q rows: lazy sums (any
                // representative, sparse schedule); Bsk rows: operands reduced on load, the dense lazy schedule
                const QBskMaps maps = split_q_bsk(lt.map_qbsk, k, dest);
                check(launch_intt_tensor(e, D, X, w_x, poly_x, kb, m * dest * kb, maps.q, kNttDeferTop | kNttAnyRep, sq),
                      "intt(tensor, q rows)");
                // (round 4: the Bsk rows may store any representative below 2p as well -- the fused floor (bfv_floor_sk_exact / _guarded) takes u, v below 2p and
                //  canonicalises; the launcher then runs the DENSE lazy schedule on the 60-bit primes, ntt_bounds.hpp section 1)
                check(launch_intt_tensor(e, D, X, w_x, poly_x, kb, m * dest * kb, maps.bsk, kNttDeferTop | kNttAnyRep, sq),
                      "intt(tensor, Bsk rows)");
                bfv_floors(e, lt, plan, D, dest, m, to.data());
                return;
            }
            // step (4) (:376-420)
            // (square: both operands are the same two transformed polynomials; the kernel then forms x_0 x_1 once and adds it
            //  to itself, :650-651)
            check(launch_tensor_product(e, X, sa, w_x, sq ? X : X + sa * poly_x, sb, w_x, D, w_d, m, lt.map_qbsk, sq), "tensor");
            bfv_inverse_and_floors(e, lt, plan, D, dest, m, to.data());
        });
    }

    void op_bfv_square(Engine &e, int k, const u64 *a, int sa, std::size_t count, u64 *out)
    {
        if (sa != 2)
            return op_bfv_multiply(e, k, a, sa, a, sa, count, out); // evaluator.cpp:579-583
        op_bfv_multiply(e, k, a, 2, nullptr, 2, count, out);
    }

    // ckks_square (evaluator.cpp:704-770) is its own path, like bfv_square: a size-2 operand goes through the tensor
    // kernel's square form -- c_0 = x_0^2, c_1 = x_0 x_1 added to itself (:752-758), c_2 = x_1^2: two polynomials read and
    // three written (five row passes per prime instead of seven), three products per coefficient instead of four; other
    // sizes go through ckks_multiply like the reference (:720-724). Parity: ref_ckks_square (oracle/sealref.c).
    void op_ckks_square(Engine &e, int k, const u64 *a, int sa, std::size_t count, u64 *out)
    {
        if (sa != 2)
            return op_ckks_multiply(e, k, a, sa, a, sa, count, out);
        LevelTools &lt = e.level(k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        SinkArm arm(e, sink_at(e, 0));
        check(launch_tensor_product(e, a, 2, 2 * poly, a, 2, 2 * poly, out, 3 * poly, count, lt.map_q, true), "tensor (square)");
    }

    // ckks_multiply (evaluator.cpp:447-527)
    void op_ckks_multiply(Engine &e, int k, const u64 *a, int sa, const u64 *b, int sb, std::size_t count, u64 *out)
    {
        LevelTools &lt = e.level(k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        SinkArm arm(e, sink_at(e, 0));
        check(launch_tensor_product(e, a, sa, sa * poly, b, sb, sb * poly, out, (sa + sb - 1) * poly, count, lt.map_q),
              "tensor");
    }

    // ------------------------------------------------------------------------------------------
    // Ciphertext inner product: sum_i a_i * b_i, one floor (BFV), one key switch
    // ------------------------------------------------------------------------------------------
    std::uint64_t dot_product_max_terms(Engine &e, int k)
    {
        if (e.scheme == 2)
            return 0xFFFFFFFFull; // (modular sums of canonical residues: any number of terms)
        return e.level_host(k).host_rns->dot_max_terms();
    }

    // The tensor products of all terms are summed in NTT form by tensor_dot_kernel, in groups of up to kDotGroup terms
    // (later groups add the canonical partial sum in). CKKS reads the operands where they are. BFV (STRICT) lifts and
    // transforms every term into the extended base q u Bsk with the launches of op_bfv_multiply's unfused path (steps 1-3),
    // holds a group of terms in the arena, and sends the SUM through that path's tail once: one inverse transform of
    // 3 (k + |Bsk|) rows and three floors, whatever the number of terms. With a key the sum's c_2 stays in the arena and the
    // key switch adds its two polynomials into (c_0, c_1) in `out`.
    // rescale (CKKS with a key): (c_0, c_1) of the sum stay in the arena next to c_2 and
    // op_switch_key_rescale writes out[count][2][k-1][N].
    void op_dot_product(Engine &e, int k, const u64 *const *a, const u64 *const *b, std::size_t n_terms, std::size_t count,
                        const KSwitchKey *key, u64 *out, bool rescale)
    {
        if (k > e.k_first)
            throw std::invalid_argument("the inner product needs a ciphertext level");
        const bool ckks = e.scheme == 2;
        if (rescale && (!ckks || !key))
            throw std::invalid_argument("the merged rescale is a CKKS operation and needs relinearization keys");
        if (rescale && k < 2)
            throw std::invalid_argument("end of modulus switching chain reached");
        if (!ckks && !e.mode_strict)
            // (as for the hoisted entries: the fork's BFV key switch does not decrypt, and there is no reference behaviour to
            //  reproduce for an operation the fork does not have)
            throw std::invalid_argument("the inner product of BFV ciphertexts needs a STRICT context");
        if (n_terms == 0 || n_terms > dot_product_max_terms(e, k))
            throw std::invalid_argument("number of terms out of range");
        LevelTools &lt = e.level(k);
        if (key && static_cast<int>(key->n_digits) < lt.h_ks.nd)
            throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
        const std::size_t N = e.n, poly_q = static_cast<std::size_t>(k) * N;
        const std::size_t out_item = (key ? 2 : 3) * poly_q;
        const std::size_t ks_bytes = key ? switch_key_arena(e, k, rescale).item_bytes() : 0;
        const std::size_t w_c2 = key ? poly_q : 0;
        const std::size_t w_c01 = rescale ? 2 * poly_q : 0; // (c_0, c_1) of the sum, when out is the level below
        // BFV: X holds a group of terms (4 polynomials of k + |Bsk| rows each), D the sum (3 polynomials)
        BfvMulPlan plan{};
        int kb = k;
        if (!ckks)
        {
            plan = plan_bfv_multiply(e, k, 2, 2, false);
            if (plan.nB != lt.h_rns.nB || plan.redc_small != (lt.h_rns.redc_small != 0))
                throw std::logic_error("op_dot_product: the plan and the level's device constants disagree");
            plan.fused_tensor = plan.lift_top = false; // (the unfused path: the sum is formed between the transforms)
            plan.deferred_top = plan.defer ? 1 : 0;
            kb = k + plan.nB;
        }
        const std::size_t poly_x = static_cast<std::size_t>(kb) * N;
        const std::size_t w_x = ckks ? 0 : 4 * poly_x, w_d = ckks ? 0 : 3 * poly_x;
        // terms held at once: a full group unless the arena cannot take one item with it; D carries the canonical partial
        // sum from one group to the next, so a pass over fewer terms is simply a smaller group
        std::size_t group = std::min<std::size_t>(kDotGroup, n_terms);
        if (!ckks)
            group = plan_pass(e, (w_c2 + w_d) * sizeof(u64), w_x * sizeof(u64), group, n_terms); // (logs the term split)
        const std::size_t work_bytes = (group * w_x + w_d) * sizeof(u64);
        // c_2 must survive op_switch_key, which re-plans the arena: it is carved first and the floor raised over it; the
        // item's bytes cover the larger of this operation's temporaries and the key switch's, so the nested plan fits what
        // is reserved here and the arena cannot move while c_2 is live
        for_chunks(e, count, (w_c2 + w_c01) * sizeof(u64) + std::max(work_bytes, ks_bytes), rescale ? 7 : 6,
                   [&](std::size_t off, std::size_t m) {
            u64 *c2 = key ? e.ws_alloc(w_c2 * m) : nullptr;
            u64 *c01 = rescale ? e.ws_alloc(w_c01 * m) : nullptr;
            FloorRestore guard(e);
            u64 *o = rescale ? c01 : out + off * out_item;
            unsigned *const flags = sink_at(e, off);
            if (ckks)
            {
                for (std::size_t g0 = 0; g0 < n_terms; g0 += group)
                {
                    DotTerms terms{};
                    terms.n = static_cast<int>(std::min(group, n_terms - g0));
                    for (int t = 0; t < terms.n; t++)
                    {
                        terms.a[t] = a[g0 + t] + off * 2 * poly_q;
                        terms.b[t] = b[g0 + t] + off * 2 * poly_q;
                    }
                    // (the flags describe the result: only the last group's stores are the result's words)
                    SinkArm arm(e, !key && g0 + group >= n_terms ? flags : nullptr);
                    check(launch_tensor_dot(e, terms, 2 * poly_q, 2 * poly_q, o, out_item, key ? c2 : o + 2 * poly_q,
                                            key ? poly_q : out_item, m, lt.map_q, false, g0 > 0),
                          "tensor_dot");
                }
            }
            else
            {
                u64 *X = e.ws_alloc(group * w_x * m);
                u64 *D = e.ws_alloc(w_d * m);
                for (std::size_t g0 = 0; g0 < n_terms; g0 += group)
                {
                    DotTerms terms{};
                    terms.n = static_cast<int>(std::min(group, n_terms - g0));
                    for (int t = 0; t < terms.n; t++)
                    {
                        // steps (1)-(3) for term g0 + t (tensor_dot_kernel reduces what it loads: the plan's unfused flags)
                        u64 *Xt = X + static_cast<std::size_t>(t) * w_x * m;
                        bfv_lift_and_transform(e, lt, plan, a[g0 + t] + off * 2 * poly_q, 2, b[g0 + t] + off * 2 * poly_q, 2, Xt, m);
                        terms.a[t] = Xt;
                        terms.b[t] = Xt + 2 * poly_x;
                    }
                    // step (4), summed over the group's terms; the operands are lazily transformed words
                    check(launch_tensor_dot(e, terms, w_x, w_x, D, w_d, D + 2 * poly_x, w_d, m, lt.map_qbsk, true, g0 > 0),
                          "tensor_dot");
                }
                // step (5) ONCE for the sum, and three floors: with a key c_2 goes to the arena and nothing is flagged here
                unsigned *const f = key ? nullptr : flags;
                const BfvFloorDst to[3] = { { o, out_item, nullptr },
                                            { o + poly_q, out_item, f },
                                            { key ? c2 : o + 2 * poly_q, key ? poly_q : out_item, f } };
                bfv_inverse_and_floors(e, lt, plan, D, 3, m, to);
            }
            if (key)
            {
                // relinearize_internal (evaluator.cpp:811-815) of the sum: (c_0, c_1) += key switch of c_2
                guard.raise(pad256(w_c2 * m) + (rescale ? pad256(w_c01 * m) : 0));
                e.lane().tsink_base = guard.base + off; // (the nested chunk loop counts its items from this chunk's first ciphertext)
                if (rescale)
                    op_switch_key_rescale(e, k, c01, 2 * poly_q, c2, poly_q, m, *key, out + off * 2 * (poly_q - N));
                else
                    op_switch_key(e, k, o, 2 * poly_q, c2, poly_q, m, *key);
            }
        });
    }

    // ------------------------------------------------------------------------------------------
    // Linear combinations with scalar weights: out_s = sum_i W[s][i] * X_i (+ K[s] on c_0)
    // ------------------------------------------------------------------------------------------
    // lincomb_kernel reads the operands where they are and writes the sums where they belong: nothing comes from the arena.
    // Sums go in tiles of kLinTile, terms in groups of kLinGroup; a later group adds the canonical partial sum in, and the
    // last group adds the constant and notes the transparency flags (sum-major, as the output is).
    void op_linear_combination(Engine &e, int k, const u64 *const *terms, std::size_t n_terms, int size, std::size_t count,
                               const u64 *weights, const u64 *constant, std::size_t n_sums, u64 *out)
    {
        if (k > e.k_first)
            throw std::invalid_argument("the linear combination needs a ciphertext level");
        if (n_terms == 0 || n_sums == 0 || size < 2)
            throw std::invalid_argument("an empty linear combination");
        LevelTools &lt = e.level(k);
        const std::size_t item = static_cast<std::size_t>(size) * k * e.n;
        if (n_terms > static_cast<std::size_t>(kLinGroup))
            log_chunk(e, n_terms, kLinGroup); // (the term split, ahead of the operation's item chunks: sealhip_debug_chunk_log)
        for_chunks(e, count, 0, 0, [&](std::size_t off, std::size_t m) {
            for (std::size_t s0 = 0; s0 < n_sums; s0 += kLinTile)
                for (std::size_t g0 = 0; g0 < n_terms; g0 += kLinGroup)
                {
                    LinTerms group{};
                    group.n = static_cast<int>(std::min<std::size_t>(kLinGroup, n_terms - g0));
                    for (int t = 0; t < group.n; t++)
                        group.x[t] = terms[g0 + t] + off * item;
                    const bool last = g0 + kLinGroup >= n_terms; // (only the last group's stores are the result's words)
                    SinkArm arm(e, last ? sink_at(e, s0 * count + off) : nullptr);
                    check(launch_lincomb(e, group, size, item, weights + (s0 * n_terms + g0) * k, n_terms * k,
                                         last && constant ? constant + s0 * k : nullptr, e.scheme == 2 ? 2 : 1,
                                         out + (s0 * count + off) * item, count * item,
                                         static_cast<int>(std::min<std::size_t>(kLinTile, n_sums - s0)), m, lt.map_q, g0 > 0, count),
                          "lincomb");
                }
        });
    }

    // The same over terms at their own level and size: CKKS, where a ciphertext at level levels[i] >= k
    // holds the level-k ciphertext in its first k rows, and a term of sizes[i] <= size polynomials stands for the one padded
    // with zero polynomials. lincomb_levels_kernel reads every term in place at its own strides: no row copy, no arena.
    void op_linear_combination_levels(Engine &e, int k, const u64 *const *terms, const std::uint32_t *levels,
                                      const std::uint32_t *sizes, std::size_t n_terms, int size, std::size_t count,
                                      const u64 *weights, const u64 *constant, std::size_t n_sums, u64 *out)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("terms at their own level are CKKS only");
        if (k > e.k_first)
            throw std::invalid_argument("the linear combination needs a ciphertext level");
        if (n_terms == 0 || n_sums == 0 || size < 2)
            throw std::invalid_argument("an empty linear combination");
        LevelTools &lt = e.level(k);
        const std::size_t item = static_cast<std::size_t>(size) * k * e.n;
        if (n_terms > static_cast<std::size_t>(kLinGroup))
            log_chunk(e, n_terms, kLinGroup); // (the term split, ahead of the operation's item chunks: sealhip_debug_chunk_log)
        for_chunks(e, count, 0, 0, [&](std::size_t off, std::size_t m) {
            for (std::size_t s0 = 0; s0 < n_sums; s0 += kLinLevelsTile)
                for (std::size_t g0 = 0; g0 < n_terms; g0 += kLinGroup)
                {
                    LinLevelTerms group{};
                    group.n = static_cast<int>(std::min<std::size_t>(kLinGroup, n_terms - g0));
                    for (int t = 0; t < group.n; t++)
                    {
                        const std::size_t i = g0 + t;
                        if (static_cast<int>(levels[i]) < k || static_cast<int>(levels[i]) > e.k_first || sizes[i] < 2 ||
                            static_cast<int>(sizes[i]) > size)
                            throw std::invalid_argument("a term's level or size does not admit the sum's");
                        group.x[t] = terms[i] + off * sizes[i] * levels[i] * e.n;
                        group.rows[t] = static_cast<unsigned char>(levels[i]);
                        group.size[t] = static_cast<unsigned char>(sizes[i]);
                    }
                    const bool last = g0 + kLinGroup >= n_terms; // (only the last group's stores are the result's words)
                    SinkArm arm(e, last ? sink_at(e, s0 * count + off) : nullptr);
                    check(launch_lincomb_levels(e, group, size, item, weights + (s0 * n_terms + g0) * k, n_terms * k,
                                                last && constant ? constant + s0 * k : nullptr, 2, out + (s0 * count + off) * item,
                                                count * item, static_cast<int>(std::min<std::size_t>(kLinLevelsTile, n_sums - s0)),
                                                m, lt.map_q, g0 > 0, count),
                          "lincomb_levels");
                }
        });
    }

    // ------------------------------------------------------------------------------------------
    // mod_switch_scale_to_next (evaluator.cpp:829-892): BFV mod_switch_to_next / CKKS rescale_to_next
    // ------------------------------------------------------------------------------------------
    namespace
    {
        void mod_switch_polys(Engine &e, int k, const u64 *ct, std::size_t in_stride, u64 *out, std::size_t out_stride,
                              std::size_t npolys, bool exact = false);
    }
    // in_item_stride (words, 0 = the ciphertexts are back to back): distance between consecutive ciphertexts of `ct` when they
    // sit in a wider container -- the size-2 result of relinearize inside its size-3 product (the reference's objects are
    // separate buffers; a contiguous batch needs the stride). Each component is then one strided pass.
    void op_mod_switch_scale(Engine &e, int k, const u64 *ct, int size, std::size_t count, u64 *out, std::size_t in_item_stride)
    {
        if (k < 2)
            throw std::invalid_argument("end of modulus switching chain reached"); // evaluator.cpp:1005-1008
        const std::size_t N = e.n;
        const std::size_t in_poly = static_cast<std::size_t>(k) * N, out_poly = static_cast<std::size_t>(k - 1) * N;
        if (in_item_stride == 0 || in_item_stride == size * in_poly)
            return mod_switch_polys(e, k, ct, in_poly, out, out_poly, count * size);
        if (in_item_stride < size * in_poly)
            throw std::invalid_argument("item stride smaller than one ciphertext");
        for (int comp = 0; comp < size; comp++)
            mod_switch_polys(e, k, ct + comp * in_poly, in_item_stride, out + comp * out_poly, size * out_poly, count);
    }

    namespace
    {
    // The CKKS division by the last prime of level k (rns.cpp:777-851) up to its forward transforms; lt = e.level(k).
    // rescale_temp: from the coefficient-form last rows of npolys polynomials (last_stride words apart) to their correction
    // over the k - 1 remaining primes in temp[npolys][k - 1][N], lazily transformed (rescale_post reduces).
    // ntt_flags: kNttStrict asks for the exact transform whatever the context's mode
    void rescale_temp(Engine &e, LevelTools &lt, int k, u64 *last, std::size_t last_stride, std::size_t npolys, u64 *temp,
                      int ntt_flags = 0)
    {
        check(launch_rescale_pre(e, lt.d_rns, lt.h_rns, last, last_stride, temp, static_cast<std::size_t>(k - 1) * e.n, npolys),
              "rescale_pre");
        check(launch_ntt(e, temp, npolys * (k - 1), e.level_host(k - 1).map_q, false, ntt_flags), "ntt(temp)");
    }
    // divround_ntt_front: the same for polys[npolys][k][N] in NTT form, whose last rows go to coefficient form in place first
    void divround_ntt_front(Engine &e, LevelTools &lt, int k, u64 *polys, std::size_t npolys, u64 *temp)
    {
        check(launch_ntt(e, polys, npolys * k, skip_map(lt.map_q, k - 1, k), true, kNttCanonical), "intt(last)");
        rescale_temp(e, lt, k, polys + static_cast<std::size_t>(k - 1) * e.n, static_cast<std::size_t>(k) * e.n, npolys, temp);
    }

    // exact (CKKS): the correction's forward transform is the exact one in both modes -- the merged finish without a
    // key-switch term, whose words the restatement defines with the exact transform
    void mod_switch_polys(Engine &e, int k, const u64 *ct, std::size_t in_stride, u64 *out, std::size_t out_stride,
                          std::size_t npolys, bool exact)
    {
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n;
        const std::size_t temp_stride = static_cast<std::size_t>(k - 1) * N;
        if (e.scheme == 1)
        {
            check(launch_divround_bfv(e, lt.d_rns, lt.h_rns, ct, in_stride, out, out_stride, npolys, k - 1), "divround");
            return;
        }
        // CKKS (rns.cpp:777-851), without the reference's full copy of the ciphertext: only the last row is
        // duplicated because only it is modified
        const std::size_t per_poly = (N + static_cast<std::size_t>(k - 1) * N) * sizeof(u64);
        for_chunks(e, npolys, per_poly, 2, [&](std::size_t off, std::size_t m) {
            u64 *last = e.ws_alloc(N * m);
            u64 *temp = e.ws_alloc(temp_stride * m);
            check(launch_copy_rows(e, ct + off * in_stride + static_cast<std::size_t>(k - 1) * N, in_stride, last, N, m, 1),
                  "copy(last)");
            RowMap one{};
            one.rows = 1;
            one.prime[0] = static_cast<unsigned short>(k - 1);
            check(launch_ntt(e, last, m, one, true, kNttCanonical), "intt(last)");
            rescale_temp(e, lt, k, last, N, m, temp, exact ? kNttStrict : 0);
            check(launch_rescale_post(e, lt.d_rns, lt.h_rns, ct + off * in_stride, in_stride, temp, temp_stride,
                                      out + off * out_stride, out_stride, m),
                  "rescale_post");
        });
    }
    } // namespace

    // divide_and_round_q_last_ntt_inplace (rns.cpp:777-851), in place like the reference (last row clobbered)
    void op_divround_ntt_inplace(Engine &e, int k, u64 *data, std::size_t count)
    {
        if (k < 2)
            throw std::invalid_argument("divide_and_round_q_last needs at least two primes");
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n;
        const std::size_t stride = static_cast<std::size_t>(k) * N, tstride = static_cast<std::size_t>(k - 1) * N;
        for_chunks(e, count, tstride * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *temp = e.ws_alloc(tstride * m);
            u64 *p = data + off * stride;
            divround_ntt_front(e, lt, k, p, m, temp);
            check(launch_rescale_post(e, lt.d_rns, lt.h_rns, p, stride, temp, tstride, p, stride, m), "rescale_post");
        });
    }

    // ------------------------------------------------------------------------------------------
    // apply_galois_inplace (evaluator.cpp:1841-1943)
    // ------------------------------------------------------------------------------------------
    namespace
    {
        void check_galois_elt(const Engine &e, std::uint32_t elt)
        {
            if (!(elt & 1) || elt >= static_cast<std::uint64_t>(e.n) * 2)
                throw std::invalid_argument("Galois element is not valid"); // :1880-1883
        }

        // One list of Galois elements with their keys, as the hoisted entries take it; tables: T_g, null for a free identity
        struct GaloisAxis
        {
            const std::uint32_t *elts;
            const KSwitchKey *const *keys;
            std::size_t n, n_gal; // elements, and those that need a key switch
            bool identity_free;   // the identity needs no key (NULL allowed) and no table
            std::vector<const std::uint32_t *> tables;
        };
        // Validates, element by element, the element and -- where it needs a key switch -- its key's digit count against the
        // level's nd. identity_free: the weighted forms; otherwise (op_apply_galois_many) every element is key-switched.
        GaloisAxis check_axis(const Engine &e, int nd, const std::uint32_t *elts, const KSwitchKey *const *keys, std::size_t n,
                              bool identity_free)
        {
            GaloisAxis ax{ elts, keys, n, 0, identity_free, {} };
            for (std::size_t i = 0; i < n; i++)
            {
                check_galois_elt(e, elts[i]);
                if (identity_free && elts[i] == 1)
                    continue;
                if (!keys[i] || static_cast<int>(keys[i]->n_digits) < nd)
                    throw std::invalid_argument("kswitch_keys is not valid for encryption parameters");
                ax.n_gal++;
            }
            return ax;
        }
        // ... and, once the call is known to do work, the tables (resident after the first call: the condition for a capture)
        void load_tables(Engine &e, GaloisAxis &ax)
        {
            ax.tables.assign(ax.n, nullptr);
            for (std::size_t i = 0; i < ax.n; i++)
                if (!ax.identity_free || ax.elts[i] != 1)
                    ax.tables[i] = e.galois_table(ax.elts[i]);
        }
    } // namespace

    void op_apply_galois(Engine &e, int k, u64 *ct, std::size_t count, std::uint32_t elt, const KSwitchKey &key)
    {
        check_galois_elt(e, elt);
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::uint32_t *table = e.scheme == 2 ? e.galois_table(elt) : nullptr;
        // The Galois image of both components (2 polys per item) must survive op_switch_key, which re-plans the
        // arena: it is carved from the FRONT of the arena (ws_floor) for the duration of this operation.
        const std::size_t per_item = 2 * poly * sizeof(u64);
        const std::size_t items = std::max<std::size_t>(1, std::min<std::size_t>(count, (1024ull << 20) / per_item));
        const std::size_t scratch_bytes = (items * per_item + 255) & ~static_cast<std::size_t>(255);
        // the arena must hold the scratch plus at least one item of the key switch; growing it may move it
        e.ws_reserve(scratch_bytes + 256);
        FloorRestore guard(e);
        guard.raise(scratch_bytes);
        for (std::size_t off = 0; off < count; off += items)
        {
            const std::size_t m = std::min(items, count - off);
            u64 *c = ct + off * 2 * poly;
            // size the arena now exactly as the nested op_switch_key will ask for, so that it cannot move while the scratch
            // is live, and re-derive the pointer after it (no scratch contents are live before this iteration's first launch)
            plan_chunk(e, m, switch_key_arena(e, k).item_bytes(), KsArena::n_buffers, false);
            u64 *scratch = static_cast<u64 *>(guard.parked());
            check(launch_galois(e, c, scratch, m * 2 * k, lt.map_q, elt, table), "galois");
            // The reference copies galois(c0) back (:1903 / :1917), zeroes c1 (:1928) and lets the key switch add its two
            // polynomials into that ciphertext (:1934-1935). Here the key switch's last kernel writes (galois(c0) + r0, r1)
            // directly: same sums, no copy pass and no fill pass over the ciphertext.
            e.lane().tsink_base = guard.base + off; // (the nested chunk loop counts its items from this chunk's first ciphertext)
            op_switch_key(e, k, c, 2 * poly, scratch + poly, 2 * poly, m, key, scratch, 2 * poly);
        }
    }
    // ------------------------------------------------------------------------------------------
    // Ring packing: LWE samples out of a ciphertext, and n = 2^l of them packed into one
    // ------------------------------------------------------------------------------------------
    void op_extract_lwe(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *idx, std::size_t n_idx,
                        u64 *lwe_a, u64 *lwe_b)
    {
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::size_t a_item = n_idx * poly, b_item = n_idx * static_cast<std::size_t>(k);
        if (e.scheme != 2) // BFV ciphertexts are in coefficient form already
        {
            check(launch_lwe_extract(e, ct, 2 * poly, count, idx, n_idx, lwe_a, lwe_b, lt.map_q), "lwe_extract");
            return;
        }
        // CKKS: a temporary copy goes back to coefficient form; the caller's ciphertext is not modified
        for_chunks(e, count, 2 * poly * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *tmp = e.ws_alloc(2 * poly * m);
            check(launch_copy_rows(e, ct + off * 2 * poly, poly, tmp, poly, 2 * m, k), "copy");
            check(launch_ntt(e, tmp, 2 * m * k, lt.map_q, true, kNttCanonical), "intt(ct)");
            check(launch_lwe_extract(e, tmp, 2 * poly, m, idx, n_idx, lwe_a + off * a_item, lwe_b + off * b_item, lt.map_q),
                  "lwe_extract");
        });
    }

    // The pack keeps its working set sample-major, W[j][item]: step t merges W[j] and W[j + half] for j < half, so both
    // operands, the result and the key switch's batch are contiguous runs of half * items ciphertexts. A step is one merge
    // launch, which leaves (E + O) + (sigma_g(E_0 - O_0), 0) in the destination and sigma_g(E_1 - O_1) in `target`, and one
    // key switch of `target` that adds into the destination: the sums of (E + O) + apply_galois(E - O, g), reordered.
    // The working set is parked at the front of the arena under a raised floor, as op_apply_galois parks its scratch, and
    // takes at most half of the arena's cap; the nested key switch plans with the whole cap as always, so the arena may
    // reach 1.5 times the cap while a pack runs. Three buffers: A for the embeddings and then every even step's
    // result; B for every odd step's, the first one's n / 2 ciphertexts above all; the targets. The last step
    // writes to `out`. When A cannot hold all embeddings of a chunk of items, the batch is walked item by item; when not
    // even those of one item, the first step walks the item's merges in groups of c: embed {j, j + n/2} for c values of
    // j, merge them into B, continue -- A then holds 2 c ciphertexts. Modular sums do not depend on the grouping, so the
    // words are the same. What must always fit is the first step's result and the second step's: 0.875 n ciphertexts.
    void op_pack_lwes(Engine &e, int k, const u64 *lwe_a, const u64 *lwe_b, int l, std::size_t count,
                      const KSwitchKey *const *keys, bool trace, bool normalize, u64 *out, SinkScope &sink)
    {
        LevelTools &lt = e.level(k);
        const bool ckks = e.scheme == 2;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N, n = static_cast<std::size_t>(1) << l;
        const int steps = trace ? e.logn : l;
        // w_r: the inverse of what the steps multiply the phase by (n, or N with the trace), else 1
        u64 w[kMaxModuli], w_shoup[kMaxModuli];
        for (int r = 0; r < k; r++)
        {
            const u64 q = e.key_moduli[static_cast<std::size_t>(r)];
            w[r] = 1;
            if (normalize && !invmod((trace ? N : n) % q, q, w[r]))
                throw std::logic_error("pack: the normalisation has no inverse");
            w_shoup[r] = shoup(w[r], q);
        }
        const u64 *mono = ckks && l ? e.pack_monomials() : nullptr;
        std::vector<const std::uint32_t *> tables(static_cast<std::size_t>(e.logn) + 1, nullptr);
        std::vector<std::uint32_t> ginv(static_cast<std::size_t>(e.logn) + 1, 1); // (2^t + 1)^{-1} mod 2N
        for (int t = 1; t <= steps; t++)
        {
            const std::uint32_t g = (1u << t) + 1;
            if (ckks)
                tables[static_cast<std::size_t>(t)] = e.galois_table(g);
            std::uint32_t &inv = ginv[static_cast<std::size_t>(t)];
            for (int it = 0; it < 5; it++) // every Newton step doubles the correct low bits, from one to 32
                inv *= 2 - g * inv;
            inv &= static_cast<std::uint32_t>(2 * N - 1);
        }

        // one item's buffers in words when the first step merges c values of j at a time (l = 0: one embedding, no merge)
        const std::size_t half0 = std::max<std::size_t>(1, n / 2);
        struct Words
        {
            std::size_t a, b, t;
            std::size_t bytes() const
            {
                return (a + b + t) * sizeof(u64);
            }
        };
        auto words_for = [&](std::size_t c) {
            const std::size_t emb = l ? 2 * c : 1;
            return Words{ steps ? std::max(emb, n / 4) * 2 * poly : 0, steps >= 2 ? half0 * 2 * poly : 0,
                          steps ? std::max(l ? c : 1, n / 4) * poly : 0 };
        };
        const std::size_t cap = workspace_budget_bytes(e) / 2 - 3 * 256;
        std::size_t c = half0, items = count;
        Words ww = words_for(c);
        if (ww.bytes() > cap) // one item at a time, its first step in groups
        {
            items = 1;
            do
                ww = words_for(c /= 2);
            while (c && ww.bytes() > cap);
            if (!c)
                throw HipError(hipErrorOutOfMemory,
                               ("pack: the smallest working set of one item (" + std::to_string(words_for(1).bytes()) +
                                " bytes) does not fit half of the workspace arena (" + std::to_string(cap) +
                                " bytes): raise SEALHIP_WORKSPACE_MB or pack fewer samples per call")
                                   .c_str());
        }
        else if (ww.bytes())
            items = std::max<std::size_t>(1, std::min(count, cap / ww.bytes()));
        const std::size_t scratch_bytes = pad256(ww.a * items) + pad256(ww.b * items) + pad256(ww.t * items);
        Lane &lane = e.lane();
        e.ws_reserve(lane.ws_floor + scratch_bytes + 256);
        FloorRestore guard(e);
        guard.raise(scratch_bytes);
        const RowMap map_c1 = ct_row_map(k, 2, 1);
        for (std::size_t off = 0; off < count; off += items)
        {
            const std::size_t m = std::min(items, count - off);
            u64 *dst_out = out + off * 2 * poly;
            const u64 *a_in = lwe_a + off * n * poly, *b_in = lwe_b + off * n * static_cast<std::size_t>(k);
            // size the arena now as the largest nested key switch will ask for, so that it cannot move while the working set
            // is live, and derive the pointers after it
            if (steps)
                plan_chunk(e, m * std::max(l ? c : 1, n / 4), switch_key_arena(e, k).item_bytes(), KsArena::n_buffers, false);
            Carver carve{ static_cast<char *>(guard.parked()) };
            u64 *bufs[2] = { carve.take(ww.a * items), nullptr };
            bufs[1] = carve.take(ww.b * items);
            u64 *target = carve.take(ww.t * items);
            // n_out embeddings (c_1 alone transformed for CKKS: an embedded c_0 is a constant, written in NTT form directly)
            auto embed = [&](std::size_t j0, std::size_t cj, std::size_t n_out, u64 *emb) {
                check(launch_lwe_embed(e, a_in, b_in, n, m, j0, cj, n_out, emb, lt.map_q, w, w_shoup, ckks), "lwe_embed");
                if (ckks)
                    check(launch_ntt(e, emb, n_out * m * 2 * k, map_c1, false, kNttCanonical), "ntt(embedded c1)");
            };
            // one launch and one key switch: ncts results of step t from src (and, merging, the ncts ciphertexts behind them)
            auto step = [&](int t, const u64 *src, std::size_t ncts, u64 *dst) {
                check(launch_pack_merge(e, src, t <= l ? src + ncts * 2 * poly : nullptr, dst, target, ncts, lt.map_q,
                                        static_cast<std::uint32_t>(N >> t), ginv[static_cast<std::size_t>(t)],
                                        tables[static_cast<std::size_t>(t)],
                                        mono ? mono + static_cast<std::size_t>(t - 1) * e.k_first * N * 2 : nullptr),
                      "pack_merge");
                if (t == steps) // one flag per output ciphertext, from the last key switch
                {
                    sink.arm();
                    lane.tsink_base = guard.base + off;
                }
                op_switch_key(e, k, dst, 2 * poly, target, poly, ncts, *keys[t]);
                lane.tsink_cur = nullptr;
            };
            if (!l)
                embed(0, 1, 1, steps ? bufs[0] : dst_out);
            else
                for (std::size_t j0 = 0; j0 < half0; j0 += c) // step 1, by groups (one group: c = n / 2)
                {
                    embed(j0, c, 2 * c, bufs[0]);
                    step(1, bufs[0], c * m, (steps == 1 ? dst_out : bufs[1]) + j0 * m * 2 * poly);
                }
            std::size_t cur = l ? half0 : 1; // ciphertexts per item
            for (int t = l ? 2 : 1; t <= steps; t++)
            {
                const std::size_t left = t <= l ? cur / 2 : cur;
                // (odd steps read A and write B, even steps the reverse: step 1 leaves its result in B, and a trace without
                // any merge starts from the embedding in A)
                const int from = (t & 1) ^ 1;
                step(t, bufs[from], left * m, t == steps ? dst_out : bufs[from ^ 1]);
                cur = left;
            }
        }
        if (!steps)
            sink.read_pass(out, 2, poly, count);
        // (after the key switches' own entries: the last pairs of sealhip_debug_chunk_log)
        if (c < half0)
            log_chunk(e, half0, c);
        log_chunk(e, count, items);
    }

    // ------------------------------------------------------------------------------------------
    // Oblivious expansion: one ciphertext into n = 2^l, one per coefficient of the phase
    // ------------------------------------------------------------------------------------------
    // The working set is item-major, W_t[item][i], i < 2^t: step t reads the m 2^(t-1) ciphertexts of W_(t-1) as one run,
    // writes source (item, j)'s even result to (item, j) and its odd one to (item, j + 2^(t-1)) of W_t, the key switch's
    // targets at the same places, and one key switch of all m 2^t targets adds into W_t: E + apply_galois(E, g) and
    // O + apply_galois(O, g), the exact sums reordered. Step 1 reads the caller's ciphertexts, step l writes the caller's
    // out. W_1 .. W_(l-1) alternate between two buffers parked at the front of the arena under a raised floor, as
    // op_pack_lwes parks its own, next to the targets: n / 2 + n / 4 ciphertexts and n target polynomials per item,
    // at most half of the arena's cap. A batch that does not fit is walked in chunks of items. One item that does not fit
    // has its LAST step walked in groups of c sources, which needs 2 c target polynomials instead of n (subtrees are
    // independent: the same words); a group's even and odd results are two runs of out, so it takes two key switches of
    // c. What must always fit is W_(l-1), W_(l-2) and the targets of step l - 1: n ciphertexts.
    void op_expand(Engine &e, int k, const u64 *ct, int l, std::size_t count, const KSwitchKey *const *keys, bool normalize,
                   u64 *out, SinkScope &sink)
    {
        LevelTools &lt = e.level(k);
        const bool ckks = e.scheme == 2;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N, n = static_cast<std::size_t>(1) << l;
        if (!l) // a copy (n^{-1} = 1)
        {
            check(launch_copy_rows(e, ct, poly, out, poly, 2 * count, k), "copy");
            sink.read_pass(out, 2, poly, count);
            log_chunk(e, count, count);
            return;
        }
        // w_r = n^{-1}: the inverse of what the l steps multiply the phase by
        u64 w[kMaxModuli], w_shoup[kMaxModuli];
        for (int r = 0; r < k && normalize; r++)
        {
            const u64 q = e.key_moduli[static_cast<std::size_t>(r)];
            if (!invmod(n % q, q, w[r]))
                throw std::logic_error("expand: the normalisation has no inverse");
            w_shoup[r] = shoup(w[r], q);
        }
        const u64 *mono = ckks ? e.expand_monomials() : nullptr;
        std::vector<const std::uint32_t *> tables(static_cast<std::size_t>(l) + 1, nullptr);
        std::vector<std::uint32_t> ginv(static_cast<std::size_t>(l) + 1, 1); // (N / 2^(t-1) + 1)^{-1} mod 2N
        for (int t = 1; t <= l; t++)
        {
            const std::uint32_t g = static_cast<std::uint32_t>(N >> (t - 1)) + 1;
            if (ckks)
                tables[static_cast<std::size_t>(t)] = e.galois_table(g);
            std::uint32_t &inv = ginv[static_cast<std::size_t>(t)];
            for (int it = 0; it < 5; it++) // every Newton step doubles the correct low bits, from one to 32
                inv *= 2 - g * inv;
            inv &= static_cast<std::uint32_t>(2 * N - 1);
        }

        // one item's buffers in words when the last step takes c sources at a time (c = n / 2: all of them)
        struct Words
        {
            std::size_t big, small, t;
            std::size_t bytes() const
            {
                return (big + small + t) * sizeof(u64);
            }
        };
        const std::size_t half = n / 2;
        auto words_for = [&](std::size_t c) {
            return Words{ l >= 2 ? half * 2 * poly : 0, l >= 3 ? (n / 4) * 2 * poly : 0, std::max(l >= 2 ? half : 0, 2 * c) * poly };
        };
        const std::size_t cap = workspace_budget_bytes(e) / 2 - 3 * 256;
        std::size_t c = half, items = count;
        Words ww = words_for(c);
        if (ww.bytes() > cap) // one item at a time, its last step in groups
        {
            items = 1;
            do
                ww = words_for(c /= 2);
            while (c && ww.bytes() > cap);
            if (!c)
                throw HipError(hipErrorOutOfMemory,
                               ("expand: the smallest working set of one item (" +
                                std::to_string(words_for(1).bytes()) +
                                " bytes) does not fit half of the workspace arena (" + std::to_string(cap) +
                                " bytes): raise SEALHIP_WORKSPACE_MB or expand into fewer ciphertexts per call")
                                   .c_str());
        }
        else
            items = std::max<std::size_t>(1, std::min(count, cap / ww.bytes()));
        int log_c = 0;
        while ((static_cast<std::size_t>(1) << log_c) < c)
            log_c++;
        const std::size_t scratch_bytes = pad256(ww.big * items) + pad256(ww.small * items) + pad256(ww.t * items);
        Lane &lane = e.lane();
        e.ws_reserve(lane.ws_floor + scratch_bytes + 256);
        FloorRestore guard(e);
        guard.raise(scratch_bytes);
        for (std::size_t off = 0; off < count; off += items)
        {
            const std::size_t m = std::min(items, count - off);
            // size the arena now as the largest nested key switch will ask for, so that it cannot move while the working set
            // is live, and derive the pointers after it
            plan_chunk(e, m * std::max(l >= 2 ? half : 0, c < half ? c : n), switch_key_arena(e, k).item_bytes(), KsArena::n_buffers,
                       false);
            Carver carve{ static_cast<char *>(guard.parked()) };
            u64 *bufs[2];
            bufs[(l - 1) & 1] = carve.take(ww.big * items); // W_(l-1), and every W_t of its parity
            bufs[l & 1] = carve.take(ww.small * items);
            u64 *target = carve.take(ww.t * items);
            u64 *dst_out = out + off * n * 2 * poly;
            for (int t = 1; t <= l; t++)
            {
                const std::size_t cur = static_cast<std::size_t>(1) << (t - 1);
                const u64 *src = t == 1 ? ct + off * 2 * poly : bufs[(t - 1) & 1];
                u64 *dst = t == l ? dst_out : bufs[t & 1];
                const std::size_t ts = static_cast<std::size_t>(t);
                const u64 *rows = mono ? mono + static_cast<std::size_t>(t - 1) * e.k_first * N * 2 : nullptr;
                const bool scaled = normalize && t == 1;
                const KSwitchKey &key = *keys[t];
                // the key switch of ncts results from `at` on; the last step's carries the flags, one per output ciphertext
                auto key_switch = [&](std::size_t at, const u64 *tg, std::size_t ncts) {
                    if (t == l)
                    {
                        sink.arm();
                        lane.tsink_base = guard.base + off * n + at;
                    }
                    op_switch_key(e, k, dst + at * 2 * poly, 2 * poly, tg, poly, ncts, key);
                    lane.tsink_cur = nullptr;
                };
                if (t == l && c < half) // (one item) by groups of c sources
                    for (std::size_t j0 = 0; j0 < half; j0 += c)
                    {
                        check(launch_expand_step(e, src + j0 * 2 * poly, 2 * poly, c, log_c, dst + j0 * 2 * poly, n, half, target, 2 * c,
                                                 c, lt.map_q, static_cast<std::uint32_t>(cur), ginv[ts], tables[ts], rows,
                                                 scaled ? w : nullptr, scaled ? w_shoup : nullptr),
                              "expand_step");
                        key_switch(j0, target, c);
                        key_switch(half + j0, target + c * poly, c);
                    }
                else
                {
                    check(launch_expand_step(e, src, 2 * poly, m * cur, t - 1, dst, 2 * cur, cur, target, 2 * cur, cur, lt.map_q,
                                             static_cast<std::uint32_t>(cur), ginv[ts], tables[ts], rows, scaled ? w : nullptr,
                                             scaled ? w_shoup : nullptr),
                          "expand_step");
                    key_switch(0, target, m * 2 * cur);
                }
            }
        }
        // (after the key switches' own entries: the last pairs of sealhip_debug_chunk_log)
        if (c < half)
            log_chunk(e, half, c);
        log_chunk(e, count, items);
    }

    // Sums against plaintext rows. dot_plain_kernel reads the ciphertexts and the plaintexts where they
    // are and writes the sums where they belong: nothing comes from the arena. Sums go in tiles of kLinTile, terms in groups
    // of kLinGroup; a later group adds the canonical partial sum in, and the last group notes the transparency flags
    // (sum-major, as the output is).
    void op_dot_plain(Engine &e, int k, const u64 *cts, std::size_t n_terms, int size, std::size_t count, const u64 *plain,
                      std::size_t n_sums, u64 *out)
    {
        if (k > e.k_first)
            throw std::invalid_argument("the sum against plaintexts needs a ciphertext level");
        if (n_terms == 0 || n_sums == 0 || size < 2)
            throw std::invalid_argument("an empty sum against plaintexts");
        LevelTools &lt = e.level(k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n, item = static_cast<std::size_t>(size) * poly;
        if (n_terms > static_cast<std::size_t>(kLinGroup))
            log_chunk(e, n_terms, kLinGroup); // (the term split, ahead of the operation's item chunks: sealhip_debug_chunk_log)
        for_chunks(e, count, 0, 0, [&](std::size_t off, std::size_t m) {
            for (std::size_t s0 = 0; s0 < n_sums; s0 += kLinTile)
                for (std::size_t g0 = 0; g0 < n_terms; g0 += kLinGroup)
                {
                    const bool last = g0 + kLinGroup >= n_terms; // (only the last group's stores are the result's words)
                    SinkArm arm(e, last ? sink_at(e, s0 * count + off) : nullptr);
                    check(launch_dot_plain(e, cts + (off * n_terms + g0) * item, size, n_terms * item,
                                           static_cast<int>(std::min<std::size_t>(kLinGroup, n_terms - g0)),
                                           plain + (s0 * n_terms + g0) * poly, n_terms * poly, out + (s0 * count + off) * item,
                                           count * item, static_cast<int>(std::min<std::size_t>(kLinTile, n_sums - s0)), m,
                                           lt.map_q, g0 > 0, count),
                          "dot_plain");
                }
        });
    }

    // ------------------------------------------------------------------------------------------
    // RGSW: the external product, CMux and the CMux tree
    // ------------------------------------------------------------------------------------------
    namespace
    {
        // a key switch's item with the digits of both components (and both components in the other form, where there is one)
        constexpr int kExtProductBuffers = 6;
        KsArena ext_product_arena(Engine &e, int k)
        {
            KsArena ar = switch_key_arena(e, k);
            ar.w_coeff *= 2;
            ar.w_ext *= 2;
            return ar;
        }
        LevelTools &ext_product_level(Engine &e, int k, const RgswKey &g)
        {
            if (k > e.k_first)
                throw std::invalid_argument("key switching needs a ciphertext level");
            if (e.scheme != 2 && !e.mode_strict)
                throw std::invalid_argument("the external product of BFV ciphertexts needs a STRICT context");
            LevelTools &lt = e.level(k);
            if (static_cast<int>(g.n_digits) < lt.h_ks.nd || (g.level && k > static_cast<int>(g.level)))
                throw std::invalid_argument("rgsw is not valid for encryption parameters");
            return lt;
        }
        // One chunk: outp[m][2][k][N] += c (x) g. The digits of c_0 and of c_1 go into one digit-major ext of 2 nd digits,
        // one launch forms the 2 nd-term inner product, one ks_finish brings it down and adds it in.
        void ext_product_chunk(Engine &e, LevelTools &lt, int k, const KsArena &ar, const u64 *c, std::size_t stride, std::size_t m,
                               const RgswKey &g, u64 *outp, unsigned *sink)
        {
            const std::size_t poly = static_cast<std::size_t>(k) * e.n, ext_item = static_cast<std::size_t>(k + e.nsp) * e.n;
            const int nd = lt.h_ks.nd;
            u64 *coeff0 = ar.w_coeff ? e.ws_alloc(ar.w_coeff / 2 * m) : nullptr;
            u64 *coeff1 = ar.w_coeff ? e.ws_alloc(ar.w_coeff / 2 * m) : nullptr;
            u64 *ext = e.ws_alloc(ar.w_ext * m);
            u64 *prod = e.ws_alloc(ar.w_prod * m);
            u64 *temp = e.ws_alloc(ar.w_temp * m);
            const KsRows in0 = ks_digits(e, lt, k, c, stride, m, coeff0, ext, 0, nd);
            const KsRows in1 = ks_digits(e, lt, k, c + poly, stride, m, coeff1, ext + nd * ext_item * m, 0, nd);
            check(launch_ext_mac(e, lt.d_ks, lt.h_ks, in0.inb, in1.inb, in0.inb_stride, ext, ext_item, ext_item * m, g.half(0), g.half(1),
                                 prod, 2 * ext_item, m),
                  "ext_mac");
            ks_finish(e, lt, k, prod, temp, outp, 2 * poly, nullptr, 0, m, sink);
        }
    } // namespace

    void op_external_product(Engine &e, int k, const u64 *ct, std::size_t ct_stride, std::size_t count, const RgswKey &g, u64 *out)
    {
        LevelTools &lt = ext_product_level(e, k, g);
        const KsArena ar = ext_product_arena(e, k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        for_chunks(e, count, ar.item_bytes(), kExtProductBuffers, [&](std::size_t off, std::size_t m) {
            ext_product_chunk(e, lt, k, ar, ct + off * ct_stride, ct_stride, m, g, out + off * 2 * poly, sink_at(e, off));
        });
    }

    // cmux_prepare_kernel reads both operands once: the difference goes to the arena, the copy of ct0 to out, and the chunk
    // goes on as an external product's
    void op_cmux(Engine &e, int k, const u64 *ct0, std::size_t stride0, const u64 *ct1, std::size_t stride1, std::size_t count,
                 const RgswKey &g, u64 *out)
    {
        LevelTools &lt = ext_product_level(e, k, g);
        const KsArena ar = ext_product_arena(e, k);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        for_chunks(e, count, ar.item_bytes() + 2 * poly * sizeof(u64), kExtProductBuffers + 1, [&](std::size_t off, std::size_t m) {
            u64 *diff = e.ws_alloc(2 * poly * m);
            u64 *outp = out + off * 2 * poly;
            check(launch_cmux_prepare(e, k, ct0 + off * stride0, stride0, ct1 + off * stride1, stride1, diff, outp, 2 * poly, m),
                  "cmux_prepare");
            ext_product_chunk(e, lt, k, ar, diff, 2 * poly, m, g, outp, sink_at(e, off));
        });
    }

    // The CMux tree. The working set is item-major and flat: level t reads the pairs (W[2i], W[2i+1]) of the m 2^(l-t)
    // ciphertexts before it as one run and writes m 2^(l-t-1). Level 0 reads the caller's ciphertexts, level l - 1 writes the
    // caller's out; the sets between alternate between two buffers parked at the front of the arena under a raised floor,
    // next to the differences: 2^(l-1) + 2^(l-2) + 2^(l-1) ciphertexts per item, at most half of the arena's cap. Each level
    // is one prepare launch and one external product of all its pairs, chunked by its own loop. A batch that does not fit
    // is walked in chunks of items.
    void op_select(Engine &e, int k, const u64 *cts, std::size_t count, int l, const RgswKey *const *bits, u64 *out, SinkScope &sink)
    {
        const std::size_t poly = static_cast<std::size_t>(k) * e.n, ct_words = 2 * poly;
        if (!l) // a copy
        {
            if (k > e.k_first)
                throw std::invalid_argument("key switching needs a ciphertext level");
            check(launch_copy_rows(e, cts, poly, out, poly, 2 * count, k), "copy");
            sink.read_pass(out, 2, poly, count);
            log_chunk(e, count, count);
            return;
        }
        for (int t = 0; t < l; t++)
            (void)ext_product_level(e, k, *bits[t]);
        const std::size_t half = static_cast<std::size_t>(1) << (l - 1);
        const std::size_t w_big = l >= 2 ? half * ct_words : 0, w_small = l >= 3 ? (half / 2) * ct_words : 0, w_diff = half * ct_words;
        const std::size_t item_bytes = (w_big + w_small + w_diff) * sizeof(u64);
        const std::size_t cap = workspace_budget_bytes(e) / 2 - 3 * 256;
        if (item_bytes > cap)
            throw HipError(hipErrorOutOfMemory, ("select: the first level of one item (" + std::to_string(item_bytes) +
                                                 " bytes) does not fit half of the workspace arena (" + std::to_string(cap) +
                                                 " bytes): raise SEALHIP_WORKSPACE_MB or select among fewer ciphertexts per call")
                                                    .c_str());
        const std::size_t items = std::max<std::size_t>(1, std::min(count, cap / item_bytes));
        const std::size_t scratch_bytes = pad256(w_big * items) + pad256(w_small * items) + pad256(w_diff * items);
        const KsArena ar = ext_product_arena(e, k);
        Lane &lane = e.lane();
        e.ws_reserve(lane.ws_floor + scratch_bytes + 256);
        FloorRestore guard(e);
        guard.raise(scratch_bytes);
        for (std::size_t off = 0; off < count; off += items)
        {
            const std::size_t m = std::min(items, count - off);
            // size the arena now as the largest nested external product will ask for, so that it cannot move while the
            // working set is live, and derive the pointers after it
            plan_chunk(e, m * half, ar.item_bytes(), kExtProductBuffers, false);
            Carver carve{ static_cast<char *>(guard.parked()) };
            u64 *bufs[2];
            bufs[0] = carve.take(w_big * items);
            bufs[1] = carve.take(w_small * items);
            u64 *diff = carve.take(w_diff * items);
            for (int t = 0; t < l; t++)
            {
                const std::size_t pairs = m << (l - t - 1);
                const u64 *src = t == 0 ? cts + (off << l) * ct_words : bufs[(t - 1) & 1];
                u64 *dst = t == l - 1 ? out + off * ct_words : bufs[t & 1];
                check(launch_cmux_prepare(e, k, src, 2 * ct_words, src + ct_words, 2 * ct_words, diff, dst, ct_words, pairs),
                      "cmux_prepare");
                if (t == l - 1) // the last level's mod-down carries the flags, one per output ciphertext
                {
                    sink.arm();
                    lane.tsink_base = guard.base + off;
                }
                op_external_product(e, k, diff, ct_words, pairs, *bits[t], dst);
                lane.tsink_cur = nullptr;
            }
        }
        log_chunk(e, count, items); // (after the external products' own entries: the last pair of sealhip_debug_chunk_log)
    }

    // ------------------------------------------------------------------------------------------
    // Blind rotation: the monomial product with an exponent per item, and the accumulator loop
    // ------------------------------------------------------------------------------------------
    namespace
    {
        // the form the scheme's ciphertexts are in, with the checks both entries share; the table where the form needs it
        const u64 *monomial_form(Engine &e, int k, bool &ntt_form)
        {
            if (k > e.k_first)
                throw std::invalid_argument("level k out of range");
            if (e.scheme != 2 && !e.mode_strict)
                throw std::invalid_argument("the monomial product of BFV ciphertexts needs a STRICT context");
            ntt_form = e.scheme == 2;
            return ntt_form ? e.psi_powers() : nullptr;
        }
    } // namespace

    void op_multiply_monomial(Engine &e, int k, const u64 *ct, std::size_t ct_stride, std::size_t count, const std::uint32_t *exps,
                              std::size_t exps_stride, bool minus_one, u64 *out)
    {
        bool ntt_form;
        const u64 *psi = monomial_form(e, k, ntt_form);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n;
        check(launch_monomial_prepare(e, k, ntt_form, minus_one, ct, ct_stride, out, 2 * poly, exps, exps_stride, 0, psi, count),
              "monomial_prepare");
    }

    // The whole step loop runs inside a chunk of items. Step 0 writes X^(e_0) tv into the caller's out, which is the
    // accumulator from then on; step t reads it once and writes only the target (X^(e_t) - 1) acc into the arena, and the
    // external product's mod-down adds into the accumulator in place: 4 polynomials moved per step around the key switch.
    // The arena is one target of 2 k N words per item beside the external product's own buffers, which every step carves
    // anew from the same mark. Nothing is read back or synchronised between the steps.
    void op_blind_rotate(Engine &e, int k, const u64 *tv, std::size_t tv_stride, std::size_t count, const std::uint32_t *exps,
                         std::size_t n_steps, const RgswKey *const *rgsw, u64 *out, SinkScope &sink)
    {
        bool ntt_form;
        const u64 *psi = monomial_form(e, k, ntt_form);
        for (std::size_t t = 0; t < n_steps; t++)
            (void)ext_product_level(e, k, *rgsw[t]);
        const std::size_t poly = static_cast<std::size_t>(k) * e.n, ct_words = 2 * poly, row = 1 + n_steps;
        if (!n_steps)
        {
            check(launch_monomial_prepare(e, k, ntt_form, false, tv, tv_stride, out, ct_words, exps, row, 0, psi, count),
                  "monomial_prepare");
            sink.read_pass(out, 2, poly, count);
            log_chunk(e, count, count);
            return;
        }
        LevelTools &lt = e.level(k);
        const KsArena ar = ext_product_arena(e, k);
        sink.begin();
        Lane &lane = e.lane();
        for_chunks(e, count, ar.item_bytes() + ct_words * sizeof(u64), kExtProductBuffers + 1, [&](std::size_t off, std::size_t m) {
            u64 *acc = out + off * ct_words;
            const std::uint32_t *ex = exps + off * row;
            u64 *target = e.ws_alloc(ct_words * m);
            const std::size_t mark = lane.ws_used;
            check(launch_monomial_prepare(e, k, ntt_form, false, tv + off * tv_stride, tv_stride, acc, ct_words, ex, row, 0, psi, m),
                  "monomial_prepare");
            for (std::size_t t = 1; t <= n_steps; t++)
            {
                lane.ws_used = mark;
                check(launch_monomial_prepare(e, k, ntt_form, true, acc, ct_words, target, ct_words, ex, row, t, psi, m),
                      "monomial_prepare");
                // (the last step's mod-down carries the flags, one per output ciphertext)
                ext_product_chunk(e, lt, k, ar, target, ct_words, m, *rgsw[t - 1], acc, t == n_steps ? sink_at(e, off) : nullptr);
            }
        });
    }

    void op_lwe_mod_switch(Engine &e, const u64 *lwe_a, const u64 *lwe_b, std::size_t n_samples, bool ternary,
                           std::uint32_t b_offset, std::uint32_t *exps)
    {
        check(launch_lwe_mod_switch(e, lwe_a, lwe_b, n_samples, ternary, b_offset, exps), "lwe_mod_switch");
    }

    // ------------------------------------------------------------------------------------------
    // Hoisted rotation: n_elts automorphisms of the same ciphertexts with one decomposition of c_1
    // ------------------------------------------------------------------------------------------
    // out_g = finish( (sigma_g(c_0), 0), sum_j sigma_g(D_j) (.) K_g ), D_j the digits op_switch_key forms for the target c_1.
    // The digits are built once per item (ks_digits); per element there is the inner product, which reads them through T_g
    // (hoist.hip), sigma_g(c_0), and the mod-down (ks_finish). out is element-major, out[slot][count][2][k][N]: element i goes
    // to slot slots[i] (increasing; null: slot i), so a caller can leave slots out for results it fills itself
    // (rotate_vector_many's step 0) and still have one decomposition for all the others.
    void op_apply_galois_many(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *elts,
                              const KSwitchKey *const *keys, std::size_t n_elts, u64 *out, const std::uint32_t *slots)
    {
        if (k > e.k_first)
            throw std::invalid_argument("key switching needs a ciphertext level");
        const bool ckks = e.scheme == 2;
        if (!ckks && !e.mode_strict)
            // (the fork multiplies the coefficient-form target rows as they are, SURVEY F3: that key switch does not decrypt,
            //  and there is no reference behaviour to reproduce for an operation the fork does not have)
            throw std::invalid_argument("hoisted rotation of BFV ciphertexts needs a STRICT context");
        LevelTools &ld = e.level(k);
        const KsDev &h = ld.h_ks;
        const int nd = h.nd, rows = k + e.nsp;
        GaloisAxis ax = check_axis(e, nd, elts, keys, n_elts, false);
        if (!n_elts || !count)
            return;
        load_tables(e, ax);
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::size_t w_coeff = poly; // (CKKS: c_1 in coefficient form; STRICT BFV: c_1 in NTT form)
        const std::size_t w_ext = static_cast<std::size_t>(nd) * rows * N;
        const std::size_t w_prod = 2ull * rows * N;
        const std::size_t w_temp = 2ull * poly;
        // arena of one item: the digits once, and per element the products, the mod-down's temporaries and sigma_g(c_0)
        const std::size_t base_bytes = (w_coeff + w_ext) * sizeof(u64), elt_bytes = (w_prod + w_temp + poly) * sizeof(u64);
        // when not even one item fits with all its elements, the element list is walked in passes and the digits stay live
        const std::size_t pass = plan_pass(e, base_bytes, elt_bytes, n_elts);
        unsigned *const sink = e.lane().tsink_cur; // one flag per output ciphertext, in output order
        for_chunks(e, count, base_bytes + pass * elt_bytes, 5, [&](std::size_t off, std::size_t m) {
            u64 *coeff = e.ws_alloc(w_coeff * m);
            u64 *ext = e.ws_alloc(w_ext * m);
            u64 *prod = e.ws_alloc(w_prod * m * pass);
            u64 *temp = e.ws_alloc(w_temp * m * pass);
            u64 *gal = e.ws_alloc(poly * m * pass);
            const u64 *c = ct + off * 2 * poly;
            const std::size_t ext_item = static_cast<std::size_t>(rows) * N;
            const KsRows in_bundle = ks_digits(e, ld, k, c + poly, 2 * poly, m, coeff, ext, 0, nd);
            for (std::size_t e0 = 0; e0 < n_elts; e0 += pass)
            {
                const std::size_t n1 = std::min(pass, n_elts - e0);
                for (std::size_t l0 = 0; l0 < n1; l0 += kHoistMaxElts)
                {
                    HoistElts he{};
                    he.n = static_cast<int>(std::min<std::size_t>(kHoistMaxElts, n1 - l0));
                    for (int i = 0; i < he.n; i++)
                    {
                        he.elt[i] = elts[e0 + l0 + i];
                        he.table[i] = ax.tables[e0 + l0 + i];
                        he.key[i] = keys[e0 + l0 + i]->d_data;
                    }
                    check(launch_hoist_mac(e, ld.d_ks, h, in_bundle.inb, in_bundle.inb_stride, ext, ext_item, ext_item * m, he,
                                           prod + l0 * m * w_prod, w_prod, m),
                          "hoist_mac");
                    check(launch_hoist_galois_c0(e, c, 2 * poly, gal + l0 * m * poly, m, ld.map_q, he, ckks), "galois(c0)");
                }
                // the back half of the key switch over the products of this pass: when the chunk is the whole batch the
                // outputs of consecutive slots are contiguous and go as one batch, else one batch per element
                const auto slot = [&](std::size_t i) { return slots ? static_cast<std::size_t>(slots[i]) : i; };
                for (std::size_t l = 0, run; l < n1; l += run)
                {
                    run = 1;
                    while (m == count && l + run < n1 && slot(e0 + l + run) == slot(e0 + l + run - 1) + 1)
                        run++;
                    const std::size_t first = slot(e0 + l) * count + off; // (output ciphertext, and its transparency flag)
                    ks_finish(e, ld, k, prod + l * m * w_prod, temp + l * m * w_temp, out + first * 2 * poly, 2 * poly,
                              gal + l * m * poly, poly, run * m, sink ? sink + first : nullptr);
                }
            }
        });
    }
    // ------------------------------------------------------------------------------------------
    // Plaintext-weighted sum of rotations: out_s = sum_i W[s][i] * sigma_{g_i}(ct), one decomposition
    // of c_1 per ciphertext and one mod-down per sum
    // ------------------------------------------------------------------------------------------
    namespace
    {
        // BFV: both components of the chunk's m ciphertexts go to NTT form in cntt; CKKS (cntt null) reads them in place
        const u64 *components_ntt(Engine &e, LevelTools &ld, int k, const u64 *c, u64 *cntt, std::size_t m)
        {
            if (!cntt)
                return c;
            const std::size_t poly = static_cast<std::size_t>(k) * e.n;
            SEALHIP_CHECK(hipMemcpyAsync(cntt, c, m * 2 * poly * sizeof(u64), hipMemcpyDeviceToDevice, e.lane().stream));
            check(launch_ntt(e, cntt, m * 2 * k, ld.map_q, false, kNttCanonical), "ntt(ct)");
            return cntt;
        }

        // Section 16's inner sums for ns sums of a chunk of m items: base_s (sums base_sum_stride words apart) from every
        // element of the axis, acc_s (acc[ns][m][2][k + nsp][N]) from those that need a key switch, both in launches of up
        // to kHoistMaxElts elements, the later ones adding in. w0: the plaintext of (first sum, element 0); cn: the
        // components in NTT form; in_bundle, ext: the digits of c_1 (ks_digits).
        void hoist_dot_sums(Engine &e, LevelTools &ld, int k, const GaloisAxis &ax, const u64 *cn, const KsRows &in_bundle,
                            const u64 *ext, std::size_t m, const u64 *w0, u64 *base, std::size_t base_sum_stride, u64 *acc,
                            std::size_t ns)
        {
            const KsDev &h = ld.h_ks;
            const std::size_t ext_item = static_cast<std::size_t>(k + e.nsp) * e.n;
            const std::size_t w_plain = static_cast<std::size_t>(h.n_total) * e.n, w_sum_stride = ax.n * w_plain;
            HoistDotElts he{};
            bool launched = false;
            for (std::size_t i = 0; i < ax.n; i++)
            {
                he.table[he.n] = ax.tables[i];
                he.key[he.n] = nullptr;
                he.w[he.n++] = w0 + i * w_plain;
                if (he.n == kHoistMaxElts || i + 1 == ax.n)
                {
                    check(launch_hoist_dot_base(e, cn, he, w_sum_stride, base, base_sum_stride, k, m, ns, launched),
                          "hoist_dot_base");
                    he.n = 0;
                    launched = true;
                }
            }
            launched = false;
            for (std::size_t i = 0, seen = 0; i < ax.n; i++)
            {
                if (ax.elts[i] == 1)
                    continue;
                he.table[he.n] = ax.tables[i];
                he.key[he.n] = ax.keys[i]->d_data;
                he.w[he.n++] = w0 + i * w_plain;
                seen++;
                if (he.n == kHoistMaxElts || seen == ax.n_gal)
                {
                    check(launch_hoist_dot_mac(e, ld.d_ks, h, in_bundle.inb, in_bundle.inb_stride, ext, ext_item, ext_item * m, he,
                                               w_sum_stride, acc, 2 * ext_item, m, ns, launched),
                          "hoist_dot_mac");
                    he.n = 0;
                    launched = true;
                }
            }
        }

        // The end of a weighted sum, for n ciphertexts: base (in NTT form, two polynomials of k rows each) goes back to
        // coefficient form for BFV, and the accumulated products (acc, with the mod-down's temp; null: no key-switch term)
        // come down into it -- ks_finish, the result replaces base. rescale (CKKS): the result goes to
        // dst at the level below instead, through the merged finish or, with acc = 0, rescale_to_next of base with the exact
        // transform: a nested chunk loop, for which the guard's floor is raised over the parked_bytes that hold base.
        // sink: the flags of these n ciphertexts (null: none); where no finish notes them, a pass over the result does.
        void finish_sum(Engine &e, LevelTools &ld, int k, u64 *base, u64 *acc, u64 *temp, u64 *dst, std::size_t n,
                        unsigned *sink, bool rescale, FloorRestore &guard, std::size_t parked_bytes)
        {
            const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
            if (e.scheme != 2)
                check(launch_ntt(e, base, n * 2 * k, ld.map_q, true, kNttCanonical), "intt(base)");
            if (rescale && acc)
                ks_finish_rescale(e, ld, k, base, 2 * poly, acc, temp, dst, n, sink);
            else if (rescale)
            {
                guard.raise(parked_bytes);
                mod_switch_polys(e, k, base, poly, dst, poly - N, n * 2, true);
                if (sink)
                    check(launch_nonzero_tail(e, dst, 2 * (poly - N), poly - N, n, sink), "transparency");
            }
            else if (acc)
                ks_finish(e, ld, k, acc, temp, base, 2 * poly, nullptr, 0, n, sink);
            else if (sink)
                check(launch_nonzero_tail(e, base, 2 * poly, poly, n, sink), "transparency");
        }

        // the checks the two weighted forms share, in the order they fire; returns the level's tools
        LevelTools &check_weighted_form(Engine &e, int k, bool rescale)
        {
            if (k > e.k_first)
                throw std::invalid_argument("key switching needs a ciphertext level");
            const bool ckks = e.scheme == 2;
            if (rescale && !ckks)
                throw std::invalid_argument("the merged rescale is a CKKS operation");
            if (rescale && k < 2)
                throw std::invalid_argument("end of modulus switching chain reached");
            if (!ckks && !e.mode_strict)
                throw std::invalid_argument("hoisted rotation of BFV ciphertexts needs a STRICT context");
            return rescale ? e.level_rescale(k) : e.level(k);
        }
    } // namespace

    // The plaintexts (key-level NTT form) multiply the key-switch inner products while these are still in the extended basis
    // (hoist.hip, hoist_dot_mac); the weighted products are summed there and ks_finish brings each sum down once, adding it
    // into base_s = (sum_i W (.) sigma_i(C_0), sum_{i identity} W (.) C_1), which the base kernel writes straight into out.
    void op_apply_galois_dot_plain(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *elts,
                                   const KSwitchKey *const *keys, std::size_t n_elts, const u64 *plain_ntt,
                                   std::size_t n_sums, u64 *out, bool rescale)
    {
        LevelTools &ld = check_weighted_form(e, k, rescale);
        const bool ckks = e.scheme == 2;
        const KsDev &h = ld.h_ks;
        const int nd = h.nd, rows = k + e.nsp;
        GaloisAxis ax = check_axis(e, nd, elts, keys, n_elts, true);
        const std::size_t n_gal = ax.n_gal;
        if (!count)
            return;
        if (!n_elts || !n_sums)
            throw std::invalid_argument("an empty sum of rotations is a transparent ciphertext");
        load_tables(e, ax);
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::size_t w_plain = static_cast<std::size_t>(h.n_total) * N, w_sum_stride = n_elts * w_plain;
        const std::size_t w_coeff = n_gal ? poly : 0;
        const std::size_t w_ext = n_gal ? static_cast<std::size_t>(nd) * rows * N : 0;
        const std::size_t w_cn = ckks ? 0 : 2 * poly; // (BFV: both components in NTT form)
        const std::size_t w_prod = n_gal ? 2ull * rows * N : 0;
        // rescale: out is the level below, out[n_sums][count][2][k-1][N], so base_s lives in the
        // arena (at its front: without a Galois element the finish is the plain rescale of base_s, a nested chunk loop, and
        // the floor is raised over base_s) and the merged finish writes out
        const std::size_t poly_out = rescale ? poly - N : poly;
        const std::size_t w_temp = n_gal ? 2ull * poly_out : 0;
        const std::size_t w_base = rescale ? 2 * poly : 0, w_ms = rescale && !n_gal ? 2 * poly : 0;
        // arena of one item: the digits (and BFV's transformed components) once, per sum the accumulated products and the
        // mod-down's temporaries; base_s lives in out
        const std::size_t base_bytes = (w_coeff + w_ext + w_cn) * sizeof(u64),
                          sum_bytes = (w_prod + w_temp + w_base + w_ms) * sizeof(u64);
        // when not even one item fits with all its sums, the sum list is walked in passes and the digits stay live
        const std::size_t pass = plan_pass(e, base_bytes, sum_bytes, n_sums);
        unsigned *const sink = e.lane().tsink_cur; // one flag per output ciphertext, in output order
        for_chunks(e, count, base_bytes + pass * sum_bytes, rescale ? 8 : 5, [&](std::size_t off, std::size_t m) {
            u64 *basebuf = rescale ? e.ws_alloc(w_base * m * pass) : nullptr;
            u64 *coeff = n_gal ? e.ws_alloc(w_coeff * m) : nullptr;
            u64 *ext = n_gal ? e.ws_alloc(w_ext * m) : nullptr;
            u64 *cntt = w_cn ? e.ws_alloc(w_cn * m) : nullptr;
            u64 *acc = n_gal ? e.ws_alloc(w_prod * m * pass) : nullptr;
            u64 *temp = n_gal ? e.ws_alloc(w_temp * m * pass) : nullptr;
            FloorRestore restore(e);
            const u64 *c = ct + off * 2 * poly;
            KsRows in_bundle{ nullptr, 0 };
            if (n_gal)
                in_bundle = ks_digits(e, ld, k, c + poly, 2 * poly, m, coeff, ext, 0, nd);
            const u64 *cn = components_ntt(e, ld, k, c, cntt, m);
            for (std::size_t s0 = 0; s0 < n_sums; s0 += pass)
            {
                const std::size_t ns = std::min(pass, n_sums - s0);
                // base of sum s0 + s of this chunk: o + s * o_sum
                u64 *o = rescale ? basebuf : out + (s0 * count + off) * 2 * poly;
                const std::size_t o_sum = rescale ? m * 2 * poly : count * 2 * poly;
                hoist_dot_sums(e, ld, k, ax, cn, in_bundle, ext, m, plain_ntt + s0 * w_sum_stride, o, o_sum, acc, ns);
                // the back half once per sum: when the chunk is the whole batch the sums of this pass are one contiguous
                // batch of ns * m ciphertexts, else one batch per sum
                const std::size_t run = m == count ? ns : 1;
                for (std::size_t s = 0; s < ns; s += run)
                {
                    const std::size_t first = (s0 + s) * count + off; // (output ciphertext, and its transparency flag)
                    finish_sum(e, ld, k, o + s * o_sum, n_gal ? acc + s * m * w_prod : nullptr, temp + s * m * w_temp,
                               out + first * 2 * poly_out, run * m, sink ? sink + first : nullptr, rescale, restore,
                               pad256(w_base * m * pass));
                }
            }
        });
    }
    // ------------------------------------------------------------------------------------------
    // Baby-step/giant-step matrix-vector product:
    //     out = sum_j sigma_{h_j}( sum_i W[j][i] * sigma_{g_i}(ct) ), the giant steps accumulated in the extended basis
    // ------------------------------------------------------------------------------------------
    // Per inner sum j section 16's base_j and acc_j go to workspace. Only component 1 of a non-identity giant's inner sum is
    // brought down (ks_finish at polynomial granularity): d_j, which the giant's key switch decomposes. Its inner product
    // with K_h, the permuted acc_j[0] and, in Q, the permuted base_j[0] are accumulated (ACC in the arena, BASE in out), and
    // ONE ks_finish brings the whole product down.
    void op_apply_galois_bsgs_plain(Engine &e, int k, const u64 *ct, std::size_t count, const std::uint32_t *baby_elts,
                                    const KSwitchKey *const *baby_keys, std::size_t n_baby, const std::uint32_t *giant_elts,
                                    const KSwitchKey *const *giant_keys, std::size_t n_giant, const u64 *plain_ntt, u64 *out,
                                    bool rescale)
    {
        LevelTools &ld = check_weighted_form(e, k, rescale);
        const bool ckks = e.scheme == 2;
        const KsDev &h = ld.h_ks;
        const int nd = h.nd, rows = k + e.nsp;
        GaloisAxis baby = check_axis(e, nd, baby_elts, baby_keys, n_baby, true);
        GaloisAxis giant = check_axis(e, nd, giant_elts, giant_keys, n_giant, true);
        const std::size_t n_gb = baby.n_gal, n_gg = giant.n_gal;
        if (!count)
            return;
        if (!n_baby || !n_giant)
            throw std::invalid_argument("an empty sum of rotations is a transparent ciphertext");
        load_tables(e, baby);
        load_tables(e, giant);
        const std::vector<const std::uint32_t *> &gtab = giant.tables;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::size_t w_plain = static_cast<std::size_t>(h.n_total) * N, w_sum_stride = n_baby * w_plain;
        const std::size_t ext_item = static_cast<std::size_t>(rows) * N;
        const std::size_t w_digits = static_cast<std::size_t>(nd) * ext_item, w_prod = 2 * ext_item;
        const bool any_acc = n_gb || n_gg;
        // arena of one item. Once: the input's digits (when a baby differs from 1), BFV's transformed components, ACC and
        // the final mod-down's temporaries (when any ACC term is formed); BASE lives in out. Per giant of a pass: base_j,
        // acc_j (when a baby differs from 1) and, when a giant differs from 1, d_j, the one-component mod-down's
        // temporaries and d_j's digits (identity giants leave theirs unused: one size for every giant keeps the plan simple).
        const std::size_t w_coeff = n_gb ? poly : 0, w_ext = n_gb ? w_digits : 0;
        const std::size_t w_cn = ckks ? 0 : 2 * poly;
        // rescale: out is the level below, so BASE lives at the front of the arena (the floor is raised
        // over it when the finish is a plain rescale: no ACC term) and the ONE final finish is the merged one
        const std::size_t poly_out = rescale ? poly - N : poly;
        const std::size_t w_BASE = rescale ? 2 * poly : 0, w_ms = rescale && !any_acc ? 2 * poly : 0;
        const std::size_t w_acc = any_acc ? w_prod : 0, w_temp = any_acc ? 2 * poly_out : 0;
        const std::size_t w_accj = n_gb ? w_prod : 0;
        const std::size_t w_d = n_gg ? poly : 0, w_temp1 = n_gg && n_gb ? poly : 0;
        const std::size_t w_coeff2 = n_gg ? poly : 0, w_ext2 = n_gg ? w_digits : 0;
        const std::size_t base_bytes = (w_coeff + w_ext + w_cn + w_acc + w_temp + w_BASE + w_ms) * sizeof(u64);
        const std::size_t giant_bytes = (2 * poly + w_accj + w_d + w_temp1 + w_coeff2 + w_ext2) * sizeof(u64);
        // when not even one item fits with all its giants, the giant list is walked in passes
        const std::size_t pass = plan_pass(e, base_bytes, giant_bytes, n_giant);
        unsigned *const sink = e.lane().tsink_cur; // one flag per output ciphertext
        for_chunks(e, count, base_bytes + pass * giant_bytes, rescale ? 14 : 11, [&](std::size_t off, std::size_t m) {
            u64 *BASEbuf = rescale ? e.ws_alloc(w_BASE * m) : nullptr;
            FloorRestore restore(e);
            u64 *coeff = w_coeff ? e.ws_alloc(w_coeff * m) : nullptr;
            u64 *ext = w_ext ? e.ws_alloc(w_ext * m) : nullptr;
            u64 *cntt = w_cn ? e.ws_alloc(w_cn * m) : nullptr;
            u64 *ACC = w_acc ? e.ws_alloc(w_acc * m) : nullptr;
            u64 *temp = w_temp ? e.ws_alloc(w_temp * m) : nullptr;
            u64 *bw = e.ws_alloc(2 * poly * m * pass);
            u64 *accj = w_accj ? e.ws_alloc(w_accj * m * pass) : nullptr;
            u64 *dbuf = w_d ? e.ws_alloc(w_d * m * pass) : nullptr;
            u64 *temp1 = w_temp1 ? e.ws_alloc(w_temp1 * m * pass) : nullptr;
            u64 *coeff2 = w_coeff2 ? e.ws_alloc(w_coeff2 * m * pass) : nullptr;
            u64 *ext2 = w_ext2 ? e.ws_alloc(w_ext2 * m * pass) : nullptr;
            const u64 *c = ct + off * 2 * poly;
            u64 *o = rescale ? BASEbuf : out + off * 2 * poly; // BASE of this chunk, then (without rescale) the result
            KsRows in_bundle{ nullptr, 0 };
            if (n_gb)
                in_bundle = ks_digits(e, ld, k, c + poly, 2 * poly, m, coeff, ext, 0, nd);
            const u64 *cn = components_ntt(e, ld, k, c, cntt, m);
            bool acc_started = false, base_started = false;
            for (std::size_t g0 = 0; g0 < n_giant; g0 += pass)
            {
                const std::size_t ng = std::min(pass, n_giant - g0);
                // base_j and acc_j of the pass's inner sums: section 16's launches, into workspace
                hoist_dot_sums(e, ld, k, baby, cn, in_bundle, ext, m, plain_ntt + g0 * w_sum_stride, bw, m * 2 * poly, accj, ng);
                // d_j of the pass's non-identity giants, back to back in dbuf (target t = slot * m + item): base_j[1], for
                // BFV in coefficient form, plus the mod-down of acc_j[1] -- one batch per run of consecutive such giants
                std::vector<std::size_t> slot(ng, 0);
                std::size_t n_nz = 0;
                for (std::size_t s = 0; s < ng; s++)
                    if (giant_elts[g0 + s] != 1)
                        slot[s] = n_nz++;
                KsRows in2{ nullptr, 0 };
                if (n_nz)
                {
                    const auto for_runs = [&](const std::function<void(std::size_t s, std::size_t run)> &fn) {
                        for (std::size_t s = 0, run; s < ng; s += run)
                        {
                            run = 1;
                            if (giant_elts[g0 + s] == 1)
                                continue;
                            while (s + run < ng && giant_elts[g0 + s + run] != 1)
                                run++;
                            fn(s, run);
                        }
                    };
                    for_runs([&](std::size_t s, std::size_t run) {
                        check(launch_copy_rows(e, bw + s * m * 2 * poly + poly, 2 * poly, dbuf + slot[s] * m * poly, poly, run * m,
                                               k),
                              "copy(base_1)");
                    });
                    if (!ckks)
                        check(launch_ntt(e, dbuf, n_nz * m * k, ld.map_q, true, kNttCanonical), "intt(base_1)");
                    if (n_gb)
                        for_runs([&](std::size_t s, std::size_t run) {
                            ks_finish(e, ld, k, accj + s * m * w_prod + ext_item, temp1 + slot[s] * m * poly,
                                      dbuf + slot[s] * m * poly, 2 * poly, nullptr, 0, run * m, nullptr, true);
                        });
                    // the giants' decompositions: the d_j of the pass as one batch of targets
                    in2 = ks_digits(e, ld, k, dbuf, poly, n_nz * m, coeff2, ext2, 0, nd);
                }
                // ACC: the giants' inner products and the acc_j (an identity giant without acc_j contributes nothing)
                HoistGiantElts ge{};
                std::size_t last = ng;
                for (std::size_t s = 0; s < ng; s++)
                    if (giant_elts[g0 + s] != 1 || n_gb)
                        last = s;
                for (std::size_t s = 0; s < ng && last < ng; s++)
                {
                    const bool ident = giant_elts[g0 + s] == 1;
                    if (!ident || n_gb)
                    {
                        ge.table[ge.n] = gtab[g0 + s];
                        ge.key[ge.n] = ident ? nullptr : giant_keys[g0 + s]->d_data;
                        ge.inb[ge.n] = ident ? nullptr : in2.inb + slot[s] * m * in2.inb_stride;
                        ge.ext[ge.n] = ident ? nullptr : ext2 + slot[s] * m * ext_item;
                        ge.accj[ge.n++] = n_gb ? accj + s * m * w_prod : nullptr;
                    }
                    if (ge.n == kHoistMaxElts || (s == last && ge.n))
                    {
                        check(launch_hoist_giant_mac(e, ld.d_ks, h, ge, in2.inb_stride, ext_item, ext_item * n_nz * m, w_prod, ACC,
                                                     w_prod, m, acc_started),
                              "hoist_giant_mac");
                        ge.n = 0;
                        acc_started = true;
                    }
                }
                // BASE: the permuted base_j[0], and base_j[1] of the identity giants
                HoistGiantBases gb{};
                for (std::size_t s = 0; s < ng; s++)
                {
                    gb.table[gb.n] = gtab[g0 + s];
                    gb.base[gb.n++] = bw + s * m * 2 * poly;
                    if (gb.n == kHoistMaxElts || s + 1 == ng)
                    {
                        check(launch_hoist_giant_base(e, gb, o, k, m, base_started), "hoist_giant_base");
                        gb.n = 0;
                        base_started = true;
                    }
                }
            }
            // ONE finish brings the whole product down (ACC is null when no term was formed)
            finish_sum(e, ld, k, o, ACC, temp, out + off * 2 * poly_out, m, sink ? sink + off : nullptr, rescale, restore,
                       pad256(w_BASE * m));
        });
    }
    // multiply_plain_normal (evaluator.cpp:1475-1603) for parameters with fast plain lift (every q_i > t): lift the
    // plaintext into the RNS base, canonical NTT, then per ciphertext polynomial lazy NTT -> dyadic product ->
    // canonical inverse NTT, in place. The monomial shortcut (:1516-1553) computes the same negacyclic product
    // exactly, so its canonical residues are identical to the generic path's; one path serves both.
    void op_multiply_plain(Engine &e, int k, u64 *ct, int size, std::size_t count, const u64 *plain,
                           std::size_t plain_stride)
    {
        if (e.scheme != 1)
            throw std::logic_error("unsupported operation for scheme type");
        const RowMap map_q = e.level_host(k).map_q;
        for (int r = 0; r < k; r++)
            if (e.key_moduli[r] <= e.t)
                throw std::logic_error("multiply_plain: parameters without fast plain lift are not supported");
        const std::size_t N = e.n;
        const std::size_t nplains = plain_stride ? count : 1;
        const std::size_t bytes = nplains * k * N * sizeof(u64);
        e.ws_reserve(e.lane().ws_floor + bytes + 256);
        e.ws_reset();
        u64 *temp = e.ws_alloc(nplains * k * N);
        check(launch_plain_lift(e, plain, plain_stride, temp, nplains, map_q, e.t), "plain_lift");
        check(launch_ntt(e, temp, nplains * k, map_q, false, kNttCanonical), "ntt(plain)");
        check(launch_ntt(e, ct, count * size * k, map_q, false, kNttAnyRep), "ntt(ct)"); // (the dyadic product reduces)
        check(launch_ct_linear(e, CtLinearOp::MulPlain, ct, size, temp, 0, plain_stride ? static_cast<std::size_t>(k) * N : 0,
                               ct, count, map_q),
              "dyadic(plain)");
        check(launch_ntt(e, ct, count * size * k, map_q, true, kNttCanonical), "intt(ct)");
    }
    // Evaluator::transform_to_ntt(Plaintext) (evaluator.cpp:1648-1744), BFV, every parameter set: each plaintext lifted to
    // the k primes of the level (one formula serves the fast and the general branch, poly.hip) straight into the
    // destination, then the canonical transform in place. (A lift fused into the single-pass transform's load phase was
    // built and measured: faster than this, slower than the transform alone -- not adopted)
    void op_transform_plain_to_ntt(Engine &e, int k, const u64 *plain, std::size_t coeff_count, std::size_t plain_stride,
                                   std::size_t count, u64 *plain_ntt)
    {
        if (count == 0)
            return;
        const RowMap map_q = e.level_host(k).map_q;
        check(launch_plain_lift_centered(e, plain, coeff_count, plain_stride ? plain_stride : coeff_count, plain_ntt, count,
                                         map_q, e.t),
              "plain_lift");
        check(launch_ntt(e, plain_ntt, count * k, map_q, false, kNttCanonical), "ntt(plain)");
    }
    namespace
    {
        // dot_product_ct_sk_array of m coefficient-form items of size >= 2 into out[m][k][N]: copies of c_1.. go to (lazy)
        // NTT form (decryptor.cpp:241-244), the sum comes back canonical (:258-262), then + c_0 (:265). The body of one arena
        // chunk: the copies ((size-1) x k x N words per item) and, when the caller passes no `out`, the result (k x N words per
        // item, for the caller's next launch) are carved from the arena. Returns the result.
        u64 *dot_product_coeff_chunk(Engine &e, int k, const RowMap &map_q, const u64 *ct, int size, std::size_t m,
                                     const u64 *sk_powers, u64 *out = nullptr)
        {
            const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
            const std::size_t sk_stride = static_cast<std::size_t>(e.n_key) * N;
            const std::size_t item = static_cast<std::size_t>(size) * poly, tail = item - poly;
            u64 *copy = e.ws_alloc(tail * m);
            if (!out)
                out = e.ws_alloc(poly * m);
            check(launch_copy_rows(e, ct + poly, item, copy, tail, m, (size - 1) * k), "copy(c1..)");
            check(launch_ntt(e, copy, m * (size - 1) * k, map_q, false, kNttAnyRep), "ntt(c1..)"); // (the dot product reduces)
            // the kernel indexes polynomials 1.. of an item: hand it a base one polynomial before the copies
            check(launch_dot_sk(e, copy - poly, size, tail, sk_powers, sk_stride, out, m, map_q, 0), "dot_sk");
            check(launch_ntt(e, out, m * k, map_q, true, kNttCanonical), "intt(dot)");
            check(launch_dot_sk(e, ct, 1, item, sk_powers, sk_stride, out, m, map_q, 2), "add c0");
            return out;
        }
    } // namespace

    // Decryptor::dot_product_ct_sk_array (decryptor.cpp:218-265): out[count][k][N] = c_0 + sum_{i>=1} c_i * s^i in the
    // form of the ciphertext. sk_powers = (size-1) polynomials s, s^2, ... in NTT form with key-level row stride.
    void op_dot_product_ct_sk(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers,
                              bool is_ntt_form, u64 *out)
    {
        const RowMap map_q = e.level_host(k).map_q;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const std::size_t sk_stride = static_cast<std::size_t>(e.n_key) * N;
        const std::size_t item = static_cast<std::size_t>(size) * poly;
        if (is_ntt_form || size == 1)
        {
            check(launch_dot_sk(e, ct, size, item, sk_powers, sk_stride, out, count, map_q, 1), "dot_sk");
            return;
        }
        const std::size_t tail = static_cast<std::size_t>(size - 1) * poly;
        for_chunks(e, count, tail * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            dot_product_coeff_chunk(e, k, map_q, ct + off * item, size, m, sk_powers, out + off * poly);
        });
    }

    void op_invariant_noise_budget(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers,
                                   std::int32_t *budgets)
    {
        const NoiseBudgetDev *consts = e.noise_budget_consts(k);
        const int q_bits = e.total_coeff_modulus_bit_count(k);
        const RowMap map_q = ct_row_map(k, 1, -1); // (the level's BEHZ tools are not needed, nor built)
        const std::size_t item = static_cast<std::size_t>(size) * k * e.n;
        // one bit count per item, at the FRONT of the arena (ws_floor) for the whole batch; the chunks use the rest
        const std::size_t flag_bytes = (count * sizeof(int) + 255) & ~static_cast<std::size_t>(255);
        FloorRestore guard(e);
        guard.raise(flag_bytes);
        int *bits = nullptr;
        for_chunks(e, count, item * sizeof(u64), 2, [&](std::size_t off, std::size_t m) {
            if (off == 0) // (sizing the chunks may have moved the arena: the flags are addressed, and cleared, after it)
            {
                bits = static_cast<int *>(guard.parked());
                check(hipMemsetAsync(bits, 0, count * sizeof(int), e.lane().stream), "memset(bits)");
            }
            const u64 *v = dot_product_coeff_chunk(e, k, map_q, ct + off * item, size, m, sk_powers);
            check(launch_noise_bits(e, consts, k, v, m, bits + off), "noise_budget");
        });
        std::vector<int> host(count);
        check(hipMemcpyAsync(host.data(), bits, count * sizeof(int), hipMemcpyDeviceToHost, e.lane().stream), "d2h(bits)");
        e.sync_and_check();
        // decryptor.cpp:318-324: the -1 accounts for scaling the invariant noise by 2
        for (std::size_t i = 0; i < count; i++)
            budgets[i] = std::max(0, q_bits - host[i] - 1);
    }

    void op_decrypt(Engine &e, int k, const u64 *ct, int size, std::size_t count, const u64 *sk_powers, u64 *plain)
    {
        if (e.scheme == 2) // ckks_decrypt (:122-150): the dot product in NTT form is the plaintext
        {
            op_dot_product_ct_sk(e, k, ct, size, count, sk_powers, true, plain);
            return;
        }
        LevelTools &lt = e.level(k);
        const std::size_t N = e.n, item = static_cast<std::size_t>(size) * k * N;
        // bfv_decrypt (:77-120): dot product, then decrypt_scale_and_round into the plaintext
        for_chunks(e, count, item * sizeof(u64), 2, [&](std::size_t off, std::size_t m) {
            const u64 *v = dot_product_coeff_chunk(e, k, lt.map_q, ct + off * item, size, m, sk_powers);
            check(launch_decrypt_scale_and_round(e, lt.d_rns, lt.h_rns, v, plain + off * N, m), "decrypt_scale_and_round");
        });
    }
    // ---------------------------------------------------------------- encrypt-side arithmetic
    namespace
    {
        // RlweArgs of the launches that write one polynomial per item (ct_item_stride words apart) from N samples per item
        // (e_item_stride apart)
        RlweArgs rlwe_args(u64 *ct, std::size_t ct_item_stride, int rows, const std::int32_t *samples,
                           std::size_t e_item_stride)
        {
            RlweArgs a{};
            a.ct = ct;
            a.ct_item_stride = ct_item_stride;
            a.polys = 1;
            a.rows = rows;
            a.e = samples;
            a.e_item_stride = e_item_stride;
            return a;
        }
        // ... and of those that write both polynomials of a ciphertext from one x per item: x[item] (.) y[j] and e[item][j]
        RlweArgs rlwe_args_pair(u64 *ct, int rows, const u64 *x, const u64 *y, std::size_t y_poly_stride,
                                const std::int32_t *noise, std::size_t N)
        {
            const std::size_t poly = static_cast<std::size_t>(rows) * N;
            RlweArgs a = rlwe_args(ct, 2 * poly, rows, noise, 2 * N);
            a.ct_poly_stride = poly;
            a.polys = 2;
            a.x = x;
            a.x_item_stride = poly;
            a.y = y;
            a.y_poly_stride = y_poly_stride;
            a.e_poly_stride = N;
            return a;
        }
        // small samples to RNS form in the polynomials `a` writes, then to NTT form: item_rows = the rows of one item
        // (ct_row_map; the polynomials `a` does not write are skipped). `lift`, `ntt`: the names of the two launches.
        void lift_to_ntt(Engine &e, const RlweArgs &a, std::size_t count, const RowMap &item_rows, const char *lift,
                         const char *ntt)
        {
            check(launch_rlwe_stage(e, 0, a, count), lift);
            check(launch_ntt(e, a.ct, count * item_rows.rows, item_rows, false, kNttCanonical), ntt);
        }
        // encrypt_zero_asymmetric (rlwe.cpp:161-201) for the m items of one chunk: u to RNS + NTT form in u_ntt[m][rows][N],
        // then P[m][2][rows][N], P_j = u (.) pk_j + e_j, with the polynomials of pk pk_poly_stride words apart. ntt_form: the
        // result stays in NTT form; else it goes back to coefficient form and e_j is added there, unless add_noise is off
        // (the caller's finish kernel adds it).
        void pk_product_chunk(Engine &e, int rows, const u64 *pk, std::size_t pk_poly_stride, const std::int32_t *u,
                              const std::int32_t *noise, std::size_t m, u64 *u_ntt, u64 *P, bool ntt_form, bool add_noise)
        {
            const std::size_t N = e.n;
            lift_to_ntt(e, rlwe_args(u_ntt, static_cast<std::size_t>(rows) * N, rows, u, N), m, ct_row_map(rows, 1, -1), "lift(u)",
                        "ntt(u)");
            const RlweArgs a = rlwe_args_pair(P, rows, u_ntt, pk, pk_poly_stride, noise, N);
            const RowMap both = ct_row_map(rows, 2, -1);
            if (ntt_form)
            {
                lift_to_ntt(e, a, m, both, "lift(e)", "ntt(e)");
                check(launch_rlwe_stage(e, 2, a, m), "c = e + u*pk");
                return;
            }
            check(launch_rlwe_stage(e, 1, a, m), "u*pk");
            check(launch_ntt(e, P, m * 2 * rows, both, true, kNttCanonical), "intt(c)");
            if (add_noise)
                check(launch_rlwe_stage(e, 3, a, m), "c += e");
        }
    } // namespace

    void op_encrypt_zero_symmetric(Engine &e, int rows, bool is_ntt_form, const u64 *a_ntt, const std::int32_t *noise,
                                   const u64 *sk_ntt, std::size_t count, u64 *ct)
    {
        const std::size_t N = e.n, poly = static_cast<std::size_t>(rows) * N;
        u64 *c1 = ct + poly;
        if (c1 != a_ntt) // c_1 = a, sampled directly in NTT form (rlwe.cpp:245-249)
            check(launch_copy_rows(e, a_ntt, poly, c1, 2 * poly, count, rows), "copy(a)");
        RlweArgs a = rlwe_args(ct, 2 * poly, rows, noise, N);
        a.x = c1;
        a.x_item_stride = 2 * poly;
        a.y = sk_ntt;
        a.negate = 1;
        if (is_ntt_form)
        {
            // noise to NTT form in the c_0 slot, then c_0 = -(noise + a*s)  (rlwe.cpp:266-284)
            lift_to_ntt(e, a, count, ct_row_map(rows, 2, 0), "lift(e)", "ntt(e)");
            check(launch_rlwe_stage(e, 2, a, count), "c0");
        }
        else
        {
            // c_0 = a*s back to coefficient form, c_0 = -(noise + c_0), and c_1 to coefficient form (:286-293)
            check(launch_rlwe_stage(e, 1, a, count), "a*s");
            check(launch_ntt(e, ct, count * 2 * rows, ct_row_map(rows, 2, -1), true, kNttCanonical), "intt(c0, c1)");
            check(launch_rlwe_stage(e, 3, a, count), "c0");
        }
    }

    // KeyGenerator::generate_one_kswitch_key (keygenerator.cpp:325-369) for every key of the batch, in the key buffers:
    //   1. c0 of every digit = NTT(lift(e_j)) over all key rows: the lift stage and the forward transform of
    //      encrypt_zero_symmetric (rlwe.cpp:266-278) with the key's digit stride 2 x n_key x N;
    //   2. c1 of every digit = sample_poly_uniform(BlakePRNG(seed_j)) (rlwe.cpp:245-249): one seed-expansion job list;
    //   3. kswitch_keygen_assemble: c0 = -(c0 + c1 (.) s), plus factor_r * new_key[r] on the digit's rows (:350-366).
    // The new key is read through the Galois permutation inside the kernel (no rotated secret key is stored); the relin
    // keys' powers sk^2.. are built once by dyadic products (compute_secret_key_array, :262-323).
    void op_generate_kswitch_keys(Engine &e, const u64 *sk_ntt, const std::uint32_t *elts, std::size_t n_keys,
                                  const std::uint64_t *seeds_host, const std::int32_t *noise, u64 *const *key_data,
                                  const u64 *s_from, int level)
    {
        if (n_keys == 0)
            return;
        const int nk = e.n_key;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(nk) * N, digit_words = 2 * poly;
        const int digits = (e.k_first + e.nsp - 1) / e.nsp;
        const RowMap c0_rows = ct_row_map(nk, 2, 0);
        for (std::size_t i = 0; i < n_keys; i++)
            lift_to_ntt(e, rlwe_args(key_data[i], digit_words, nk, noise + i * digits * N, N), digits, c0_rows, "lift(e)",
                        "ntt(e)");
        std::vector<SeedJob> jobs(n_keys * digits);
        for (std::size_t i = 0; i < n_keys; i++)
            for (int j = 0; j < digits; j++)
                jobs[i * digits + j] = SeedJob{ seeds_host + 8 * (i * digits + j), key_data[i] + j * digit_words + poly };
        op_expand_seeds(e, nk, jobs.data(), jobs.size());

        hipError_t err = hipSuccess;
        u64 *powers = nullptr; // relin keys: sk^2 .. sk^(n_keys+1), in the lane's arena (free again once expansion is enqueued)
        if (!elts && !s_from)
        {
            e.ws_reset();
            e.ws_reserve(e.lane().ws_floor + n_keys * poly * sizeof(u64) + 256);
            powers = e.ws_alloc(n_keys * poly);
            const RowMap rows = ct_row_map(nk, 1, -1);
            for (std::size_t i = 0; i < n_keys && err == hipSuccess; i++)
                err = launch_poly_op(e, PolyOp::Dyadic, i ? powers + (i - 1) * poly : sk_ntt, sk_ntt, 0, powers + i * poly, nk,
                                     rows);
        }
        KeygenArgs g{};
        g.sk = sk_ntt;
        g.digits = digits;
        g.n_key = nk;
        g.nsp = e.nsp;
        g.n_ct = e.k_first;
        for (int r = 0; r < e.k_first; r++)
        {
            u64 f = 1;
            for (int k = 0; k < e.nsp; k++)
                f = mulmod(f, e.key_moduli[e.k_first + k], e.key_moduli[r]); // multiply_uint_mod, keygenerator.cpp:355-359
            g.factor[r] = f;
        }
        for (std::size_t off = 0; off < n_keys && err == hipSuccess; off += kKeygenMaxKeys)
        {
            g.n_keys = static_cast<int>(std::min<std::size_t>(kKeygenMaxKeys, n_keys - off));
            for (int i = 0; i < g.n_keys; i++)
            {
                g.key[i] = key_data[off + i];
                g.s_new[i] = elts ? sk_ntt : (s_from ? s_from : powers) + (off + i) * poly;
                g.elt[i] = elts ? elts[off + i] : 1u;
            }
            err = launch_keygen_assemble(e, g);
        }
        check(err, "kswitch_keygen_assemble");
        if (s_from && level > 0 && level < e.k_first)
        {
            // what a key for levels <= level never shows: rows level .. n_ct-1 of both components of the digits it keeps,
            // and the digits past ceil(level / nsp) whole
            const int kept = (level + e.nsp - 1) / e.nsp;
            hipStream_t stream = e.lane().stream;
            for (std::size_t i = 0; i < n_keys; i++)
            {
                for (int c = 0; c < 2 * kept; c++)
                    SEALHIP_CHECK(hipMemsetAsync(key_data[i] + (static_cast<std::size_t>(c) * nk + level) * N, 0,
                                                 static_cast<std::size_t>(e.k_first - level) * N * sizeof(u64), stream));
                if (kept < digits)
                    SEALHIP_CHECK(hipMemsetAsync(key_data[i] + kept * digit_words, 0, (digits - kept) * digit_words * sizeof(u64),
                                                 stream));
            }
        }
    }

    // RGSW(m_i): m_i is lifted over the key primes as a secret key is and transformed, m_i s is a
    // dyadic product, and the 2 n halves are the switching keys op_generate_kswitch_keys makes for the new keys
    // {NTT(m_i), NTT(m_i) (.) s}, half h of message i with the seeds and the noise [i][h]. scratch: n x 2 x n_key x N words,
    // erased in stream order once the halves are assembled.
    void op_generate_rgsw(Engine &e, const u64 *sk_ntt, const std::int32_t *m_coeff, std::size_t n, int level,
                          const std::uint64_t *seeds_host, const std::int32_t *noise, u64 *scratch, u64 *const *rgsw)
    {
        if (n == 0)
            return;
        const int nk = e.n_key;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(nk) * N;
        const std::size_t half_words = static_cast<std::size_t>((e.k_first + e.nsp - 1) / e.nsp) * 2 * poly;
        lift_to_ntt(e, rlwe_args(scratch, 2 * poly, nk, m_coeff, N), n, ct_row_map(nk, 2, 0), "lift(m)", "ntt(m)");
        const RowMap rows = ct_row_map(nk, 1, -1);
        std::vector<u64 *> halves(2 * n);
        for (std::size_t i = 0; i < n; i++)
        {
            check(launch_poly_op(e, PolyOp::Dyadic, scratch + 2 * i * poly, sk_ntt, 0, scratch + (2 * i + 1) * poly, nk, rows),
                  "m (.) s");
            halves[2 * i] = rgsw[i];
            halves[2 * i + 1] = rgsw[i] + half_words;
        }
        op_generate_kswitch_keys(e, sk_ntt, nullptr, 2 * n, seeds_host, noise, halves.data(), scratch, level);
        SEALHIP_CHECK(hipMemsetAsync(scratch, 0, 2 * n * poly * sizeof(u64), e.lane().stream));
    }

    void op_encrypt_zero_asymmetric(Engine &e, int rows, bool is_ntt_form, const u64 *pk, const std::int32_t *u,
                                    const std::int32_t *noise, std::size_t count, u64 *ct)
    {
        const std::size_t N = e.n, poly = static_cast<std::size_t>(rows) * N;
        for_chunks(e, count, poly * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *u_ntt = e.ws_alloc(poly * m);
            pk_product_chunk(e, rows, pk, poly, u + off * N, noise + off * 2 * N, m, u_ntt, ct + off * 2 * poly, is_ntt_form, true);
        });
    }

    void fill_scaling_args(const Engine &e, int k, ScalingArgs &a)
    {
        a.k = k;
        a.t = e.t;
        HostModulus tm(e.t);
        a.t_cr0 = tm.cr0;
        a.t_cr1 = tm.cr1;
        a.threshold = (e.t + 1) >> 1; // plain_upper_half_threshold, context.cpp:317
        // coeff_div_plain_modulus = floor(q / t) in RNS form and q mod t (context.cpp:303-321)
        std::vector<u64> q(static_cast<std::size_t>(k), 0), quot(static_cast<std::size_t>(k), 0);
        q[0] = 1;
        for (int i = 0; i < k; i++)
        {
            u128 carry = 0;
            for (int l = 0; l < k; l++)
            {
                const u128 v = static_cast<u128>(q[l]) * e.key_moduli[i] + carry;
                q[l] = static_cast<u64>(v);
                carry = v >> 64;
            }
        }
        u128 rem = 0;
        for (int l = k; l-- > 0;)
        {
            const u128 cur = (rem << 64) | q[l];
            quot[l] = static_cast<u64>(cur / e.t);
            rem = cur % e.t;
        }
        a.q_mod_t = static_cast<u64>(rem);
        for (int j = 0; j < k; j++)
        {
            u128 r = 0;
            for (int l = k; l-- > 0;)
                r = ((r << 64) | quot[l]) % e.key_moduli[j];
            a.div[j] = static_cast<u64>(r);
        }
    }

    void op_scaling_variant(Engine &e, int k, const u64 *plain, std::size_t plain_item_stride, u64 *ct,
                            std::size_t ct_item_stride, std::size_t count, bool sub)
    {
        if (e.scheme != 1)
            throw std::invalid_argument("unsupported scheme");
        ScalingArgs a{};
        fill_scaling_args(e, k, a);
        a.plain = plain;
        a.plain_item_stride = plain_item_stride;
        a.c0 = ct;
        a.c0_item_stride = ct_item_stride;
        a.sub = sub ? 1 : 0;
        check(launch_scaling_variant(e, a, count), "scaling_variant");
    }

    // ---------------------------------------------------------------- Encryptor (encryptor.cpp:106-259)
    // Public key, per chunk of items:
    //   1. u to RNS + NTT form over the R = k + 1 rows of the previous level (k = n_key: R = k) (rlwe.cpp:161-170);
    //   2. BFV: P_j = INTT(u (.) pk_j) (:171-201); the fused tail adds e_j, divides by q_k (rns.cpp:731-775) and adds
    //      Delta m (scalingvariant.cpp:31-51) straight into ct;
    //      CKKS: P_j = NTT(lift(e_j)) + u (.) pk_j; the last row goes through divide_and_round_q_last_ntt_inplace
    //      (rns.cpp:777-851) up to its forward transforms, and the fused tail (rescale_post) writes ct and adds the plaintext.
    // The previous level of the first level has k_first + 1 rows, whatever nsp is (context.cpp:524-538 moves first_parms_id
    // forward by nsp - 1 levels), so the prime dropped can be a special prime.
    void op_encrypt(Engine &e, int k, const u64 *pk, const u64 *plain, std::size_t plain_item_stride, const std::int32_t *u,
                    const std::int32_t *noise, std::size_t count, u64 *ct)
    {
        const bool ckks = e.scheme == 2;
        const int R = k < e.n_key ? k + 1 : k;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(R) * N, out_poly = static_cast<std::size_t>(k) * N;
        const std::size_t pk_poly = static_cast<std::size_t>(e.n_key) * N;
        const bool divide = R == k + 1;
        EncryptArgs f{};
        f.k = k;
        f.rows = R;
        f.ct_item_stride = 2 * out_poly;
        f.src_item_stride = 2 * poly;
        f.plain = plain;
        f.plain_item_stride = plain_item_stride;
        LevelTools *lt = nullptr; // CKKS: the previous level's device constants for rescale_pre
        if (divide)
        {
            // inv_q_last_mod_q of the previous level (rns.cpp:719-728); BFV needs no other RNSTool constant of that level
            for (int i = 0; i < k; i++)
                if (!invmod(e.key_moduli[k], e.key_moduli[i], f.inv_q_last[i]))
                    throw std::logic_error("invalid rns bases");
            if (ckks)
                lt = &e.level(R);
        }
        if (!ckks && plain)
            fill_scaling_args(e, k, f.sc);
        // CKKS at the key level: encrypt_zero_asymmetric straight into ct (no plaintext is valid there)
        const bool direct = ckks && !divide;
        const std::size_t per_item = poly + (direct ? 0 : 2 * poly) + (ckks && divide ? 2 * out_poly : 0);
        for_chunks(e, count, per_item * sizeof(u64), 3, [&](std::size_t off, std::size_t m) {
            u64 *u_ntt = e.ws_alloc(poly * m);
            u64 *P = direct ? ct + off * 2 * out_poly : e.ws_alloc(2 * poly * m);
            f.ct = ct + off * 2 * out_poly;
            f.src = P;
            f.e = noise + off * 2 * N;
            f.plain = plain ? plain + off * plain_item_stride : nullptr;
            pk_product_chunk(e, R, pk, pk_poly, u + off * N, f.e, m, u_ntt, P, ckks, false);
            if (!ckks)
            {
                check(launch_encrypt_finish(e, EncryptFinish::AsymBfv, f, m), "encrypt_asym_bfv_finish");
                return;
            }
            if (direct)
                return;
            u64 *temp = e.ws_alloc(2 * out_poly * m);
            divround_ntt_front(e, *lt, R, P, m * 2, temp);
            f.temp = temp;
            check(launch_encrypt_finish(e, EncryptFinish::AsymCkks, f, m), "encrypt_asym_ckks_finish");
        });
    }

    // Secret key (rlwe.cpp:204-300), for the whole batch at once:
    //   c_1 = sample_poly_uniform(BlakePRNG(seed)) expanded on the device (one seed job list);
    //   BFV: c_0 = INTT(A (.) s) with A = c_1 (taken as NTT form), or NTT(c_1) in the arena when seeded (c_1 stays the
    //        coefficient-form sample, :233-243); unseeded c_1 goes back to coefficient form (:286-293); the fused tail
    //        negates, adds e and Delta m;
    //   CKKS: c_0 = NTT(lift(e)), then the fused tail c_0 = -(c_0 + c_1 (.) s) + plain.
    void op_encrypt_symmetric(Engine &e, int k, const u64 *sk, const u64 *plain, std::size_t plain_item_stride,
                              const std::uint64_t *seeds_host, const std::int32_t *noise, bool seeded, std::size_t count,
                              u64 *ct)
    {
        const bool ckks = e.scheme == 2;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        std::vector<SeedJob> jobs(count);
        for (std::size_t i = 0; i < count; i++)
            jobs[i] = SeedJob{ seeds_host + 8 * i, ct + i * 2 * poly + poly };
        op_expand_seeds(e, k, jobs.data(), count);
        EncryptArgs f{};
        f.k = k;
        f.rows = k;
        f.ct = ct;
        f.ct_item_stride = 2 * poly;
        f.e = noise;
        f.plain = plain;
        f.plain_item_stride = plain_item_stride;
        RlweArgs a = rlwe_args(ct, 2 * poly, k, noise, N);
        if (ckks)
        {
            f.src = sk;
            lift_to_ntt(e, a, count, ct_row_map(k, 2, 0), "lift(e)", "ntt(e)");
            check(launch_encrypt_finish(e, EncryptFinish::SymCkks, f, count), "encrypt_sym_ckks_finish");
            return;
        }
        if (plain)
            fill_scaling_args(e, k, f.sc);
        a.y = sk;
        if (!seeded)
        {
            a.x = ct + poly;
            a.x_item_stride = 2 * poly;
            check(launch_rlwe_stage(e, 1, a, count), "a*s");
            check(launch_ntt(e, ct, count * 2 * k, ct_row_map(k, 2, -1), true, kNttCanonical), "intt(c0, c1)");
            check(launch_encrypt_finish(e, EncryptFinish::SymBfv, f, count), "encrypt_sym_bfv_finish");
            return;
        }
        for_chunks(e, count, poly * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *a_ntt = e.ws_alloc(poly * m);
            u64 *c = ct + off * 2 * poly;
            check(launch_copy_rows(e, c + poly, 2 * poly, a_ntt, poly, m, k), "copy(a)");
            check(launch_ntt(e, a_ntt, m * k, ct_row_map(k, 1, -1), false, kNttCanonical), "ntt(a)");
            a.ct = c;
            a.x = a_ntt;
            a.x_item_stride = poly;
            check(launch_rlwe_stage(e, 1, a, m), "a*s");
            check(launch_ntt(e, c, m * 2 * k, ct_row_map(k, 2, 0), true, kNttCanonical), "intt(c0)");
            f.ct = c;
            f.e = noise + off * N;
            f.plain = plain ? plain + off * plain_item_stride : nullptr;
            check(launch_encrypt_finish(e, EncryptFinish::SymBfv, f, m), "encrypt_sym_bfv_finish");
        });
    }

    // ---------------------------------------------------------------- BatchEncoder
    namespace
    {
        RowMap plain_row_map(const Engine &e)
        {
            if (e.plain_prime < 0)
                throw std::invalid_argument("encryption parameters are not valid for batching"); // batchencoder.cpp:35-38
            RowMap m{};
            m.rows = 1;
            m.prime[0] = static_cast<unsigned short>(e.plain_prime);
            return m;
        }
    } // namespace

    void op_batch_encode(Engine &e, const u64 *values, std::size_t nvalues, std::size_t count, u64 *plain, bool is_signed)
    {
        const RowMap map = plain_row_map(e);
        if (nvalues > e.n)
            throw std::logic_error("values_matrix size is too large"); // batchencoder.cpp:119-122
        check(launch_batch_permute(e, true, values, nvalues, nvalues, plain, e.batch_map(), count, is_signed ? e.t : 0),
              "batch scatter");
        check(launch_ntt(e, plain, count, map, true, kNttCanonical), "intt(plain)");
    }

    void op_batch_decode(Engine &e, const u64 *plain, std::size_t count, u64 *values, bool is_signed)
    {
        const RowMap map = plain_row_map(e);
        const std::size_t N = e.n;
        for_chunks(e, count, N * sizeof(u64), 1, [&](std::size_t off, std::size_t m) {
            u64 *tmp = e.ws_alloc(N * m);
            check(launch_copy_rows(e, plain + off * N, N, tmp, N, m, 1), "copy(plain)");
            check(launch_ntt(e, tmp, m, map, false, kNttCanonical), "ntt(plain)");
            check(launch_batch_permute(e, false, tmp, N, N, values + off * N, e.batch_map(), m, is_signed ? e.t : 0), "batch gather");
        });
    }
    // ---------------------------------------------------------------- CKKSEncoder
    void op_ckks_encode(Engine &e, int k, const double *values, std::size_t n_values, std::size_t count, double scale,
                        u64 *plain)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("unsupported scheme"); // ckks.cpp:27-30
        if (n_values > e.n / 2)
            throw std::invalid_argument("values_size is too large"); // ckks.h:419-422
        const int total_bits = e.total_coeff_modulus_bit_count(k);
        if (scale <= 0 || (static_cast<int>(std::log2(scale)) + 1 >= total_bits))
            throw std::invalid_argument("scale out of bounds"); // :440-444
        e.ckks_tables();
        const RowMap map_q = e.level_host(k).map_q;
        const std::size_t N = e.n;
        double n_inv = 1.0 / static_cast<double>(N); // :484-487
        n_inv *= scale;
        // :489-504: the bit count is static_cast<int>(log2(d)) + 2 of the largest d = max(|coefficient|, 1). The device finds
        // d, the logarithm is the host's libm's (where the root tables come from too): a d a few ulps below 2^j has
        // log2(d) == j there, and an exponent or a logarithm taken on the device need not agree with it in that last bit.
        double h_max = 1.0;
        for_chunks(e, count, N * 2 * sizeof(double), 2, [&](std::size_t off, std::size_t m) {
            unsigned long long *d_max = reinterpret_cast<unsigned long long *>(e.ws_alloc(1));
            double *cv = reinterpret_cast<double *>(e.ws_alloc(2 * N * m));
            SEALHIP_CHECK(hipMemsetAsync(d_max, 0, sizeof(unsigned long long), e.lane().stream));
            check(launch_ckks_encode_front(e, values + off * n_values * 2, n_values, m, n_inv, cv,
                                           plain + off * static_cast<std::size_t>(k) * N, k, e.d_ckks_map, e.d_ckks_inv_roots, d_max),
                  "ckks encode");
            unsigned long long got = 0;
            SEALHIP_CHECK(hipMemcpyAsync(&got, d_max, sizeof(got), hipMemcpyDeviceToHost, e.lane().stream));
            SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
            double d;
            std::memcpy(&d, &got, sizeof(d)); // (0 when no coefficient exceeds 1)
            h_max = std::max(h_max, d);
        });
        // (an infinite coefficient is too large whatever the cast of log2(inf) would give)
        if (!std::isfinite(h_max) || static_cast<int>(std::log2(h_max)) + 2 >= total_bits)
            throw std::invalid_argument("encoded values are too large"); // :501-504
        check(launch_ntt(e, plain, count * k, map_q, false, kNttCanonical), "ntt(plain)"); // :609-613
    }

    void op_ckks_decode(Engine &e, int k, const u64 *plain, std::size_t count, double scale, double *values)
    {
        if (e.scheme != 2)
            throw std::invalid_argument("unsupported scheme");
        if (scale <= 0 || (static_cast<int>(std::log2(scale)) >= e.total_coeff_modulus_bit_count(k)))
            throw std::invalid_argument("scale out of bounds"); // ckks.h:651-656
        e.ckks_tables();
        const CkksDecodeDev *consts = e.ckks_decode_consts(k);
        const RowMap map_q = e.level_host(k).map_q;
        const std::size_t N = e.n, poly = static_cast<std::size_t>(k) * N;
        const double inv_scale = 1.0 / scale; // :668
        for_chunks(e, count, poly * sizeof(u64) + N * 2 * sizeof(double), 2, [&](std::size_t off, std::size_t m) {
            u64 *copy = e.ws_alloc(poly * m);
            double *res = reinterpret_cast<double *>(e.ws_alloc(2 * N * m));
            if (ntt_can_gather(e)) // the single-pass inverse kernel reads the plaintext rows where they are
                check(launch_intt_from(e, copy, plain + off * poly, poly, m * k, map_q, kNttCanonical), "intt(plain)");
            else
            {
                check(launch_copy_rows(e, plain + off * poly, poly, copy, poly, m, k), "copy(plain)");
                check(launch_ntt(e, copy, m * k, map_q, true, kNttCanonical), "intt(plain)"); // :674-678
            }
            check(launch_ckks_decode_back(e, copy, consts, k, m, inv_scale, res, values + off * N, e.d_ckks_map, e.d_ckks_roots),
                  "ckks decode");
        });
    }
} // namespace sealhip
