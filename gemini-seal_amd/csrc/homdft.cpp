// homdft.cpp -- the homomorphic DFT over the pipelines: the stage values on the device and their host
// restatement, the tables (values -> op_ckks_encode at the key level), and CoeffToSlot / SlotToCoeff as chains of
// op_apply_galois_bsgs_plain with the merged rescale around the split and merge kernels. The plan is homdft_plan.hpp's; the
// argument checks are the ABI entries' (api.cpp). A transform's temporaries are blocks of the context's pool (pool.cpp) that
// the tables hold under the rule of held_workspace.hpp: one current block per lane, grown on demand, the earlier ones held
// until the tables are destroyed. (Not a Scratch per call: a pool block cannot be released during a capture. Not the lane
// arena under ws_floor: see DESIGN.md section 23.)
#include "../../include/sealhip.h"

#include <cmath>
#include <cstring>

#include "engine.hpp"
#include "homdft_entry.hpp"
#include "homdft_plan.hpp"

namespace sealhip
{
    struct DftTables
    {
        dftplan::Plan plan;
        int device = -1;
        std::vector<u64 *> stage; // device, [n_giant][n_baby][n_key][N] each
        const Engine *engine = nullptr; // the context the tables were made on: its ring, its pool, its lanes
        // a transform's temporaries, keyed by the lane. A context's lanes live as long as the context (LanePool owns them and
        // hands the lane of a thread that exited to the next one), and the tables are destroyed before it, so the key
        // cannot dangle.
        mutable HeldWorkspace<Engine> held;
        Carver workspace(const Engine &e, std::size_t bytes) const
        {
            Lane &l = e.lane();
            return Carver{ held.get(e, &l, l.capturing, bytes,
                                    "the transform's workspace would be allocated during a graph capture: run the call once "
                                    "before capturing") };
        }
        ~DftTables()
        {
            for (u64 *p : stage)
                if (p)
                    (void)hipFree(p);
        }
    };

    double dft_stage_gain(const dftplan::Plan &p, std::size_t stage, double gain)
    {
        const bool c2s = p.direction == dftplan::kCoeffsToSlots;
        double g = 1.0;
        if (c2s)
            g = std::ldexp(1.0, -static_cast<int>(p.stages[stage].r));
        if (c2s && stage + 1 == p.stages.size())
            g *= 0.5 * gain; // (powers of two: the product is gain's mantissa, whichever way it is bracketed)
        if (!c2s && stage == 0)
            g *= gain;
        return g;
    }

    // The generator kernel's loop on the host: the same indices, the same entry function, the same tables (the encoder's
    // roots and slot map, built as Engine::ckks_tables builds them).
    void dft_stage_values_host(const Engine &h, const dftplan::Plan &p, std::size_t stage, double gain, double *values)
    {
        const dftplan::Stage &s = p.stages.at(stage);
        const int logn = h.logn;
        const std::uint32_t N = 1u << logn, n = N >> 1;
        std::vector<std::uint32_t> map(n);
        std::uint64_t pos = 1;
        for (std::uint32_t i = 0; i < n; i++)
        {
            map[i] = reverse_bits(static_cast<std::uint32_t>((pos - 1) >> 1), logn);
            pos = (pos * 5) & (2 * static_cast<std::uint64_t>(N) - 1);
        }
        std::vector<double> roots(2 * static_cast<std::size_t>(N));
        for (std::uint32_t i = 0; i < N; i++)
            complex_root(2 * static_cast<std::size_t>(N), reverse_bits(i, logn), roots[2 * i], roots[2 * i + 1]);
        const bool inverse = p.direction == dftplan::kCoeffsToSlots;
        const double g_eff = dft_stage_gain(p, stage, gain);
        const int block_shift = static_cast<int>(s.s0 - 1 + s.r);
        for (std::uint32_t g = 0; g < s.n_giant; g++)
            for (std::uint32_t b = 0; b < s.n_baby; b++)
            {
                const long long c = s.giant_coeff(g) * static_cast<long long>(s.n_baby) + b;
                const std::uint32_t giant = static_cast<std::uint32_t>(s.giant[g]);
                double *cell = values + 2 * ((static_cast<std::size_t>(g) * s.n_baby + b) * n);
                for (std::uint32_t q = 0; q < n; q++)
                {
                    const std::uint32_t i = (q - giant) & (n - 1);
                    const long long col_raw = static_cast<long long>(i) + c * static_cast<long long>(s.h0);
                    const std::uint32_t col = static_cast<std::uint32_t>(col_raw) & (n - 1);
                    const bool inside = s.folded || (col_raw >= 0 && col_raw < static_cast<long long>(n) &&
                                                     (col >> block_shift) == (i >> block_shift));
                    double re = 0.0, im = 0.0;
                    if (inside)
                        dft_stage_entry(roots.data(), map.data(), logn, static_cast<int>(s.s0), static_cast<int>(s.r), inverse, i,
                                        col, g_eff, re, im);
                    cell[2 * q] = re;
                    cell[2 * q + 1] = im;
                }
            }
    }

    void op_dft_stage_values(Engine &e, const dftplan::Plan &p, std::size_t stage, double gain, double *values)
    {
        const dftplan::Stage &s = p.stages.at(stage);
        e.ckks_tables();
        check(launch_dft_stage_values(e, static_cast<int>(s.s0), static_cast<int>(s.r), p.direction == dftplan::kCoeffsToSlots,
                                      s.folded, s.n_baby, s.n_giant, dft_stage_gain(p, stage, gain), values),
              "dft stage values");
    }

    DftTables *dft_tables_create(Engine &e, const dftplan::Plan &p, double gain)
    {
        std::unique_ptr<DftTables> t(new DftTables);
        t->plan = p;
        t->device = e.device;
        t->engine = &e;
        const std::size_t n = e.n >> 1, plain_words = static_cast<std::size_t>(e.n_key) * e.n;
        for (std::size_t st = 0; st < p.stages.size(); st++)
        {
            const dftplan::Stage &s = p.stages[st];
            u64 *d = nullptr;
            SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&d), s.cells() * plain_words * sizeof(u64)));
            t->stage.push_back(d);
            Scratch scratch(e); // the values are a temporary: back to the pool before the next stage takes its own
            double *values = reinterpret_cast<double *>(scratch.take(s.cells() * n * 2 * sizeof(double)));
            op_dft_stage_values(e, p, st, gain, values);
            op_ckks_encode(e, e.n_key, values, n, s.cells(), s.scale, d);
        }
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
        e.check_fault();
        return t.release();
    }

    // the workspace blocks go back to the pool (on the calling thread's lane), then the tables' own memory is freed; the
    // caller's current device is left as it was
    void dft_tables_destroy(DftTables *t)
    {
        if (t)
            destroy_held_tables(t, "DFT tables cannot be destroyed during a graph capture", [t] { delete t; });
    }

    const Engine *dft_tables_engine(const DftTables &t)
    {
        return t.engine;
    }

    const dftplan::Plan &dft_tables_plan(const DftTables &t)
    {
        return t.plan;
    }

    const u64 *dft_tables_stage(const DftTables &t, std::size_t stage)
    {
        return t.stage.at(stage);
    }

    namespace
    {
        // stage st of the chain: in at the stage's level -> out one level below
        void run_stage(Engine &e, const DftTables &t, std::size_t st, const DftStageKeys &k, const u64 *in, std::size_t count,
                       u64 *out)
        {
            const dftplan::Stage &s = t.plan.stages[st];
            op_apply_galois_bsgs_plain(e, static_cast<int>(s.level), in, count, k.baby.data(), k.baby_keys.data(), k.baby.size(),
                                       k.giant.data(), k.giant_keys.data(), k.giant.size(), t.stage[st], out, true);
        }
    } // namespace

    void op_coeffs_to_slots(Engine &e, const DftTables &t, const u64 *ct, std::size_t count, const std::vector<DftStageKeys> &keys,
                            const KSwitchKey &conj_key, u64 *out_re, u64 *out_im)
    {
        const dftplan::Plan &p = t.plan;
        const std::size_t n_stages = p.stages.size(), N = e.n;
        const std::size_t wide = count * 2 * (p.in_level - 1) * N, low = count * 2 * p.out_level * N;
        Carver ws = t.workspace(e, (wide * sizeof(u64) + 256) * (n_stages >= 2 ? 2 : 1) + low * sizeof(u64) + 256);
        u64 *buf[2] = { ws.take(wide), n_stages >= 2 ? ws.take(wide) : nullptr };
        u64 *conj = ws.take(low);
        const u64 *cur = ct;
        for (std::size_t st = 0; st < n_stages; st++)
        {
            run_stage(e, t, st, keys[st], cur, count, buf[st & 1]);
            cur = buf[st & 1];
        }
        SEALHIP_CHECK(hipMemcpyAsync(conj, cur, low * sizeof(u64), hipMemcpyDeviceToDevice, e.lane().stream));
        op_apply_galois(e, static_cast<int>(p.out_level), conj, count, static_cast<std::uint32_t>(2 * N - 1), conj_key);
        check(launch_dft_conj_split(e, cur, conj, out_re, out_im, count, e.map_for(static_cast<int>(p.out_level), SEALHIP_BASE_Q)),
              "dft conj split");
    }

    void op_slots_to_coeffs(Engine &e, const DftTables &t, const u64 *ct_re, const u64 *ct_im, std::size_t count,
                            const std::vector<DftStageKeys> &keys, u64 *out)
    {
        const dftplan::Plan &p = t.plan;
        const std::size_t n_stages = p.stages.size(), N = e.n;
        const std::size_t wide = count * 2 * (p.in_level - 1) * N, top = count * 2 * p.in_level * N;
        const std::size_t n_wide = n_stages >= 3 ? 2 : n_stages - 1;
        Carver ws = t.workspace(e, top * sizeof(u64) + 256 + (wide * sizeof(u64) + 256) * n_wide);
        u64 *merged = ws.take(top);
        u64 *buf[2] = { n_stages >= 2 ? ws.take(wide) : nullptr, n_stages >= 3 ? ws.take(wide) : nullptr };
        check(launch_dft_merge(e, ct_re, ct_im, merged, count, e.map_for(static_cast<int>(p.in_level), SEALHIP_BASE_Q)), "dft merge");
        const u64 *cur = merged;
        for (std::size_t st = 0; st < n_stages; st++)
        {
            u64 *dst = st + 1 == n_stages ? out : buf[st & 1];
            run_stage(e, t, st, keys[st], cur, count, dst);
            cur = dst;
        }
    }
} // namespace sealhip
