// bootstrap.cpp -- CKKS bootstrapping as one call: ModRaise, CoeffToSlot, EvalMod over both halves at
// once, SlotToCoeff. The plans are homdft_plan.hpp's and evalmod_plan.hpp's; the argument checks are the ABI entries'
// (api.cpp). The intermediates are one block of the context's pool per lane that the tables hold, under the rule of
// held_workspace.hpp: a larger batch takes a larger block, the earlier ones stay held, destroy releases all of them.
#include "../../include/sealhip.h"

#include "engine.hpp"
#include "evalmod_plan.hpp"
#include "homdft_plan.hpp"

namespace sealhip
{
    struct BootstrapTables
    {
        const Engine *engine = nullptr;
        int device = -1;
        std::uint32_t k_top = 0;
        evalmod::Plan evalmod;
        DftTables *c2s = nullptr, *s2c = nullptr;
        mutable HeldWorkspace<Engine> held;
    };

    // per ciphertext: the raised input at k_top, CoeffToSlot's two outputs, EvalMod's two outputs
    std::size_t bootstrap_temp_words(std::uint32_t k_top, const dftplan::Plan &c2s, const evalmod::Plan &em, std::size_t N)
    {
        return 2 * N * (static_cast<std::size_t>(k_top) + 2 * static_cast<std::size_t>(c2s.out_level) +
                        2 * static_cast<std::size_t>(em.out_level));
    }

    BootstrapTables *bootstrap_tables_create(Engine &e, std::uint32_t k_top, const dftplan::Plan &c2s, const evalmod::Plan &em,
                                             const dftplan::Plan &s2c, double s2c_gain)
    {
        std::unique_ptr<BootstrapTables> t(new BootstrapTables);
        t->engine = &e;
        t->device = e.device;
        t->k_top = k_top;
        t->evalmod = em;
        t->c2s = dft_tables_create(e, c2s, 1.0);
        try
        {
            t->s2c = dft_tables_create(e, s2c, s2c_gain);
        }
        catch (...)
        {
            dft_tables_destroy(t->c2s);
            throw;
        }
        return t.release();
    }

    void bootstrap_tables_destroy(BootstrapTables *t)
    {
        if (t)
            destroy_held_tables(t, "bootstrap tables cannot be destroyed during a graph capture", [t] {
                dft_tables_destroy(t->c2s);
                dft_tables_destroy(t->s2c);
                delete t;
            });
    }

    const Engine *bootstrap_tables_engine(const BootstrapTables &t)
    {
        return t.engine;
    }
    const DftTables &bootstrap_tables_c2s(const BootstrapTables &t)
    {
        return *t.c2s;
    }
    const DftTables &bootstrap_tables_s2c(const BootstrapTables &t)
    {
        return *t.s2c;
    }

    void op_bootstrap(Engine &e, const BootstrapTables &t, int k_in, const u64 *ct, std::size_t count,
                      const std::vector<DftStageKeys> &c2s_keys, const KSwitchKey &conj_key,
                      const std::vector<DftStageKeys> &s2c_keys, const KSwitchKey &relin_key, u64 *out,
                      const KSwitchKey *to_sparse, const KSwitchKey *to_dense)
    {
        const dftplan::Plan &c2s = dft_tables_plan(*t.c2s);
        const evalmod::Plan &em = t.evalmod;
        const std::size_t N = e.n;
        const std::size_t w_top = count * 2 * t.k_top * N, w_slots = count * 2 * c2s.out_level * N,
                          w_sine = count * 2 * static_cast<std::size_t>(em.out_level) * N;
        Lane &l = e.lane();
        // encapsulated: the level-1 ciphertext under the sparse secret and the raised one under it, both while `slots` is
        // still free (2 w_slots >= w_top + 2 count N needs c2s.out_level >= k_top / 2 + 1; else they take room of their own)
        const std::size_t w_low = count * 2 * N;
        const bool encapsulated = to_sparse && to_dense, borrow = 2 * w_slots * sizeof(u64) >= pad256(w_top) + pad256(w_low);
        const std::size_t extra = encapsulated && !borrow ? pad256(w_top) + pad256(w_low) : 0;
        Carver ws{ t.held.get(e, &l, l.capturing, (w_top + 2 * w_slots + 2 * w_sine) * sizeof(u64) + 3 * 256 + extra,
                              "the bootstrap's workspace would be allocated during a graph capture") };
        u64 *raised = ws.take(w_top);
        u64 *slots = ws.take(2 * w_slots); // re, then im: ONE batch of 2 count items
        u64 *sine = ws.take(2 * w_sine);   // likewise
        if (encapsulated)
        {
            Carver early{ reinterpret_cast<char *>(borrow ? slots : ws.take(0)) };
            u64 *low = early.take(w_low), *raised_sparse = early.take(w_top);
            // the q_0 rows of ct are the level-1 ciphertext, its item stride the input's (no entry has armed the sink: these
            // key switches write no flags)
            const std::size_t in_poly = static_cast<std::size_t>(k_in) * N, top_poly = static_cast<std::size_t>(t.k_top) * N;
            op_switch_secret(e, 1, ct, ct + in_poly, 2 * in_poly, count, *to_sparse, low);
            op_mod_raise(e, 1, low, count, static_cast<int>(t.k_top), raised_sparse);
            op_switch_secret(e, static_cast<int>(t.k_top), raised_sparse, raised_sparse + top_poly, 2 * top_poly, count, *to_dense,
                             raised);
        }
        else
            op_mod_raise(e, k_in, ct, count, static_cast<int>(t.k_top), raised);
        op_coeffs_to_slots(e, *t.c2s, raised, count, c2s_keys, conj_key, slots, slots + w_slots);
        {
            SinkScope quiet(e, 0); // (an intermediate: the caller's flags describe `out` alone)
            quiet.on = false;
            op_eval_mod(e, em, c2s.out_level, slots, 2 * count, &relin_key, sine, quiet);
        }
        op_slots_to_coeffs(e, *t.s2c, sine, sine + w_sine, count, s2c_keys, out);
    }
} // namespace sealhip
