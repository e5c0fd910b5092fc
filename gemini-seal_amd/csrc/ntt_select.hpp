// ntt_select.hpp -- which instance of the single-pass NTT kernels (N = 2^14 .. 2^16) a launch runs: the launch flags, the
// names of the kernels' template codes, the tables of the instances that exist, and the rule that picks one, as pure
// functions of plain facts. No HIP: tests/ntt_select_check.cpp compiles this header with a host compiler and pins the
// rule over its whole domain (tests/golden/ntt_select_table.json). The launchers (ntt_fwd.hip launch_half, ntt_inv.hip
// launch_half_inv) gather the facts, call the function, and launch and register from the same tables. DESIGN.md
// section 6 lists the instances and who launches them.
#pragma once
#include <cstdint>

#include "ntt_bounds.hpp"

namespace sealhip
{
    // ---- launch flags (the kernels read them as immediates)
    constexpr int kNttCanonical = 1; // fuse the canonicalising wrapper (ntt.h:236-245 / :328-333)
    constexpr int kNttStrict = 2;    // Harvey-corrected forward butterflies
    constexpr int kNttAnyRep = 8;    // inverse: the consumer canonicalises, any representative below 2p may be stored
    constexpr int kNttReduceOut = 0x10; // forward, single-pass kernel: one more conditional subtraction, outputs in [0, 2p)
    constexpr int kNttApprox = 0x20;   // forward, with kNttAnyRep or a consumer that takes outputs below (2 + g) p: approximate quotient (ntt_bounds.hpp section 2)
    constexpr int kNttPolyMajor = 0x4000;        // forward half kernel: live positions grouped item by item (ntt_half.hpp block_place; group size in bits 16-23)
    constexpr int kNttSmallQuot = 0x1000000;     // (launcher-internal) canonical approximate-quotient launch: single-precision quotient estimate in the store
    constexpr int kNttDebugNoSignal = 0x40; // forward half kernel: never send the hand-off signal (tests of the time-out path)
    // forward, single-pass kernel, with kNttReduceOut, in place: the producer of the rows has already applied the top layer
    // (gap N/2) -- bfv_lift_exact does for the Bsk rows it writes. Each workgroup then loads its own half only: no second read of
    // the row, no duplicated products (both workgroups of a row compute the top layer's products otherwise), no hand-off.
    constexpr int kNttTopDone = 0x80;
    constexpr int kNttDeferTop = 4;  // inverse, single-pass kernels only: leave the top layer (gap N/2) to the consumer
    // forward, single-pass kernel, gathered out-of-place launches whose consumer applies the transform's LAST layer (DESIGN.md
    // section 6b): workgroup `half` of a row transforms the parity class src[2i + half] as a ring of N/2 and stores it to
    // words [half N/2, (half + 1) N/2) of the row. No top layer, no duplicated products, no hand-off. Integer instances
    // of kFwdSplitInstances only, live primes in bounds::fwd_split_admits: anything else is refused.
    constexpr int kNttSplitLast = 0x100;
    // Primes below this bound have double-precision twiddle tables: the single-pass kernels then run their butterflies
    // on the FP64 pipe (exact, devmath.hpp) whenever the launch promises nothing about representatives that only the
    // integer sequence would deliver (canonical outputs, or kNttAnyRep). SEALHIP_NTT_NO_FP64=1 switches it off.
    // (the bound is what the schedules' worst-case recurrences in ntt_bounds.hpp admit: 50 bits)
    constexpr bounds::u64 kFpPrimeBound = bounds::u64(1) << bounds::kFpPrimeBits;

    // ---- the kernels' template codes (values fixed: the kernels' symbols carry them, profiles/ and tools/ are keyed by those)
    // forward schedule (ntt_fwd_half_kernel's STRICT)
    constexpr int kSchedLazy = 0;   // the reference's lazy sequence (ForwardLazy / ForwardLazyLast)
    constexpr int kSchedHarvey = 1; // Harvey-corrected: one conditional subtraction per butterfly, nothing wraps on any prime
    constexpr int kSchedApprox = 2; // approximate Shoup quotient (ntt_bounds.hpp section 2)
    constexpr int kSchedFp64 = 3;   // butterflies on the FP64 pipe (primes below kFpPrimeBound), canonical residues out
    constexpr int kSchedDense = 4;  // dense lazy schedule (ntt_bounds.hpp section 2b)
    // forward load/store treatment (ntt_fwd_half_kernel's REDUCE; NttSource::reduce_mode takes the load treatments)
    constexpr int kTreatNone = 0;
    constexpr int kTreatBarrett = 1;        // gathered words: barrett_reduce_63 w.r.t. the row's prime on load
    constexpr int kTreatCondSub = 2;        // gathered words: one conditional subtraction on load
    constexpr int kTreatReduceOut = 3;      // kNttReduceOut: outputs brought into [0, 2p) by the store
    constexpr int kTreatNegSpecial = 4;     // gathered words become -(x mod aux_p): the CKKS mod-down's special-prime residue
    constexpr int kTreatNegSpecialTop = 5;  // the same on a source row whose top inverse layer was deferred to this load
    constexpr int kTreatReduceOutTopDone = 6; // kNttReduceOut | kNttTopDone: the producer applied the top layer
    constexpr int kTreatModDownStore = 7;   // kTreatNegSpecialTop plus the rest of the mod-down as the store phase
    // inverse schedule (ntt_inv_half_kernel's LZ)
    constexpr int kInvExact = 0;   // the reference's sequence
    constexpr int kInvLazySum = 1; // sparse lazy sums (ntt_bounds.hpp section 1)
    constexpr int kInvFp64 = 2;
    constexpr int kInvDense = 3;   // dense lazy sums, primes up to 2^60
    // inverse shape: what one workgroup of ntt_inv_half_kernel transforms
    constexpr int kShapeHalf = 0;       // half a row; the top layer follows (or is left to the consumer)
    constexpr int kShapeHalfTensor = 1; // half a row, the ciphertext tensor product formed on load (DY)
    constexpr int kShapeWhole = 2;      // a whole row, top layer included (WHOLE, rings of 2^14 and 2^15)
    constexpr int kShapeQuarter = 3;    // a quarter row (QUARTER, rings of 2^16); the radix-4 top pass follows
    // which streaming pass follows the inverse kernel
    constexpr int kTopNone = 0, kTopLayer = 1 /* ntt_inv_top_kernel */, kTopRadix4 = 2 /* ntt_inv_top2_kernel */;

    // The environment switches that run the reference's own operation sequences instead of the proved shortcuts:
    // SEALHIP_NTT_NO_FP64, SEALHIP_NTT_EXACT_FWD, SEALHIP_NTT_EXACT_INV, SEALHIP_NTT_CANON_EXACT. Read once per process by
    // ntt_switches() (ntt.hip), nowhere else.
    struct NttSwitches
    {
        bool no_fp64, exact_fwd, exact_inv, canon_exact;
    };

    // ---- forward instances: ntt_fwd_half_kernel<LOGN, sched, treatment>
    struct FwdInstance
    {
        int sched, treatment;
    };
    constexpr FwdInstance kFwdInstances[] = {
        { kSchedLazy, kTreatNone },          { kSchedLazy, kTreatBarrett },        { kSchedLazy, kTreatCondSub },
        { kSchedLazy, kTreatReduceOut },     { kSchedLazy, kTreatNegSpecial },     { kSchedLazy, kTreatNegSpecialTop },
        { kSchedLazy, kTreatReduceOutTopDone },
        { kSchedHarvey, kTreatNone },        { kSchedHarvey, kTreatBarrett },      { kSchedHarvey, kTreatCondSub },
        { kSchedHarvey, kTreatReduceOut },   { kSchedHarvey, kTreatNegSpecial },   { kSchedHarvey, kTreatNegSpecialTop },
        { kSchedApprox, kTreatNone },        { kSchedApprox, kTreatBarrett },      { kSchedApprox, kTreatCondSub },
        { kSchedFp64, kTreatNone },          { kSchedFp64, kTreatBarrett },        { kSchedFp64, kTreatCondSub },
        { kSchedFp64, kTreatNegSpecial },    { kSchedFp64, kTreatNegSpecialTop },  { kSchedFp64, kTreatModDownStore },
        { kSchedDense, kTreatReduceOut },    { kSchedDense, kTreatReduceOutTopDone },
    };
    constexpr int kFwdInstanceCount = static_cast<int>(sizeof(kFwdInstances) / sizeof(kFwdInstances[0]));
    // The mod-down store is the LDS trip back to arrangement 1 (ntt_fwd.hip kStoreExchange), which exists where the final
    // round holds at least two index bits: half-row shapes T = log n - 1 >= 14.
    constexpr bool fwd_store_exchange(int T, int treatment)
    {
        return (T - 12) >= 2 && treatment == kTreatModDownStore;
    }
    constexpr bool fwd_instance_at(int logn, FwdInstance i)
    {
        return i.treatment != kTreatModDownStore || fwd_store_exchange(logn - 1, i.treatment);
    }
    // index into kFwdInstances of the instance that exists at this ring size, -1: none
    constexpr int fwd_instance_index(int logn, int sched, int treatment)
    {
        for (int i = 0; i < kFwdInstanceCount; i++)
            if (kFwdInstances[i].sched == sched && kFwdInstances[i].treatment == treatment)
                return fwd_instance_at(logn, kFwdInstances[i]) ? i : -1;
        return -1;
    }

    // ---- forward instances without the last layer (kNttSplitLast): ntt_fwd_half_kernel<LOGN, sched, treatment, true>, a
    // table of its own (FwdChoice::split says which table FwdChoice::instance indexes). They exist at every ring size.
    constexpr FwdInstance kFwdSplitInstances[] = {
        { kSchedLazy, kTreatNone },   { kSchedLazy, kTreatBarrett },   { kSchedLazy, kTreatCondSub },
        { kSchedApprox, kTreatNone }, { kSchedApprox, kTreatBarrett }, { kSchedApprox, kTreatCondSub },
    };
    constexpr int kFwdSplitInstanceCount = static_cast<int>(sizeof(kFwdSplitInstances) / sizeof(kFwdSplitInstances[0]));
    constexpr int fwd_split_instance_index(int sched, int treatment)
    {
        for (int i = 0; i < kFwdSplitInstanceCount; i++)
            if (kFwdSplitInstances[i].sched == sched && kFwdSplitInstances[i].treatment == treatment)
                return i;
        return -1;
    }

    // ---- inverse instances: ntt_inv_half_kernel<inv_kernel_logn(shape, logn), sched, DY, WHOLE, QUARTER>
    struct InvInstance
    {
        int shape, sched;
        constexpr bool tensor_load() const
        {
            return shape == kShapeHalfTensor;
        }
    };
    constexpr InvInstance kInvInstances[] = {
        { kShapeHalf, kInvExact },       { kShapeHalf, kInvLazySum },       { kShapeHalf, kInvFp64 },    { kShapeHalf, kInvDense },
        { kShapeHalfTensor, kInvExact }, { kShapeHalfTensor, kInvLazySum }, { kShapeHalfTensor, kInvDense }, // (never FP64)
        { kShapeWhole, kInvExact },      { kShapeWhole, kInvLazySum },      { kShapeWhole, kInvFp64 },   { kShapeWhole, kInvDense },
        { kShapeQuarter, kInvExact },    { kShapeQuarter, kInvLazySum },    { kShapeQuarter, kInvFp64 }, { kShapeQuarter, kInvDense },
    };
    constexpr int kInvInstanceCount = static_cast<int>(sizeof(kInvInstances) / sizeof(kInvInstances[0]));
    constexpr bool inv_instance_at(int logn, InvInstance i)
    {
        return i.shape == kShapeWhole ? logn <= 15 : (i.shape == kShapeQuarter ? logn == 16 : true);
    }
    constexpr int inv_instance_index(int logn, int shape, int sched)
    {
        for (int i = 0; i < kInvInstanceCount; i++)
            if (kInvInstances[i].shape == shape && kInvInstances[i].sched == sched)
                return inv_instance_at(logn, kInvInstances[i]) ? i : -1;
        return -1;
    }
    // The kernel's first template argument for a shape at a ring of 2^logn: the whole-row form of a ring is the half-row
    // kernel of the ring twice as large, the quarter-row form that of the ring half as large.
    constexpr int inv_kernel_logn(int shape, int logn)
    {
        return shape == kShapeWhole ? logn + 1 : (shape == kShapeQuarter ? logn - 1 : logn);
    }
    // on-chip layers of the inverse kernel instance ntt_inv_half_kernel<KLOGN, ...>: what bounds::inv_lazy_admits and
    // bounds::inv_dense_admits are asked about -- the layer count of the instance that is launched
    template <int KLOGN>
    constexpr int kInvLayers = KLOGN - 1;
    constexpr int inv_layers(int shape, int logn)
    {
        return inv_kernel_logn(shape, logn) - 1;
    }
    constexpr int inv_blocks_per_row(int shape)
    {
        return shape == kShapeWhole ? 1 : (shape == kShapeQuarter ? 4 : 2);
    }

    // ---- the forward rule
    struct FwdFacts
    {
        int logn;              // 14 .. 16
        int flags;             // the caller's
        const bounds::u64 *live; // the primes of the launch's live rows
        int live_n;
        bool gathers;          // the launch has a gather source (NttSource::base[0])
        bool all_gathered;     // ... and every live row reads it
        bool same_source;      // ... and all of them the same source row (a key-switch digit)
        int treatment;         // NttSource::reduce_mode
        bounds::u64 aux_p;     // NttSource::aux_p (treatments on the special prime)
        bool key_moduli_fp;    // every key modulus is below bounds::kFpInputBound (what a gathered word can be)
        NttSwitches sw;
        bool suppress_signal;  // Engine::ntt_suppress_signal (sealhip_debug_ntt_handoff: drive the time-out path)
    };
    struct FwdChoice
    {
        bool valid;          // false: the launch is refused (hipErrorInvalidValue)
        int instance;        // index into kFwdInstances
        int sched, treatment;
        int flags;           // what the kernel gets: kNttStrict dropped, kNttAnyRep cleared or added, kNttSmallQuot,
                             // kNttPolyMajor with its group size, kNttDebugNoSignal
        bool tickets;        // the two workgroups of a row hand off through a ticket: the launch needs Engine::ntt_tickets
        bool aux_as_doubles; // the special prime's constants go in as doubles (h_load_top's floating-point treatments)
        bool split;          // kNttSplitLast: `instance` indexes kFwdSplitInstances
    };

    // (The ring size is a template argument so that the predicates get it as a constant: they are worst-case recurrences,
    //  folded at compile time then, and cost a launch some ten microseconds of host time when they run.)
    template <int LOGN>
    FwdChoice select_fwd_half_at(const FwdFacts &f)
    {
        FwdChoice c{};
        int flags = f.flags;
        const auto every_live = [&f](auto admits) {
            for (int i = 0; i < f.live_n; i++)
                if (!admits(f.live[i]))
                    return false;
            return true;
        };
        // STRICT mode means "no wrap-around": Harvey's corrected butterflies (one conditional subtraction each)
        // guarantee it for any prime. Where the consumer takes any representative (kNttAnyRep, kNttApprox) or the
        // canonical residue is what is returned (kNttCanonical), and every live prime leaves the head-room that the cheaper
        // schedules are proved on (ntt_bounds.hpp section 2: nothing can wrap there either), the residues are the same and
        // the flag is dropped for the launch (round 4). The `_lazy` entries and the 60-bit rows keep the corrected sequence.
        if ((flags & kNttStrict) != 0 && (flags & (kNttAnyRep | kNttCanonical | kNttApprox)) != 0 && (flags & kNttReduceOut) == 0)
        {
            if (!f.sw.exact_fwd && every_live([&](bounds::u64 p) { return bounds::fwd_canon_admits(p, LOGN); }))
                flags &= ~kNttStrict;
        }
        // STRICT launches on primes without the head-room of the rule above (the 60-bit Bsk rows of a BFV multiply) whose
        // consumer takes any representative below 2p (kNttReduceOut | kNttAnyRep): the dense lazy schedule of
        // ntt_bounds.hpp section 2b instead of a conditional subtraction per butterfly -- the reference's own butterfly,
        // every word brought back below 2p before rounds 2 and 3 and in the store. Same residues, nothing wraps.
        const bool dense = (flags & kNttStrict) != 0 && (flags & kNttReduceOut) != 0 && (flags & kNttAnyRep) != 0 &&
                           (flags & kNttCanonical) == 0 && !f.gathers && !f.sw.exact_fwd &&
                           every_live([&](bounds::u64 p) { return bounds::fwd_dense_admits(p, LOGN); });
        // (kNttTopDone: no workgroup reads the other's half, nothing to hand off)
        const bool top_done = (flags & kNttTopDone) != 0;
        // (a STRICT launch may start below the top layer only on the dense schedule: Harvey's sequence has no such instance)
        if (top_done && (((flags & (kNttReduceOut | kNttStrict | kNttCanonical)) != kNttReduceOut && !dense) || f.gathers))
            return c;
        // a launch whose live rows are all gathered from another buffer writes no row that anybody reads: nothing to
        // hand off either
        const bool all_gathered = f.gathers && f.all_gathered;
        // kNttSplitLast: out of place by definition (every live row gathered), no in-place option beside it
        const bool split = (flags & kNttSplitLast) != 0;
        if (split && (!all_gathered || (flags & (kNttCanonical | kNttReduceOut | kNttTopDone)) != 0))
            return c;
        c.tickets = !(top_done || all_gathered);
        if (f.suppress_signal)
            flags |= kNttDebugNoSignal;
        // (see ntt_half.hpp block_place)
        const bool one_source = all_gathered && f.treatment <= kTreatCondSub && f.live_n > 1 && f.same_source;
        // Floating-point instance (devmath.hpp): every live prime below 2^50, inputs below 2^52 (residues, or gathered
        // words of another key prime, or the output of a load treatment), and a launch that does not ask for the
        // integer sequence's own representatives (canonical output, or a consumer that reduces whatever it reads).
        // The result is the canonical residue, so the integer instances' flags play no further role.
        bool fp = !f.sw.no_fp64 && (flags & (kNttAnyRep | kNttCanonical)) != 0 && (flags & kNttReduceOut) == 0 &&
                  every_live([](bounds::u64 p) { return p < kFpPrimeBound; });
        const bool special = f.treatment == kTreatNegSpecial || f.treatment == kTreatNegSpecialTop || f.treatment == kTreatModDownStore;
        if (fp && f.gathers)
        {
            if (special)
                fp = f.aux_p < (f.treatment == kTreatNegSpecial ? bounds::kFpInputBound : kFpPrimeBound); // (else: sums of two words below 2P)
            else
                fp = f.key_moduli_fp;
        }
        if (one_source && !fp) // (the integer digit launches)
        {
            const int g = 4 < f.live_n ? 4 : f.live_n;
            flags |= kNttPolyMajor | (g << 16);
        }
        if (flags & kNttAnyRep)
        {
            // the last layer may keep its first operand unreduced only if the grown values cannot wrap
            // (below (2 log n + 3) p < 2^64 for p < 2^58) and nothing expects the [0, 4p) output range
            const bool ok = !f.sw.exact_fwd && (flags & (kNttCanonical | kNttStrict)) == 0 &&
                            every_live([&](bounds::u64 p) { return bounds::fwd_lazy_admits(p, LOGN); });
            if (!ok)
                flags &= ~kNttAnyRep;
        }
        int red = f.gathers ? f.treatment : kTreatNone;
        if (flags & kNttReduceOut)
        {
            if (red != kTreatNone || (flags & kNttCanonical))
                return c; // an in-place, non-canonical launch option
            red = top_done ? kTreatReduceOutTopDone : kTreatReduceOut;
        }
        // approximate Shoup quotient (one multiplier instruction less per butterfly): the product then
        // lies in [0, 3p), every layer adds 3p instead of 2p and the outputs are below 50p (kNttAnyRep) or 5p. Only where
        // the consumer reduces whatever representative it reads, nothing expects the [0, 4p) range (no canonicalising
        // wrapper, no kNttReduceOut) and 50p cannot wrap: every live prime below 2^58.
        const bool no_apx = f.sw.exact_fwd;
        bool apx = !no_apx && (flags & kNttApprox) != 0 && (flags & (kNttStrict | kNttCanonical | kNttReduceOut)) == 0 &&
                   !(f.gathers && special) && every_live([&](bounds::u64 p) { return bounds::fwd_lazy_admits(p, LOGN); });
        // The canonicalising wrapper (ntt.h:225-246) on primes with head-room: the canonical residue does not depend on
        // the representatives the layers pass on, so an in-place canonical transform runs the cheapest exact schedule --
        // approximate quotient, no Barrett step in the last layer, values below (4 + g log n) p for inputs below 4p
        // (ntt_bounds.hpp section 2: fwd_canon_admits) -- and canonicalises with one reduction as it stores.
        // SEALHIP_NTT_CANON_EXACT=1: the reference's sequence.
        const bool capx = !no_apx && !f.sw.canon_exact && !fp && red == kTreatNone && (flags & kNttCanonical) != 0 &&
                          (flags & (kNttStrict | kNttReduceOut)) == 0 && // (inputs below 4p, the range include/sealhip.h documents)
                          every_live([&](bounds::u64 p) { return bounds::fwd_canon_admits(p, LOGN); });
        if (capx)
        {
            apx = true;
            flags |= kNttAnyRep;
            // (else the Barrett step, as in round 3)
            if (every_live([&](bounds::u64 p) { return bounds::small_quot_admits(p, bounds::fwd_canon_output_mult(LOGN)); }))
                flags |= kNttSmallQuot;
        }
        if (red == kTreatModDownStore && !fp)
            return c; // ntt_can_fuse_moddown said no: the caller runs moddown_post itself
        c.sched = fp ? kSchedFp64 : (apx ? kSchedApprox : (dense ? kSchedDense : ((flags & kNttStrict) ? kSchedHarvey : kSchedLazy)));
        c.treatment = red;
        c.flags = flags;
        c.aux_as_doubles = fp && f.gathers && special;
        if (split)
        {
            // the consumer forms the last layer from words that must not have wrapped (its 128-bit sums: the launcher's
            // caller checks nd, here one digit); no floating-point, Harvey or special-prime instance of this form exists
            if (fp || !every_live([&](bounds::u64 p) { return bounds::fwd_split_admits(p, LOGN, 1); }))
                return c;
            c.split = true;
            c.instance = fwd_split_instance_index(c.sched, c.treatment);
            c.valid = c.instance >= 0;
            return c;
        }
        c.instance = fwd_instance_index(LOGN, c.sched, c.treatment); // (kTreatModDownStore at 2^14: none)
        c.valid = c.instance >= 0;
        return c;
    }
    inline FwdChoice select_fwd_half(const FwdFacts &f)
    {
        switch (f.logn)
        {
        case 14: return select_fwd_half_at<14>(f);
        case 15: return select_fwd_half_at<15>(f);
        case 16: return select_fwd_half_at<16>(f);
        default: return FwdChoice{};
        }
    }

    // ---- the inverse rule
    struct InvFacts
    {
        int logn;
        int flags;
        const bounds::u64 *live;
        int live_n;
        bool tensor_load; // the launch forms the ciphertext tensor product on load (ntt_inv_tensor)
        NttSwitches sw;
    };
    struct InvChoice
    {
        bool valid;
        int instance; // index into kInvInstances
        int shape, sched;
        int canon;    // the kernel's `canonical` argument (the whole-row form applies the wrapper itself)
        int top;      // kTopNone, kTopLayer, kTopRadix4
    };

    // every live prime admitted by the lazy-sum / the dense schedule of an instance with LAYERS on-chip layers
    template <int LAYERS>
    bool inv_lazy_all(const InvFacts &f)
    {
        for (int i = 0; i < f.live_n; i++)
            if (!bounds::inv_lazy_admits(LAYERS, f.live[i]))
                return false;
        return true;
    }
    template <int LAYERS>
    bool inv_dense_all(const InvFacts &f)
    {
        for (int i = 0; i < f.live_n; i++)
            if (!bounds::inv_dense_admits(LAYERS, f.live[i]))
                return false;
        return true;
    }

    template <int LOGN> // (a template argument for the predicates' sake: see select_fwd_half_at)
    InvChoice select_inv_half_at(const InvFacts &f)
    {
        InvChoice c{};
        // whole-row form (rings of 2^14, 2^15) and quarter-row form (2^16): standalone transforms -- the top layer is not
        // left to a consumer
        const bool standalone = !f.tensor_load && !(f.flags & kNttDeferTop);
        c.shape = f.tensor_load ? kShapeHalfTensor : (!standalone ? kShapeHalf : (LOGN <= 15 ? kShapeWhole : kShapeQuarter));
        // lazy-sum schedule (InvLazy): the stored values keep their residue class and stay below 2p, but not the
        // reference's representative -- only where the caller says so (kNttAnyRep: its inputs are below 2p and
        // the consuming kernel canonicalises) and no live prime can wrap
        // (the canonicalising wrapper, ntt.h:328-333, erases the representative too: its inputs are what the reference
        //  itself requires of an inverse transform, values below 2p)
        // (round 4) the dense schedule where the sparse one has no head-room: primes of 2^45 .. 2^60
        const bool any_rep = (f.flags & (kNttAnyRep | kNttCanonical)) != 0, lazy_ok = any_rep && !f.sw.exact_inv;
        // (the predicates take the layer count of the instance that is launched; the whole-row form, one layer more than the
        //  half-row shape of its ring, is admitted only where the half-row shape's predicate holds too)
        bool lazy = lazy_ok && inv_lazy_all<kInvLayers<LOGN>>(f), dense = lazy_ok && inv_dense_all<kInvLayers<LOGN>>(f) && !lazy;
        if (c.shape == kShapeWhole)
        {
            constexpr int W = kInvLayers<inv_kernel_logn(kShapeWhole, LOGN)>;
            dense = (lazy || dense) && inv_dense_all<W>(f);
            lazy = lazy && inv_lazy_all<W>(f);
        }
        else if (c.shape == kShapeQuarter)
        {
            constexpr int Q = kInvLayers<inv_kernel_logn(kShapeQuarter, LOGN)>;
            lazy = lazy_ok && inv_lazy_all<Q>(f);
            dense = lazy_ok && inv_dense_all<Q>(f);
        }
        // floating-point instance: same contract (inputs below 2p, any representative out), every live prime below 2^50
        bool fp = any_rep && !f.sw.no_fp64 && !f.tensor_load;
        for (int i = 0; fp && i < f.live_n; i++)
            fp = f.live[i] < kFpPrimeBound;
        c.sched = fp ? kInvFp64 : (lazy ? kInvLazySum : (dense ? kInvDense : kInvExact));
        c.canon = (c.shape == kShapeWhole && (f.flags & kNttCanonical)) ? 1 : 0;
        // (kNttDeferTop: the consumer applies the top layer, and the canonicalisation, on load)
        c.top = c.shape == kShapeWhole ? kTopNone
                                       : (c.shape == kShapeQuarter ? kTopRadix4 : ((f.flags & kNttDeferTop) ? kTopNone : kTopLayer));
        c.instance = inv_instance_index(LOGN, c.shape, c.sched);
        c.valid = c.instance >= 0;
        return c;
    }
    inline InvChoice select_inv_half(const InvFacts &f)
    {
        switch (f.logn)
        {
        case 14: return select_inv_half_at<14>(f);
        case 15: return select_inv_half_at<15>(f);
        case 16: return select_inv_half_at<16>(f);
        default: return InvChoice{};
        }
    }
} // namespace sealhip
