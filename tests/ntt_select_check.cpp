// ntt_select_check.cpp -- CPU test of gemini-seal_amd/csrc/ntt_select.hpp (built and run by tests/test_ntt_select_host.py):
// the rule that picks the single-pass NTT kernel instance of a launch, evaluated without a device.
// Domain: rings 2^14..2^16 x the environment switches (none, each alone, all) x live prime sets on both sides of every
// boundary a predicate of the rule has x forward in-place launches with all 64 combinations of the six caller flags,
// gathered launches with the flag combinations the pipelines pass (each with and without kNttStrict) over the load
// treatments, gather forms, live counts, key moduli and special primes; inverse launches with all 8 combinations of
// kNttCanonical, kNttAnyRep, kNttDeferTop, with and without the tensor load.
// 1. Closure: every valid choice names an instance of the table that exists at that ring size, every instance is chosen
//    by some input at every ring size it exists at, and the rule refuses exactly what is stated below (parent_refuses).
// 2. Anchors: choices derived by hand from the launchers' ladders, asserted literally.
// 3. --table: prints the choice for every input of the domain as JSON (tests/golden/ntt_select_table.json; the host
//    test requires equality). Rows of choices and the ways live sets map to them are written once each (struct Table).
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "ntt_select.hpp"

using namespace sealhip;
using bounds::u64;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do                                                       \
    {                                                        \
        if (!(cond))                                         \
        {                                                    \
            failures++;                                      \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                        \
            std::printf("\n");                               \
        }                                                    \
    } while (0)

// ---- the domain
// largest p in [2^45, 2^61] a predicate admits (every predicate here is monotone above 2^45, which each admits)
template <class Pred>
static u64 largest_admitted(Pred pred)
{
    u64 a = bounds::kSmallQuotMinPrime, b = u64(1) << bounds::kMaxPrimeBits;
    if (pred(b))
        return b;
    while (b - a > 1)
    {
        const u64 m = a + (b - a) / 2;
        (pred(m) ? a : b) = m;
    }
    return a;
}

struct Edges
{
    u64 fp64, fwd_canon, fwd_canon_small_quot, fwd_dense, fwd_lazy;
    u64 inv_lazy[4], inv_dense[4]; // per inverse shape (0 where the shape does not exist at the ring size)
};
static Edges edges_of(int logn)
{
    Edges e{};
    e.fp64 = kFpPrimeBound - 1;
    e.fwd_canon = largest_admitted([&](u64 p) { return bounds::fwd_canon_admits(p, logn); });
    e.fwd_canon_small_quot = largest_admitted([&](u64 p) { return bounds::small_quot_admits(p, bounds::fwd_canon_output_mult(logn)); });
    e.fwd_dense = largest_admitted([&](u64 p) { return bounds::fwd_dense_admits(p, logn); });
    e.fwd_lazy = largest_admitted([&](u64 p) { return bounds::fwd_lazy_admits(p, logn); });
    for (int shape : { kShapeHalf, kShapeWhole, kShapeQuarter })
    {
        if (!inv_instance_at(logn, InvInstance{ shape, kInvExact }))
            continue;
        const int layers = inv_layers(shape, logn);
        e.inv_lazy[shape] = largest_admitted([&](u64 p) { return bounds::inv_lazy_admits(layers, p); });
        e.inv_dense[shape] = largest_admitted([&](u64 p) { return bounds::inv_dense_admits(layers, p); });
    }
    return e;
}

// one value on each side of every boundary, 2^60 - 1, 2^61 - 1, and one mixed set (a prime the FP64 instances take next to one
// they do not). The predicates take plain integers: the values need not be prime.
static std::vector<std::vector<u64>> live_sets(int logn)
{
    const Edges e = edges_of(logn);
    std::set<u64> v;
    const auto both_sides = [&](u64 largest) {
        if (largest)
        {
            v.insert(largest);
            v.insert(largest + 1);
        }
    };
    both_sides(e.fp64);
    both_sides(e.fwd_canon);
    both_sides(e.fwd_canon_small_quot);
    both_sides(e.fwd_dense);
    both_sides(e.fwd_lazy);
    both_sides(bounds::kFpInputBound - 1);
    both_sides(bounds::kSmallQuotMinPrime - 1); // (the lower edge of the single-precision quotient estimate)
    for (int s = 0; s < 4; s++)
    {
        both_sides(e.inv_lazy[s]);
        both_sides(e.inv_dense[s]);
    }
    v.insert((u64(1) << 60) - 1);
    v.insert((u64(1) << 61) - 1);
    std::vector<std::vector<u64>> sets;
    for (u64 p : v)
        sets.push_back({ p });
    sets.push_back({ (u64(1) << 49) + 1, (u64(1) << 60) - 1 });
    return sets;
}

static const NttSwitches kSwitchSettings[] = {
    { false, false, false, false }, { true, false, false, false }, { false, true, false, false },
    { false, false, true, false },  { false, false, false, true }, { true, true, true, true },
};
static const char *const kSwitchNames[] = { "none", "NO_FP64", "EXACT_FWD", "EXACT_INV", "CANON_EXACT", "all" };

// the six caller flags of a forward launch, in the order of the in-place columns (bit i of the column index)
static const int kFwdCallerFlags[6] = { kNttCanonical, kNttStrict, kNttAnyRep, kNttReduceOut, kNttApprox, kNttTopDone };
// what the pipelines pass to a gathered launch, and each of those with kNttStrict (launch_ntt_gather adds it in STRICT mode)
static const int kGatherFlags[8] = { 0,          kNttAnyRep,
                                     kNttApprox, kNttAnyRep | kNttApprox,
                                     kNttStrict, kNttStrict | kNttAnyRep,
                                     kNttStrict | kNttApprox, kNttStrict | kNttAnyRep | kNttApprox };

struct FwdSource
{
    std::string name;
    bool gathers, all_gathered, same_source;
    int treatment, live_n; // live_n 0: as many as the live set has
    u64 aux_p;
    bool key_moduli_fp;
};
static std::vector<FwdSource> fwd_sources()
{
    std::vector<FwdSource> s;
    s.push_back({ "inplace", false, false, false, kTreatNone, 0, 0, true });
    const char *const forms[3] = { "partial", "distinct", "one" };
    for (int t : { kTreatNone, kTreatBarrett, kTreatCondSub })
        for (int form = 0; form < 3; form++)
            for (int n : { 1, 5 })
                for (int key_fp = 0; key_fp < 2; key_fp++)
                    s.push_back({ "t" + std::to_string(t) + "." + forms[form] + ".n" + std::to_string(n) + (key_fp ? ".key<2^52" : ".key>=2^52"),
                                  true, form != 0, form == 2, t, n, 0, key_fp != 0 });
    for (int t : { kTreatNegSpecial, kTreatNegSpecialTop, kTreatModDownStore })
        for (int n : { 1, 5 })
            for (u64 aux : { kFpPrimeBound - 1, kFpPrimeBound, bounds::kFpInputBound - 1, bounds::kFpInputBound })
                s.push_back({ "t" + std::to_string(t) + ".one.n" + std::to_string(n) + ".P" + std::to_string(aux), true, true, true, t, n,
                              aux, true });
    return s;
}

// the live primes of a launch: the set's values, repeated in turn up to the live count
static std::vector<u64> live_rows(const std::vector<u64> &set, int n)
{
    std::vector<u64> rows;
    const int count = n ? n : static_cast<int>(set.size());
    for (int i = 0; i < count; i++)
        rows.push_back(set[i % set.size()]);
    return rows;
}

static FwdFacts fwd_facts(int logn, const NttSwitches &sw, const FwdSource &s, const std::vector<u64> &rows, int flags)
{
    FwdFacts f{};
    f.logn = logn;
    f.flags = flags;
    f.live = rows.data();
    f.live_n = static_cast<int>(rows.size());
    f.gathers = s.gathers;
    f.all_gathered = s.all_gathered;
    f.same_source = s.same_source;
    f.treatment = s.treatment;
    f.aux_p = s.aux_p;
    f.key_moduli_fp = s.key_moduli_fp;
    f.sw = sw;
    f.suppress_signal = false;
    return f;
}

// visit(logn, switch index, source, live set, its index, column, facts) for every forward input of the domain
template <class Visit>
static void for_each_fwd(Visit visit)
{
    const std::vector<FwdSource> sources = fwd_sources();
    for (int logn = 14; logn <= 16; logn++)
    {
        const std::vector<std::vector<u64>> sets = live_sets(logn);
        for (int sw = 0; sw < 6; sw++)
            for (const FwdSource &s : sources)
                for (std::size_t si = 0; si < sets.size(); si++)
                {
                    const std::vector<u64> &set = sets[si];
                    const std::vector<u64> rows = live_rows(set, s.live_n);
                    const int columns = s.gathers ? 8 : 64;
                    for (int col = 0; col < columns; col++)
                    {
                        int flags = 0;
                        if (s.gathers)
                            flags = kGatherFlags[col];
                        else
                            for (int b = 0; b < 6; b++)
                                flags |= (col >> b & 1) ? kFwdCallerFlags[b] : 0;
                        visit(logn, sw, s, set, static_cast<int>(si), col, fwd_facts(logn, kSwitchSettings[sw], s, rows, flags));
                    }
                }
    }
}

// inverse columns: bit 0 kNttCanonical, bit 1 kNttAnyRep, bit 2 kNttDeferTop, bit 3 the tensor load
template <class Visit>
static void for_each_inv(Visit visit)
{
    for (int logn = 14; logn <= 16; logn++)
    {
        const std::vector<std::vector<u64>> sets = live_sets(logn);
        for (int sw = 0; sw < 6; sw++)
            for (std::size_t si = 0; si < sets.size(); si++)
                for (int col = 0; col < 16; col++)
                {
                    const std::vector<u64> &set = sets[si];
                    InvFacts f{};
                    f.logn = logn;
                    f.flags = ((col & 1) ? kNttCanonical : 0) | ((col & 2) ? kNttAnyRep : 0) | ((col & 4) ? kNttDeferTop : 0);
                    f.live = set.data();
                    f.live_n = static_cast<int>(set.size());
                    f.tensor_load = (col & 8) != 0;
                    f.sw = kSwitchSettings[sw];
                    visit(logn, sw, set, static_cast<int>(si), col, f);
                }
    }
}

// ---- 3. the table
static std::string show(const FwdChoice &c)
{
    if (!c.valid)
        return "-";
    char buf[48];
    std::snprintf(buf, sizeof buf, "%d%d.%x%s%s", c.sched, c.treatment, c.flags, c.tickets ? "t" : "", c.aux_as_doubles ? "d" : "");
    return buf;
}
static std::string show(const InvChoice &c)
{
    if (!c.valid)
        return "-";
    char buf[16];
    std::snprintf(buf, sizeof buf, "%d%d%d%d", c.shape, c.sched, c.canon, c.top);
    return buf;
}
static std::string show(const std::vector<u64> &set)
{
    std::string s;
    for (u64 p : set)
        s += (s.empty() ? "" : "+") + std::to_string(p);
    return s;
}

// The table, with everything that repeats written once: "rows" are the distinct rows of choices (one choice per column);
// "patterns" the distinct ways one (ring, switches, source) maps its live sets to rows ("first-last:row ...", live sets by
// their place in live_sets, consecutive ones with the same row as a range); "cells" gives, per (ring, switches), the pattern
// of every source in the order of "sources".
struct Table
{
    std::vector<std::string> rows, patterns;
    std::vector<std::pair<std::string, std::string>> cells;
    std::string key, pattern, choices, cur_choices;
    int first = -1, last = -1, cur_set = -1;
    static std::size_t intern(std::vector<std::string> &v, const std::string &s)
    {
        for (std::size_t i = 0; i < v.size(); i++)
            if (v[i] == s)
                return i;
        v.push_back(s);
        return v.size() - 1;
    }
    void flush_set()
    {
        if (cur_set < 0)
            return;
        if (first >= 0 && cur_choices == choices)
            last = cur_set;
        else
        {
            flush_run();
            first = last = cur_set;
            choices = cur_choices;
        }
        cur_set = -1;
        cur_choices.clear();
    }
    void flush_run()
    {
        if (first >= 0)
            pattern += (pattern.empty() ? "" : " ") + std::to_string(first) + (last > first ? "-" + std::to_string(last) : "") + ":" +
                       std::to_string(intern(rows, choices));
        first = -1;
    }
    void flush_key()
    {
        flush_set();
        flush_run();
        if (!pattern.empty())
            cells.back().second += (cells.back().second.empty() ? "" : " ") + std::to_string(intern(patterns, pattern));
        pattern.clear();
    }
    // cell: "ring switches"; k: the source within it
    void add(const std::string &cell, const std::string &k, int set, int col, const std::string &choice)
    {
        if (col == 0)
        {
            if (cell + k != key)
            {
                flush_key();
                if (cells.empty() || cells.back().first != cell)
                    cells.push_back({ cell, "" });
                key = cell + k;
            }
            else
                flush_set();
            cur_set = set;
        }
        cur_choices += (cur_choices.empty() ? "" : " ") + choice;
    }
    static void print_list(const char *name, const std::vector<std::string> &v)
    {
        std::printf("    \"%s\": [\n", name);
        for (std::size_t i = 0; i < v.size(); i++)
            std::printf("      \"%s\"%s\n", v[i].c_str(), i + 1 < v.size() ? "," : "");
        std::printf("    ],\n");
    }
    void print(const char *name, const std::vector<std::string> &sources, bool last_one)
    {
        flush_key();
        std::printf("  \"%s\": {\n", name);
        print_list("sources", sources);
        print_list("rows", rows);
        print_list("patterns", patterns);
        std::printf("    \"cells\": {\n");
        for (std::size_t i = 0; i < cells.size(); i++)
            std::printf("      \"%s\": \"%s\"%s\n", cells[i].first.c_str(), cells[i].second.c_str(), i + 1 < cells.size() ? "," : "");
        std::printf("    }\n  }%s\n", last_one ? "" : ",");
    }
};

static int print_table()
{
    std::printf("{\n");
    std::printf("  \"format\": \"cells: per (ring, switches) the pattern of each source, in the order of sources; a pattern maps live "
                "sets (first-last, by their place in live_sets) to a row; a row holds one choice per column. "
                "forward choice: <schedule><treatment>.<flags, hex>[t: tickets][d: special prime as doubles], in-place column = bits "
                "(canonical, strict, any-rep, reduce-out, approx, top-done), gathered column = 0, any-rep, approx, both, then "
                "the same with strict; inverse choice: <shape><schedule><canon><top pass>, column = bits (canonical, any-rep, "
                "defer-top, tensor load); -: refused\",\n");
    std::printf("  \"live_sets\": {\n"); // (the values of a mixed set joined by +)
    for (int logn = 14; logn <= 16; logn++)
    {
        std::printf("    \"%d\": [", logn);
        const std::vector<std::vector<u64>> sets = live_sets(logn);
        for (std::size_t i = 0; i < sets.size(); i++)
            std::printf("\"%s\"%s", show(sets[i]).c_str(), i + 1 < sets.size() ? ", " : "");
        std::printf("]%s\n", logn < 16 ? "," : "");
    }
    std::printf("  },\n");
    Table fwd, inv;
    for_each_fwd([&](int logn, int sw, const FwdSource &s, const std::vector<u64> &, int si, int col, const FwdFacts &f) {
        fwd.add(std::to_string(logn) + " " + kSwitchNames[sw], s.name, si, col, show(select_fwd_half(f)));
    });
    for_each_inv([&](int logn, int sw, const std::vector<u64> &, int si, int col, const InvFacts &f) {
        inv.add(std::to_string(logn) + " " + kSwitchNames[sw], "", si, col, show(select_inv_half(f)));
    });
    std::vector<std::string> names;
    for (const FwdSource &s : fwd_sources())
        names.push_back(s.name);
    fwd.print("forward", names, false);
    inv.print("inverse", { "" }, true);
    std::printf("}\n");
    return 0;
}

// ---- 1. closure
static bool all_rows(const FwdFacts &f, bool (*pred)(u64, int))
{
    for (int i = 0; i < f.live_n; i++)
        if (!pred(f.live[i], f.logn))
            return false;
    return true;
}
// What the launcher refused before the rule moved here, stated independently of select_fwd_half:
//  - kNttTopDone on a gathered launch, without kNttReduceOut, with kNttCanonical, or with kNttStrict where the dense
//    schedule does not apply (it needs kNttAnyRep, no SEALHIP_NTT_EXACT_FWD, every live prime in fwd_dense_admits);
//  - kNttReduceOut on a gathered launch or with kNttCanonical;
//  - the mod-down store (treatment 7) where the FP64 instance does not apply or the ring is 2^14.
static bool parent_refuses(const FwdFacts &f)
{
    const int fl = f.flags;
    if (fl & kNttTopDone)
    {
        const bool dense = (fl & kNttAnyRep) && !f.sw.exact_fwd && all_rows(f, bounds::fwd_dense_admits);
        if (f.gathers || !(fl & kNttReduceOut) || (fl & kNttCanonical) || ((fl & kNttStrict) && !dense))
            return true;
    }
    if ((fl & kNttReduceOut) && (f.gathers || (fl & kNttCanonical)))
        return true;
    if (f.gathers && f.treatment == kTreatModDownStore)
    {
        const bool fp = !f.sw.no_fp64 && (fl & (kNttAnyRep | kNttCanonical)) && !(fl & kNttReduceOut) &&
                        all_rows(f, [](u64 p, int) { return p < kFpPrimeBound; }) && f.aux_p < kFpPrimeBound;
        if (!fp || f.logn < 15)
            return true;
    }
    return false;
}

static void closure()
{
    bool fwd_reached[17][kFwdInstanceCount] = {}, inv_reached[17][kInvInstanceCount] = {};
    long n_fwd = 0, n_inv = 0;
    for_each_fwd([&](int logn, int, const FwdSource &s, const std::vector<u64> &set, int, int col, const FwdFacts &f) {
        const FwdChoice c = select_fwd_half(f);
        n_fwd++;
        CHECK(c.valid == !parent_refuses(f), "forward %d %s %s column %d: valid = %d", logn, s.name.c_str(), show(set).c_str(), col, c.valid);
        if (!c.valid)
            return;
        const bool in_table = c.instance >= 0 && c.instance < kFwdInstanceCount && kFwdInstances[c.instance].sched == c.sched &&
                              kFwdInstances[c.instance].treatment == c.treatment && fwd_instance_at(logn, kFwdInstances[c.instance]);
        CHECK(in_table, "forward %d %s %s column %d: (%d, %d) is no instance at this ring size", logn, s.name.c_str(),
              show(set).c_str(), col, c.sched, c.treatment);
        if (in_table)
            fwd_reached[logn][c.instance] = true;
    });
    for_each_inv([&](int logn, int, const std::vector<u64> &set, int, int col, const InvFacts &f) {
        const InvChoice c = select_inv_half(f);
        n_inv++;
        const bool in_table = c.valid && c.instance >= 0 && c.instance < kInvInstanceCount && kInvInstances[c.instance].shape == c.shape &&
                              kInvInstances[c.instance].sched == c.sched && inv_instance_at(logn, kInvInstances[c.instance]);
        CHECK(in_table, "inverse %d %s column %d: (%d, %d) is no instance at this ring size", logn, show(set).c_str(), col, c.shape, c.sched);
        if (in_table)
            inv_reached[logn][c.instance] = true;
    });
    bool inv_any[kInvInstanceCount] = {};
    for (int logn = 14; logn <= 16; logn++)
    {
        int n = 0;
        for (int i = 0; i < kFwdInstanceCount; i++)
        {
            const bool exists = fwd_instance_at(logn, kFwdInstances[i]);
            CHECK(fwd_reached[logn][i] == exists, "forward instance (%d, %d) at 2^%d: exists %d, reached %d", kFwdInstances[i].sched,
                  kFwdInstances[i].treatment, logn, exists, fwd_reached[logn][i]);
            n += fwd_reached[logn][i];
        }
        CHECK(n == (logn == 14 ? 23 : 24), "forward instances reached at 2^%d: %d", logn, n);
        n = 0;
        for (int i = 0; i < kInvInstanceCount; i++)
        {
            const bool exists = inv_instance_at(logn, kInvInstances[i]);
            CHECK(inv_reached[logn][i] == exists, "inverse instance (%d, %d) at 2^%d: exists %d, reached %d", kInvInstances[i].shape,
                  kInvInstances[i].sched, logn, exists, inv_reached[logn][i]);
            n += inv_reached[logn][i];
            inv_any[i] = inv_any[i] || inv_reached[logn][i];
        }
        CHECK(n == 11, "inverse instances reached at 2^%d: %d", logn, n);
    }
    CHECK(kFwdInstanceCount == 24 && kInvInstanceCount == 15, "table sizes");
    for (int i = 0; i < kInvInstanceCount; i++)
        CHECK(inv_any[i], "inverse instance %d never reached", i);
    std::printf("closure: %ld forward and %ld inverse inputs\n", n_fwd, n_inv);
}

// ---- 2. anchors
static const NttSwitches kNoSwitches = { false, false, false, false };
static FwdFacts inplace(int logn, int flags, const std::vector<u64> &rows, NttSwitches sw = kNoSwitches)
{
    return fwd_facts(logn, sw, FwdSource{ "inplace", false, false, false, kTreatNone, 0, 0, true }, rows, flags);
}
static FwdFacts gathered(int logn, int flags, const std::vector<u64> &rows, int treatment, u64 aux_p, NttSwitches sw = kNoSwitches)
{
    return fwd_facts(logn, sw, FwdSource{ "special", true, true, true, treatment, 0, aux_p, true }, rows, flags);
}

static void anchors()
{
    const NttSwitches no_fp64 = { true, false, false, false }, exact_inv = { false, false, true, false };
    for (int logn = 14; logn <= 16; logn++)
    {
        const Edges e = edges_of(logn);
        const std::vector<u64> p49 = { (u64(1) << 49) + 1 }, p61 = { (u64(1) << 61) - 1 };
        FwdChoice c = select_fwd_half(inplace(logn, kNttCanonical, { kFpPrimeBound - 1 }));
        CHECK(c.valid && c.sched == kSchedFp64 && c.treatment == kTreatNone && c.tickets, "canonical below 2^50: %s", show(c).c_str());
        CHECK(bounds::fwd_canon_admits(p49[0], logn), "2^49 + 1 is a fwd_canon prime");
        c = select_fwd_half(inplace(logn, kNttCanonical, p49, no_fp64));
        CHECK(c.valid && c.sched == kSchedApprox && c.treatment == kTreatNone && (c.flags & kNttAnyRep) && (c.flags & kNttCanonical),
              "canonical, NO_FP64: %s", show(c).c_str());
        c = select_fwd_half(inplace(logn, kNttCanonical | kNttStrict, p61));
        CHECK(c.valid && c.sched == kSchedHarvey && c.treatment == kTreatNone && (c.flags & kNttStrict), "canonical | strict at 61 bits: %s",
              show(c).c_str());
        c = select_fwd_half(inplace(logn, kNttReduceOut | kNttAnyRep | kNttStrict | kNttTopDone, { e.fwd_dense }));
        CHECK(c.valid && c.sched == kSchedDense && c.treatment == kTreatReduceOutTopDone && c.treatment == 6 && !c.tickets &&
                  !(c.flags & kNttAnyRep),
              "dense, top done: %s", show(c).c_str());
        {
            const std::vector<u64> rows(5, (u64(1) << 55) - 55); // key modulus of 60 bits: not every one below kFpInputBound
            const FwdSource digit = { "digit", true, true, true, kTreatBarrett, 5, 0, false };
            c = select_fwd_half(fwd_facts(logn, kNoSwitches, digit, rows, kNttAnyRep | kNttApprox));
            CHECK(c.valid && c.sched == kSchedApprox && c.treatment == kTreatBarrett && c.treatment == 1 && (c.flags & kNttPolyMajor) &&
                      ((c.flags >> 16) & 0xFF) == 4 && !c.tickets,
                  "key-switch digit launch: %s", show(c).c_str());
        }
        // refused
        CHECK(!select_fwd_half(gathered(logn, kNttAnyRep, p49, kTreatModDownStore, p49[0], no_fp64)).valid, "treatment 7 with NO_FP64");
        CHECK(select_fwd_half(gathered(logn, kNttAnyRep, p49, kTreatModDownStore, p49[0])).valid == (logn >= 15), "treatment 7 at 2^%d", logn);
        CHECK(!select_fwd_half(inplace(logn, kNttReduceOut | kNttCanonical, p49)).valid, "reduce-out | canonical");
        CHECK(!select_fwd_half(inplace(logn, kNttTopDone, p49)).valid, "top-done without reduce-out");
        CHECK(!select_fwd_half(gathered(logn, kNttReduceOut | kNttTopDone, p49, kTreatNone, 0)).valid, "top-done on a gathered launch");

        // inverse
        InvFacts f{};
        f.logn = logn;
        f.sw = kNoSwitches;
        const std::vector<u64> fp_rows = { kFpPrimeBound - 1 };
        f.live = fp_rows.data();
        f.live_n = 1;
        f.flags = kNttCanonical;
        InvChoice ic = select_inv_half(f);
        if (logn <= 15)
            CHECK(ic.valid && ic.shape == kShapeWhole && ic.sched == kInvFp64 && ic.canon == 1 && ic.top == kTopNone, "whole row: %s", show(ic).c_str());
        else
            CHECK(ic.valid && ic.shape == kShapeQuarter && ic.sched == kInvFp64 && ic.top == kTopRadix4, "quarter row: %s", show(ic).c_str());
        f.sw = exact_inv; // switches lazy-sum and dense off, FP64 stays
        CHECK(select_inv_half(f).sched == kInvFp64, "EXACT_INV keeps FP64");
        for (const std::vector<u64> &set : live_sets(logn))
        {
            f.live = set.data();
            f.live_n = static_cast<int>(set.size());
            f.flags = kNttAnyRep | kNttDeferTop;
            f.tensor_load = true;
            f.sw = kNoSwitches;
            bool lazy = true, dense = true;
            for (u64 p : set)
            {
                lazy = lazy && bounds::inv_lazy_admits(logn - 1, p);
                dense = dense && bounds::inv_dense_admits(logn - 1, p);
            }
            ic = select_inv_half(f);
            CHECK(ic.valid && ic.shape == kShapeHalfTensor && ic.top == kTopNone && ic.canon == 0 &&
                      ic.sched == (lazy ? kInvLazySum : (dense ? kInvDense : kInvExact)),
                  "tensor load at %s: %s", show(set).c_str(), show(ic).c_str());
            f.sw = exact_inv;
            f.tensor_load = false;
            f.flags = kNttAnyRep;
            ic = select_inv_half(f);
            CHECK(ic.sched == kInvExact || ic.sched == kInvFp64, "EXACT_INV at %s: %s", show(set).c_str(), show(ic).c_str());
        }
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "--table")
        return print_table();
    closure();
    anchors();
    std::printf(failures ? "ntt_select_check: %d FAILURES\n" : "ntt_select_check: OK\n", failures);
    return failures ? 1 : 0;
}
