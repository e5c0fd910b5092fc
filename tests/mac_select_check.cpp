// mac_select_check.cpp -- CPU test of gemini-seal_amd/csrc/mac_select.hpp and instance_dispatch.hpp (built and run by
// tests/test_ks_instances_host.py): what launch_ks_mac, launch_hoist_mac, launch_hoist_dot_mac and launch_hoist_giant_mac
// run, evaluated without a device by the very functions the launchers call.
// 1. `mac_select_check --calls FILE`: every line of FILE is a call in plain numbers,
//        op logn nd rows n_elts count n_sums j0 j1 pair        (op: ks | hoist | dot | giant)
//    and gets one line: family nd slots prefetch group n_groups blocks. The Python statement of the rules must print the same.
// 2. No argument: invariants over rings 2^6..2^16 x nd 1..17 x n_elts 1..16 x counts around every threshold.
//    The group is in {min(count, 8), 16, 32, 64}; a group above 8 leaves kMacMinWorkgroups workgroups (counted here from the
//    launch's own geometry) and the next larger candidate, where the key's size admits one, would not; the pair form is
//    chosen only inside ks_mac_has_pair_form and refused outside; instances only for nd <= 16 (and, in hoist.hip, rings of
//    a workgroup or more); the grid covers the launch's lanes exactly; the dispatchers call the instance of the value and
//    no other, and every nd a choice names has an instance. Prints `mac_select_check: OK`.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mac_select.hpp"

using namespace sealhip;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do                                                       \
    {                                                        \
        if (!(cond))                                         \
        {                                                    \
            if (failures++ < 20)                             \
            {                                                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                    \
                std::printf("\n");                           \
            }                                                \
        }                                                    \
    } while (0)

static const char *kFamilyNames[] = { "refused", "loop", "items", "pair" };

static int print_calls(const char *path)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f)
    {
        std::printf("cannot open %s\n", path);
        return 2;
    }
    char op[16];
    int logn, nd, n_elts, j0, j1, pair;
    unsigned long long rows, count, n_sums;
    while (std::fscanf(f, "%15s %d %d %llu %d %llu %llu %d %d %d", op, &logn, &nd, &rows, &n_elts, &count, &n_sums, &j0, &j1, &pair) == 10)
    {
        MacChoice c{};
        if (!std::strcmp(op, "ks"))
            c = select_ks_mac(logn, nd, rows, count, j0, j1, pair != 0);
        else if (!std::strcmp(op, "hoist"))
            c = select_hoist_mac(logn, nd, rows, n_elts, count);
        else if (!std::strcmp(op, "dot"))
            c = select_hoist_dot_mac(logn, nd, rows, n_elts, count, n_sums);
        else if (!std::strcmp(op, "giant"))
            c = select_hoist_giant_mac(logn, nd, rows, n_elts, count);
        else
        {
            std::printf("unknown op %s\n", op);
            std::fclose(f);
            return 2;
        }
        std::printf("%s %d %d %d %zu %zu %u\n", kFamilyNames[c.family], c.nd, c.slots, c.prefetch ? 1 : 0, c.group, c.n_groups,
                    c.blocks);
    }
    const bool whole = std::feof(f) != 0;
    std::fclose(f);
    if (!whole)
        std::printf("malformed line\n");
    return whole ? 0 : 2;
}

// ---- the dispatchers: the instance called is the value's, exactly one is, and the result says whether one was
template <int Lo, int Hi>
static void check_dispatch_int()
{
    for (int v = Lo - 2; v <= Hi + 2; v++)
    {
        int calls = 0, got = 0;
        const bool hit = dispatch_int<Lo, Hi>(v, [&](auto c) { calls++, got = decltype(c)::value; });
        const bool in = v >= Lo && v <= Hi;
        CHECK(hit == in && calls == (in ? 1 : 0) && (!in || got == v), "dispatch_int<%d, %d>(%d): hit %d, %d calls, instance %d", Lo,
              Hi, v, hit, calls, got);
    }
}
static void check_dispatchers()
{
    check_dispatch_int<1, kMacMaxDigits>();
    check_dispatch_int<2, 4>();
    check_dispatch_int<1, 15>();
    check_dispatch_int<1, 4>();
    check_dispatch_int<-3, 0>();
    check_dispatch_int<5, 5>();
    for (int v = 0; v <= 70; v++)
    {
        int calls = 0, got = 0;
        const bool hit = dispatch_among<4, 8, 16, 32, 64>(v, [&](auto c) { calls++, got = decltype(c)::value; });
        const bool in = v == 4 || v == 8 || v == 16 || v == 32 || v == 64;
        CHECK(hit == in && calls == (in ? 1 : 0) && (!in || got == v), "dispatch_among(%d): hit %d, %d calls, instance %d", v, hit, calls, got);
    }
    for (int v = 0; v <= 1; v++)
    {
        int calls = 0, got = -1;
        dispatch_bool(v != 0, [&](auto c) { calls++, got = decltype(c)::value ? 1 : 0; });
        CHECK(calls == 1 && got == v, "dispatch_bool(%d): %d calls, instance %d", v, calls, got);
    }
    // every digit count a choice can name has its instance, the loop kernel's 0 and the first count without one have none
    for (int nd = 0; nd <= kMacMaxDigits + 1; nd++)
    {
        int got = 0;
        const bool hit = dispatch_mac_digits(nd, [&](auto c) { got = decltype(c)::value; });
        CHECK(hit == mac_has_instance(nd) && (!hit || got == nd), "dispatch_mac_digits(%d): hit %d, instance %d", nd, hit, got);
    }
}

// ---- the rule
static std::size_t workgroups(std::size_t n_groups, std::size_t rows, std::size_t n_elts, int logn)
{
    return ((n_groups * rows * n_elts) << logn) / 256;
}
// the group rule's invariants for a launch of `count` ciphertexts whose lanes are (group, row, element, coefficient)
static void check_group(const char *who, const MacChoice &c, int logn, int nd, std::size_t rows, std::size_t n_elts, std::size_t count)
{
    const std::size_t small = count < 8 ? count : 8;
    CHECK(c.group == small || c.group == 16 || c.group == 32 || c.group == 64, "%s: group %zu", who, c.group);
    CHECK(c.group >= 1 && c.n_groups == (count + c.group - 1) / c.group, "%s: %zu groups of %zu for %zu", who, c.n_groups, c.group, count);
    const bool large_key = 2 * static_cast<std::size_t>(nd) * rows * n_elts * 8 * (std::size_t(1) << logn) > (std::size_t(48) << 20);
    const std::size_t cap = large_key ? 64 : 16;
    CHECK(c.group <= cap, "%s: group %zu above the cap %zu", who, c.group, cap);
    if (c.group > 8)
        CHECK(workgroups(c.n_groups, rows, n_elts, logn) >= 4096, "%s: group %zu leaves %zu workgroups", who, c.group,
              workgroups(c.n_groups, rows, n_elts, logn));
    // every larger candidate the key's size admits would leave fewer than 4096
    for (std::size_t g = c.group > 8 ? 2 * c.group : 16; g <= cap; g *= 2)
        CHECK(workgroups((count + g - 1) / g, rows, n_elts, logn) < 4096, "%s: group %zu although %zu leaves %zu workgroups", who,
              c.group, g, workgroups((count + g - 1) / g, rows, n_elts, logn));
}
static unsigned cover(std::size_t lanes)
{
    return static_cast<unsigned>((lanes + 255) / 256);
}

static void check_rule()
{
    static_assert(kThreads == 256 && kMacMaxDigits == 16 && kHoistMaxElts == 16, "the figures this program restates");
    const std::size_t counts[] = { 1, 7, 8, 15, 16, 17, 49, 255, 256, 1000, 4096, 5000 };
    long long chosen[4][4] = {}; // [launcher][family]
    bool group_seen[65] = {};
    for (int logn = 6; logn <= 16; logn++)
        for (int nd = 1; nd <= 17; nd++)
            for (int nsp : { 1, 3 })
                for (std::size_t count : counts)
                {
                    const std::size_t rows = static_cast<std::size_t>(nd) * nsp + nsp, N = std::size_t(1) << logn;
                    const bool ring_ok = N >= 256, inst = nd <= 16;
                    // launch_ks_mac
                    for (int pair = 0; pair <= 1; pair++)
                        for (int jr = 0; jr < 5; jr++)
                        {
                            const int j0 = jr == 1 ? 1 : (jr == 3 ? -1 : (jr == 4 ? 2 : 0)), j1 = jr == 2 ? nd - 1 : (jr == 3 ? nd : (jr == 4 ? 1 : nd));
                            const MacChoice c = select_ks_mac(logn, nd, rows, count, j0, j1, pair != 0);
                            const bool range_ok = j0 >= 0 && j0 <= j1 && j1 <= nd, all = j0 == 0 && j1 == nd;
                            const bool form = ks_mac_has_pair_form(logn, nd, count, j0, j1);
                            CHECK(form == (logn >= 14 && count >= 16 && all && inst), "pair form at logn %d nd %d count %zu [%d, %d)", logn, nd, count, j0, j1);
                            chosen[0][c.family]++;
                            if (!range_ok || (pair && !form))
                            {
                                CHECK(c.family == kMacRefused, "ks_mac: family %d for a call to refuse", c.family);
                                continue;
                            }
                            CHECK(c.family != kMacRefused, "ks_mac refuses a valid call");
                            CHECK((c.family == kMacPair) == (pair != 0), "ks_mac: pair %d, family %d", pair, c.family);
                            if (c.family == kMacPair)
                                CHECK(form, "ks_mac: the pair form outside ks_mac_has_pair_form");
                            if (c.family == kMacLoop)
                            {
                                CHECK(!(count >= 16 && all && inst), "ks_mac: loop kernel where an instance exists");
                                CHECK(c.nd == 0 && c.blocks == cover((count * rows) << logn), "ks_mac loop: nd %d blocks %u", c.nd, c.blocks);
                                continue;
                            }
                            CHECK(count >= 16 && all && inst && c.nd == nd && mac_has_instance(c.nd), "ks_mac: instance %d at nd %d count %zu", c.nd, nd, count);
                            CHECK(c.prefetch == (c.family == kMacPair && nd <= 8), "ks_mac: prefetch %d at nd %d", c.prefetch, nd);
                            check_group("ks_mac", c, logn, nd, rows, 1, count);
                            group_seen[c.group] = true;
                            CHECK(c.group >= 8, "ks_mac: its instances run from 16 ciphertexts on, min(count, 8) is 8");
                            const std::size_t lanes = (c.n_groups * rows) << logn;
                            CHECK(c.blocks == cover(c.family == kMacPair ? lanes / 2 : lanes), "ks_mac: %u blocks", c.blocks);
                        }
                    // the hoisted launchers
                    for (int n_elts = 1; n_elts <= 16; n_elts++)
                    {
                        const MacChoice c = select_hoist_mac(logn, nd, rows, n_elts, count);
                        chosen[1][c.family]++;
                        CHECK((c.family == kMacItems) == (ring_ok && inst) && (c.family == kMacLoop) == !(ring_ok && inst), "hoist_mac: family %d", c.family);
                        if (c.family == kMacItems)
                        {
                            check_group("hoist_mac", c, logn, nd, rows, n_elts, count);
                            group_seen[c.group] = true;
                            CHECK(c.nd == nd && c.blocks == cover((c.n_groups * rows * n_elts) << logn), "hoist_mac: nd %d blocks %u", c.nd, c.blocks);
                        }
                        else
                            CHECK(c.nd == 0 && c.blocks == cover((count * rows * n_elts) << logn), "hoist_mac loop: blocks %u", c.blocks);
                        const MacChoice g = select_hoist_giant_mac(logn, nd, rows, n_elts, count);
                        chosen[3][g.family]++;
                        CHECK(g.family == (ring_ok && inst ? kMacItems : kMacLoop) && g.nd == (g.family == kMacItems ? nd : 0), "hoist_giant_mac: family %d", g.family);
                        CHECK(g.blocks == cover(((g.family == kMacItems ? (count + 3) / 4 : count) * rows) << logn), "hoist_giant_mac: blocks %u", g.blocks);
                        for (std::size_t n_sums = 1; n_sums <= 9; n_sums++)
                        {
                            const MacChoice s = select_hoist_dot_mac(logn, nd, rows, n_elts, count, n_sums);
                            chosen[2][s.family]++;
                            CHECK(s.family == (ring_ok && inst ? kMacItems : kMacLoop), "hoist_dot_mac: family %d", s.family);
                            if (s.family == kMacLoop)
                            {
                                CHECK(s.nd == 0 && s.slots == 0 && s.blocks == cover((n_sums * count * rows) << logn), "hoist_dot_mac loop: blocks %u", s.blocks);
                                continue;
                            }
                            const std::size_t S = static_cast<std::size_t>(s.slots);
                            CHECK(s.nd == nd && (S == 1 || S == 2 || S == 4) && S == (n_sums >= 3 ? 4 : n_sums), "hoist_dot_mac: S %zu for %zu sums", S, n_sums);
                            // the lanes' slots hold every (sum, ciphertext), and no lane group could be spared
                            const std::size_t sum_tiles = (n_sums + S - 1) / S, ct_tiles = (count + 4 / S - 1) / (4 / S);
                            CHECK(s.n_groups == sum_tiles * ct_tiles && sum_tiles * S >= n_sums && (sum_tiles - 1) * S < n_sums &&
                                      ct_tiles * (4 / S) >= count && (ct_tiles - 1) * (4 / S) < count,
                                  "hoist_dot_mac: %zu lane groups", s.n_groups);
                            CHECK(s.blocks == cover((s.n_groups * rows) << logn), "hoist_dot_mac: blocks %u", s.blocks);
                        }
                    }
                    // element counts outside a launch
                    for (int n_elts : { -1, 17 })
                        CHECK(select_hoist_mac(logn, nd, rows, n_elts, count).family == kMacRefused &&
                                  select_hoist_dot_mac(logn, nd, rows, n_elts, count, 1).family == kMacRefused &&
                                  select_hoist_giant_mac(logn, nd, rows, n_elts, count).family == kMacRefused,
                              "%d elements not refused", n_elts);
                }
    // the grid exercises what it claims to: every family of every launcher, every group size
    CHECK(chosen[0][kMacRefused] && chosen[0][kMacLoop] && chosen[0][kMacItems] && chosen[0][kMacPair], "ks_mac: a family never chosen");
    for (int l = 1; l <= 3; l++)
        CHECK(chosen[l][kMacLoop] && chosen[l][kMacItems] && !chosen[l][kMacPair], "launcher %d: families chosen", l);
    CHECK(group_seen[1] && group_seen[7] && group_seen[8] && group_seen[16] && group_seen[32] && group_seen[64], "a group size never chosen");
    // anchors: the measured configurations the constants come from (profiles/r02/ks_mac_group.txt), 4096 ciphertexts
    CHECK(select_ks_mac(15, 7, 8, 4096, 0, 7, false).group == 16, "config 3 (29 MB of key): group 16");
    CHECK(select_ks_mac(15, 7, 8, 4096, 0, 7, true).prefetch && !select_ks_mac(15, 9, 10, 4096, 0, 9, true).prefetch, "the prefetch cut");
    CHECK(select_ks_mac(16, 8, 34, 4096, 0, 8, false).group == 64, "more than 48 MiB of key: group 64");
    // tests/test_gpu_ks_instances.py group16: 49 ciphertexts, 16 elements, 17 rows, N = 2^10: 4 x 17 x 16 x 4 = 4352 workgroups
    CHECK(select_hoist_mac(10, 16, 17, 16, 49).group == 16 && select_hoist_mac(10, 16, 17, 16, 48).group == 8, "the group16 case");
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "--calls"))
        return print_calls(argv[2]);
    check_dispatchers();
    check_rule();
    if (failures)
    {
        std::printf("mac_select_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("mac_select_check: OK\n");
    return 0;
}
