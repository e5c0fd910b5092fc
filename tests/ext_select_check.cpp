// ext_select_check.cpp -- CPU test of select_ext_mac (gemini-seal_amd/csrc/mac_select.hpp), what launch_ext_mac (rgsw.hip)
// runs for the external product's inner product (built and run by tests/test_rgsw_host.py).
// 1. `ext_select_check --calls FILE`: every line of FILE is a call in plain numbers, `logn nd rows count`, and gets one
//    line: family nd2 group n_groups blocks. The Python statement of the rule must print the same.
// 2. No argument: invariants over rings 2^3..2^16 x nd 1..17 x counts around every threshold. The items family runs from
//    16 items on, on rings of a workgroup or more, while 2 nd has an instance, and names the even instance 2 nd; everything
//    else is the loop kernel; nd < 1 is refused; the item group is min(count, 8), 16, 32 or 64, chosen for a key of 2 nd
//    slices (twice the key switch's at the same level); the grid covers the launch's lanes exactly and every instance a
//    choice names exists. Prints `ext_select_check: OK`.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mac_select.hpp"

using namespace sealhip;

static int failures = 0;
#define CHECK(cond, ...)                                         \
    do                                                           \
    {                                                            \
        if (!(cond))                                             \
        {                                                        \
            if (failures++ < 20)                                 \
            {                                                    \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
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
    int logn, nd;
    unsigned long long rows, count;
    while (std::fscanf(f, "%d %d %llu %llu", &logn, &nd, &rows, &count) == 4)
    {
        const MacChoice c = select_ext_mac(logn, nd, rows, count);
        std::printf("%s %d %zu %zu %u\n", kFamilyNames[c.family], c.nd, c.group, c.n_groups, c.blocks);
    }
    const bool whole = std::feof(f) != 0;
    std::fclose(f);
    if (!whole)
        std::printf("malformed line\n");
    return whole ? 0 : 2;
}

static unsigned cover(std::size_t lanes)
{
    return static_cast<unsigned>((lanes + 255) / 256);
}

static void check_rule()
{
    static_assert(kThreads == 256 && kMacMaxDigits == 16, "the figures this program restates");
    const std::size_t counts[] = { 1, 7, 8, 15, 16, 17, 33, 49, 255, 256, 1000, 4096, 5000 };
    long long chosen[4] = {};
    bool group_seen[65] = {};
    for (int logn = 3; logn <= 16; logn++)
        for (int nd = 1; nd <= 17; nd++)
            for (int nsp : { 1, 3 })
                for (std::size_t count : counts)
                {
                    const std::size_t rows = static_cast<std::size_t>(nd) * nsp + nsp;
                    const MacChoice c = select_ext_mac(logn, nd, rows, count);
                    chosen[c.family]++;
                    const bool items = count >= 16 && logn >= 8 && 2 * nd <= 16;
                    CHECK(c.family == (items ? kMacItems : kMacLoop), "family %d at logn %d nd %d count %zu", c.family, logn, nd, count);
                    if (!items)
                    {
                        CHECK(c.nd == 0 && c.group == 0 && c.blocks == cover((count * rows) << logn), "loop: nd %d blocks %u", c.nd, c.blocks);
                        continue;
                    }
                    CHECK(c.nd == 2 * nd && c.nd % 2 == 0 && mac_has_instance(c.nd), "instance %d at nd %d", c.nd, nd);
                    int got = 0;
                    CHECK(dispatch_mac_digits(c.nd, [&](auto v) { got = decltype(v)::value; }) && got == c.nd, "no instance %d", c.nd);
                    // the group: the key switch's rule for a key of 2 nd slices
                    CHECK(c.group == mac_item_group(logn, 2 * nd, rows, 1, count), "group %zu", c.group);
                    CHECK(c.group == 8 || c.group == 16 || c.group == 32 || c.group == 64, "group %zu", c.group);
                    const bool large_key = 2 * static_cast<std::size_t>(2 * nd) * rows * 8 * (std::size_t(1) << logn) > (std::size_t(48) << 20);
                    CHECK(c.group <= (large_key ? 64u : 16u), "group %zu above its cap", c.group);
                    if (c.group > 8)
                        CHECK(((c.n_groups * rows) << logn) / 256 >= 4096, "group %zu leaves too few workgroups", c.group);
                    group_seen[c.group] = true;
                    CHECK(c.n_groups == (count + c.group - 1) / c.group, "%zu groups", c.n_groups);
                    CHECK(c.blocks == cover((c.n_groups * rows) << logn) && ((c.n_groups * rows) << logn) % 256 == 0, "blocks %u", c.blocks);
                }
    for (int nd : { 0, -1 })
        CHECK(select_ext_mac(12, nd, 4, 64).family == kMacRefused, "nd %d not refused", nd);
    CHECK(chosen[kMacLoop] && chosen[kMacItems] && !chosen[kMacRefused] && !chosen[kMacPair], "families chosen");
    CHECK(group_seen[8] && group_seen[16] && group_seen[32] && group_seen[64], "a group size never chosen");
    // the thresholds the device tests stand on: batches 15 | 16, rings 2^7 | 2^8, nd 8 | 9
    CHECK(select_ext_mac(12, 3, 4, 15).family == kMacLoop && select_ext_mac(12, 3, 4, 16).family == kMacItems, "the batch threshold");
    CHECK(select_ext_mac(7, 3, 4, 64).family == kMacLoop && select_ext_mac(8, 3, 4, 64).family == kMacItems, "the ring threshold");
    CHECK(select_ext_mac(12, 8, 9, 64).nd == 16 && select_ext_mac(12, 9, 10, 64).family == kMacLoop, "the digit threshold");
}

int main(int argc, char **argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "--calls"))
        return print_calls(argv[2]);
    check_rule();
    if (failures)
    {
        std::printf("ext_select_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("ext_select_check: OK\n");
    return 0;
}
