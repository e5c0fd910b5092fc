// mac_select.hpp -- which kernel the key switch's inner-product launchers run and with what launch shape: launch_ks_mac
// (keyswitch.hip), launch_hoist_mac, launch_hoist_dot_mac and launch_hoist_giant_mac (hoist.hip), launch_ext_mac (rgsw.hip;
// its check program is tests/ext_select_check.cpp, its second statement in tests/test_rgsw_host.py), as pure functions of plain
// numbers. No Engine, no HIP: tests/mac_select_check.cpp compiles this header with a host compiler, checks the rule's
// invariants over a grid and prints the choice for any call; tests/test_ks_instances_host.py holds the second statement of
// the rule and requires the two to agree call by call. The launchers gather the numbers, call the selector and dispatch
// on the result (instance_dispatch.hpp); they compute none of this themselves.
//   logn          the ring is 2^logn
//   nd, rows      digits of the level (KsDev::nd) and rows of the extended basis (k + nsp)
//   n_elts        Galois elements (giants) of the launch
//   count, n_sums ciphertexts and weighted sums of the launch
#pragma once
#include <cstddef>

#include "instance_dispatch.hpp"

namespace sealhip
{
    constexpr int kThreads = 256;        // lanes of a workgroup, every elementwise launch of the engine
    constexpr int kMacMaxDigits = 16;    // the families are instantiated for ND = 1 .. kMacMaxDigits
    constexpr int kHoistMaxElts = 16;    // elements of one hoisted launch (HoistElts and its kin, engine.hpp)
    // digits up to which the pair form keeps the next ciphertext's words in flight (194 registers at nd = 7; without it 138 and the
    // same time within the spread, profiles/r18/ks_split_last_ab.txt; 24 registers more per digit: from nd = 10 on the prefetch
    // would leave one wave per SIMD. Measured at nd = 7 only.)
    constexpr int kKsPairPrefetchDigits = 8;

    // ---- the item group: ciphertexts that share one key load
    // 8 for small batches (enough workgroups to fill the chip), else 16 -- or 64 when the key slices the kernel reads
    // (2 * nd * rows rows per element) are too large to stay in the memory-side cache between groups
    // (profiles/r02/ks_mac_group.txt: config 4, 69 MB of key: 9.15 -> 7.96 ms per step; config 5, 251 MB: 9.38 -> 7.66;
    // config 3, 29 MB: 3.68 -> 3.60 at 16, but 3.9-4.1 at 32)
    constexpr std::size_t kMacKeyCacheBytes = std::size_t(48) << 20;
    // a larger group must still leave this many workgroups: two full rounds of the chip's resident set
    constexpr std::size_t kMacMinWorkgroups = 4096;
    constexpr std::size_t kMacSmallGroup = 8;

    constexpr std::size_t mac_ceil_div(std::size_t a, std::size_t b)
    {
        return (a + b - 1) / b;
    }
    constexpr unsigned blocks_for(std::size_t lanes)
    {
        return static_cast<unsigned>(mac_ceil_div(lanes, kThreads));
    }
    // The largest candidate (64 or 16, halving down to 16) that leaves kMacMinWorkgroups, else min(count, 8).
    // launch_hoist_mac runs its instances at any count, hence the min; ks_mac_items and ks_mac_pair run only at
    // count >= 16 (select_ks_mac), where min(count, 8) is the 8 that launch_ks_mac used to start from.
    constexpr std::size_t mac_item_group(int logn, int nd, std::size_t rows, std::size_t n_elts, std::size_t count)
    {
        const std::size_t key_bytes = (2ull * nd * rows * n_elts) << (logn + 3);
        for (std::size_t g = key_bytes > kMacKeyCacheBytes ? 64 : 16; g > kMacSmallGroup; g >>= 1)
            if (((mac_ceil_div(count, g) * rows * n_elts) << logn) / kThreads >= kMacMinWorkgroups)
                return g;
        return count < kMacSmallGroup ? count : kMacSmallGroup;
    }

    // ---- what a launcher runs
    enum MacFamily
    {
        kMacRefused = 0, // hipErrorInvalidValue
        kMacLoop,        // one lane per (ciphertext, row, coefficient), the digit count a run-time bound
        kMacItems,       // <nd>: a lane walks the ciphertexts of its item group (or its four slots) per key load
        kMacPair,        // ks_mac_pair_kernel<nd, prefetch>: the items form over pairs of coefficients
    };
    struct MacChoice
    {
        int family;
        int nd;               // the instance's ND (0: the loop kernel)
        int slots;            // hoist_dot_mac's S in {1, 2, 4}: sums per lane, the rest of its four slots ciphertexts (else 0)
        bool prefetch;        // the pair form's second template argument
        std::size_t group;    // ciphertexts per key load (ks_mac, hoist_mac; else 0)
        std::size_t n_groups; // item groups (lane groups of hoist_dot_mac and hoist_giant_mac) of the launch
        unsigned blocks;      // the grid
    };
    constexpr bool mac_has_instance(int nd)
    {
        return nd >= 1 && nd <= kMacMaxDigits;
    }
    // f(std::integral_constant<int, ND>{}) for MacChoice::nd: the one range all five families are instantiated over, so a
    // choice with an instance always finds it (false: nd == 0, the loop kernel)
    template <class F>
    bool dispatch_mac_digits(int nd, F &&f)
    {
        return dispatch_int<1, kMacMaxDigits>(nd, f);
    }
    // hoist.hip's instances tile a row with whole workgroups; a ring below one runs the per-lane kernel
    constexpr bool hoist_has_instance(int logn, int nd)
    {
        return (std::size_t(1) << logn) >= static_cast<std::size_t>(kThreads) && mac_has_instance(nd);
    }

    // the pair form exists where the items kernel does: all digits in one call, batches of at least 16, up to 16 digits
    constexpr bool ks_mac_has_pair_form(int logn, int nd, std::size_t count, int j0, int j1)
    {
        return logn >= 14 && count >= 16 && j0 == 0 && j1 == nd && mac_has_instance(nd);
    }

    // launch_ks_mac over digits [j0, j1) of nd (the launcher has replaced j1 < 0 by nd); pair: the digit rows lack their
    // last layer (kNttSplitLast), which only the pair form applies -- no other kernel may read them
    constexpr MacChoice select_ks_mac(int logn, int nd, std::size_t rows, std::size_t count, int j0, int j1, bool pair)
    {
        MacChoice c{};
        if (j0 < 0 || j0 > j1 || j1 > nd || (pair && !ks_mac_has_pair_form(logn, nd, count, j0, j1)))
            return c;
        if (count >= 16 && j0 == 0 && j1 == nd && mac_has_instance(nd))
        {
            c.family = pair ? kMacPair : kMacItems;
            c.nd = nd;
            c.prefetch = pair && nd <= kKsPairPrefetchDigits;
            c.group = mac_item_group(logn, nd, rows, 1, count);
            c.n_groups = mac_ceil_div(count, c.group);
            // (pair: one lane per pair of coefficients -- half the lanes, the items kernel's group size)
            c.blocks = blocks_for((c.n_groups * rows) << (pair ? logn - 1 : logn));
            return c;
        }
        // small batches, a digit range or more than 16 digits
        c.family = kMacLoop;
        c.blocks = blocks_for((count * rows) << logn);
        return c;
    }

    // launch_ext_mac (rgsw.hip): the 2 nd digits of a ciphertext's two components against the two
    // halves of one RGSW block. The items family is instantiated for even ND2 = 2 nd up to kMacMaxDigits and tiles a row
    // with whole workgroups; its key words are twice a key switch's, which is what mac_item_group is told. The batch
    // threshold and the group constants are the key switch's, not tuned for this kernel (section 29, "Open").
    constexpr bool ext_mac_has_instance(int logn, int nd)
    {
        return nd >= 1 && (std::size_t(1) << logn) >= static_cast<std::size_t>(kThreads) && mac_has_instance(2 * nd);
    }
    constexpr MacChoice select_ext_mac(int logn, int nd, std::size_t rows, std::size_t count)
    {
        MacChoice c{};
        if (nd < 1)
            return c;
        if (count >= 16 && ext_mac_has_instance(logn, nd))
        {
            c.family = kMacItems;
            c.nd = 2 * nd;
            c.group = mac_item_group(logn, 2 * nd, rows, 1, count);
            c.n_groups = mac_ceil_div(count, c.group);
            c.blocks = blocks_for((c.n_groups * rows) << logn);
            return c;
        }
        // small batches, rings below one workgroup per row, 2 nd > kMacMaxDigits
        c.family = kMacLoop;
        c.blocks = blocks_for((count * rows) << logn);
        return c;
    }

    constexpr MacChoice select_hoist_mac(int logn, int nd, std::size_t rows, int n_elts, std::size_t count)
    {
        MacChoice c{};
        if (n_elts < 0 || n_elts > kHoistMaxElts)
            return c;
        const std::size_t ne = static_cast<std::size_t>(n_elts);
        if (hoist_has_instance(logn, nd))
        {
            c.family = kMacItems;
            c.nd = nd;
            c.group = mac_item_group(logn, nd, rows, ne, count);
            c.n_groups = mac_ceil_div(count, c.group);
            c.blocks = blocks_for((c.n_groups * rows * ne) << logn);
            return c;
        }
        c.family = kMacLoop;
        c.blocks = blocks_for((count * rows * ne) << logn);
        return c;
    }

    // the four slots of a lane: as many sums as the call has (1, 2 or 4), the rest ciphertexts
    constexpr MacChoice select_hoist_dot_mac(int logn, int nd, std::size_t rows, int n_elts, std::size_t count, std::size_t n_sums)
    {
        MacChoice c{};
        if (n_elts < 0 || n_elts > kHoistMaxElts || n_sums < 1)
            return c;
        if (hoist_has_instance(logn, nd))
        {
            const std::size_t S = n_sums >= 3 ? 4 : n_sums;
            c.family = kMacItems;
            c.nd = nd;
            c.slots = static_cast<int>(S);
            c.n_groups = mac_ceil_div(n_sums, S) * mac_ceil_div(count, 4 / S);
            c.blocks = blocks_for((c.n_groups * rows) << logn);
            return c;
        }
        c.family = kMacLoop;
        c.blocks = blocks_for((n_sums * count * rows) << logn);
        return c;
    }

    // four ciphertexts per lane
    constexpr MacChoice select_hoist_giant_mac(int logn, int nd, std::size_t rows, int n_elts, std::size_t count)
    {
        MacChoice c{};
        if (n_elts < 0 || n_elts > kHoistMaxElts)
            return c;
        if (hoist_has_instance(logn, nd))
        {
            c.family = kMacItems;
            c.nd = nd;
            c.n_groups = mac_ceil_div(count, 4);
            c.blocks = blocks_for((c.n_groups * rows) << logn);
            return c;
        }
        c.family = kMacLoop;
        c.blocks = blocks_for((count * rows) << logn);
        return c;
    }
} // namespace sealhip
