// homdft_plan_check.cpp -- gemini-seal_amd/csrc/homdft_plan.hpp (the planner of sealhip_evaluator_coeffs_to_slots /
// _slots_to_coeffs) executed on the host as a program of its own: the very header api.cpp includes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/homdft_plan_check.cpp -o homdft_plan_check
// (built and run by tests/test_homdft_host.py). For log2 N = 2 .. 16, both directions, every split of L into up to three
// stages and every legal n_baby of the first stage: the layers of the stages tile 1 .. L in the direction's order; levels and
// scales follow the primes; every rotation (giant + baby) mod n of a stage is c h0 mod n for exactly the c of its cell, every
// c of (-2^r, 2^r) (or [0, 2^r) when folded) occurs once and the one extra cell is c = -2^r; the key list is the sorted set of
// the non-zero steps. Then the refusals. What the sanitizers watch: every index into the primes and the step lists.
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "homdft_plan.hpp"

using namespace sealhip::dftplan;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do                                         \
    {                                          \
        if (!(cond))                           \
        {                                      \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            failures++;                        \
        }                                      \
    } while (0)

static void splits(std::uint32_t left, std::size_t max_parts, std::vector<std::uint32_t> &cur,
                   std::vector<std::vector<std::uint32_t>> &out)
{
    if (left == 0)
    {
        out.push_back(cur);
        return;
    }
    if (cur.size() == max_parts)
        return;
    for (std::uint32_t first = 1; first <= left; first++)
    {
        cur.push_back(first);
        splits(left - first, max_parts, cur, out);
        cur.pop_back();
    }
}

static void check_plan(const Ring &ring, std::uint32_t direction, std::uint32_t k, const std::vector<std::uint32_t> &counts,
                       const std::vector<std::uint32_t> *n_baby)
{
    const Plan p = make_plan(ring, direction, k, counts.data(), static_cast<std::uint32_t>(counts.size()),
                             n_baby ? n_baby->data() : nullptr);
    const std::uint32_t L = ring.logn - 1, n = 1u << L;
    CHECK(p.stages.size() == counts.size() && p.in_level == k && p.out_level == k - counts.size(), "levels");
    CHECK(p.needs_conjugation == (direction == kCoeffsToSlots), "conjugation");
    std::uint32_t next = direction == kSlotsToCoeffs ? 1 : L;
    std::set<std::uint32_t> steps;
    u64 words = 0;
    for (std::size_t t = 0; t < p.stages.size(); t++)
    {
        const Stage &s = p.stages[t];
        CHECK(s.r == counts[t] && s.h0 == (1u << (s.s0 - 1)), "stage shape");
        if (direction == kSlotsToCoeffs)
        {
            CHECK(s.s0 == next, "SlotToCoeff starts at the bottom");
            next = s.s0 + s.r;
        }
        else
        {
            CHECK(s.s0 + s.r - 1 == next, "CoeffToSlot starts at the top");
            next = s.s0 - 1;
        }
        CHECK(s.level == k - t && s.scale == static_cast<double>(ring.key_moduli[s.level - 1]), "level and scale");
        CHECK(s.folded == (s.s0 + s.r - 1 == L), "folded");
        CHECK(s.baby.size() == s.n_baby && s.giant.size() == s.n_giant, "step lists");
        CHECK(s.cells() == (s.folded ? 1u << s.r : 2u << s.r), "cells");
        std::set<long long> seen;
        for (std::uint32_t g = 0; g < s.n_giant; g++)
            for (std::uint32_t b = 0; b < s.n_baby; b++)
            {
                const long long c = s.giant_coeff(g) * static_cast<long long>(s.n_baby) + b;
                const std::uint32_t rotation = static_cast<std::uint32_t>(s.giant[g] + s.baby[b]) & (n - 1);
                CHECK(rotation == (static_cast<std::uint32_t>(c * static_cast<long long>(s.h0)) & (n - 1)), "rotation of a cell");
                CHECK(s.giant[g] >= 0 && s.giant[g] < static_cast<std::int32_t>(n) && s.baby[b] >= 0 &&
                          s.baby[b] < static_cast<std::int32_t>(n),
                      "steps in [0, n)");
                CHECK(seen.insert(c).second, "a diagonal twice");
                if (s.giant[g])
                    steps.insert(static_cast<std::uint32_t>(s.giant[g]));
                if (s.baby[b])
                    steps.insert(static_cast<std::uint32_t>(s.baby[b]));
            }
        const long long lo = s.folded ? 0 : -(1ll << s.r), hi = (1ll << s.r) - 1;
        CHECK(*seen.begin() == lo && *seen.rbegin() == hi && seen.size() == static_cast<std::size_t>(hi - lo + 1), "diagonal set");
        words += static_cast<u64>(s.cells()) * ring.n_key << ring.logn;
    }
    CHECK(next == (direction == kSlotsToCoeffs ? L + 1 : 0), "the layers tile 1 .. L");
    CHECK(p.table_words == words, "table words");
    CHECK(p.temp_bytes_per_item > 0, "temporaries");
    CHECK(std::vector<std::uint32_t>(steps.begin(), steps.end()) == p.key_steps, "key steps");
}

template <class F>
static bool refuses(F &&f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument &)
    {
        return true;
    }
    return false;
}

int main()
{
    std::vector<u64> primes;
    for (u64 i = 0; i < 8; i++)
        primes.push_back((1ull << 40) + 2 * i + 1); // (the plan only casts them to double)
    for (std::uint32_t logn = 2; logn <= 16; logn++)
    {
        Ring ring;
        ring.scheme = 2;
        ring.logn = logn;
        ring.n_key = 8;
        ring.k_first = 7;
        ring.key_moduli = primes.data();
        std::vector<std::vector<std::uint32_t>> all;
        std::vector<std::uint32_t> cur;
        splits(logn - 1, 3, cur, all);
        for (const auto &counts : all)
            for (std::uint32_t direction : { kCoeffsToSlots, kSlotsToCoeffs })
            {
                check_plan(ring, direction, 7, counts, nullptr);
                check_plan(ring, direction, static_cast<std::uint32_t>(counts.size()) + 1, counts, nullptr);
                for (std::uint32_t nb = 1; nb <= (1u << counts[0]); nb <<= 1)
                {
                    std::vector<std::uint32_t> n_baby(counts.size(), 0);
                    n_baby[0] = nb;
                    check_plan(ring, direction, 7, counts, &n_baby);
                }
            }
        // refusals
        const std::uint32_t L = logn - 1;
        std::vector<std::uint32_t> one{ L }, zero{ L, 0 }, more{ L, 1 }, bad_baby{ 3 }, big_baby{ 2u << L };
        CHECK(refuses([&] { make_plan(ring, 0, 7, more.data(), 2, nullptr); }), "a sum above L is accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 7, zero.data(), 2, nullptr); }), "a zero count is accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 7, one.data(), 0, nullptr); }), "no stages accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 1, one.data(), 1, nullptr); }), "one stage at level 1 accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 8, one.data(), 1, nullptr); }), "the key level accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 0, one.data(), 1, nullptr); }), "level 0 accepted");
        CHECK(refuses([&] { make_plan(ring, 2, 7, one.data(), 1, nullptr); }), "direction 2 accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 7, one.data(), 1, bad_baby.data()); }), "n_baby 3 accepted");
        CHECK(refuses([&] { make_plan(ring, 0, 7, one.data(), 1, big_baby.data()); }), "n_baby above 2^r accepted");
        if (L >= 2)
        {
            std::vector<std::uint32_t> less{ L - 1 };
            CHECK(refuses([&] { make_plan(ring, 1, 7, less.data(), 1, nullptr); }), "a sum below L is accepted");
            std::vector<std::uint32_t> ones(L, 1);
            if (L >= 7)
                CHECK(refuses([&] { make_plan(ring, 1, 7, ones.data(), L, nullptr); }), "more stages than levels accepted");
        }
        Ring bfv = ring;
        bfv.scheme = 1;
        CHECK(refuses([&] { make_plan(bfv, 0, 7, one.data(), 1, nullptr); }), "BFV accepted");
    }
    if (failures)
    {
        std::printf("homdft_plan_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("homdft_plan_check: OK\n");
    return 0;
}
