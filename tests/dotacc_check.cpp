// dotacc_check.cpp -- csrc/dotacc.hpp (DotAcc31, the carry-free dot product of the exact-k BEHZ instances) executed on the
// host: the very header the kernels include, compiled as plain 64-bit arithmetic.
//   g++ -std=c++17 -O2 -I gemini-seal_amd/csrc tests/dotacc_check.cpp -o dotacc_check && ./dotacc_check
// For every term count 1..17 (the kernels instantiate up to k + 2 = 17) and operands all 2^61 - 1, all 0, alternating
// and random: every 64-bit accumulator is shadowed in 128 bits and must stay below 2^64 (and equal its shadow), and the
// assembled (lo, hi) must equal the sum of the 128-bit products. The packed constant must round-trip.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "dotacc.hpp"

using namespace sealhip;
using u64 = unsigned long long;
using u128 = unsigned __int128;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do                                        \
    {                                         \
        if (!(cond))                          \
        {                                     \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                \
            failures++;                       \
        }                                     \
    } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd61() // xorshift64*, below 2^61
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (rng_state * 0x2545F4914F6CDD1Dull) >> 3;
}

constexpr u64 kTop = (1ull << 61) - 1;
constexpr u128 kWord = static_cast<u128>(1) << 64;

// 0: all 2^61 - 1; 1: all 0; 2: t alternating top / 0, c top; 3: t top, c alternating 0 / top; 4..: random
static void operands(int pattern, int n, u64 *t, u64 *c)
{
    for (int i = 0; i < n; i++)
    {
        switch (pattern)
        {
        case 0: t[i] = kTop, c[i] = kTop; break;
        case 1: t[i] = 0, c[i] = 0; break;
        case 2: t[i] = (i & 1) ? 0 : kTop, c[i] = kTop; break;
        case 3: t[i] = kTop, c[i] = (i & 1) ? kTop : 0; break;
        default: t[i] = rnd61(), c[i] = rnd61(); break;
        }
    }
}

template <int N>
struct Shadow // the same dealing of products as DotAcc31<N>::add, in 128 bits
{
    u128 l[DotAcc31<N>::NL] = {}, m[DotAcc31<N>::NM] = {}, h[DotAcc31<N>::NH] = {};
    void add(int idx, u64 t, u64 c)
    {
        const u64 t0 = t & 0x7FFFFFFFull, t1 = t >> 31, c0 = c & 0x7FFFFFFFull, c1 = c >> 31;
        l[idx % DotAcc31<N>::NL] += static_cast<u128>(t0) * c0;
        m[(2 * idx) % DotAcc31<N>::NM] += static_cast<u128>(t0) * c1;
        m[(2 * idx + 1) % DotAcc31<N>::NM] += static_cast<u128>(t1) * c0;
        h[idx % DotAcc31<N>::NH] += static_cast<u128>(t1) * c1;
    }
};

template <int N, int I = 0>
static void add_all(DotAcc31<N> &acc, const u64 *t, const u64 *c)
{
    if constexpr (I < N)
    {
        acc.template add<I>(Split31(t[I]), dot31_pack(c[I]));
        add_all<N, I + 1>(acc, t, c);
    }
}

template <int N>
static void run_terms()
{
    static_assert(bounds::dotacc31_ok(N, bounds::kDotAccOperandBits), "admitted");
    for (int pattern = 0; pattern < 4 + 64; pattern++)
    {
        u64 t[N], c[N];
        operands(pattern, N, t, c);
        DotAcc31<N> acc;
        Shadow<N> sh;
        u128 exact = 0;
        add_all<N>(acc, t, c);
        for (int i = 0; i < N; i++)
        {
            sh.add(i, t[i], c[i]);
            exact += static_cast<u128>(t[i]) * c[i];
        }
        for (int i = 0; i < DotAcc31<N>::NL; i++)
            CHECK(sh.l[i] < kWord && acc.l[i] == static_cast<u64>(sh.l[i]), "N=%d pattern %d: low accumulator %d", N, pattern, i);
        for (int i = 0; i < DotAcc31<N>::NM; i++)
            CHECK(sh.m[i] < kWord && acc.m[i] == static_cast<u64>(sh.m[i]), "N=%d pattern %d: cross accumulator %d", N, pattern, i);
        for (int i = 0; i < DotAcc31<N>::NH; i++)
            CHECK(sh.h[i] < kWord && acc.h[i] == static_cast<u64>(sh.h[i]), "N=%d pattern %d: high accumulator %d", N, pattern, i);
        u64 lo, hi;
        acc.finish(lo, hi);
        CHECK(lo == static_cast<u64>(exact) && hi == static_cast<u64>(exact >> 64), "N=%d pattern %d: assembled sum", N, pattern);
    }
}

template <int N>
static void run_all()
{
    run_terms<N>();
    if constexpr (N > 1)
        run_all<N - 1>();
}

int main()
{
    run_all<17>();
    // the accumulators' shares per term count are what the predicate counts
    for (int n = 1; n <= 17; n++)
    {
        const int nl = bounds::dotacc31_nl(n), nm = bounds::dotacc31_nm(n), nh = bounds::dotacc31_nh(n);
        CHECK((n + nl - 1) / nl <= 4 && (2 * n + nm - 1) / nm <= 8 && (n + nh - 1) / nh <= 16, "shares at %d terms", n);
    }
    // tight: one more operand bit and the cross accumulators (eight products each at 8 terms) no longer fit
    CHECK(bounds::dotacc31_ok(8, 61) && !bounds::dotacc31_ok(8, 62), "predicate not tight at 62 bits");
    // the packed constant: halves below 2^31 / 2^30, round trip, and the split of a lane's factor is the same split
    const u64 edge[] = { 0, 1, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 1ull << 32, kTop, kTop - 1, 1ull << 60 };
    for (int i = 0; i < 4096 + 9; i++)
    {
        const u64 c = i < 9 ? edge[i] : rnd61();
        const u64 pk = dot31_pack(c);
        const Split31 s(c);
        CHECK(dot31_unpack(pk) == c, "round trip of %llx", c);
        CHECK((pk & 0xFFFFFFFFull) < (1ull << 31) && (pk >> 32) < (1ull << 30), "halves of %llx", c);
        CHECK(s.t0 == static_cast<unsigned>(pk) && s.t1 == static_cast<unsigned>(pk >> 32), "Split31 of %llx", c);
    }
    if (failures)
    {
        std::printf("dotacc_check: %d failures\n", failures);
        return 1;
    }
    std::printf("dotacc_check: OK\n");
    return 0;
}
