// dotacc_split_check.cpp -- csrc/dotacc.hpp with the split position as a parameter (DotAccSplit<S, ...>, S = 30 and 31)
// executed on the host: the very header the kernels include, compiled as plain 64-bit arithmetic.
//   g++ -std=c++17 -O2 -I gemini-seal_amd/csrc tests/dotacc_split_check.cpp -o dotacc_split_check && ./dotacc_split_check
// Shapes: every dot product of every exact-k BEHZ instance (bounds::behz_built_shape: four kinds, k = 1..15, term counts
// 2..17) at both splits, and the one-term shapes. Operands: the maxima of each operand class (all-ones of the class width;
// the floor rows' non-canonical input x at 2p - 1 for the largest 60-bit prime p), zero, alternating, seeded random within
// the class widths. Every 64-bit accumulator is shadowed in 128 bits and must stay below 2^64 (and equal its shadow); the
// assembled (lo, hi) must equal the sum of the 128-bit products; the accumulator counts must be the ones the bounds
// function derives. Then the predicate at its edge: the widest primes it admits run without a wrap, the narrowest it
// refuses do wrap an accumulator of the S = 30 instance, and S = 31 is selected for them.
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
static u64 rnd64() // xorshift64*
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static u64 ones(int bits)
{
    return (1ull << bits) - 1;
}

constexpr u128 kWord = static_cast<u128>(1) << 64;
constexpr u64 kP60 = (1ull << 60) - 93; // the largest prime below 2^60
constexpr int kPatterns = 5 + 48;

// widths (first, lane, constant) the operands are drawn from -- the accumulator's own shape unless a case says otherwise
struct Widths
{
    int first, lane, cst;
};

// 0: all-ones of each class; 1: all 0; 2: t alternating top / 0, c top; 3: t top, c alternating 0 / top;
// 4: as 0 with term 0 at 2 p - 1 where its class has 61 bits; 5..: random within the widths
static void operands(int pattern, int n, const Widths &w, u64 *t, u64 *c)
{
    for (int i = 0; i < n; i++)
    {
        const u64 tt = ones(i == 0 ? w.first : w.lane), ct = ones(w.cst);
        switch (pattern)
        {
        case 0: t[i] = tt, c[i] = ct; break;
        case 1: t[i] = 0, c[i] = 0; break;
        case 2: t[i] = (i & 1) ? 0 : tt, c[i] = ct; break;
        case 3: t[i] = tt, c[i] = (i & 1) ? ct : 0; break;
        case 4: t[i] = (i == 0 && w.first == 61) ? 2 * kP60 - 1 : tt, c[i] = (w.cst == 60) ? kP60 - 1 : ct; break;
        default: t[i] = rnd64() & tt, c[i] = rnd64() & ct; break;
        }
    }
}

template <class Acc, int S>
struct Shadow // the same dealing of products as DotAccSplit::add, in 128 bits
{
    u128 l[Acc::NL] = {}, m[Acc::NM] = {}, h[Acc::NH] = {};
    void add(int idx, u64 t, u64 c)
    {
        const u64 mask = (1ull << S) - 1, t0 = t & mask, t1 = t >> S, c0 = c & mask, c1 = c >> S;
        l[idx % Acc::NL] += static_cast<u128>(t0) * c0;
        m[(2 * idx) % Acc::NM] += static_cast<u128>(t0) * c1;
        m[(2 * idx + 1) % Acc::NM] += static_cast<u128>(t1) * c0;
        h[idx % Acc::NH] += static_cast<u128>(t1) * c1;
    }
    bool wrapped() const
    {
        bool w = false;
        for (int i = 0; i < Acc::NL; i++)
            w = w || l[i] >= kWord;
        for (int i = 0; i < Acc::NM; i++)
            w = w || m[i] >= kWord;
        for (int i = 0; i < Acc::NH; i++)
            w = w || h[i] >= kWord;
        return w;
    }
};

template <class Acc, int S, int N, int I = 0>
static void add_all(Acc &acc, const u64 *t, const u64 *c)
{
    if constexpr (I < N)
    {
        acc.template add<I>(Split<S>(t[I]), dot_pack<S>(c[I]));
        add_all<Acc, S, N, I + 1>(acc, t, c);
    }
}

static long shapes_run = 0;

// one accumulator type on operands of widths w; returns whether any pattern wrapped an accumulator
template <class Acc, int S>
static bool run_shape(const Widths &w, bool expect_fit, const char *what)
{
    constexpr int N = Acc::kShape.nterms;
    bool any_wrap = false;
    for (int pattern = 0; pattern < kPatterns; pattern++)
    {
        u64 t[N], c[N];
        operands(pattern, N, w, t, c);
        Acc acc;
        Shadow<Acc, S> sh;
        u128 exact = 0;
        add_all<Acc, S, N>(acc, t, c);
        for (int i = 0; i < N; i++)
        {
            sh.add(i, t[i], c[i]);
            exact += static_cast<u128>(t[i]) * c[i];
        }
        any_wrap = any_wrap || sh.wrapped();
        if (!expect_fit)
            continue;
        for (int i = 0; i < Acc::NL; i++)
            CHECK(sh.l[i] < kWord && acc.l[i] == static_cast<u64>(sh.l[i]), "%s S=%d N=%d pattern %d: low accumulator %d", what, S, N, pattern, i);
        for (int i = 0; i < Acc::NM; i++)
            CHECK(sh.m[i] < kWord && acc.m[i] == static_cast<u64>(sh.m[i]), "%s S=%d N=%d pattern %d: cross accumulator %d", what, S, N, pattern, i);
        for (int i = 0; i < Acc::NH; i++)
            CHECK(sh.h[i] < kWord && acc.h[i] == static_cast<u64>(sh.h[i]), "%s S=%d N=%d pattern %d: high accumulator %d", what, S, N, pattern, i);
        u64 lo, hi;
        acc.finish(lo, hi);
        CHECK(lo == static_cast<u64>(exact) && hi == static_cast<u64>(exact >> 64), "%s S=%d N=%d pattern %d: assembled sum", what, S, N, pattern);
    }
    shapes_run++;
    return any_wrap;
}

template <class Acc, int S>
static void run_own_shape(const char *what)
{
    constexpr bounds::DotShape d = Acc::kShape;
    // the counts are the fewest that fit: derived, admitted, and one fewer of any part is refused
    static_assert(bounds::dotsplit_ok(S, d, Acc::NL, Acc::NM, Acc::NH), "admitted");
    CHECK(Acc::NL == bounds::dotsplit_count(S, d, 0) && Acc::NM == bounds::dotsplit_count(S, d, 1) && Acc::NH == bounds::dotsplit_count(S, d, 2),
          "%s S=%d N=%d: accumulator counts", what, S, d.nterms);
    CHECK(!bounds::dotsplit_ok(S, d, Acc::NL - 1, Acc::NM, Acc::NH) && !bounds::dotsplit_ok(S, d, Acc::NL, Acc::NM - 1, Acc::NH) &&
              !bounds::dotsplit_ok(S, d, Acc::NL, Acc::NM, Acc::NH - 1),
          "%s S=%d N=%d: a smaller count admitted", what, S, d.nterms);
    run_shape<Acc, S>(Widths{ d.first_bits, d.lane_bits, d.const_bits }, true, what);
}

template <int S, int K>
static void run_level()
{
    run_own_shape<BehzDot<S, 0, K>, S>("lift row");
    run_own_shape<BehzDot<S, 1, K>, S>("floor Bsk row");
    run_own_shape<BehzDot<S, 2, K>, S>("conv_sk");
    run_own_shape<BehzDot<S, 3, K>, S>("floor q row");
    if constexpr (K > 1)
        run_level<S, K - 1>();
}

// term counts 1..17 with every operand at the widest the split's instances meet
template <int S, int N>
static void run_terms()
{
    if constexpr (S == 30)
    {
        run_own_shape<DotAccSplit<30, N, 61, 60, 60>, 30>("61/60/60");
        run_own_shape<DotAccSplit<30, N, 60, 60, 60>, 30>("60/60/60");
        run_own_shape<DotAccSplit<30, N, 61, 58, 60>, 30>("61/58/60");
    }
    else
        run_own_shape<DotAccSplit<31, N, 61, 61, 61>, 31>("61/61/61");
    if constexpr (N > 1)
        run_terms<S, N - 1>();
}

// the edge of the level predicate at k = K with 60-bit auxiliary primes: QB_OK-bit ciphertext primes are the widest
// admitted at S = 30 (they run in the S = 30 instance's accumulators without a wrap), QB_OK + 1 bits are refused, do
// wrap an accumulator of that instance on all-ones operands, and get S = 31, whose instance takes them
template <int K, int QB_OK>
static void run_edge()
{
    const u64 b = ones(60), q_ok = ones(QB_OK), q_no = ones(QB_OK + 1);
    CHECK(bounds::behz_split_admits(30, K, q_ok, b) && bounds::behz_select_split(K, q_ok, b) == 30, "k=%d: %d-bit primes refused", K, QB_OK);
    CHECK(!bounds::behz_split_admits(30, K, q_no, b) && bounds::behz_select_split(K, q_no, b) == 31, "k=%d: %d-bit primes admitted", K, QB_OK + 1);
    CHECK(bounds::behz_split_admits(31, K, q_no, b), "k=%d: S = 31 refuses %d-bit primes", K, QB_OK + 1);
    bool wrap_ok = false, wrap_no = false;
    const Widths ok[4] = { { 60, QB_OK, 60 }, { 61, QB_OK, 60 }, { 60, 60, 60 }, { 60, 60, QB_OK } };
    const Widths no[4] = { { 60, QB_OK + 1, 60 }, { 61, QB_OK + 1, 60 }, { 60, 60, 60 }, { 60, 60, QB_OK + 1 } };
    wrap_ok = run_shape<BehzDot<30, 0, K>, 30>(ok[0], true, "edge lift row") || wrap_ok;
    wrap_ok = run_shape<BehzDot<30, 1, K>, 30>(ok[1], true, "edge floor Bsk row") || wrap_ok;
    wrap_ok = run_shape<BehzDot<30, 2, K>, 30>(ok[2], true, "edge conv_sk") || wrap_ok;
    wrap_ok = run_shape<BehzDot<30, 3, K>, 30>(ok[3], true, "edge floor q row") || wrap_ok;
    wrap_no = run_shape<BehzDot<30, 0, K>, 30>(no[0], false, "") || wrap_no;
    wrap_no = run_shape<BehzDot<30, 1, K>, 30>(no[1], false, "") || wrap_no;
    wrap_no = run_shape<BehzDot<30, 2, K>, 30>(no[2], false, "") || wrap_no;
    wrap_no = run_shape<BehzDot<30, 3, K>, 30>(no[3], false, "") || wrap_no;
    CHECK(!wrap_ok, "k=%d: an accumulator wraps at the admitted width", K);
    CHECK(wrap_no, "k=%d: the predicate is not tight, nothing wraps at %d bits", K, QB_OK + 1);
    run_shape<BehzDot<31, 0, K>, 31>(no[0], true, "S = 31 lift row");
    run_shape<BehzDot<31, 1, K>, 31>(no[1], true, "S = 31 floor Bsk row");
    run_shape<BehzDot<31, 2, K>, 31>(no[2], true, "S = 31 conv_sk");
    run_shape<BehzDot<31, 3, K>, 31>(no[3], true, "S = 31 floor q row");
}

template <int S>
static void pack_round_trip()
{
    const int top = S == 30 ? 62 : 61; // the widest operand either half of which is a 32-bit word: S + 32
    const u64 edge[] = { 0, 1, ones(S), 1ull << S, 0xFFFFFFFFull, 1ull << 32, ones(60), ones(61), 2 * kP60 - 1, kP60 - 1, ones(top) };
    const int nedge = static_cast<int>(sizeof edge / sizeof edge[0]);
    for (int i = 0; i < 4096 + nedge; i++)
    {
        const u64 c = i < nedge ? edge[i] : rnd64() & ones(61);
        const u64 pk = dot_pack<S>(c);
        const Split<S> s(c);
        CHECK(dot_unpack<S>(pk) == c && dot_pack(S, c) == pk, "S=%d: round trip of %llx", S, c);
        CHECK((pk & 0xFFFFFFFFull) < (1ull << S), "S=%d: low half of %llx", S, c);
        CHECK(s.t0 == static_cast<unsigned>(pk) && s.t1 == static_cast<unsigned>(pk >> 32), "S=%d: Split of %llx", S, c);
    }
}

int main()
{
    run_level<30, 15>();
    run_level<31, 15>();
    run_terms<30, 17>();
    run_terms<31, 17>();
    // the one-accumulator cases the split at 30 is for, and what refuses them
    CHECK(bounds::dotsplit_ok(30, bounds::DotShape{ 8, 60, 60, 60 }, 1, 1, 1), "8 terms of 60-bit operands: one accumulator per part");
    CHECK(!bounds::dotsplit_ok(30, bounds::DotShape{ 9, 60, 60, 60 }, 1, 1, 1), "9 terms: 18 cross products in one accumulator");
    CHECK(!bounds::dotsplit_ok(30, bounds::DotShape{ 8, 61, 60, 60 }, 1, 1, 1), "8 terms with a 61-bit first factor");
    CHECK(bounds::dotsplit_ok(30, bounds::DotShape{ 8, 61, 58, 60 }, 1, 1, 1), "the floor rows at k = 7: x below 2^61, 58-bit t");
    CHECK(!bounds::dotsplit_ok(30, bounds::DotShape{ 17, 60, 60, 58 }, 1, 2, 1), "17 low products of 2^60");
    CHECK(!bounds::dotsplit_ok(31, bounds::DotShape{ 8, 62, 62, 62 }, 2, 2, 1), "S = 31 at 62 bits");
    CHECK(!bounds::dotsplit_ok(30, bounds::DotShape{ 2, 63, 60, 60 }, 2, 2, 2), "a high half above 32 bits");
    // (k = 1: three or four products of 2^60 per accumulator -- every prime the context admits takes S = 30)
    CHECK(bounds::behz_select_split(1, ones(60), ones(60)) == 30, "k = 1 with 60-bit primes");
    run_edge<7, 59>();
    run_edge<8, 59>();
    run_edge<15, 59>();
    // levels above the exact-k instances keep 31 (they never read the packed tables)
    CHECK(bounds::behz_select_split(16, ones(40), ones(60)) == 31, "k = 16");
    pack_round_trip<30>();
    pack_round_trip<31>();
    if (failures)
    {
        std::printf("dotacc_split_check: %d failures\n", failures);
        return 1;
    }
    std::printf("dotacc_split_check: OK (%ld shapes)\n", shapes_run);
    return 0;
}
