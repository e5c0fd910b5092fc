// lincomb_bounds_check.cpp -- CPU test of ntt_bounds.hpp's lincomb_group_admits (built and run by tests/test_poly_eval_host.py).
// lincomb_kernel (gemini-seal_amd/csrc/poly.hip) sums a group of products weight * word in plain 128-bit integers, adds the
// canonical partial sum of the groups before and the constant, and reduces once per output word;
// bounds::lincomb_group_admits(terms, bits) says when that sum cannot wrap.
// 1. The predicate against exact arithmetic: for operand sizes 20..63 bits and 1..80 terms the worst sum -- every operand and
//    weight 2^bits - 1, the partial and the constant 2^bits - 1 -- is formed in 256 bits; admitted => it is below 2^128; and the
//    predicate is tight to within one term (it bounds a product by 2^(2 bits), not by (2^bits - 1)^2).
// 2. The kernel's accumulation executed word for word (mac128, the carries of the partial sum and of the constant,
//    barrett_reduce_128 as uintarithsmallmod.h:140-178 has it) on worst-case and random operands of 61-bit, 60-bit and small
//    primes, groups of 1, 2, 15 and 16 terms chained over several groups, zero weights included: equal to the composition's
//    canonical residue (products reduced one by one and added modulo p, the constant added last).
#include <cstdint>
#include <cstdio>
#include <random>

#include "../gemini-seal_amd/csrc/ntt_bounds.hpp"

using namespace sealhip::bounds;
// (u64 and u128 are the header's)

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

// 256-bit unsigned: just enough to add 128-bit products without wrapping
struct U256
{
    u128 lo = 0, hi = 0;
    void add(u128 x)
    {
        const u128 n = lo + x;
        hi += n < lo;
        lo = n;
    }
};

static u64 mulhi(u64 a, u64 b)
{
    return static_cast<u64>((static_cast<u128>(a) * b) >> 64);
}
// the kernel's primitives, as devmath.hpp and poly.hip write them
static void mac128(u64 &lo, u64 &hi, u64 a, u64 b)
{
    const u64 pl = a * b, ph = mulhi(a, b);
    const u64 nl = lo + pl;
    hi += ph + (nl < lo);
    lo = nl;
}
static void add_word(u64 &lo, u64 &hi, u64 w)
{
    const u64 nl = lo + w;
    hi += nl < lo;
    lo = nl;
}
static u64 barrett_reduce_128(u64 lo, u64 hi, u64 p, u64 cr0, u64 cr1)
{
    const u64 carry = mulhi(lo, cr0);
    const u64 t_lo = lo * cr1, t_hi = mulhi(lo, cr1);
    const u64 tmp1 = t_lo + carry;
    const u64 tmp3 = t_hi + (tmp1 < t_lo);
    const u64 u_lo = hi * cr0, u_hi = mulhi(hi, cr0);
    const u64 tmp1b = tmp1 + u_lo;
    const u64 carry2 = u_hi + (tmp1b < tmp1);
    const u64 q = hi * cr1 + tmp3 + carry2;
    const u64 r = lo - q * p;
    return r >= p ? r - p : r;
}
static void const_ratio(u64 p, u64 &cr0, u64 &cr1)
{
    const u128 top = (~static_cast<u128>(0)) / p; // floor((2^128 - 1) / p) == floor(2^128 / p) unless p divides 2^128
    cr0 = static_cast<u64>(top);
    cr1 = static_cast<u64>(top >> 64);
}
static u64 mulmod(u64 a, u64 b, u64 p)
{
    return static_cast<u64>(static_cast<u128>(a) * b % p);
}

static void check_predicate()
{
    for (int bits = 20; bits <= 63; bits++)
        for (int terms = 1; terms <= 80; terms++)
        {
            const u128 x = (static_cast<u128>(1) << bits) - 1;
            U256 sum;
            for (int t = 0; t < terms; t++)
                sum.add(x * x);
            sum.add(x); // the partial sum
            sum.add(x); // the constant
            const bool fits = sum.hi == 0;
            if (lincomb_group_admits(terms, bits))
                CHECK(fits, "admitted but the sum wraps: %d terms of %d bits", terms, bits);
            else
            {
                U256 more = sum;
                more.add(x * x);
                CHECK(more.hi != 0, "rejected with more than a term of slack: %d terms of %d bits", terms, bits);
            }
        }
    CHECK(lincomb_group_admits(kLinGroupTerms, kDotAccOperandBits), "the group of the kernel at 61 bits");
    CHECK(!lincomb_group_admits(0, 61) && !lincomb_group_admits(1, 64) && !lincomb_group_admits(1, 0), "degenerate arguments");
    CHECK(kLinGroupTerms == 16 && kLinTileSums >= 1 && kLinTileSums <= 8, "the kernel's group and tile");
}

static void check_execution()
{
    std::mt19937_64 rng(20);
    const u64 primes[] = { (u64(1) << 61) - 1,          // 2^61 - 1 (Mersenne prime): the largest operand size
                           (u64(1) << 60) - (u64(1) << 14) + 1, 1152921504606830593ull, 786433ull, 1099511603201ull,
                           3ull }; // (moduli: primality plays no part in the arithmetic checked here)
    const int group_sizes[] = { 1, 2, 15, 16 };
    for (u64 p : primes)
    {
        u64 cr0, cr1;
        const_ratio(p, cr0, cr1);
        for (int worst = 0; worst < 2; worst++)
            for (int gs : group_sizes)
            {
                // three groups chained through the canonical partial sum, the constant added by the last one
                u64 part = 0, want = 0;
                const u64 kc = worst ? p - 1 : rng() % p;
                for (int g = 0; g < 3; g++)
                {
                    u64 lo = 0, hi = 0;
                    for (int t = 0; t < gs; t++)
                    {
                        const u64 x = worst ? p - 1 : rng() % p;
                        const u64 w = worst ? p - 1 : (t % 5 == 4 ? 0 : rng() % p); // (a weight of zero now and then)
                        mac128(lo, hi, x, w);
                        want = (want + mulmod(x, w, p)) % p;
                    }
                    if (g > 0)
                        add_word(lo, hi, part);
                    if (g == 2)
                    {
                        add_word(lo, hi, kc);
                        want = (want + kc) % p;
                    }
                    part = barrett_reduce_128(lo, hi, p, cr0, cr1);
                    CHECK(part == want, "p = %llu, group of %d, group %d: %llu != %llu", (unsigned long long)p, gs, g,
                          (unsigned long long)part, (unsigned long long)want);
                }
            }
    }
}

int main()
{
    check_predicate();
    check_execution();
    if (failures)
    {
        std::printf("lincomb_bounds_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("lincomb_bounds_check: OK\n");
    return 0;
}
