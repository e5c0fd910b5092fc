// dot_plain_bounds_check.cpp -- CPU test that ntt_bounds.hpp's lincomb_group_admits covers dot_plain_kernel (built and run
// by tests/test_expand_host.py). dot_plain_kernel (gemini-seal_amd/csrc/poly.hip) sums a group of products
// ciphertext word * plaintext word in plain 128-bit integers, adds the canonical partial sum of the groups before, and
// reduces once per output word: lincomb_kernel's sum without the constant.
// 1. The predicate against exact arithmetic: for operand sizes 20..63 bits and 1..80 terms the worst sum of this kernel --
//    every word 2^bits - 1, the partial sum 2^bits - 1 -- is formed in 256 bits; admitted => it is below 2^128.
// 2. The kernel's accumulation executed word for word (mac128, the carry of the partial sum, barrett_reduce_128) on
//    worst-case (every word p - 1) and random words of 61-bit, 60-bit and small primes, for 1, 16, 17 and 33 terms in
//    groups of kLinGroupTerms: equal to the composition's canonical residue (products reduced one by one and added
//    modulo p, left to right).
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
    const u128 top = (~static_cast<u128>(0)) / p;
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
            if (!lincomb_group_admits(terms, bits))
                continue;
            const u128 x = (static_cast<u128>(1) << bits) - 1;
            U256 sum;
            for (int t = 0; t < terms; t++)
                sum.add(x * x);
            sum.add(x); // the partial sum (the kernel has no constant: one word fewer than the predicate allows for)
            CHECK(sum.hi == 0, "admitted but the sum wraps: %d terms of %d bits", terms, bits);
        }
    CHECK(lincomb_group_admits(kLinGroupTerms, kDotAccOperandBits), "the group of the kernel at 61 bits");
}

static void check_execution()
{
    std::mt19937_64 rng(28);
    const u64 primes[] = { (u64(1) << 61) - 1, (u64(1) << 60) - (u64(1) << 14) + 1, 1152921504606830593ull, 786433ull,
                           1099511603201ull, 3ull }; // (moduli: primality plays no part in the arithmetic checked here)
    const int term_counts[] = { 1, 16, 17, 33 };
    for (u64 p : primes)
    {
        u64 cr0, cr1;
        const_ratio(p, cr0, cr1);
        for (int worst = 0; worst < 2; worst++)
            for (int n_terms : term_counts)
            {
                u64 part = 0, want = 0;
                for (int g0 = 0; g0 < n_terms; g0 += kLinGroupTerms)
                {
                    u64 lo = 0, hi = 0;
                    for (int t = g0; t < n_terms && t < g0 + kLinGroupTerms; t++)
                    {
                        const u64 x = worst ? p - 1 : rng() % p;
                        const u64 w = worst ? p - 1 : (t % 5 == 4 ? 0 : rng() % p); // (a plaintext word of zero now and then)
                        mac128(lo, hi, x, w);
                        want = (want + mulmod(x, w, p)) % p;
                    }
                    if (g0 > 0)
                        add_word(lo, hi, part);
                    part = barrett_reduce_128(lo, hi, p, cr0, cr1);
                    CHECK(part == want, "p = %llu, %d terms, group at %d: %llu != %llu", (unsigned long long)p, n_terms, g0,
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
        std::printf("dot_plain_bounds_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("dot_plain_bounds_check: OK\n");
    return 0;
}
