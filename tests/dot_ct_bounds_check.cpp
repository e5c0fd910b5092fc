// dot_ct_bounds_check.cpp -- CPU test of ntt_bounds.hpp section 8 (built and run by tests/test_dot_ct_host.py).
// tensor_dot_kernel (gemini-seal_amd/csrc/poly.hip) sums the tensor products of a group of terms in plain 128-bit integers
// and reduces once per output word; bounds::dot_group_admits(terms, bits) says when the widest sum (c_1: two products per
// term plus the canonical partial sum of the groups before) cannot wrap.
// 1. The predicate against exact arithmetic: for operand sizes 20..63 bits and 1..64 terms the worst sum -- every operand
//    2^bits - 1, the partial 2^bits - 1 -- is formed in 256 bits; admitted => it is below 2^128; and the predicate is tight to
//    within one term (it bounds a product by 2^(2 bits), not by (2^bits - 1)^2).
// 2. The kernel's accumulation executed word for word (mac128, the carry of the partial sum, barrett_reduce_128 as
//    uintarithsmallmod.h:140-178 has it) on worst-case and random operands of 61-bit, 60-bit and small primes, groups of 1,
//    2, 15 and 16 terms chained over several groups: equal to the composition's canonical residue (products reduced one by
//    one and added modulo p).
// 3. The reduction on load: x - floor(x floor(2^64 / p) / 2^64) p lands in [0, 2p) for every 64-bit word, so one conditional
//    subtraction gives the canonical residue (the operand range the BFV launches rely on: any 64-bit word).
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
// the kernel's primitives, as devmath.hpp writes them
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
    // floor(2^128 / p) as two words
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
        for (int terms = 1; terms <= 64; terms++)
        {
            const u128 x = (static_cast<u128>(1) << bits) - 1;
            U256 sum;
            for (int t = 0; t < 2 * terms; t++)
                sum.add(x * x);
            sum.add(x);
            const bool fits = sum.hi == 0;
            if (dot_group_admits(terms, bits))
                CHECK(fits, "admitted but the sum wraps: %d terms of %d bits", terms, bits);
            else
            {
                // tight to one term: one term more certainly wraps
                U256 more = sum;
                more.add(x * x);
                more.add(x * x);
                CHECK(more.hi != 0, "rejected with more than a term of slack: %d terms of %d bits", terms, bits);
            }
        }
    CHECK(dot_group_admits(kDotGroupTerms, kDotAccOperandBits), "the group of the kernel at 61 bits");
    CHECK(!dot_group_admits(0, 61) && !dot_group_admits(1, 64) && !dot_group_admits(1, 0), "degenerate arguments");
}

static void check_execution()
{
    std::mt19937_64 rng(18);
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
                // three groups chained through the canonical partial sum, as op_dot_product chains its launches
                u64 part[3] = { 0, 0, 0 }, want[3] = { 0, 0, 0 };
                for (int g = 0; g < 3; g++)
                {
                    u64 lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
                    for (int t = 0; t < gs; t++)
                    {
                        u64 a0 = worst ? p - 1 : rng() % p, a1 = worst ? p - 1 : rng() % p;
                        u64 b0 = worst ? p - 1 : rng() % p, b1 = worst ? p - 1 : rng() % p;
                        mac128(lo[0], hi[0], a0, b0);
                        mac128(lo[1], hi[1], a1, b0);
                        mac128(lo[1], hi[1], a0, b1);
                        mac128(lo[2], hi[2], a1, b1);
                        want[0] = (want[0] + mulmod(a0, b0, p)) % p;
                        want[1] = (want[1] + mulmod(a1, b0, p)) % p;
                        want[1] = (want[1] + mulmod(a0, b1, p)) % p;
                        want[2] = (want[2] + mulmod(a1, b1, p)) % p;
                    }
                    for (int c = 0; c < 3; c++)
                    {
                        if (g > 0)
                            add_word(lo[c], hi[c], part[c]);
                        part[c] = barrett_reduce_128(lo[c], hi[c], p, cr0, cr1);
                        CHECK(part[c] == want[c], "p = %llu, group of %d, group %d, c_%d: %llu != %llu", (unsigned long long)p, gs,
                              g, c, (unsigned long long)part[c], (unsigned long long)want[c]);
                    }
                }
            }
    }
}

static void check_reduce_on_load()
{
    std::mt19937_64 rng(81);
    const u64 primes[] = { (u64(1) << 61) - 1, (u64(1) << 60) - (u64(1) << 14) + 1, 786433ull, 3ull };
    for (u64 p : primes)
    {
        const u64 rdp = static_cast<u64>((static_cast<u128>(1) << 64) / p); // floor(2^64 / p) = the high word of const_ratio
        u64 cr0, cr1;
        const_ratio(p, cr0, cr1);
        CHECK(cr1 == rdp, "const_ratio[1] is floor(2^64 / p) for p = %llu", (unsigned long long)p);
        for (int i = 0; i < 200000; i++)
        {
            u64 x = rng();
            if (i < 64)
                x = ~u64(0) - static_cast<u64>(i);
            else if (i < 128)
                x = (~u64(0) / p) * p - static_cast<u64>(i - 96); // around the largest multiple of p
            u64 r = x - mulhi(x, rdp) * p;
            CHECK(r < 2 * p || 2 * p < p, "lazy reduction of %llu mod %llu gives %llu", (unsigned long long)x, (unsigned long long)p,
                  (unsigned long long)r);
            r = r >= p ? r - p : r;
            CHECK(r == x % p, "canonical reduction of %llu mod %llu", (unsigned long long)x, (unsigned long long)p);
        }
    }
}

int main()
{
    check_predicate();
    check_execution();
    check_reduce_on_load();
    if (failures)
    {
        std::printf("dot_ct_bounds_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("dot_ct_bounds_check: OK\n");
    return 0;
}
