// ext_mac_bounds_check.cpp -- CPU test that ntt_bounds.hpp's ext_mac_sum_fits covers the external product's inner product
// (built and run by tests/test_rgsw_host.py). ext_mac_kernel and ext_mac_items_kernel (gemini-seal_amd/csrc/rgsw.hip) sum
// 2 nd products digit word * key word in plain 128-bit integers and reduce once -- or, where the predicate refuses 2 nd
// terms, reduce after the first nd and carry that canonical residue into the second half.
// 1. The predicate against exact arithmetic: for prime sizes 20..61 bits, digit words of 58..64 bits and 1..40 terms the
//    worst sum -- every digit word 2^rep - 1, every key word p - 1, plus one carried residue p - 1 -- is formed in 256 bits;
//    admitted => it is below 2^128, and the first count not admitted really passes 2^128 - 1 (the predicate is tight).
// 2. The launcher's rule (one sum if 2 nd terms fit, else two halves, which must fit nd terms) over nd 1..8 and the largest
//    prime of every size: every level a context can have (nd p < 2^64) is served.
// 3. The kernels' accumulation executed word for word (mac128, barrett_reduce_128, the split) on worst-case words (digit
//    words 2^64 - 1, key words p - 1) and random ones, for 61-bit, 60-bit and small primes and nd 1..9: the unsplit sum,
//    where admitted, and the split sum give the composition's canonical residue (products reduced one by one and added
//    modulo p).
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
// the kernels' primitives, as devmath.hpp writes them
static void mac128(u64 &lo, u64 &hi, u64 a, u64 b)
{
    const u64 pl = a * b, ph = mulhi(a, b);
    const u64 nl = lo + pl;
    hi += ph + (nl < lo);
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

static U256 worst_sum(int terms, u64 p, int rep_bits)
{
    const u128 x = max_prime_of_bits(rep_bits), k = p - 1;
    U256 sum;
    for (int t = 0; t < terms; t++)
        sum.add(x * k);
    sum.add(k); // the carried residue of the split form
    return sum;
}

static void check_predicate()
{
    for (int bits = 20; bits <= 61; bits++)
        for (int rep = 58; rep <= 64; rep++)
        {
            const u64 p = max_prime_of_bits(bits);
            int first_refused = 0;
            for (int terms = 1; terms <= 40; terms++)
            {
                const bool fits = ext_mac_sum_fits(terms, p, rep);
                const U256 sum = worst_sum(terms, p, rep);
                CHECK(!fits || sum.hi == 0, "admitted but the sum wraps: %d terms, %d-bit prime, %d-bit words", terms, bits, rep);
                CHECK(fits || sum.hi != 0, "refused but the sum fits: %d terms, %d-bit prime, %d-bit words", terms, bits, rep);
                if (!fits && !first_refused)
                    first_refused = terms;
                CHECK(fits == !first_refused, "the predicate is not monotone in the term count");
            }
        }
    CHECK(!ext_mac_sum_fits(0, 3, 64) && !ext_mac_sum_fits(1, 1, 64) && !ext_mac_sum_fits(1, 3, 65) && !ext_mac_sum_fits(1, 3, 0),
          "arguments outside the predicate's domain");
}

// the launcher's rule (rgsw.hip ext_mac_plan): 0 one sum, 1 two halves, -1 refused
static int plan(int nd, u64 pmax)
{
    if (ext_mac_sum_fits(2 * nd, pmax, kKsDigitRepBits))
        return 0;
    return ext_mac_sum_fits(nd, pmax, kKsDigitRepBits) ? 1 : -1;
}

static void check_rule()
{
    for (int bits = 20; bits <= 61; bits++)
        for (int nd = 1; nd <= 8; nd++)
        {
            const u64 p = max_prime_of_bits(bits);
            const int got = plan(nd, p);
            // a context's levels have nd p < 2^64 (the key switch's own sum): all of them are served
            if (static_cast<u128>(nd) * p < kWord)
                CHECK(got >= 0, "nd %d at %d bits refused", nd, bits);
            CHECK((got == 0) == (worst_sum(2 * nd, p, 64).hi == 0), "nd %d at %d bits: one sum exactly while it fits", nd, bits);
            CHECK(got != 1 || worst_sum(nd, p, 64).hi == 0, "nd %d at %d bits: a half wraps", nd, bits);
        }
    CHECK(plan(4, max_prime_of_bits(61)) == 0 && plan(5, max_prime_of_bits(61)) == 1 && plan(8, max_prime_of_bits(61)) == 1,
          "61-bit primes: one sum up to nd = 4, two halves up to nd = 8");
    CHECK(plan(8, max_prime_of_bits(60)) == 0 && plan(9, max_prime_of_bits(60)) == 1, "60-bit primes: one sum up to nd = 8");
}

static void check_execution()
{
    std::mt19937_64 rng(29);
    const u64 primes[] = { (u64(1) << 61) - 1, 2305843009213554689ull, (u64(1) << 60) - (u64(1) << 14) + 1, 1152921504606830593ull,
                           1099511603201ull, 786433ull, 3ull }; // (moduli: primality plays no part in the arithmetic checked here)
    for (u64 p : primes)
    {
        u64 cr0, cr1;
        const_ratio(p, cr0, cr1);
        for (int worst = 0; worst < 2; worst++)
            for (int nd = 1; nd <= 9; nd++)
            {
                if (plan(nd, p) < 0)
                    continue;
                u64 x[18], k0[18];
                u64 want = 0;
                for (int j = 0; j < 2 * nd; j++)
                {
                    x[j] = worst ? ~u64(0) : rng();
                    k0[j] = worst ? p - 1 : rng() % p;
                    want = static_cast<u64>((want + static_cast<u128>(x[j] % p) * k0[j]) % p);
                }
                for (int split = 0; split < 2; split++)
                {
                    if (!split && plan(nd, p) != 0)
                        continue; // (the launcher never runs the unsplit sum here)
                    u64 lo = 0, hi = 0;
                    for (int j = 0; j < nd; j++)
                        mac128(lo, hi, x[j], k0[j]);
                    if (split)
                    {
                        lo = barrett_reduce_128(lo, hi, p, cr0, cr1);
                        hi = 0;
                    }
                    for (int j = nd; j < 2 * nd; j++)
                        mac128(lo, hi, x[j], k0[j]);
                    const u64 got = barrett_reduce_128(lo, hi, p, cr0, cr1);
                    CHECK(got == want, "p = %llu, nd %d, split %d, worst %d: %llu != %llu", (unsigned long long)p, nd, split, worst,
                          (unsigned long long)got, (unsigned long long)want);
                }
            }
    }
}

int main()
{
    check_predicate();
    check_rule();
    check_execution();
    if (failures)
    {
        std::printf("ext_mac_bounds_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("ext_mac_bounds_check: OK\n");
    return 0;
}
