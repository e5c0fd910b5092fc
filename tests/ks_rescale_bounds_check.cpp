// ks_rescale_bounds_check.cpp -- CPU test of the arithmetic of the merged mod-down and rescale (DESIGN.md section 19;
// built and run by tests/test_ks_rescale_host.py). The kernels of gemini-seal_amd/csrc/keyswitch.hip are executed here word
// for word (the primitives as devmath.hpp writes them) against unsigned __int128 arithmetic on extreme operands:
// 1. step 3's term floor(z * C_d / 2^64) = z * cr1 + mulhi(z, cr0) fits one word and is that floor, for z up to d - 1;
// 2. step 4's sum of up to 64 products of 61-bit residues plus v * (-D mod q) plus (-half mod q) stays below 2^128 exactly
//    when bounds::ks_rescale_sum_fits admits it (ntt_bounds.hpp section 9), and the mac128 chain with one
//    barrett_reduce_128 gives the canonical residue;
// 3. step 5: mul_add_mod, sub_mod and the Shoup product give canonical residues on the largest operands;
// 4. steps 2-4 end to end on dropped sets of 2, 4 and 10 small primes: the converted word is ((Y + half) mod D) - half
//    modulo the kept prime, Y reconstructed exactly.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

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

// ---- the kernels' primitives, as devmath.hpp writes them
static u64 mulhi(u64 a, u64 b)
{
    return static_cast<u64>((static_cast<u128>(a) * b) >> 64);
}
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
static u64 mul_add_mod(u64 a, u64 b, u64 c, u64 p, u64 cr0, u64 cr1)
{
    u64 lo = a * b, hi = mulhi(a, b);
    const u64 lo2 = lo + c;
    hi += (lo2 < lo);
    return barrett_reduce_128(lo2, hi, p, cr0, cr1);
}
static u64 mulmod_shoup(u64 x, u64 y, u64 yshoup, u64 p)
{
    const u64 t = x * y - mulhi(x, yshoup) * p;
    return t >= p ? t - p : t;
}
static u64 add_mod(u64 a, u64 b, u64 p)
{
    const u64 s = a + b;
    return s >= p ? s - p : s;
}
static u64 sub_mod(u64 a, u64 b, u64 p)
{
    const u64 d = a - b;
    return a < b ? d + p : d;
}
// ---- host helpers
static void const_ratio(u64 p, u64 &cr0, u64 &cr1)
{
    const u128 top = (~static_cast<u128>(0)) / p; // == floor(2^128 / p) for every p that does not divide 2^128
    cr0 = static_cast<u64>(top);
    cr1 = static_cast<u64>(top >> 64);
}
static u64 shoup(u64 y, u64 p)
{
    return static_cast<u64>((static_cast<u128>(y) << 64) / p);
}
static u64 mulmod(u64 a, u64 b, u64 p)
{
    return static_cast<u64>(static_cast<u128>(a) * b % p);
}
static u64 powmod(u64 a, u64 e, u64 p)
{
    u64 r = 1 % p;
    for (a %= p; e; e >>= 1, a = mulmod(a, a, p))
        if (e & 1)
            r = mulmod(r, a, p);
    return r;
}

static const u64 kBig[] = { (u64(1) << 61) - 1, 2305843009213554689ull, 1152921504606830593ull, 1099511603201ull, 786433ull };

// the kernel's rescale_z: step 2 and the term of step 3 added into (slo, shi)
static u64 rescale_z(u64 y, u64 half_d, u64 inv_hat, u64 inv_hat_shoup, u64 d, u64 cr0, u64 cr1, u64 &slo, u64 &shi)
{
    const u64 z = mulmod_shoup(add_mod(y, half_d, d), inv_hat, inv_hat_shoup, d);
    const u64 t = z * cr1 + mulhi(z, cr0);
    const u64 nl = slo + t;
    shi += nl < slo;
    slo = nl;
    return z;
}

static void check_quotient_term()
{
    std::mt19937_64 rng(19);
    for (u64 d : kBig)
    {
        u64 cr0, cr1;
        const_ratio(d, cr0, cr1);
        const u128 C = (static_cast<u128>(cr1) << 64) | cr0;
        for (int i = 0; i < 100000; i++)
        {
            const u64 z = i == 0 ? 0 : i == 1 ? d - 1 : i == 2 ? d / 2 : rng() % d;
            // z * C < 2^128: the exact floor in 128 bits
            const u128 exact = (static_cast<u128>(z) * C) >> 64;
            const u128 wide = static_cast<u128>(z) * cr1 + mulhi(z, cr0);
            CHECK(static_cast<u128>(z) * cr1 < (static_cast<u128>(1) << 64), "z * cr1 wraps: d = %llu", (unsigned long long)d);
            CHECK(wide == exact && (wide >> 64) == 0, "floor(z C / 2^64) in one word: d = %llu z = %llu", (unsigned long long)d,
                  (unsigned long long)z);
            CHECK(static_cast<u64>(wide) == z * cr1 + mulhi(z, cr0), "the 64-bit form");
        }
    }
}

static void check_sum_predicate()
{
    for (int bits = 20; bits <= 63; bits++)
        for (int dropped = 1; dropped <= 70; dropped++)
        {
            const u128 m = (static_cast<u128>(1) << bits) - 1;
            U256 sum;
            for (int a = 0; a < dropped; a++)
                sum.add(m * m); // z_d * hat_d
            sum.add(static_cast<u128>(dropped) * m); // v <= dropped times a canonical residue
            sum.add(m);                               // (-half) mod q
            CHECK((sum.hi == 0) == ks_rescale_sum_fits(dropped, bits), "predicate and exact sum disagree: %d primes of %d bits",
                  dropped, bits);
        }
    CHECK(ks_rescale_sum_fits(64, 61) && !ks_rescale_sum_fits(65, 61), "64 dropped primes of 61 bits, not 65");
    CHECK(!ks_rescale_sum_fits(0, 61) && !ks_rescale_sum_fits(1, 64) && !ks_rescale_sum_fits(1, 0), "degenerate arguments");
}

static void check_sum_execution()
{
    std::mt19937_64 rng(91);
    for (u64 q : kBig)
    {
        u64 cr0, cr1;
        const_ratio(q, cr0, cr1);
        for (int dropped : { 2, 3, 4, 10, 64 })
            for (int worst = 0; worst < 2; worst++)
            {
                const u64 top = (u64(1) << 61) - 1; // z_d below a 61-bit prime whatever q is
                u64 lo = worst ? q - 1 : rng() % q, hi = 0; // (-half) mod q
                u64 want = lo % q;
                for (int a = 0; a < dropped; a++)
                {
                    const u64 z = worst ? top - 1 : rng() % top, hat = worst ? q - 1 : rng() % q;
                    mac128(lo, hi, z, hat);
                    want = (want + mulmod(z % q, hat, q)) % q;
                }
                const u64 v = worst ? static_cast<u64>(dropped) : rng() % dropped, negD = worst ? q - 1 : rng() % q;
                mac128(lo, hi, v, negD);
                want = (want + mulmod(v % q, negD, q)) % q;
                CHECK(barrett_reduce_128(lo, hi, q, cr0, cr1) == want, "sum of %d dropped primes mod %llu", dropped,
                      (unsigned long long)q);
            }
    }
}

static void check_step5()
{
    std::mt19937_64 rng(5);
    for (u64 q : kBig)
    {
        u64 cr0, cr1;
        const_ratio(q, cr0, cr1);
        for (int i = 0; i < 100000; i++)
        {
            const bool ext = i < 16;
            const u64 b = ext ? ((i & 1) ? q - 1 : 0) : rng() % q, Pq = ext ? ((i & 2) ? q - 1 : 1) : rng() % q;
            const u64 a = ext ? ((i & 4) ? q - 1 : 0) : rng() % q, t = ext ? ((i & 8) ? q - 1 : 0) : rng() % q;
            const u64 invD = ext ? q - 1 : 1 + rng() % (q - 1);
            const u64 s = mul_add_mod(b, Pq, a, q, cr0, cr1);
            CHECK(s == static_cast<u64>((static_cast<u128>(b) * Pq + a) % q), "mul_add_mod mod %llu", (unsigned long long)q);
            const u64 x = sub_mod(s, t, q);
            CHECK(x < q && x == (s + q - t) % q, "sub_mod mod %llu", (unsigned long long)q);
            const u64 w = mulmod_shoup(x, invD, shoup(invD, q), q);
            CHECK(w == mulmod(x, invD, q), "Shoup product mod %llu", (unsigned long long)q);
        }
    }
}

static void check_end_to_end()
{
    // distinct small odd primes: ten of them keep D below 2^115, so Y and every exact quantity fit 128 bits
    const u64 small[] = { 2039, 2029, 2027, 2017, 2011, 2003, 1999, 1997, 1993, 1987 };
    std::mt19937_64 rng(4);
    for (int nd1 : { 2, 4, 10 })
        for (u64 q : { kBig[0], kBig[2], kBig[3] })
        {
            u128 D = 1;
            for (int a = 0; a < nd1; a++)
                D *= small[a];
            const u128 half = D / 2;
            std::vector<u64> inv_hat(nd1), inv_hat_s(nd1), half_d(nd1), hat(nd1), c0(nd1), c1(nd1);
            for (int a = 0; a < nd1; a++)
            {
                const u64 d = small[a];
                inv_hat[a] = powmod(static_cast<u64>((D / d) % d), d - 2, d);
                inv_hat_s[a] = shoup(inv_hat[a], d);
                half_d[a] = static_cast<u64>(half % d);
                hat[a] = static_cast<u64>((D / d) % q);
                const_ratio(d, c0[a], c1[a]);
            }
            u64 cr0, cr1;
            const_ratio(q, cr0, cr1);
            const u64 Dq = static_cast<u64>(D % q), hq = static_cast<u64>(half % q);
            const u64 negD = Dq ? q - Dq : 0, neg_half = hq ? q - hq : 0;
            for (int i = 0; i < 20000; i++)
            {
                // Y with z_d all 0 (Y = -half), z_d all d - 1, around 0 and D, else random
                u128 Y = (static_cast<u128>(rng()) << 64 | rng()) % D;
                if (i == 0)
                    Y = D - half;
                else if (i < 8)
                    Y = static_cast<u128>(i - 1);
                else if (i < 16)
                    Y = D - static_cast<u128>(i - 7);
                u64 slo = 0, shi = 0, lo = neg_half, hi = 0;
                bool all_top = i == 16;
                for (int a = 0; a < nd1; a++)
                {
                    const u64 d = small[a];
                    u64 y = static_cast<u64>(Y % d);
                    if (all_top) // choose y so that z_d = d - 1: y = (d - 1) * hat_d - half mod d
                        y = static_cast<u64>((static_cast<u128>(d - 1) * ((D / d) % d) + d - half_d[a]) % d);
                    const u64 z = rescale_z(y, half_d[a], inv_hat[a], inv_hat_s[a], d, c0[a], c1[a], slo, shi);
                    if (all_top)
                        CHECK(z == d - 1, "z_d = d - 1");
                    mac128(lo, hi, z, hat[a]);
                }
                if (all_top)
                {
                    // reconstruct Y from z_d = d - 1: (Y + half) mod D = sum (d - 1) (D / d) mod D
                    u128 s = 0;
                    for (int a = 0; a < nd1; a++)
                        s = (s + static_cast<u128>(small[a] - 1) * (D / small[a])) % D;
                    Y = (s + D - half) % D;
                }
                const u64 v = shi;
                CHECK(v < static_cast<u64>(nd1), "v < |Dset|");
                mac128(lo, hi, v, negD);
                const u64 temp = barrett_reduce_128(lo, hi, q, cr0, cr1);
                const u128 r = (Y + half) % D; // what the conversion must reproduce exactly
                const u64 want = static_cast<u64>(((r % q) + q - hq) % q);
                CHECK(temp == want, "end to end: %d dropped primes, q = %llu, case %d", nd1, (unsigned long long)q, i);
            }
        }
}

int main()
{
    check_quotient_term();
    check_sum_predicate();
    check_sum_execution();
    check_step5();
    check_end_to_end();
    if (failures)
    {
        std::printf("ks_rescale_bounds_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("ks_rescale_bounds_check: OK\n");
    return 0;
}
