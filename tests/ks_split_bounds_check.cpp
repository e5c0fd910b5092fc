// ks_split_bounds_check.cpp -- CPU test of ntt_bounds.hpp section 2c (built and run by tests/test_ks_split_bounds_host.py): the key
// switch's digit rows stored without the forward transform's last layer (kNttSplitLast) and finished by the inner product's
// pair form (keyswitch.hip ks_mac_pair_kernel).
// 1. Predicate: fwd_split_admits is the recurrence fwd_split_peak below 2^64 at the largest prime of the admitted size at log n
//    14..16, one bit more really overflows, and it never admits nd p >= 2^64.
// 2. Execution at the largest admitted prime: the log n - 1 layers of a ring of N/2 with the level-2 approximate quotient on
//    64-bit words (inputs below 2p, adversarial words and twiddles), then the pair butterfly with the exact lazy Shoup product,
//    then the 128-bit sums of nd = 16 products with key words p - 1 -- every true value shadowed in 128 bits: nothing wraps,
//    nothing exceeds the recurrence, every word stays in the residue class of an exact shadow, and the reduced sums equal the
//    shadow's. The exact-quotient instance (growth 2p per layer) runs through the same code.
// 4. Selection (ntt_select.hpp, pure): with kNttSplitLast a key-switch digit launch selects an instance of kFwdSplitInstances
//    (approximate quotient, or the exact one under SEALHIP_NTT_EXACT_FWD), keeps its other flags and needs no tickets; a launch
//    that has no such instance is refused: a row that is not gathered, a Harvey, floating-point or special-prime choice, a
//    canonical launch, a prime outside the bound. Without the flag nothing is split (tests/ntt_select_check.cpp pins that domain).
// 3. Just above the bound (one bit more, the same adversarial words): the recurrence says 2^64 is passed, and the predicate refuses.
// `ks_split_bounds_check --bits` only prints the admitted prime sizes (tests/test_ks_instances_host.py holds them against its own).
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../gemini-seal_amd/csrc/ntt_bounds.hpp"
#include "../gemini-seal_amd/csrc/ntt_select.hpp"

using namespace sealhip;
using namespace sealhip::bounds;
typedef __int128 i128;

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

// devmath.hpp mulhi_apx2 (level 2) and the exact Shoup quotient (level 0) as limb arithmetic
static u64 quotient_model(u64 y, u64 s, int level)
{
    const u64 y0 = y & 0xFFFFFFFFu, y1 = y >> 32, s0 = s & 0xFFFFFFFFu, s1 = s >> 32;
    if (level == 0)
        return static_cast<u64>((static_cast<u128>(y) * s) >> 64);
    return y1 * s1 + ((y0 * s1) >> 32) + ((y1 * s0) >> 32);
}
static u64 shoup(u64 w, u64 p)
{
    return static_cast<u64>((static_cast<u128>(w) << 64) / p);
}

static void predicate()
{
    for (int logn = kMinHalfLogn; logn <= kMaxHalfLogn; logn++)
    {
        const int bits = fwd_split_prime_bits(logn);
        const u64 p = max_prime_of_bits(bits), above = max_prime_of_bits(bits + 1);
        CHECK(fwd_split_admits(p, logn, 1) && fwd_split_peak(logn, p) < kWord, "log n %d: %d bits admitted", logn, bits);
        CHECK(!fwd_split_admits(above, logn, 1) && !fwd_split_admits(p + 1, logn, 1), "log n %d: one more is refused", logn);
        CHECK(fwd_split_peak(logn, above) >= kWord, "log n %d: the predicate is not tight", logn);
        CHECK(fwd_split_peak(logn, p) <= static_cast<u128>(fwd_split_output_mult(logn) + 2) * p, "log n %d: documented multiple", logn);
        // the 128-bit sums: nd words below 2^64 times key words below p
        for (int nd = 1; nd <= 64; nd++)
            CHECK(fwd_split_admits(p, logn, nd) == (static_cast<u128>(nd) * p < kWord), "log n %d nd %d: sum bound", logn, nd);
        CHECK(fwd_split_admits(p, logn, 16), "log n %d: sixteen digits (the pair form's most) at the largest prime", logn);
    }
    CHECK(!fwd_split_admits(max_prime_of_bits(50), 13, 1) && !fwd_split_admits(max_prime_of_bits(50), 17, 1), "ring sizes");
}

// -> false if some true value left the 64-bit word
static bool execution(int logn, u64 p, int level, bool expect_fits)
{
    const int h = 1 << (logn - 1), nd = 16;
    std::mt19937_64 rng(logn * 11 + level);
    const u64 g = static_cast<u64>(level ? kFwdApxGrowth : 2) * p;
    bool wrapped = false;
    u128 peak = 0;
    std::vector<u128> lo(h, 0), lo_shadow(h, 0); // sums of X[2j] over the digits, and of the exact residues
    std::vector<u64> half[2], shadow[2];
    for (int d = 0; d < nd; d++)
    {
        for (int par = 0; par < 2; par++) // E and O: the same network on each parity class
        {
            std::vector<u64> &x = half[par], &sh = shadow[par];
            x.assign(h, 0);
            sh.assign(h, 0);
            for (int i = 0; i < h; i++)
            {
                x[i] = (i % 3 == 0 || d == 0) ? 2 * p - 1 : rng() % (2 * p);
                sh[i] = x[i] % p;
            }
            for (int l = logn - 2; l >= 0; l--)
            {
                const int gap = 1 << l;
                for (int blk = 0; blk < h; blk += 2 * gap)
                {
                    const u64 w = ((blk / (2 * gap)) % 5 == 0 || d == 0) ? p - 1 : rng() % p, ws = shoup(w, p);
                    for (int j = blk; j < blk + gap; j++)
                    {
                        const u64 u = x[j], y = x[j + gap], q = quotient_model(y, ws, level);
                        const u128 v = static_cast<u128>(y) * w - static_cast<u128>(q) * p;
                        const u128 X = static_cast<u128>(u) + v;
                        const i128 Y = static_cast<i128>(u) - static_cast<i128>(v) + g;
                        wrapped = wrapped || v >= g || X >= kWord || Y < 0 || static_cast<u128>(Y) >= kWord;
                        peak = X > peak ? X : peak;
                        peak = static_cast<u128>(Y) > peak ? static_cast<u128>(Y) : peak;
                        x[j] = u + (y * w - q * p);
                        x[j + gap] = (u << 1) + g - x[j];
                        const u64 sv = static_cast<u64>(static_cast<u128>(sh[j + gap]) * w % p), su = sh[j];
                        sh[j] = (su + sv) % p;
                        sh[j + gap] = (su + p - sv) % p;
                    }
                }
            }
        }
        // the pair butterfly of ks_mac_pair_kernel and one component's sum for the even word, key word p - 1
        for (int j = 0; j < h; j++)
        {
            const u64 w = (j % 5 == 0) ? p - 1 : rng() % p, ws = shoup(w, p);
            const u64 e = half[0][j], o = half[1][j];
            const u128 t = static_cast<u128>(o) * w - static_cast<u128>(quotient_model(o, ws, 0)) * p;
            const u128 X0 = static_cast<u128>(e) + t;
            const i128 X1 = static_cast<i128>(e) - static_cast<i128>(t) + 2 * static_cast<i128>(p);
            wrapped = wrapped || t >= 2 * static_cast<u128>(p) || X0 >= kWord || X1 < 0 || static_cast<u128>(X1) >= kWord;
            peak = X0 > peak ? X0 : peak;
            peak = static_cast<u128>(X1) > peak ? static_cast<u128>(X1) : peak;
            const u64 x0 = e + static_cast<u64>(t), x1 = e - static_cast<u64>(t) + 2 * p; // the kernel's words
            const u64 st = static_cast<u64>(static_cast<u128>(shadow[1][j]) * w % p);
            const u64 s0 = (shadow[0][j] + st) % p, s1 = (shadow[0][j] + p - st) % p;
            if (!wrapped)
                CHECK(x0 % p == s0 && x1 % p == s1, "log n %d level %d: pair %d leaves its residue class", logn, level, j);
            const u128 term = static_cast<u128>(x0) * (p - 1);
            wrapped = wrapped || lo[j] + term < lo[j]; // the 128-bit accumulator itself
            lo[j] += term;
            lo_shadow[j] = (lo_shadow[j] + static_cast<u128>(s0) * (p - 1)) % p;
        }
    }
    if (expect_fits)
    {
        CHECK(!wrapped, "log n %d level %d p=%llu: a value left its word", logn, level, p);
        CHECK(peak <= fwd_split_peak(logn, p), "log n %d level %d: execution above the recurrence", logn, level);
        int bad = 0;
        for (int j = 0; j < h; j++)
            bad += lo[j] % p != lo_shadow[j];
        CHECK(bad == 0, "log n %d level %d: %d sums differ from the exact shadow", logn, level, bad);
    }
    return !wrapped;
}

static void selection()
{
    for (int logn = kMinHalfLogn; logn <= kMaxHalfLogn; logn++)
    {
        const u64 p55 = (u64(1) << 55) - 55, p59 = (u64(1) << 59) - 55, p49 = (u64(1) << 49) + 1;
        const u64 rows[5] = { p55, p55, p55, p55, p55 };
        FwdFacts f{};
        f.logn = logn;
        f.flags = kNttAnyRep | kNttApprox | kNttSplitLast;
        f.live = rows;
        f.live_n = 5;
        f.gathers = f.all_gathered = f.same_source = true;
        f.treatment = kTreatBarrett;
        f.key_moduli_fp = false;
        FwdChoice c = select_fwd_half(f);
        CHECK(c.valid && c.split && c.sched == kSchedApprox && c.treatment == kTreatBarrett && !c.tickets &&
                  c.instance == fwd_split_instance_index(kSchedApprox, kTreatBarrett) && c.instance >= 0 && c.instance < kFwdSplitInstanceCount &&
                  (c.flags & kNttPolyMajor) && (c.flags & kNttSplitLast),
              "log n %d: digit launch with the flag", logn);
        FwdFacts g = f;
        g.flags &= ~kNttSplitLast;
        c = select_fwd_half(g);
        CHECK(c.valid && !c.split && c.sched == kSchedApprox && c.instance == fwd_instance_index(logn, kSchedApprox, kTreatBarrett), "log n %d: without the flag", logn);
        g = f;
        g.sw.exact_fwd = true;
        c = select_fwd_half(g);
        CHECK(c.valid && c.split && c.sched == kSchedLazy && c.instance == fwd_split_instance_index(kSchedLazy, kTreatBarrett), "log n %d: exact instance", logn);
        g.flags |= kNttStrict; // (EXACT_FWD keeps the Harvey sequence: no split instance)
        CHECK(!select_fwd_half(g).valid, "log n %d: Harvey is refused", logn);
        g = f;
        g.all_gathered = false;
        CHECK(!select_fwd_half(g).valid, "log n %d: a row in place is refused", logn);
        g = f;
        g.flags |= kNttCanonical;
        CHECK(!select_fwd_half(g).valid, "log n %d: canonical is refused", logn);
        g = f;
        g.treatment = kTreatNegSpecial;
        g.aux_p = p55;
        CHECK(!select_fwd_half(g).valid, "log n %d: special-prime treatment is refused", logn);
        const u64 big[5] = { p55, p59, p55, p55, p55 };
        g = f;
        g.live = big;
        CHECK(!select_fwd_half(g).valid, "log n %d: a 59-bit row is refused", logn);
        const u64 small[5] = { p49, p49, p49, p49, p49 };
        g = f;
        g.live = small;
        g.key_moduli_fp = true;
        CHECK(!select_fwd_half(g).valid, "log n %d: the floating-point choice is refused", logn);
        g.sw.no_fp64 = true;
        CHECK(select_fwd_half(g).valid && select_fwd_half(g).split, "log n %d: small primes on the integer instance", logn);
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--bits"))
    {
        // what tests/test_ks_instances_host.py restates: per ring the prime sizes the split form and the lazy schedule admit,
        // then the size below which a launch takes the floating-point schedule and the size of its raw inputs
        for (int logn = kMinHalfLogn; logn <= kMaxHalfLogn; logn++)
            std::printf("ring %d split %d lazy %d\n", logn, fwd_split_prime_bits(logn), fwd_lazy_prime_bits(logn));
        int input_bits = 0;
        while ((u64(1) << input_bits) < kFpInputBound)
            input_bits++;
        std::printf("fp %d input %d\n", kFpPrimeBits, input_bits);
        return 0;
    }
    predicate();
    selection();
    for (int logn = kMinHalfLogn; logn <= kMaxHalfLogn; logn++)
    {
        const int bits = fwd_split_prime_bits(logn);
        execution(logn, max_prime_of_bits(bits), kFwdApxLevel, true);
        execution(logn, max_prime_of_bits(bits), 0, true);
        // just above: the worst case passes 2^64 by the recurrence; whether these words do is reported, not required
        const bool fits = execution(logn, max_prime_of_bits(bits + 1), kFwdApxLevel, false);
        std::printf("log n %d: %d bits admitted (peak %.1f p); the same words at %d bits %s\n", logn, bits,
                    static_cast<double>(fwd_split_peak(logn, max_prime_of_bits(bits))) / static_cast<double>(max_prime_of_bits(bits)),
                    bits + 1, fits ? "happen to fit" : "leave the word");
    }
    std::printf(failures ? "ks_split_bounds_check: %d FAILURES\n" : "ks_split_bounds_check: OK\n", failures);
    return failures ? 1 : 0;
}
