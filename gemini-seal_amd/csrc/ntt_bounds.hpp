// ntt_bounds.hpp -- every "this shortcut cannot overflow" argument of the engine in ONE place, as code.
//
// The reference's invariant is that every intermediate of its lazy arithmetic fits a 64-bit word for moduli up to
// SEAL_MOD_BIT_COUNT_MAX = 61 bits (native/src/seal/util/defines.h:33,52-53; butterflies util/ntt.cpp:245-281). The engine
// takes shortcuts that are only bit-exact while *their* intermediates fit too (64-bit words for the integer kernels, the
// 53-bit significand for the FP64 ones). Each shortcut has
//   * its reduction SCHEDULE (which layer reduces what) -- the kernels in ntt.hip read it from here, nowhere else;
//   * a worst-case magnitude RECURRENCE that walks that schedule layer by layer;
//   * an ADMISSION predicate for the launchers, defined as "the recurrence stays below the limit for the largest prime of
//     that size at every supported ring size" -- a constant derived at compile time, not a hand-written inequality.
// tests/bounds_check.cpp enumerates prime sizes 20..61 bits x log n 14..16 x every schedule: admitted => peak below the
// limit, one bit more => the recurrence really overflows (the predicates are tight, not just safe); and a model of the
// floating-point modular product checks the per-product bound used here against exact integer arithmetic on
// adversarial operands. (Round 2 shipped a whole-row inverse with the half-row shape's bound for 24 minutes; with this
// header the same mistake fails a static_assert.)
//
// Plain C++17, no HIP: included by ntt.hip / pipeline.cpp and compiled on its own by the CPU test.
#pragma once
#include <cstdint>

namespace sealhip
{
    namespace bounds
    {
        using u64 = unsigned long long;
        using u128 = unsigned __int128;

        constexpr int kMinHalfLogn = 14, kMaxHalfLogn = 16; // ring sizes served by the single-pass (half-row) kernels
        constexpr int kMaxPrimeBits = 61;                   // SEAL_MOD_BIT_COUNT_MAX (util/defines.h:33)
        constexpr u128 kWord = static_cast<u128>(1) << 64;  // integer kernels: every true value must stay below 2^64
        constexpr long double kFpLimit = 9007199254740992.0L; // 2^53: FP64 kernels hold integers exactly below it

        constexpr u64 max_prime_of_bits(int bits) // the worst case of a predicate "p < 2^bits"
        {
            return (bits >= 64 ? ~u64(0) : (u64(1) << bits) - 1);
        }
        // ... and where a handful of units matter (the FP64 inverse runs to 8p + O(1) against 2^53): the largest value an
        // NTT prime of that size can have, p = 1 (mod 2N) (the context refuses anything else: ntt.cpp:37-52)
        constexpr u64 max_ntt_prime_of_bits(int bits, int logn)
        {
            return bits > logn + 1 ? (u64(1) << bits) - (u64(1) << (logn + 1)) + 1 : 0;
        }

        // =====================================================================================================
        // 1. Inverse transform, integer, lazy sums (ntt_inv_half_kernel<.., LZ = 1>, butterflies_inv_hs<MODE>).
        // A shape with T on-chip layers (T = log n - 1 for the half-row form whose top layer is left to a consumer or to
        // ntt_inv_top_kernel; T = log n for the whole-row form, whose layer T - 1 is BackwardLazyLast with n^-1 folded in).
        // Layer l reduces its sum with barrett_lazy (MODE 2, -> [0, 2p)) only for l == r1 and l == T - 1; elsewhere the sum
        // is left as it is (MODE 1). Values entering layer l are below 2^shift(l) * p; the difference operand gets exactly
        // that bound added so that it stays non-negative. The product is a Shoup product of a 64-bit word: below 2p with the
        // exact quotient (the two reducing layers; in the dense schedule also the first f = log n - 13 layers, whose plain
        // instances would spill with the zero-high pairs live), below kInvLazyProductMult p = 4p with the level-2 quotient
        // (section 2: quotient_shortfall) that every other MODE 1 layer uses since round 4. A MODE 1 layer's outputs are bounded by its unreduced sum, 2^(shift + 1) p >= 4p, so the
        // recurrence below takes the maximum of the two and finds the schedule unchanged.
        constexpr int kInvLazyProductMult = 4;
        // Two schedules (`sched`):
        //   0  SPARSE (rounds 1-3): two reducing layers, r1 and T - 1; for primes with head-room (2^55 / 2^56 per shape);
        //   1  DENSE (round 4): every third layer (l % 3 == 2) and the last reduce, so values never pass 16p: for primes up to
        //      2^60 -- the 60-bit Bsk rows of a BFV multiply, and ciphertext primes of 56 to 60 bits -- which ran the
        //      reference's own sequence (a conditional subtraction in every butterfly) for want of head-room. The reducing
        //      layers bring their SUM below 2p with the single-precision quotient estimate (section 6: quotient below 16) and
        //      form their product with the exact quotient (below 2p); the two layers in between leave sums of up to 4p / 8p
        //      entering and products below 4p (level-2 quotient).
        constexpr int inv_lazy_r1(int T)
        {
            return (T - 1) / 2;
        }
        constexpr int inv_lazy_mode(int T, int l, int sched = 0)
        {
            if (sched == 1)
                return (l % 3 == 2 || l == T - 1) ? 2 : 1;
            return (l == inv_lazy_r1(T) || l == T - 1) ? 2 : 1;
        }
        constexpr int inv_lazy_shift(int T, int l, int sched = 0)
        {
            if (sched == 1)
                return 1 + l % 3; // entering: 2p after a reducing layer (and at the start), then 4p, then 8p
            return 1 + (l <= inv_lazy_r1(T) ? l : l - inv_lazy_r1(T) - 1);
        }
        // worst-case recurrence: the largest true value any instruction of the schedule forms (sum u + y, difference
        // u - y + addend), for inputs below 2p. Also checks the schedule's own claim "values entering layer l are below
        // 2^shift(l) p" -- returns 2^64 (overflow) if the claim were violated, so a wrong shift table cannot pass.
        constexpr u128 inv_lazy_peak(int T, u64 p, int sched = 0)
        {
            u128 bound = static_cast<u128>(2) * p; // inputs: what the reference requires of an inverse transform's input
            u128 peak = bound;
            for (int l = 0; l < T; l++)
            {
                const u128 claimed = static_cast<u128>(p) << inv_lazy_shift(T, l, sched);
                if (bound > claimed)
                    return kWord; // schedule inconsistent
                const u128 sum = 2 * claimed;       // u + y < 2 * claimed
                const u128 diff = 2 * claimed;      // u - y + claimed < 2 * claimed
                peak = sum > peak ? sum : peak;
                peak = diff > peak ? diff : peak;
                // outputs: a reducing layer (MODE 2) leaves sum and product (exact quotient) below 2p; a MODE 1 layer keeps
                // the sum and may leave its product anywhere below 4p (level-2 quotient)
                const u128 prod = static_cast<u128>(kInvLazyProductMult) * p;
                bound = inv_lazy_mode(T, l, sched) == 2 ? static_cast<u128>(2) * p : (sum > prod ? sum : prod);
            }
            return peak;
        }
        constexpr int inv_lazy_max_shift(int T, int sched = 0)
        {
            int m = 0;
            for (int l = 0; l < T; l++)
                m = inv_lazy_shift(T, l, sched) > m ? inv_lazy_shift(T, l, sched) : m;
            return m;
        }
        // admission: largest prime size (bits) for which the recurrence stays below 2^64
        constexpr int inv_lazy_prime_bits(int T, int sched = 0)
        {
            int bits = 0;
            for (int b = 1; b <= kMaxPrimeBits; b++)
                if (inv_lazy_peak(T, max_prime_of_bits(b), sched) < kWord)
                    bits = b;
            return bits;
        }
        constexpr bool inv_lazy_admits(int T, u64 p)
        {
            return p <= max_prime_of_bits(inv_lazy_prime_bits(T));
        }
        constexpr u64 kSmallQuotMinPrime = u64(1) << 45; // section 6
        // the dense schedule: sums up to 16p must fit the word (primes below 2^60) and its reducing layers estimate a quotient
        // below 16 in single precision (section 6: p at least 2^45; the predicate calls small_quot_admits itself)
        constexpr bool small_quot_admits(u64 p, int mult);
        constexpr int kInvDenseSumMult = 16;
        constexpr bool inv_dense_admits(int T, u64 p)
        {
            return T >= 3 && p <= max_prime_of_bits(inv_lazy_prime_bits(T, 1)) && small_quot_admits(p, kInvDenseSumMult);
        }
        static_assert(inv_lazy_prime_bits(13, 1) == 60 && inv_lazy_prime_bits(14, 1) == 60 && inv_lazy_prime_bits(15, 1) == 60 &&
                          inv_lazy_prime_bits(16, 1) == 60,
                      "dense lazy inverse: primes below 2^60 in every shape");
        static_assert(inv_lazy_max_shift(16, 1) == 3, "dense lazy inverse: values entering a layer are below 8p");

        // =====================================================================================================
        // 2. Forward transform, integer (ntt_fwd_half_kernel<.., STRICT = 0 / 2>). The fork's forward butterfly
        // (ForwardLazy, ntt.cpp:245-252) never reduces its first operand: u' = u + v, y' = u - v + 2p with v a lazy Shoup
        // product below 2p, so values grow by 2p per layer; only the last layer (ForwardLazyLast, :254-261) brings its first
        // operand below 2p with a Barrett step. On the 60-bit Bsk rows that growth wraps mod 2^64 and the wrapped words
        // ARE the reference's result: the exact instances have no predicate. Shortcuts that change the
        // representative (only where the consumer reduces whatever it reads):
        //   kNttAnyRep   the last layer keeps its first operand unreduced (fin & 2);
        //   kNttApprox   approximate Shoup quotient (STRICT = 2): the product v lands below g p and y' = u - v + g p, so the
        //                values grow by g p per layer. g = kFwdApxGrowth: 3 for round 2's form (hi32(y0 s0) dropped from the
        //                exact quotient: one unit short at most), 4 for round 4's carry-free form (devmath.hpp mulhi_apx2:
        //                q = y1 s1 + hi32(y0 s1) + hi32(y1 s0) drops the low halves of both cross products as well, three
        //                units short of floor(y w / p) at most, quotient_shortfall below);
        //   unreduced gathered inputs (key-switch mod-up without the conditional subtraction): inputs below 2p not p.
        // All log n layers count (the top one is applied on load).
        constexpr int kFwdApxLevel = 2;
        static_assert(kFwdApxLevel == 1 || kFwdApxLevel == 2, "approximate-quotient form");
        // how far below floor(y w / p) the quotient estimate can fall, as the number of dropped terms that each lose less
        // than one unit: Shoup's floor(w 2^64 / p) itself (1), hi32(y0 s0) (level 1 and 2: together with the floor of the
        // sum of the cross products, 1), and at level 2 the low halves of the two cross products (1 more: the three dropped
        // pieces sum to less than 3 * 2^32, i.e. lose at most 2 units of 2^32 after the floor).
        constexpr int quotient_shortfall(int level)
        {
            return level == 0 ? 1 : (level == 1 ? 2 : 3);
        }
        constexpr int kFwdApxGrowth = quotient_shortfall(kFwdApxLevel) + 1; // v = y w - q p < (shortfall + 1) p
        constexpr u128 fwd_int_peak(int logn, u64 p, int in_mult, bool apx, bool skip_last_barrett)
        {
            const u128 g = static_cast<u128>(apx ? kFwdApxGrowth : 2) * p; // growth per layer = bound of the product
            u128 bound = static_cast<u128>(in_mult) * p, peak = bound;
            for (int l = 0; l < logn; l++)
            {
                u128 u = bound;
                if (l == logn - 1 && !skip_last_barrett)
                    u = static_cast<u128>(2) * p; // barrett_lazy of the first operand
                const u128 out = u + g;           // u + v < u + g;  u - v + g <= u + g
                peak = out > peak ? out : peak;
                bound = out;
            }
            return peak;
        }
        // one predicate for both shortcuts together with unreduced inputs (the key-switch digit launches use all three),
        // per ring size (the growth is per layer)
        constexpr int fwd_lazy_prime_bits(int logn)
        {
            int bits = 0;
            for (int b = 1; b <= kMaxPrimeBits; b++)
                if (fwd_int_peak(logn, max_prime_of_bits(b), 2, true, true) < kWord)
                    bits = b;
            return bits;
        }
        static_assert(kFwdApxLevel != 1 || (fwd_lazy_prime_bits(14) == 58 && fwd_lazy_prime_bits(16) == 58),
                      "level 1: kNttAnyRep / kNttApprox / unreduced mod-up: primes below 2^58 (50p at log n = 16)");
        static_assert(kFwdApxLevel != 2 || (fwd_lazy_prime_bits(14) == 58 && fwd_lazy_prime_bits(15) == 58 && fwd_lazy_prime_bits(16) == 57),
                      "level 2: 58p / 62p below 2^64 for primes below 2^58 at log n = 14 / 15; 66p at log n = 16: below 2^57");
        constexpr bool fwd_lazy_admits(u64 p, int logn) // kNttAnyRep, kNttApprox, mod-up without the conditional subtraction
        {
            return logn >= kMinHalfLogn && logn <= kMaxHalfLogn && p <= max_prime_of_bits(fwd_lazy_prime_bits(logn));
        }
        // The canonicalising public entry (sealhip_ntt_negacyclic_harvey) documents operands below 4p (include/sealhip.h: what
        // the reference's butterflies are written for), and it is handed caller-owned words: its cheap schedule (approximate
        // quotient, no Barrett step in the last layer, one reduction in the store) is admitted on THAT range, not on the
        // [0, 2p) of the internal launches: inputs below kCanonInMult p.
        constexpr int kCanonInMult = 4;
        constexpr int fwd_canon_output_mult(int logn)
        {
            return kCanonInMult + kFwdApxGrowth * logn;
        }
        constexpr bool fwd_canon_admits(u64 p, int logn)
        {
            return logn >= kMinHalfLogn && logn <= kMaxHalfLogn && fwd_lazy_admits(p, logn) &&
                   fwd_int_peak(logn, p, kCanonInMult, true, true) < kWord;
        }
        // largest output of an approximate-quotient launch, in units of p (documentation + test): 2 + g log n with
        // kNttAnyRep (50 / 66 at log n = 16), else 2 + g (the last layer's first operand is brought below 2p)
        constexpr int fwd_apx_output_mult(int logn, bool anyrep)
        {
            return anyrep ? 2 + kFwdApxGrowth * logn : 2 + kFwdApxGrowth;
        }

        // ---- 2b. Dense lazy FORWARD schedule (round 4; STRICT mode's 56-60-bit rows, ntt_fwd_half_kernel<.., STRICT = 4>).
        // STRICT means "nothing wraps" (SURVEY B.6); Harvey's corrected butterflies guarantee it for any prime with a
        // conditional subtraction per butterfly. Where the consumer takes any representative below 2p (the Bsk rows of the BFV
        // multiply: the tensor product reduces whatever it reads) the same residues come out of the reference's own
        // butterfly -- exact quotient, product below 2p, first operand left as it is: values grow by 2p per layer -- if all 32
        // words of a lane are brought back below 2p often enough that nothing reaches 2^64: with the single-precision quotient
        // estimate (section 6) before rounds 2 and 3 and in the store. Inputs below kFwdDenseInMult p (the range the entry
        // documents), top layer +2p, round 1 +8p = 14p; rounds 2 and 3 from 2p to 10p; the final round's f = log n - 13 layers
        // from 10p to at most 16p: every value is BELOW fwd_dense_peak_mult(log n) p <= 16p < 2^64 for p < 2^60.
        constexpr int kFwdDenseInMult = 4;
        constexpr bool fwd_dense_reduce_before_round(int r) // r = 1..3 register rounds, 4 = the final round
        {
            return r == 2 || r == 3;
        }
        constexpr int fwd_dense_peak_mult(int logn)
        {
            int b = kFwdDenseInMult + 2, peak = b; // after the top layer
            for (int r = 1; r <= 4; r++)
            {
                if (fwd_dense_reduce_before_round(r))
                    b = 2;
                const int layers = r <= 3 ? 4 : logn - 13;
                for (int l = 0; l < layers; l++)
                    b += 2;
                peak = b > peak ? b : peak;
            }
            return peak; // (also the bound of the stored words before the store's reduction)
        }
        constexpr bool fwd_dense_admits(u64 p, int logn)
        {
            // (p below 2^60 in every shape although 14p would allow a little more: the stored words, below 2p, are operands of
            //  the carry-free dot products of section 3, which take words below 2^61)
            return logn >= kMinHalfLogn && logn <= kMaxHalfLogn && p < (u64(1) << 60) &&
                   small_quot_admits(p, fwd_dense_peak_mult(logn)) && static_cast<u128>(fwd_dense_peak_mult(logn)) * p <= kWord;
        }
        static_assert(fwd_dense_peak_mult(14) == 14 && fwd_dense_peak_mult(15) == 14 && fwd_dense_peak_mult(16) == 16,
                      "dense forward schedule: 14p after round 1, at most 16p after the final round at N = 2^16");

        // ---- 2c. Forward transform without its last layer (kNttSplitLast): each half-row workgroup
        // runs the log n - 1 layers of a ring of N/2 on one parity class of the gathered row (inputs below 2p, as above), so
        // E[j], O[j] are below fwd_split_output_mult(log n) p = (2 + g (log n - 1)) p with the approximate quotient (the exact
        // instance grows by 2p per layer and lies below that). The consumer (ks_mac_pair_kernel) finishes the pair:
        // T = the exact lazy Shoup product of O[j] (any 64-bit word) by psi^brev(N/2 + j), below 2p; X0 = E + T and
        // X1 = E - T + 2p, both below (fwd_split_output_mult + 2) p, which must stay below 2^64 -- and the 128-bit sums of nd
        // products of such words with key words below p must stay below 2^128: nd p < 2^64.
        constexpr int fwd_split_output_mult(int logn)
        {
            return 2 + kFwdApxGrowth * (logn - 1);
        }
        constexpr u128 fwd_split_peak(int logn, u64 p) // the largest word the split form makes, pair butterfly included
        {
            return fwd_int_peak(logn - 1, p, 2, true, true) + static_cast<u128>(2) * p;
        }
        constexpr int fwd_split_prime_bits(int logn)
        {
            int bits = 0;
            for (int b = 1; b <= kMaxPrimeBits; b++)
                if (fwd_split_peak(logn, max_prime_of_bits(b)) < kWord)
                    bits = b;
            return bits;
        }
        static_assert(kFwdApxLevel != 2 || (fwd_split_prime_bits(14) == 58 && fwd_split_prime_bits(15) == 58 && fwd_split_prime_bits(16) == 58),
                      "split form at level 2: 56p / 60p / 64p at log n = 14 / 15 / 16, below 2^64 for primes below 2^58");
        constexpr bool fwd_split_admits(u64 p, int logn, int nd)
        {
            return logn >= kMinHalfLogn && logn <= kMaxHalfLogn && nd >= 1 && p <= max_prime_of_bits(fwd_split_prime_bits(logn)) &&
                   static_cast<u128>(nd) * p < kWord;
        }

        // =====================================================================================================
        // 3. Tensor product formed by the inverse transform's load (dyadic_redc in ntt.hip): t = (sum of NP products) *
        // 2^-64 mod p as ONE Montgomery reduction, t < sum / 2^64 + p. Carry-free accumulation needs operands below 2^61
        // (upper halves below 2^29: the middle accumulator holds 2 NP products below 2^61 each, NP <= 2). For the inverse
        // transform's inputs t must be below 2p: sum / 2^64 <= p.
        constexpr bool tensor_redc_ok(u64 p, int operand_mult, int np)
        {
            const u128 ob = static_cast<u128>(operand_mult) * p; // operands below operand_mult * p, i.e. at most ob - 1
            if (ob > (static_cast<u128>(1) << 61) || np > 2)
                return false;
            // sum <= np (ob - 1)^2 < 2^123; t < sum / 2^64 + p, so t < 2p as soon as sum <= p 2^64 (< 2^125): exact in u128
            return (ob - 1) * (ob - 1) * np <= static_cast<u128>(p) * kWord;
        }
        // operands below 4p (what the lazy forward transform stores) for primes below 2^59 ...
        constexpr int tensor_prime_bits(int operand_mult)
        {
            int bits = 0;
            for (int b = 1; b <= kMaxPrimeBits; b++)
                if (tensor_redc_ok(max_prime_of_bits(b), operand_mult, 2))
                    bits = b;
            return bits;
        }
        constexpr int kTensorPrimeBits4p = tensor_prime_bits(4);
        constexpr int kTensorPrimeBits2p = tensor_prime_bits(2);
        static_assert(kTensorPrimeBits4p == 59, "fused tensor product on [0, 4p) operands: ciphertext primes below 2^59");
        static_assert(kTensorPrimeBits2p == 60, "... on [0, 2p) operands (kNttReduceOut rows): the 60-bit Bsk primes");
        constexpr bool tensor_admits_4p(u64 p)
        {
            return p <= max_prime_of_bits(kTensorPrimeBits4p);
        }
        constexpr bool tensor_admits_2p(u64 p)
        {
            return p <= max_prime_of_bits(kTensorPrimeBits2p);
        }
        // ... and on what an approximate-quotient forward launch WITHOUT kNttAnyRep stores (op_bfv_multiply's q rows when the
        // tensor product is fused: the last layer keeps its Barrett step, outputs below (2 + g) p, section 2)
        constexpr int kTensorPrimeBitsApx = tensor_prime_bits(fwd_apx_output_mult(kMaxHalfLogn, false));
        static_assert(kTensorPrimeBitsApx == (kFwdApxLevel == 2 ? 57 : 58), "fused tensor product on approximate-quotient rows");
        constexpr bool tensor_admits_apx(u64 p)
        {
            return p <= max_prime_of_bits(kTensorPrimeBitsApx);
        }

        // =====================================================================================================
        // 4. FP64 instances (primes below 2^50; devmath.hpp fp_mulmod / fp_reduce). With u = 2^-53 the unit roundoff:
        //   h = fl(y w), l = y w - h exactly (|l| <= u |y w|); t = fl(h * fl(1/p)) = (h / p)(1 + e), |e| <= 2u + u^2;
        //   q = rint(t) (|q - t| <= 1/2; for |t| >= 2^52 t is an integer already); r = (h - q p) + l.
        //   |h - q p| <= |h| |e| + p / 2 and |l| <= u |h|(1 + u), so
        //       |r| <= p / 2 + 3 u |y| w (1 + 2^-50)  <=  (1/2 + 3 * 2^-53 |y|) p        (+ the tiny slack below)
        // -- NOT (1/2 + 2^-52 |y|) p as round 2 assumed: the exact rounding error l and the rounding of h * (1/p) add up
        // (p = 1125899886395393, y = 3857024279003347, w = 1125899289087767 gives |r| / p = 1.4006 against 1.3564).
        // h - q p and the final sum are integers: exact as long as they stay below 2^53 in magnitude.
        // A forward layer therefore takes a bound B (on every value) to B + (1/2 + 3 * 2^-53 B) p; with p <= U = 2^50 that
        // is 1.375 B + U / 2: from a reduction (B = U / 2) FIVE layers stay below 8 U = 2^53 (1.19, 2.13, 3.43, 5.22,
        // 7.68), the sixth does not (11.06). Round 2's schedule had two spans of six layers.
        constexpr long double kFpSlack = 1.0L + 0x1p-40L;
        constexpr long double fp_mul_bound(long double y, long double p) // |fp_mulmod(y, w, p)| for |y| <= y, 0 <= w < p
        {
            return 0.5L * p + 3.0L * 0x1p-53L * y * p * kFpSlack;
        }
        constexpr long double fp_reduce_bound(long double x, long double p) // |fp_reduce(x)| for |x| <= x < 2^53
        {
            return 0.5L * p + x * 0x1p-51L + 1.0L;
        }
        // Forward schedule (ntt_fwd_half_kernel<.., STRICT = 3>): the top layer on raw inputs (below in_bound: 2^52 for
        // gathered words, p for residues), all values reduced; then the T = log n - 1 on-chip layers i = 0 .. T - 1
        // (rounds 1-3: four each, final round: the rest), all 32 values of a lane reduced BEFORE layers 5 and 10; the store
        // canonicalises (a reduction of values below 2^53).
        constexpr bool fp_fwd_reduce_before_layer(int i)
        {
            return i == 5 || i == 10;
        }
        constexpr long double fp_fwd_peak(int logn, long double p, long double in_bound)
        {
            long double b = in_bound, peak = in_bound;
            // top layer: u + r, u - r with r = fp_mulmod(y, w)
            b = b + fp_mul_bound(b, p);
            peak = b > peak ? b : peak;
            b = fp_reduce_bound(b, p);
            for (int i = 0; i < logn - 1; i++)
            {
                if (fp_fwd_reduce_before_layer(i))
                    b = fp_reduce_bound(b, p);
                b = b + fp_mul_bound(b, p);
                peak = b > peak ? b : peak;
            }
            return peak; // (the canonicalisation reads values up to `peak`)
        }
        // Inverse schedule (ntt_inv_half_kernel<.., LZ = 2>): Gentleman-Sande layers l = 0 .. T - 1 on inputs below 2p,
        // u' = u + y (the bound doubles), y' = fp_mulmod(u - y, w); both outputs reduced after layers l % 4 == 1 except the
        // last on-chip layer (whose outputs the store, or the whole-row form's top layer, takes as they are).
        constexpr bool fp_inv_reduce_after_layer(int T, int l)
        {
            return l % 4 == 1 && l != T - 1;
        }
        constexpr long double fp_inv_peak(int T, long double p)
        {
            long double b = 2.0L * p, peak = b;
            for (int l = 0; l < T; l++)
            {
                const long double s = 2.0L * b; // |u + y|, |u - y| <= 2b
                peak = s > peak ? s : peak;
                const long double r = fp_mul_bound(s, p);
                b = s > r ? s : r;
                if (fp_inv_reduce_after_layer(T, l))
                    b = fp_reduce_bound(b, p);
            }
            return peak;
        }
        constexpr int fp_prime_bits()
        {
            int bits = 0;
            for (int b = kMaxHalfLogn + 2; b <= 52; b++)
            {
                bool ok = true;
                for (int logn = kMinHalfLogn; logn <= kMaxHalfLogn; logn++)
                {
                    const long double p = static_cast<long double>(max_ntt_prime_of_bits(b, logn));
                    ok = ok && fp_fwd_peak(logn, p, 0x1p52L) < kFpLimit;
                    ok = ok && fp_inv_peak(logn - 1, p) < kFpLimit; // half-row form
                    if (logn <= 15)
                        ok = ok && fp_inv_peak(logn, p) < kFpLimit; // whole-row form (N = 2^14, 2^15)
                }
                if (ok)
                    bits = b;
            }
            return bits;
        }
        constexpr int kFpPrimeBits = fp_prime_bits();
        static_assert(kFpPrimeBits == 50, "FP64 instances: primes below 2^50 (and raw inputs below 2^52)");
        constexpr u64 kFpInputBound = u64(1) << 52; // raw words a forward FP64 launch may be handed (fp_from_u64's range too)
        constexpr bool fp_admits(u64 p)
        {
            return p <= max_prime_of_bits(kFpPrimeBits);
        }
        // =====================================================================================================
        // 5. Carry-free 128-bit dot products of the BEHZ kernels (devmath.hpp DotAcc<NTERMS>): sum_i t_i c_i with every
        // partial product in a 64-bit accumulator that is only assembled at the end. With operands below 2^bits
        // (t = t1 2^32 + t0, t0 = t01 2^16 + t00; c = c1 2^32 + c0): l0 += t00 c0 and l1 += t01 c0 (below 2^48 each), h +=
        // t1 c1 (below 2^(2 bits - 64)), and NM = (2 NTERMS + 7) / 8 middle accumulators that take the 2 NTERMS products
        // t0 c1, t1 c0 (below 2^(bits)) round-robin -- at most ceil(2 NTERMS / NM) each. Every accumulator must stay below 2^64.
        constexpr bool dotacc_ok(int nterms, int bits)
        {
            if (nterms < 1 || bits < 33 || bits > 64)
                return false;
            const u128 lim = kWord;
            const int nm = (2 * nterms + 7) / 8;
            const int per_m = (2 * nterms + nm - 1) / nm;
            const u128 low = static_cast<u128>(nterms) << 48;                  // l0, l1
            const u128 mid = static_cast<u128>(per_m) << bits;                 // t0 c1 < 2^32 2^(bits-32)
            const u128 high = static_cast<u128>(nterms) << (2 * (bits - 32));  // t1 c1
            return low <= lim && mid <= lim && high <= lim;
        }
        constexpr int kDotAccOperandBits = 61; // SEAL_MOD_BIT_COUNT_MAX: residues and constants of every prime the context admits
        constexpr int dotacc_max_terms()
        {
            int n = 0;
            for (int t = 1; t <= 4096; t++)
                if (dotacc_ok(t, kDotAccOperandBits))
                    n = t;
                else
                    break;
            return n;
        }
        static_assert(dotacc_max_terms() >= 64, "DotAcc on 61-bit operands: at least 64 terms (the kernels use up to k + 2 <= 34)");
        // The form the exact-k BEHZ instances use (dotacc.hpp DotAcc31<NTERMS>): both factors split at bit 31 (t = t1 2^31 + t0,
        // c = c1 2^31 + c0, low halves below 2^31 and high halves below 2^(bits - 31)), four products per term, dealt
        // round-robin: t0 c0 (below 2^62) over NL accumulators, the 2 NTERMS cross products (below 2^bits) over NM, t1 c1
        // (below 2^(2 bits - 62)) over NH. Every accumulator must stay below 2^64 and the assembled sum below 2^128.
        constexpr int dotacc31_nl(int nterms) { return (nterms + 3) / 4; }
        constexpr int dotacc31_nm(int nterms) { return (2 * nterms + 7) / 8; }
        constexpr int dotacc31_nh(int nterms) { return (nterms + 15) / 16; }
        constexpr bool dotacc31_ok(int nterms, int bits)
        {
            if (nterms < 1 || nterms > 64 || bits < 32 || bits > 62)
                return false;
            const u128 lim = kWord;
            const int nl = dotacc31_nl(nterms), nm = dotacc31_nm(nterms), nh = dotacc31_nh(nterms);
            const u128 low = static_cast<u128>((nterms + nl - 1) / nl) << 62;
            const u128 mid = static_cast<u128>((2 * nterms + nm - 1) / nm) << bits;
            const u128 high = static_cast<u128>((nterms + nh - 1) / nh) << (2 * (bits - 31));
            // the sum itself: nterms products below 2^(2 bits)
            const bool sum_fits = 2 * bits + 6 <= 128;
            return low <= lim && mid <= lim && high <= lim && sum_fits;
        }
        constexpr bool dotacc31_all_ok(int max_terms)
        {
            for (int t = 1; t <= max_terms; t++)
                if (!dotacc31_ok(t, kDotAccOperandBits))
                    return false;
            return true;
        }
        // The same form with the split position S as a parameter (dotacc.hpp DotAccSplit<S, ...>): t = t1 2^S + t0 and
        // c = c1 2^S + c0. A dot product is described by the widths of its operand classes: the per-lane factor of term 0
        // (below 2^first_bits), the per-lane factors of the other terms (below 2^lane_bits) and the wave-uniform constants
        // (below 2^const_bits). An operand below 2^w has a low part of at most 2^min(w, S) - 1 and a high part of at most
        // 2^(w - S) - 1, both reached by 2^w - 1. The products are dealt as DotAccSplit::add deals them: t0 c0 of term i to
        // L[i % NL], t0 c1 to M[2i % NM], t1 c0 to M[(2i + 1) % NM], t1 c1 to H[i % NH].
        struct DotShape
        {
            int nterms, first_bits, lane_bits, const_bits;
        };
        constexpr u128 split_lo_max(int bits, int s) { return (static_cast<u128>(1) << (bits < s ? bits : s)) - 1; }
        constexpr u128 split_hi_max(int bits, int s) { return bits > s ? (static_cast<u128>(1) << (bits - s)) - 1 : 0; }
        constexpr bool dotsplit_shape_ok(int s, const DotShape &d)
        {
            // both halves of every operand are 32-bit words (one v_mad_u64_u32 per product)
            return s >= 1 && s <= 32 && d.nterms >= 1 && d.nterms <= 64 && d.first_bits >= 1 && d.lane_bits >= 1 &&
                   d.const_bits >= 1 && d.first_bits - s <= 32 && d.lane_bits - s <= 32 && d.const_bits - s <= 32;
        }
        // part 0, 1, 2 = L, M, H: the worst-case sum of every one of the part's `count` accumulators stays below 2^64
        constexpr bool dotsplit_part_fits(int s, const DotShape &d, int part, int count)
        {
            if (!dotsplit_shape_ok(s, d) || count < 1 || count > 2 * d.nterms)
                return false;
            const u128 c0 = split_lo_max(d.const_bits, s), c1 = split_hi_max(d.const_bits, s);
            for (int a = 0; a < count; a++)
            {
                u128 sum = 0;
                for (int i = 0; i < d.nterms; i++)
                {
                    const int w = i == 0 ? d.first_bits : d.lane_bits;
                    const u128 t0 = split_lo_max(w, s), t1 = split_hi_max(w, s);
                    if (part == 0 && i % count == a)
                        sum += t0 * c0;
                    if (part == 1 && (2 * i) % count == a)
                        sum += t0 * c1;
                    if (part == 1 && (2 * i + 1) % count == a)
                        sum += t1 * c0;
                    if (part == 2 && i % count == a)
                        sum += t1 * c1;
                }
                if (sum > kWord - 1)
                    return false;
            }
            return true;
        }
        // the fewest accumulators of a part that fit (0: the shape is not admitted at all)
        constexpr int dotsplit_count(int s, const DotShape &d, int part)
        {
            for (int n = 1; n <= 2 * d.nterms; n++)
                if (dotsplit_part_fits(s, d, part, n))
                    return n;
            return 0;
        }
        // the assembled sum: nterms products of the operands themselves, below 2^128
        constexpr bool dotsplit_total_fits(const DotShape &d)
        {
            if (d.first_bits + d.const_bits > 126 || d.lane_bits + d.const_bits > 126)
                return false;
            const u128 c = (static_cast<u128>(1) << d.const_bits) - 1;
            const u128 first = ((static_cast<u128>(1) << d.first_bits) - 1) * c;
            const u128 other = ((static_cast<u128>(1) << d.lane_bits) - 1) * c;
            u128 sum = first;
            for (int i = 1; i < d.nterms; i++)
            {
                if (other > ~static_cast<u128>(0) - sum)
                    return false;
                sum += other;
            }
            return true;
        }
        // THE predicate: a dot product of shape d, accumulated at split s in (nl, nm, nh) accumulators, never wraps
        constexpr bool dotsplit_ok(int s, const DotShape &d, int nl, int nm, int nh)
        {
            return dotsplit_part_fits(s, d, 0, nl) && dotsplit_part_fits(s, d, 1, nm) && dotsplit_part_fits(s, d, 2, nh) &&
                   dotsplit_total_fits(d);
        }
        // split at 31 on 61-bit operands throughout is DotAcc31: the derived counts are the closed forms above
        constexpr bool dotsplit31_matches(int max_terms)
        {
            for (int t = 1; t <= max_terms; t++)
            {
                const DotShape d{ t, kDotAccOperandBits, kDotAccOperandBits, kDotAccOperandBits };
                if (dotsplit_count(31, d, 0) != dotacc31_nl(t) || dotsplit_count(31, d, 1) != dotacc31_nm(t) ||
                    dotsplit_count(31, d, 2) != dotacc31_nh(t) || !dotsplit_total_fits(d))
                    return false;
            }
            return true;
        }
        static_assert(dotsplit31_matches(34), "DotAccSplit<31> on 61-bit operands has DotAcc31's accumulators");
        // The dot products of the exact-k BEHZ instances (rns.hip) and their operand classes, for ciphertext primes below
        // 2^qb and auxiliary primes (the base Bsk) below 2^bb:
        //   t[i]   lift and floor: a canonical Shoup product modulo q_i                                  below 2^qb
        //   temp   lift, term 0: the centred r_m_tilde, below 2^31 or 2^32 - r below b_j (bb >= 32)       below 2^bb
        //   x      floor Bsk rows, term 0: before_top<true> leaves it below 2 b_j, NOT canonical          below 2^(bb + 1)
        //   tb[j]  floor: a canonical REDC modulo b_j                                                     below 2^bb
        //   a2     floor q rows, term 0: min(alpha, m_sk - alpha), at most m_sk / 2                       below 2^bb
        //   constants: host-folded Montgomery forms, canonical modulo the row's prime: below 2^bb on the Bsk rows and in
        //              conv_sk (modulo m_sk), below 2^qb on the q rows
        // kind 0: lift row {temp, t[0..k-1]} x b_j;  1: floor Bsk row {x, t[0..k-1]} x b_j;  2: conv_sk {tb[0..k]} x m_sk (an
        // instance holds k + 1 terms; a level with |B| = k adds k of them);  3: floor q row {a2, tb[0..k]} x q_i
        constexpr int kBehzDotKinds = 4;
        constexpr DotShape behz_dot_shape(int kind, int k, int qb, int bb)
        {
            return kind == 0   ? DotShape{ k + 1, bb, qb, bb }
                   : kind == 1 ? DotShape{ k + 1, bb + 1, qb, bb }
                   : kind == 2 ? DotShape{ k + 1, bb, bb, bb }
                               : DotShape{ k + 2, bb, bb, qb };
        }
        // The widths the S = 30 instances are built for: auxiliary primes are 60-bit (engine.cpp get_primes(n, 60, ...)),
        // ciphertext primes below 2^59, the widest the fused tensor path takes (pipeline.cpp plan_bfv_multiply). Up to k = 8
        // and from k = 12 on the accumulators are the ones 58-bit primes would get; k = 9, 10, 11 pay one more cross
        // accumulator for the last bit. At S = 31 the instances keep 61 bits throughout.
        constexpr int kSplit30QBits = 59, kSplit30BBits = 60;
        constexpr DotShape behz_built_shape(int s, int kind, int k)
        {
            return s == 30 ? behz_dot_shape(kind, k, kSplit30QBits, kSplit30BBits)
                           : DotShape{ kind == 3 ? k + 2 : k + 1, kDotAccOperandBits, kDotAccOperandBits, kDotAccOperandBits };
        }
        constexpr int bit_width(u64 v)
        {
            int b = 0;
            while (v)
            {
                b++;
                v >>= 1;
            }
            return b;
        }
        // Selection (engine.cpp, per level): the instances of split s, with the accumulators they were built with, admit
        // a level whose largest ciphertext prime is max_q and whose largest auxiliary prime is max_b
        constexpr bool behz_split_admits(int s, int k, u64 max_q, u64 max_b)
        {
            const int qb = bit_width(max_q), bb = bit_width(max_b);
            if (k < 1 || k > 15 || bb < 32) // (temp's class; kBehzExactMaxK, section 7)
                return false;
            for (int kind = 0; kind < kBehzDotKinds; kind++)
            {
                const DotShape built = behz_built_shape(s, kind, k), have = behz_dot_shape(kind, k, qb, bb);
                if (!dotsplit_ok(s, have, dotsplit_count(s, built, 0), dotsplit_count(s, built, 1), dotsplit_count(s, built, 2)))
                    return false;
            }
            return true;
        }
        constexpr int behz_select_split(int k, u64 max_q, u64 max_b) { return behz_split_admits(30, k, max_q, max_b) ? 30 : 31; }
        constexpr bool behz_split_all_ok(int s, u64 max_q, u64 max_b)
        {
            for (int k = 1; k <= 15; k++)
                if (!behz_split_admits(s, k, max_q, max_b))
                    return false;
            return true;
        }
        static_assert(behz_split_all_ok(30, (u64(1) << kSplit30QBits) - 1, (u64(1) << kSplit30BBits) - 1),
                      "S = 30: every dot product of every exact-k instance (term counts up to k + 2 = 17) at the widths it is built for");
        static_assert(behz_split_all_ok(31, (u64(1) << 60) - 1, (u64(1) << 60) - 1),
                      "S = 31 serves every level the context admits: x below 2^61, everything else below 2^60");
        // one accumulator per part is what the split at 30 buys at the headline level (k = 7 and 8, |B| = k + 1 at most)
        static_assert(dotsplit_count(30, behz_built_shape(30, 1, 7), 0) == 1 && dotsplit_count(30, behz_built_shape(30, 1, 7), 1) == 1 &&
                          dotsplit_count(30, behz_built_shape(30, 1, 7), 2) == 1 && dotsplit_count(30, behz_built_shape(30, 3, 7), 1) == 1,
                      "k = 7 at S = 30: single accumulators");
        // 60-bit ciphertext primes put 2 (k + 1) + 1 cross products of 2^60 into the floor rows' one M accumulator: refused
        // from k = 7 on, where S = 31 is selected
        static_assert(!behz_split_admits(30, 7, (u64(1) << 60) - 1, (u64(1) << 60) - 1) &&
                          behz_split_admits(30, 7, (u64(1) << 59) - 1, (u64(1) << 60) - 1),
                      "the edge of S = 30 at k = 7 lies between 59- and 60-bit ciphertext primes");

        // =====================================================================================================
        // 6. Small quotients estimated in single precision (devmath.hpp reduce_small_quot): for a word x below M p the
        // quotient estimate is q' = trunc(fl(fl(x >> 32) * c)) with c = fl32(fl64(2^32 / p) (1 - 2^-20)); the reduced value
        // x - q' p must land in [0, 2p), i.e. q' in {floor(x / p) - 1, floor(x / p)}.
        //   * never too large: with e = 2^-24 the unit roundoff, fl(x >> 32) <= (x / 2^32)(1 + e), c <= (2^32 / p)(1 - 2^-20)
        //     (1 + 2^-52)(1 + e), and the product rounds once more: q' <= (x / p)(1 - 2^-20)(1 + e)^3 (1 + 2^-52) < x / p.
        //   * at most one short: fl(x >> 32) >= ((x - 2^32) / 2^32)(1 - e) drops the low half (less than 2^32 / p of
        //     quotient), every rounding loses at most e relatively and the bias 2^-20: x / p - q'real < 2^32 / p +
        //     M (2^-20 + 3 e + 2^-51) =: loss(M, p); trunc loses less than one more. loss < 1 makes q' >= floor(x / p) - 1.
        // Admission: loss(M, p) <= 1/2 (a factor two of margin), which needs p >= 2^33 and M <= 2^18; the launchers ask for
        // M <= 128 and p >= 2^45 (the hi word must also fit single precision's exponent range trivially, and M p < 2^64).
        constexpr bool small_quot_admits(u64 p, int mult)
        {
            if (p < kSmallQuotMinPrime || mult < 1 || mult > 128 || static_cast<u128>(mult) * p > kWord)
                return false;
            const long double loss = 0x1p32L / static_cast<long double>(p) +
                                     static_cast<long double>(mult) * (0x1p-20L + 3 * 0x1p-24L + 0x1p-51L);
            return loss <= 0.5L;
        }

        // =====================================================================================================
        // 7. The fused BEHZ kernels' Montgomery reductions (rns.hip bfv_lift2_kernel / bfv_floor_sk2_kernel, devmath.hpp
        // redc128 + redc_finish). A REDC of acc = sum_i x_i c_i modulo p, with every constant c_i < p (host-folded
        // Montgomery forms) and every variable factor x_i < X_i, returns (acc + m p) / 2^64 with m < 2^64, so it lands below
        // acc / 2^64 + p < p (sum_i X_i / 2^64 + 1): below 2p whenever S = sum_i X_i <= 2^64. The sums, per stage:
        //   lift Bsk rows:   k terms t_i < q_i, plus temp < b_j (the centred r_m_tilde)            S <= k max_q + max_b
        //   floor Bsk rows:  k terms < q_i, plus the Bsk input < 2 b_j (a lazy value when the inverse NTT deferred its
        //                    top layer)                                                                S <= k max_q + 2 max_b
        //   conv_sk:         B terms tb_j < b_j                                                        S <= B max_b
        //   floor q rows:    B terms tb_j < b_j, plus the alpha term < m_sk                            S <= (B + 1) max_b
        // where max_q bounds the level's k ciphertext primes and max_b the |Bsk| = B + 1 auxiliary ones. The first two
        // are dominated by s1 = k max_q + 2 max_b, the last two by s2 = (B + 1) max_b. When this holds the exact-k
        // instances skip redc_finish's second reduction (RnsDev::redc_small); otherwise the generic instance keeps it.
        constexpr bool behz_redc_small(int k, int B, u64 max_q, u64 max_b)
        {
            const u128 s1 = static_cast<u128>(k) * max_q + 2 * static_cast<u128>(max_b);
            const u128 s2 = static_cast<u128>(B + 1) * max_b;
            return k >= 1 && B >= 1 && s1 <= kWord && s2 <= kWord;
        }
        // max_b is m_sk, the largest 60-bit prime = 1 (mod 2N) (engine.cpp: get_primes(n, 60, ...)), within 2^55 of 2^60 at
        // every ring size: s2 at |B| = 16 is then above 2^64, so no level with k >= 16 (|B| >= k) has an exact-k instance
        static_assert(!behz_redc_small(15, 16, u64(1) << 40, (u64(1) << 60) - (u64(1) << 55)),
                      "s2 at |B| = 16 for every m_sk");
        constexpr int kBehzExactMaxK = 15; // the largest k with an exact-k BEHZ instance (rns.hip)
        static_assert(dotacc31_all_ok(kBehzExactMaxK + 2),
                      "DotAcc31 on 61-bit operands: every term count of the exact-k instances (up to k + 2)");

        // =====================================================================================================
        // 8. The ciphertext inner product's plain 128-bit sums (poly.hip tensor_dot_kernel). One launch
        // accumulates a group of `terms` tensor products with mac128 and reduces once per output word. The widest sum is
        // c_1: two products per term, each below 2^(2 bits) for operands below 2^bits, plus the canonical partial sum of
        // the groups before it (below 2^bits). It must stay below 2^128.
        // The kernel's operands are canonical residues of primes below 2^61 (SEAL_MOD_BIT_COUNT_MAX): CKKS operands as the
        // caller hands them over, BFV operands after the kernel's own reduction on load (any 64-bit word is accepted there).
        constexpr bool dot_group_admits(int terms, int bits)
        {
            if (terms < 1 || bits < 1 || bits > 63)
                return false;
            // 2 terms 2^(2 bits) + 2^bits <= 2^128 - 1, in units that fit u128: divide by 2^bits
            const int shift = 128 - bits; // (2 terms 2^bits + 1) 2^bits < 2^128  <=>  2 terms 2^bits + 1 <= 2^shift
            if (shift <= bits)
                return false;
            return (static_cast<u128>(2 * terms) << bits) + 1 <= (static_cast<u128>(1) << shift);
        }
        constexpr int kDotGroupTerms = 16; // terms per launch of tensor_dot_kernel
        static_assert(dot_group_admits(kDotGroupTerms, kDotAccOperandBits), "16 terms of 61-bit operands fit 128 bits");
        static_assert(dot_group_admits(31, kDotAccOperandBits) && !dot_group_admits(32, kDotAccOperandBits),
                      "this (conservative) count admits 31 terms at 61 bits: the group of 16 leaves almost a factor two");
        // The linear combination's sums (poly.hip lincomb_kernel): one launch accumulates a group of
        // `terms` products weight * word, each below 2^(2 bits) for operands and weights below 2^bits, then adds the canonical
        // partial sum of the groups before it and the constant (each below 2^bits), and reduces once. It must stay below 2^128.
        constexpr bool lincomb_group_admits(int terms, int bits)
        {
            if (terms < 1 || bits < 1 || bits > 63)
                return false;
            // terms 2^(2 bits) + 2 2^bits <= 2^128 - 1  <=>  (terms 2^bits + 2) 2^bits < 2^128  <=>  terms 2^bits + 2 <= 2^shift
            const int shift = 128 - bits;
            if (shift <= bits)
                return false;
            return (static_cast<u128>(terms) << bits) + 2 <= (static_cast<u128>(1) << shift);
        }
        constexpr int kLinGroupTerms = 16; // terms per launch of lincomb_kernel
        constexpr int kLinTileSums = 4;    // sums per launch (every sum has its own pair of 128-bit accumulators)
        static_assert(lincomb_group_admits(kLinGroupTerms, kDotAccOperandBits), "16 products of 61-bit words fit 128 bits");
        static_assert(lincomb_group_admits(63, kDotAccOperandBits) && !lincomb_group_admits(64, kDotAccOperandBits),
                      "this (conservative) count admits 63 terms at 61 bits: the group of 16 leaves almost a factor four");
        // The sums against plaintext rows (poly.hip dot_plain_kernel): a group of `terms` products
        // ciphertext word * plaintext word of canonical residues, then the canonical partial sum, and no constant -- at most
        // terms 2^(2 bits) + 2^bits, below what lincomb_group_admits bounds. The kernel uses the same group and tile; its
        // launcher asserts the predicate, and tests/dot_plain_bounds_check.cpp runs the sum on the CPU.
        static_assert(lincomb_group_admits(kLinGroupTerms, kDotAccOperandBits), "dot_plain_kernel's group of 61-bit words fits 128 bits");
        // The sums over terms at their own level and size (poly.hip lincomb_levels_kernel): the same
        // arithmetic per output word, so the same group and the same predicate. The tile is a constant of its own because the
        // per-term strides add uniform state to a kernel family that must not spill (the register table of section 21).
        constexpr int kLinLevelsTileSums = 4;
        static_assert(kLinLevelsTileSums >= 1 && kLinLevelsTileSums <= kLinTileSums,
                      "the levels kernel is instantiated for 1 .. kLinLevelsTileSums sums and never for more than lincomb_kernel");

        // =====================================================================================================
        // 9. The merged mod-down and rescale's conversion sum (keyswitch.hip ks_moddown_rescale_pre_kernel, DESIGN.md section
        // 19): per kept prime, `dropped` products z_d * hat_d of canonical residues, the quotient v <= dropped times a
        // canonical residue, and one canonical residue, accumulated with mac128 and reduced once. With every residue at most
        // m = 2^bits - 1 the sum is at most dropped m^2 + (dropped + 1) m; it must stay below 2^128.
        constexpr bool ks_rescale_sum_fits(int dropped, int bits)
        {
            if (dropped < 1 || bits < 1 || bits > 63)
                return false;
            const u128 m = (static_cast<u128>(1) << bits) - 1, max = ~static_cast<u128>(0);
            const u128 tail = static_cast<u128>(dropped + 1) * m; // (below 2^71)
            return static_cast<u128>(dropped) <= (max - tail) / (m * m);
        }
        static_assert(ks_rescale_sum_fits(64, kDotAccOperandBits) && !ks_rescale_sum_fits(65, kDotAccOperandBits),
                      "the last prime and up to 63 special primes of 61 bits: 64 dropped primes fit, 65 would not");

        // =====================================================================================================
        // 10. The external product's inner product (rgsw.hip ext_mac_kernel / ext_mac_items_kernel):
        // `terms` products digit word * key word accumulated with mac128 and reduced once. A key word is a canonical
        // residue (at most pmax - 1); a digit word is whatever representative ks_digits stored, below 2^rep_bits. The split
        // form reduces after the first half and carries that canonical residue into the second, so one more word of at
        // most pmax - 1 is counted -- for the unsplit sum it is slack. The sum must stay below 2^128.
        // The key switch's own argument ("words below 2^64 and nd p < 2^64") is this predicate at terms = nd and
        // rep_bits = 64; the external product has 2 nd terms, where it fails first for 61-bit primes: 2 nd > 8.
        constexpr int kKsDigitRepBits = 64; // ks_digits transforms the digit rows with kNttAnyRep: any 64-bit word
        constexpr bool ext_mac_sum_fits(int terms, u64 pmax, int rep_bits)
        {
            if (terms < 1 || pmax < 2 || rep_bits < 1 || rep_bits > 64)
                return false;
            const u128 x = max_prime_of_bits(rep_bits), k = pmax - 1, max = ~static_cast<u128>(0);
            return static_cast<u128>(terms) <= (max - k) / (x * k); // terms x k + k <= 2^128 - 1
        }
        static_assert(ext_mac_sum_fits(8, max_prime_of_bits(61), kKsDigitRepBits) && !ext_mac_sum_fits(9, max_prime_of_bits(61), kKsDigitRepBits),
                      "61-bit primes: eight terms in one sum (nd <= 4 unsplit, nd <= 8 in two halves)");
        static_assert(ext_mac_sum_fits(16, max_prime_of_bits(60), kKsDigitRepBits) && !ext_mac_sum_fits(17, max_prime_of_bits(60), kKsDigitRepBits),
                      "60-bit primes: sixteen terms, every instance of the items family unsplit");
    } // namespace bounds
} // namespace sealhip
