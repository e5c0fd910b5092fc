// homdft_plan.hpp -- the plan of the homomorphic DFT of CKKS bootstrapping: CoeffToSlot and SlotToCoeff
// as a few baby-step/giant-step matrix-vector products, each a run of consecutive layers of the encoder's special FFT. Host
// code with no HIP dependency: sealhip_dft_* (api.cpp, homdft.cpp) and the stand-alone tests/homdft_plan_check.cpp include this
// very header, and tests/homdft_ref.py restates it from the layer matrices.
//
// With n = N/2 slots, L = log2 n and zeta = exp(i pi / N), the slot values of m(X) are z = U w, U[j][t] = zeta^((5^j mod 2N) t),
// w_t = m_t + i m_(t+n), and U = F_L ... F_1 R with R the bit reversal and F_s the butterfly layer of span 2^s
//     a = v[b+j], c = v[b+j+h] omega_(s,j):  v[b+j] = a + c, v[b+j+h] = a - c      (h = 2^(s-1), j < h),
//     omega_(s,j) = exp(2 pi i (5^j mod 4 2^s) / (4 2^s)),    F_s^-1 = F_s^H / 2.
// CoeffToSlot applies F_1^-1 ... F_L^-1 (top layer first), SlotToCoeff F_L ... F_1 (bottom layer first); the bit reversal is
// dropped on both sides. A STAGE is r consecutive layers s0 .. s0+r-1 multiplied together: its non-zeros M[i][col] have
// col - i = c h0 (h0 = 2^(s0-1)) for a signed c in (-2^r, 2^r), i and col in one aligned block of 2^r h0, and
//     M v = sum_c diag_c (.) rot_(c h0 mod n)(v),    diag_c[i] = M[i][i + c h0]  (zero outside the block).
// The stage that holds the top layer has 2^r h0 = n: c and c + 2^r name the same rotation and are FOLDED into c mod 2^r.
// BSGS: c = c_g n_baby + c_b, 0 <= c_b < n_baby; cell [g][b] of the table holds diag_c rotated by minus the giant step
// (rot_s moves slot j+s to slot j), the one cell c = -2^r of an unfolded stage is a zero plaintext.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace sealhip
{
    namespace dftplan
    {
        using u64 = unsigned long long; // (the engine's word type)
        constexpr std::uint32_t kCoeffsToSlots = 0, kSlotsToCoeffs = 1;

        struct Stage
        {
            std::uint32_t s0 = 0, r = 0, h0 = 0; // layers s0 .. s0+r-1, h0 = 2^(s0-1)
            std::uint32_t level = 0;             // of the stage's input; its output is one below
            std::uint32_t n_baby = 0, n_giant = 0;
            bool folded = false;                 // holds the top layer: 2^r diagonals, no empty cell
            double scale = 0;                    // of its plaintexts: (double) q_(level-1), the prime its rescale drops
            std::vector<std::int32_t> baby, giant; // rotation steps in [0, n), 0 the identity
            // signed giant coefficient of row g: the giant step is c_g n_baby h0 mod n
            std::int64_t giant_coeff(std::uint32_t g) const
            {
                return folded ? static_cast<std::int64_t>(g) : static_cast<std::int64_t>(g) - n_giant / 2;
            }
            std::size_t cells() const
            {
                return static_cast<std::size_t>(n_baby) * n_giant;
            }
        };

        struct Plan
        {
            std::uint32_t direction = 0, logn = 0, in_level = 0, out_level = 0;
            bool needs_conjugation = false; // CoeffToSlot's split: the key of element 2N - 1
            std::vector<Stage> stages;      // in application order
            u64 table_words = 0;            // key-level NTT plaintexts of all stages
            u64 temp_bytes_per_item = 0;    // the transform's workspace per ciphertext of the batch (held by the tables)
            std::vector<std::uint32_t> key_steps; // sorted distinct non-zero steps: the Galois keys the client must make
        };

        struct Ring // what the plan needs of a context
        {
            int scheme = 0;      // 2 = CKKS
            std::uint32_t logn = 0, n_key = 0, k_first = 0;
            const u64 *key_moduli = nullptr;
        };

        inline std::uint32_t default_n_baby(std::uint32_t r)
        {
            return 1u << ((r + 2) / 2); // 2^ceil((r+1)/2)
        }

        // layer_counts: the stages in application order, summing to L; n_baby: per stage or null (the default)
        inline Plan make_plan(const Ring &ring, std::uint32_t direction, std::uint32_t k, const std::uint32_t *layer_counts,
                              std::uint32_t n_stages, const std::uint32_t *n_baby)
        {
            if (ring.scheme != 2)
                throw std::invalid_argument("the homomorphic DFT is CKKS only");
            if (direction != kCoeffsToSlots && direction != kSlotsToCoeffs)
                throw std::invalid_argument("direction must be 0 (CoeffToSlot) or 1 (SlotToCoeff)");
            if (ring.logn < 2)
                throw std::invalid_argument("the ring has fewer than two slots");
            if (k < 1 || k > ring.k_first)
                throw std::invalid_argument("level k out of range");
            const std::uint32_t L = ring.logn - 1, n = 1u << L;
            if (n_stages == 0 || !layer_counts)
                throw std::invalid_argument("the stages' layer counts must sum to log2(N/2)");
            std::uint32_t sum = 0;
            for (std::uint32_t t = 0; t < n_stages; t++)
            {
                if (layer_counts[t] == 0)
                    throw std::invalid_argument("a stage of zero layers");
                if (layer_counts[t] > L)
                    throw std::invalid_argument("the stages' layer counts must sum to log2(N/2)");
                sum += layer_counts[t];
            }
            if (sum != L)
                throw std::invalid_argument("the stages' layer counts must sum to log2(N/2)");
            if (n_stages >= k)
                throw std::invalid_argument("more stages than levels below k");

            Plan p;
            p.direction = direction;
            p.logn = ring.logn;
            p.in_level = k;
            p.out_level = k - n_stages;
            p.needs_conjugation = direction == kCoeffsToSlots;
            std::uint32_t below = 0; // layers under the current stage (SlotToCoeff) / above it (CoeffToSlot)
            for (std::uint32_t t = 0; t < n_stages; t++)
            {
                Stage s;
                s.r = layer_counts[t];
                s.s0 = direction == kSlotsToCoeffs ? below + 1 : L - below - s.r + 1;
                below += s.r;
                s.h0 = 1u << (s.s0 - 1);
                s.level = k - t;
                s.scale = static_cast<double>(ring.key_moduli[s.level - 1]);
                s.folded = s.s0 + s.r - 1 == L;
                const std::uint32_t n_diag = s.folded ? 1u << s.r : 2u << s.r;
                s.n_baby = n_baby && n_baby[t] ? n_baby[t] : default_n_baby(s.r);
                if ((s.n_baby & (s.n_baby - 1)) || s.n_baby > (1u << s.r))
                    throw std::invalid_argument("n_baby must be a power of two, at most 2^r");
                s.n_giant = n_diag / s.n_baby;
                for (std::uint32_t b = 0; b < s.n_baby; b++)
                    s.baby.push_back(static_cast<std::int32_t>(b * s.h0));
                for (std::uint32_t g = 0; g < s.n_giant; g++)
                {
                    const std::int64_t step = s.giant_coeff(g) * static_cast<std::int64_t>(s.n_baby) * s.h0;
                    s.giant.push_back(static_cast<std::int32_t>(step & (n - 1)));
                }
                for (std::int32_t st : s.baby)
                    if (st)
                        p.key_steps.push_back(static_cast<std::uint32_t>(st));
                for (std::int32_t st : s.giant)
                    if (st)
                        p.key_steps.push_back(static_cast<std::uint32_t>(st));
                p.table_words += static_cast<u64>(s.cells()) * ring.n_key << ring.logn;
                p.stages.push_back(std::move(s));
            }
            std::sort(p.key_steps.begin(), p.key_steps.end());
            p.key_steps.erase(std::unique(p.key_steps.begin(), p.key_steps.end()), p.key_steps.end());
            // temporaries of a transform, in ciphertext rows: CoeffToSlot keeps the stages' results in two buffers at level
            // k - 1 (one when there is one stage) and the conjugate of the last; SlotToCoeff the merged input at level k and
            // the results of all stages but the last in up to two buffers at level k - 1
            u64 rows;
            if (direction == kCoeffsToSlots)
                rows = static_cast<u64>(k - 1) * (n_stages >= 2 ? 2 : 1) + p.out_level;
            else
                rows = k + static_cast<u64>(k - 1) * (n_stages >= 3 ? 2 : n_stages - 1);
            p.temp_bytes_per_item = (rows * 2 * sizeof(u64)) << ring.logn;
            return p;
        }
    } // namespace dftplan
} // namespace sealhip
