// lintrans_plan.hpp -- the plan of an encrypted matrix-vector product from a caller's matrix. Host code
// with no HIP dependency: sealhip_linear_transform_* (api.cpp, lintrans.cpp) and the stand-alone tests/lintrans_plan_check.cpp
// include this very header, and tests/lintrans_ref.py restates it.
//
// With n = N/2 slots and M a d x d matrix, d a power of two <= n, diagonal c in [0, d) is the slot vector
//     u_c[p] = M[p mod d][(p + c) mod d],   p < n,
// and the transform of a ciphertext with slots z is  out[p] = sum_{c in D} u_c[p] z[(p + c) mod n],  D the diagonals in use.
// BSGS with the baby stride n1 (a power of two <= d): c = g + b, b = c mod n1, g = c - b. The babies are the distinct b over
// D, the giants the distinct g, both ascending; cell [gi][bi] of the grid holds u_(g+b) rotated by minus its giant step
// (rot_s moves slot j+s to slot j), and is zero when g + b is not in D. Step 0 on either axis is the identity: no key.
// n1 == 0 asks for the power of two that minimises  nb + 2 ng  (nb, ng the NON-ZERO baby and giant steps: a giant costs a
// decomposition and a half mod-down, a baby an inner product only), ties to the larger n1. On the dense grid of d = 2^r,
// r >= 1, that is 2^ceil((r+1)/2), the homomorphic DFT's default (d = 1 has the one stride 1).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace sealhip
{
    namespace ltplan
    {
        struct Plan
        {
            std::uint32_t log_slots = 0, d = 0, n1 = 0;
            std::uint32_t n_diagonals = 0;             // |D|
            std::vector<std::uint8_t> mask;            // d bytes, 1 where the diagonal is in D
            std::vector<std::int32_t> baby, giant;     // rotation steps in [0, d), ascending, 0 the identity
            std::vector<std::uint32_t> key_steps;      // sorted distinct non-zero steps: the Galois keys the client must make
            std::size_t cells() const
            {
                return baby.size() * giant.size();
            }
        };

        inline bool is_pow2(std::uint32_t v)
        {
            return v && !(v & (v - 1));
        }

        // the distinct b = c mod n1 and g = c - b over the diagonals in use, ascending
        inline void steps_for(const std::vector<std::uint8_t> &mask, std::uint32_t n1, std::vector<std::int32_t> &baby,
                              std::vector<std::int32_t> &giant)
        {
            const std::uint32_t d = static_cast<std::uint32_t>(mask.size());
            std::vector<std::uint8_t> has_b(n1, 0), has_g(d / n1, 0);
            for (std::uint32_t c = 0; c < d; c++)
                if (mask[c])
                    has_b[c % n1] = has_g[c / n1] = 1;
            baby.clear();
            giant.clear();
            for (std::uint32_t b = 0; b < n1; b++)
                if (has_b[b])
                    baby.push_back(static_cast<std::int32_t>(b));
            for (std::uint32_t g = 0; g < d / n1; g++)
                if (has_g[g])
                    giant.push_back(static_cast<std::int32_t>(g * n1));
        }

        inline std::uint32_t default_n1(const std::vector<std::uint8_t> &mask)
        {
            const std::uint32_t d = static_cast<std::uint32_t>(mask.size());
            std::uint32_t best = 1;
            std::size_t best_cost = ~static_cast<std::size_t>(0);
            std::vector<std::int32_t> baby, giant;
            for (std::uint32_t n1 = 1; n1 <= d; n1 <<= 1)
            {
                steps_for(mask, n1, baby, giant);
                const std::size_t nb = baby.size() - (!baby.empty() && baby[0] == 0);
                const std::size_t ng = giant.size() - (!giant.empty() && giant[0] == 0);
                const std::size_t cost = nb + 2 * ng;
                if (cost <= best_cost) // (<=: ties to the larger stride)
                {
                    best_cost = cost;
                    best = n1;
                }
            }
            return best;
        }

        // mask: d bytes, non-zero = in D; null = every diagonal
        inline Plan make_plan(std::uint32_t log_slots, std::uint32_t d, const std::uint8_t *mask, std::uint32_t n1)
        {
            if (log_slots > 30 || !is_pow2(d) || d > (1u << log_slots))
                throw std::invalid_argument("d must be a power of two between 1 and N/2");
            if (n1 && (!is_pow2(n1) || n1 > d))
                throw std::invalid_argument("n1 must be 0 or a power of two at most d");
            Plan p;
            p.log_slots = log_slots;
            p.d = d;
            p.mask.assign(d, 1);
            if (mask)
                for (std::uint32_t c = 0; c < d; c++)
                    p.mask[c] = mask[c] ? 1 : 0;
            p.n_diagonals = static_cast<std::uint32_t>(std::count(p.mask.begin(), p.mask.end(), 1));
            if (p.n_diagonals == 0)
                throw std::invalid_argument("no diagonal in use: an empty sum of rotations is a transparent ciphertext");
            p.n1 = n1 ? n1 : default_n1(p.mask);
            steps_for(p.mask, p.n1, p.baby, p.giant);
            for (std::int32_t s : p.baby)
                if (s)
                    p.key_steps.push_back(static_cast<std::uint32_t>(s));
            for (std::int32_t s : p.giant)
                if (s)
                    p.key_steps.push_back(static_cast<std::uint32_t>(s));
            std::sort(p.key_steps.begin(), p.key_steps.end());
            p.key_steps.erase(std::unique(p.key_steps.begin(), p.key_steps.end()), p.key_steps.end());
            return p;
        }

        // values[gi][bi][p] = {re * gain, im * gain} of M[q mod d][(q + c) mod d], q = (p - g) mod n, c = g + b; zero when c
        // is not in D. The loop of lintrans_values_kernel on the host: the same indices, the same two multiplies.
        inline void values_host(const Plan &p, const double *matrix, double gain, double *values)
        {
            const std::uint32_t n = 1u << p.log_slots, d = p.d;
            const std::size_t nb = p.baby.size();
            for (std::size_t gi = 0; gi < p.giant.size(); gi++)
                for (std::size_t bi = 0; bi < nb; bi++)
                {
                    const std::uint32_t g = static_cast<std::uint32_t>(p.giant[gi]), c = g + static_cast<std::uint32_t>(p.baby[bi]);
                    double *cell = values + 2 * ((gi * nb + bi) << p.log_slots);
                    for (std::uint32_t q = 0; q < n; q++)
                    {
                        double re = 0.0, im = 0.0;
                        if (p.mask[c])
                        {
                            const std::uint32_t i = (q - g) & (n - 1);
                            const std::size_t at = 2 * (static_cast<std::size_t>(i & (d - 1)) * d + ((i + c) & (d - 1)));
                            re = matrix[at] * gain; // (two multiplies and no sum: nothing to contract)
                            im = matrix[at + 1] * gain;
                        }
                        cell[2 * q] = re;
                        cell[2 * q + 1] = im;
                    }
                }
        }

        // one byte per diagonal: 1 if an entry of it is non-zero, re or im (-0.0 is zero); returns whether every entry of the
        // matrix is finite. The host form of lintrans_occupancy_kernel.
        inline bool occupancy_host(std::uint32_t d, const double *matrix, std::uint8_t *occupied)
        {
            bool finite = true;
            for (std::uint32_t c = 0; c < d; c++)
            {
                std::uint8_t any = 0;
                for (std::uint32_t i = 0; i < d; i++)
                {
                    const std::size_t at = 2 * (static_cast<std::size_t>(i) * d + ((i + c) & (d - 1)));
                    const double re = matrix[at], im = matrix[at + 1];
                    any |= (re != 0.0 || im != 0.0) ? 1 : 0;
                    finite = finite && (re - re == 0.0) && (im - im == 0.0);
                }
                occupied[c] = any;
            }
            return finite;
        }
    } // namespace ltplan
} // namespace sealhip
