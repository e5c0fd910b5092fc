// poly_plan.hpp -- the plan of a polynomial evaluation on CKKS ciphertexts: which powers are formed at
// which level and scale, the chunks of Paterson-Stockmeyer in the monomial or the Chebyshev basis, and the integer weights
// that put every term of every inner sum on ONE scale. Host code with no HIP dependency: sealhip_evaluator_*_ckks (api.cpp)
// and the stand-alone tests/poly_plan_check.cpp include this very header, and tests/poly_eval_ckks_ref.py restates it.
//
// Reproducibility: all scale arithmetic is IEEE double in exactly the order written here, and no expression below is a
// multiply-add (products, quotients and sums of two values only; the one doubling is written as a sum), so a compiler's
// contraction setting cannot change a result. rint rounds half to even (std::nearbyint in the default rounding mode,
// Python's round(float)); the integer is taken exactly as mantissa * 2^exponent and reduced per prime, so a weight beyond
// 2^63 is as exact as a small one.
//
// Coefficient growth (Chebyshev): the chunks are the T_m-adic expansion p = sum_j r_j(x) T_m(x)^j, and every division by T_m
// doubles the quotient's coefficients, so a chunk's coefficients grow by up to about 2^(g-1) over the polynomial's (173 for
// random coefficients at d = 63, m = 8). The result is still p(x); what grows is the noise that the inner sums scale up.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace sealhip
{
    namespace polyplan
    {
        using u64 = unsigned long long; // (the engine's word type)

        // ceil(log2 e): the multiplicative depth of E_e built by halves
        inline int delta(std::size_t e)
        {
            int b = 0;
            while ((static_cast<std::size_t>(1) << b) < e)
                b++;
            return b;
        }

        // rint(x) mod q as a canonical residue; a negative integer -I becomes q - (I mod q), or 0 when q divides I
        inline u64 rint_residue(double x, u64 q)
        {
            const double y = std::nearbyint(x);
            const double a = std::fabs(y);
            if (a == 0)
                return 0;
            int e = 0;
            const double f = std::frexp(a, &e);                   // a = f 2^e, 1/2 <= f < 1
            u64 mant = static_cast<u64>(std::ldexp(f, 53));       // an integer below 2^53: the cast is exact
            const int exp = e - 53;                               // a = mant 2^exp
            u64 r;
            if (exp <= 0)
                r = (mant >> -exp) % q; // (a is an integer: the bits shifted out are zero)
            else
            {
                r = mant % q;
                for (int i = 0; i < exp; i++) // (q < 2^63: r + r does not wrap)
                    r = (r + r) % q;
            }
            return y < 0 && r ? q - r : r;
        }

        struct Element
        {
            int level = 0; // rows
            double scale = 0;
        };

        struct Plan
        {
            std::size_t d = 0, m = 0, g = 0, mi = 0; // mi: terms of an inner sum, E_1 .. E_mi
            int basis = 0, k = 0;
            std::vector<Element> baby;           // [e], 1 <= e <= min(m, d)
            std::vector<double> cheb_sub;        // [e], e >= 2, Chebyshev: rint(sc(hi) sc(lo)) or rint(sc(hi) sc(lo) / sc(1)), SUBTRACTED
            std::vector<std::vector<double>> chunks; // [j][i], j < g, i < m
            std::vector<char> formed;            // [j]: sum j is formed (j == 0 or chunk j is not identically zero)
            std::vector<std::size_t> J;          // the j >= 1 among them
            std::vector<char> needed;            // [j]: giant power Y_j is built
            std::vector<Element> giant;          // [j], 1 <= j < g where needed
            int inner_level = 0, sums_level = 0, outer_level = 0, out_level = 0; // L_in, L_I, L_out, the result's
            double scale_out = 0, sigma = 0;
            std::vector<double> tau;             // [j]: the scale of I_j
            std::size_t n_products = 0;          // key-switched products: baby, giant and the outer sum
            std::vector<u64> W;                  // [g][mi][inner_level]
            std::vector<u64> K;                  // [g][inner_level]
        };

        // a / T_m in the Chebyshev basis (T_i = 2 T_m T_{i-m} - T_{|i-2m|}): returns the quotient, leaves the remainder in
        // a[0 .. m-1]. a has n + 1 >= m + 1 coefficients.
        inline std::vector<double> divide_by_tm(std::vector<double> &a, std::size_t m)
        {
            const std::size_t n = a.size() - 1;
            std::vector<double> q(n - m + 1, 0.0);
            for (std::size_t i = n; i > m; i--)
            {
                const double twice = a[i] + a[i];
                q[i - m] = q[i - m] + twice;
                const std::size_t back = i >= 2 * m ? i - 2 * m : 2 * m - i;
                a[back] = a[back] - a[i];
                a[i] = 0;
            }
            q[0] = q[0] + a[m];
            a[m] = 0;
            return q;
        }

        // q: the data primes of the first level, q[0 .. k-1] those of level k. Throws std::invalid_argument in the order the
        // header documents (the level and the scheme are the caller's).
        inline Plan make_plan(const u64 *q, int k, double scale, const double *coeffs, std::size_t degree, unsigned basis,
                              std::size_t n_baby, double scale_out, bool tables = true)
        {
            Plan p;
            if (!std::isfinite(scale) || scale <= 0 || !std::isfinite(scale_out) || scale_out < 0)
                throw std::invalid_argument("scale out of bounds");
            for (std::size_t i = 0; i <= degree; i++)
                if (!std::isfinite(coeffs[i]))
                    throw std::invalid_argument("a coefficient is not finite");
            if (basis > 1)
                throw std::invalid_argument("basis must be 0 (monomial) or 1 (Chebyshev)");
            std::size_t d = degree;
            while (d > 0 && coeffs[d] == 0)
                d--;
            if (d < 1)
                throw std::invalid_argument("a constant polynomial is not an operation on a ciphertext");
            if (n_baby == 1 || n_baby > d + 1)
                throw std::invalid_argument("n_baby must be 0 (automatic) or between 2 and the degree plus one");
            std::size_t m = n_baby;
            if (m == 0)
                for (m = 1; m * m < d + 1;)
                    m++; // ceil(sqrt(d + 1))
            const std::size_t g = (d + m) / m; // ceil((d + 1) / m)
            p.d = d, p.m = m, p.g = g, p.mi = m - 1, p.basis = static_cast<int>(basis), p.k = k;
            p.scale_out = scale_out == 0 ? scale : scale_out;

            // chunks
            p.chunks.assign(g, std::vector<double>(m, 0.0));
            if (basis == 0)
                for (std::size_t e = 0; e <= d; e++)
                    p.chunks[e / m][e % m] = coeffs[e];
            else
            {
                std::vector<double> cur(coeffs, coeffs + d + 1);
                std::size_t j = 0;
                while (cur.size() > m)
                {
                    std::vector<double> quot = divide_by_tm(cur, m);
                    for (std::size_t i = 0; i < m; i++)
                        p.chunks[j][i] = cur[i];
                    cur.swap(quot);
                    j++;
                }
                if (j != g - 1)
                    throw std::logic_error("poly_plan: the T_m-adic expansion does not have g chunks");
                for (std::size_t i = 0; i < cur.size(); i++)
                    p.chunks[j][i] = cur[i];
            }
            for (const std::vector<double> &ch : p.chunks)
                for (double v : ch)
                    if (!std::isfinite(v))
                        throw std::invalid_argument("a coefficient is not finite");
            p.formed.assign(g, 0);
            p.formed[0] = 1;
            for (std::size_t j = 1; j < g; j++)
                for (double v : p.chunks[j])
                    if (v != 0)
                        p.formed[j] = 1;
            for (std::size_t j = 1; j < g; j++)
                if (p.formed[j])
                    p.J.push_back(j);
            p.needed.assign(g, 0);
            for (std::size_t j : p.J)
                p.needed[j] = 1;
            for (std::size_t j = g; j-- > 2;)
                if (p.needed[j])
                    p.needed[(j + 1) / 2] = p.needed[j / 2] = 1;

            // levels (integers only: nothing indexes the primes before the chain is known to be long enough)
            const std::size_t nb = std::min(m, d);
            p.baby.assign(nb + 1, Element{});
            for (std::size_t e = 1; e <= nb; e++)
                p.baby[e].level = k - delta(e);
            p.giant.assign(g, Element{});
            for (std::size_t j = 1; j < g; j++)
                if (p.needed[j])
                    p.giant[j].level = k - delta(m) - delta(j);
            p.inner_level = k - delta(p.mi);
            p.sums_level = p.inner_level - 1;
            p.outer_level = p.sums_level;
            for (std::size_t j : p.J)
                p.outer_level = std::min(p.outer_level, p.giant[j].level);
            p.out_level = p.J.empty() ? p.sums_level : p.outer_level - 1;
            if (p.out_level < 1)
                throw std::invalid_argument("end of modulus switching chain reached");
            p.n_products = (nb - 1) + (p.J.empty() ? 0 : 1);
            for (std::size_t j = 2; j < g; j++)
                p.n_products += p.needed[j] ? 1 : 0;

            // scales
            const auto dbl = [&](int row) { return static_cast<double>(q[row]); };
            p.baby[1].scale = scale;
            p.cheb_sub.assign(nb + 1, 0.0);
            for (std::size_t e = 2; e <= nb; e++)
            {
                const std::size_t hi = (e + 1) / 2, lo = e / 2;
                const int L = p.baby[hi].level;
                const double prod = p.baby[hi].scale * p.baby[lo].scale;
                p.baby[e].scale = prod / dbl(L - 1);
                if (basis == 1)
                    p.cheb_sub[e] = std::nearbyint(hi == lo ? prod : prod / p.baby[1].scale);
            }
            if (g > 1)
                p.giant[1].scale = p.baby[m].scale;
            for (std::size_t j = 2; j < g; j++)
                if (p.needed[j])
                {
                    const std::size_t hi = (j + 1) / 2, lo = j / 2;
                    const int L = p.giant[hi].level;
                    p.giant[j].scale = p.giant[hi].scale * p.giant[lo].scale / dbl(L - 1);
                }
            p.tau.assign(g, 0.0);
            p.tau[0] = p.scale_out;
            if (!p.J.empty())
            {
                p.sigma = p.scale_out * dbl(p.outer_level - 1);
                for (std::size_t j : p.J)
                    p.tau[j] = p.sigma / p.giant[j].scale;
            }
            for (const Element &el : p.baby)
                if (!std::isfinite(el.scale))
                    throw std::invalid_argument("scale out of bounds");
            if (!tables)
                return p;

            // the tables of the inner sums: rows of sums that are not formed stay zero
            const int Lin = p.inner_level;
            p.W.assign(g * p.mi * Lin, 0);
            p.K.assign(g * Lin, 0);
            for (std::size_t j = 0; j < g; j++)
            {
                if (!p.formed[j])
                    continue;
                const double up = p.tau[j] * dbl(Lin - 1);
                for (std::size_t i = 1; i <= p.mi; i++)
                {
                    const double w = p.chunks[j][i] * (up / p.baby[i].scale);
                    if (!std::isfinite(w))
                        throw std::invalid_argument("scale out of bounds");
                    for (int r = 0; r < Lin; r++)
                        p.W[(j * p.mi + (i - 1)) * Lin + r] = rint_residue(w, q[r]);
                }
                const double c = p.chunks[j][0] * up;
                if (!std::isfinite(c))
                    throw std::invalid_argument("scale out of bounds");
                for (int r = 0; r < Lin; r++)
                    p.K[j * Lin + r] = rint_residue(c, q[r]);
            }
            return p;
        }
    } // namespace polyplan
} // namespace sealhip
