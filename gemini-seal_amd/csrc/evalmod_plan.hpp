// evalmod_plan.hpp -- the plan of EvalMod, the scaled sine of CKKS bootstrapping: the Chebyshev
// coefficients of the function the polynomial evaluator approximates, and the scales of the double-angle steps that follow
// it. Host code with no HIP dependency: sealhip_evaluator_evalmod_plan / sealhip_evalmod_coeffs / _eval_mod (api.cpp) and the
// stand-alone tests/evalmod_plan_check.cpp include this very header, and tests/bootstrap_ref.py restates the scales.
//
// After ModRaise a coefficient is c = m + q_0 I with |I| < K. With u = c / q_0 and x = u / K in [-1, 1],
//     p(x) ~ cos((2 pi K x - pi / 2) / 2^r),     then r times  y -> 2 y^2 - 1      (cos 2a = 2 cos^2 a - 1)
// gives cos(2 pi u - pi / 2) = sin(2 pi u) = sin(2 pi m / q_0), which is 2 pi m / q_0 up to the relative error
// (2 pi m / q_0)^2 / 6. The argument of the cosine shrinks by 2^r, and with it the degree an approximation needs.
//
// Scales. A double-angle step at scale s and level L leaves scale s * s / dbl(q_(L-1)); r of them square a deviation from the
// primes r times over. So the scales are planned backwards from the one the caller wants:
//     t_r = scale_out,   t_(i-1) = sqrt(t_i * dbl(q_(L_0 - i)))     (step i = 1 .. r runs at level L_0 - i + 1),
// the polynomial is evaluated with scale_out = t_0, and the scales the ciphertext really has are the forward ones
//     s_0 = t_0,   s_i = s_(i-1) * s_(i-1) / dbl(q_(L_0 - i)),
// all IEEE doubles in exactly this order (products and quotients of two values, std::sqrt: nothing a compiler may contract).
// s_r differs from scale_out by rounding only: |s_r / scale_out - 1| <= 2^(r+3) 2^-53 (two roundings per step, the error
// doubling at each squaring, the backward pass likewise).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "poly_plan.hpp"

namespace sealhip
{
    namespace evalmod
    {
        using u64 = unsigned long long; // (the engine's word type)
        constexpr unsigned kMaxDoublings = 8;
        constexpr unsigned kMaxDegree = 1023;

        // f(x) = cos((2 pi K x - pi / 2) / 2^r)
        inline long double target(unsigned K, unsigned r, long double x)
        {
            const long double pi = 3.14159265358979323846264338327950288L;
            return std::cos((2.0L * pi * static_cast<long double>(K) * x - pi / 2.0L) / std::ldexp(1.0L, static_cast<int>(r)));
        }

        // The degree-d Chebyshev interpolant of f at the d + 1 Chebyshev nodes x_j = cos(pi (j + 1/2) / (d + 1)):
        //     c_i = (2 - [i == 0]) / (d + 1) * sum_j f(x_j) cos(i pi (j + 1/2) / (d + 1)),
        // the sums formed in long double, lowest degree first.
        inline std::vector<double> coeffs(unsigned K, unsigned r, unsigned d)
        {
            if (K < 1)
                throw std::invalid_argument("K must be at least 1");
            if (r > kMaxDoublings)
                throw std::invalid_argument("r must be at most 8");
            if (d < 1 || d > kMaxDegree)
                throw std::invalid_argument("degree out of range");
            const long double pi = 3.14159265358979323846264338327950288L;
            const std::size_t n = static_cast<std::size_t>(d) + 1;
            std::vector<long double> f(n);
            for (std::size_t j = 0; j < n; j++)
                f[j] = target(K, r, std::cos(pi * (static_cast<long double>(j) + 0.5L) / static_cast<long double>(n)));
            std::vector<double> c(n);
            for (std::size_t i = 0; i < n; i++)
            {
                long double sum = 0.0L;
                for (std::size_t j = 0; j < n; j++)
                    sum += f[j] * std::cos(pi * static_cast<long double>(i) * (static_cast<long double>(j) + 0.5L) /
                                           static_cast<long double>(n));
                c[i] = static_cast<double>(sum * (i == 0 ? 1.0L : 2.0L) / static_cast<long double>(n));
            }
            return c;
        }

        struct Plan
        {
            unsigned K = 0, r = 0, d = 0;
            int poly_level = 0, out_level = 0; // L_0 and L_0 - r
            double t0 = 0;                     // the polynomial's scale_out
            std::vector<double> scales;        // s_0 .. s_r
            std::size_t n_products = 0;        // key-switched products: the polynomial's and the r steps
            std::vector<double> c;             // the coefficients
            polyplan::Plan poly;               // of the polynomial, with scale_out = t_0
        };

        inline bool scale_ok(double s)
        {
            return std::isfinite(s) && s > 0 && s < 4611686018427387904.0; // 2^62
        }

        // q: the data primes of the first level. Throws std::invalid_argument.
        inline Plan make_plan(const u64 *q, int k, double s_x, unsigned K, unsigned r, unsigned d, std::size_t n_baby,
                              double scale_out, bool tables = true)
        {
            Plan p;
            p.K = K, p.r = r, p.d = d;
            p.c = coeffs(K, r, d);
            if (!std::isfinite(s_x) || s_x <= 0 || !std::isfinite(scale_out) || scale_out < 0)
                throw std::invalid_argument("scale out of bounds");
            // the levels depend on the shape alone: plan once for L_0, then again with the scale the steps need
            const polyplan::Plan shape = polyplan::make_plan(q, k, s_x, p.c.data(), d, 1, n_baby, 0.0, false);
            p.poly_level = shape.out_level;
            p.out_level = shape.out_level - static_cast<int>(r);
            if (p.out_level < 1)
                throw std::invalid_argument("end of modulus switching chain reached");
            const auto dbl = [&](int row) { return static_cast<double>(q[row]); };
            double t = scale_out == 0 ? s_x : scale_out;
            for (int i = static_cast<int>(r); i >= 1; i--)
            {
                const double prod = t * dbl(p.poly_level - i);
                t = std::sqrt(prod);
            }
            p.t0 = t;
            p.scales.assign(1, t);
            for (int i = 1; i <= static_cast<int>(r); i++)
            {
                const double sq = p.scales.back() * p.scales.back();
                p.scales.push_back(sq / dbl(p.poly_level - i));
            }
            for (double s : p.scales)
                if (!scale_ok(s))
                    throw std::invalid_argument("scale out of bounds: the primes at the EvalMod levels should be near the scale");
            p.poly = polyplan::make_plan(q, k, s_x, p.c.data(), d, 1, n_baby, p.t0, tables);
            // every element's scale (sigma is the outer sum's before its rescale: a product of two by construction)
            bool ok = scale_ok(p.poly.scale_out);
            for (std::size_t e = 1; e < p.poly.baby.size(); e++)
                ok = ok && scale_ok(p.poly.baby[e].scale);
            for (std::size_t j = 1; j < p.poly.g; j++)
                if (p.poly.needed[j])
                    ok = ok && scale_ok(p.poly.giant[j].scale);
            for (std::size_t j : p.poly.J)
                ok = ok && scale_ok(p.poly.tau[j]);
            if (!ok)
                throw std::invalid_argument("scale out of bounds: the primes at the EvalMod levels should be near the scale");
            p.n_products = p.poly.n_products + r;
            return p;
        }
    } // namespace evalmod
} // namespace sealhip
