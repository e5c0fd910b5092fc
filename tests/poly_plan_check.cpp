// poly_plan_check.cpp -- gemini-seal_amd/csrc/poly_plan.hpp (the planner of sealhip_evaluator_evaluate_polynomial_ckks,
// DESIGN.md section 21) executed on the host as a program of its own: the very header api.cpp includes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/poly_plan_check.cpp -o poly_plan_check
// (built and run by tests/test_poly_eval_ckks_host.py). Checks: rint_residue against exact 128-bit arithmetic for small,
// half-way, negative and beyond-2^63 values; the shape, the levels and the number of chunks for degrees 1 .. 63 in both bases
// and with every legal n_baby; the Chebyshev chunks against a direct evaluation; the refusals in their order; tables whose
// weights exceed 2^64. What the sanitizers watch: every index into the primes, the chunks and the tables.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "poly_plan.hpp"

using namespace sealhip::polyplan;
using u128 = unsigned __int128;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do                                         \
    {                                          \
        if (!(cond))                           \
        {                                      \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            failures++;                        \
        }                                      \
    } while (0)

// twelve primes = 1 mod 128 alternating below 2^39 and 2^41 (found by trial division here, so the file stands alone)
static bool is_prime(u64 v)
{
    if (v < 2)
        return false;
    for (u64 f = 2; f * f <= v; f += (f == 2 ? 1 : 2))
        if (v % f == 0)
            return false;
    return true;
}
static std::vector<u64> primes()
{
    std::vector<u64> out;
    u64 lo = (1ull << 39) - 127, hi = (1ull << 41) - 127; // = 1 mod 128
    while (out.size() < 12)
    {
        u64 &c = out.size() % 2 == 0 ? lo : hi;
        while (!is_prime(c))
            c -= 128;
        out.push_back(c);
        c -= 128;
    }
    return out;
}

static double cheb_t(std::size_t e, double x)
{
    double a = 1, b = x;
    if (e == 0)
        return a;
    for (std::size_t i = 1; i < e; i++)
    {
        const double c = 2 * x * b - a;
        a = b, b = c;
    }
    return b;
}

template <class F>
static std::string refusal(F f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument &e)
    {
        return e.what();
    }
    return "";
}

int main()
{
    const std::vector<u64> q = primes();
    // ---- rint_residue
    {
        const u64 p = q[0];
        CHECK(rint_residue(0.0, p) == 0 && rint_residue(-0.0, p) == 0 && rint_residue(0.4, p) == 0, "zeros");
        CHECK(rint_residue(0.5, p) == 0 && rint_residue(1.5, p) == 2 && rint_residue(2.5, p) == 2, "halves go to even");
        CHECK(rint_residue(-1.0, p) == p - 1 && rint_residue(-2.5, p) == p - 2, "negatives");
        CHECK(rint_residue(static_cast<double>(p), p) == 0 && rint_residue(-static_cast<double>(p), p) == 0, "multiples of q");
        for (int e = 0; e < 200; e++)
        {
            // 1.3125 * 2^e = 21 * 2^(e - 4): an integer from e = 4 on
            const double x = std::ldexp(1.3125, e);
            u64 r;
            if (e >= 4)
            {
                u128 acc = 21 % p;
                for (int i = 0; i < e - 4; i++)
                    acc = acc * 2 % p;
                r = static_cast<u64>(acc);
            }
            else
                r = static_cast<u64>(std::nearbyint(x)) % p;
            CHECK(rint_residue(x, p) == r, "rint_residue(1.3125 * 2^%d)", e);
            CHECK(rint_residue(-x, p) == (r ? p - r : 0), "rint_residue(-1.3125 * 2^%d)", e);
        }
        CHECK(rint_residue(std::ldexp(1.0, 53) + 2, p) == static_cast<u64>(((static_cast<u128>(1) << 53) + 2) % p), "2^53 + 2");
    }
    // ---- shapes, levels, chunks
    const double s = std::ldexp(1.0, 40);
    for (unsigned basis = 0; basis < 2; basis++)
        for (std::size_t d = 1; d <= 63; d++)
        {
            std::vector<double> c(d + 3, 0.0); // two trailing zeros to trim
            for (std::size_t e = 0; e <= d; e++)
                c[e] = std::sin(1.0 + 3.0 * e) * (e % 5 == 4 ? 0.0 : 1.0);
            c[d] = 0.75;
            for (std::size_t n_baby = 0; n_baby <= d + 1; n_baby += (n_baby == 0 ? 2 : 1))
            {
                Plan p;
                try
                {
                    p = make_plan(q.data(), 12, s, c.data(), d + 2, basis, n_baby, 0.0);
                }
                catch (const std::invalid_argument &e)
                {
                    CHECK(std::string(e.what()).find("chain") != std::string::npos, "d %zu n_baby %zu: %s", d, n_baby, e.what());
                    continue;
                }
                CHECK(p.d == d && p.g == (d + p.m) / p.m && p.chunks.size() == p.g, "shape d %zu n_baby %zu", d, n_baby);
                CHECK(p.out_level >= 1 && p.out_level < p.inner_level && p.inner_level <= 12, "levels d %zu n_baby %zu", d, n_baby);
                CHECK(p.W.size() == p.g * p.mi * p.inner_level && p.K.size() == p.g * p.inner_level, "table sizes");
                for (std::size_t e = 2; e < p.baby.size(); e++)
                    CHECK(p.baby[e].level == p.baby[(e + 1) / 2].level - 1 && p.baby[e].scale > 0, "baby level %zu", e);
                for (std::size_t i = 0; i < p.W.size(); i++)
                    CHECK(p.W[i] < q[i % p.inner_level], "a weight is not canonical");
                // the chunks are the polynomial: sum_j r_j(x) G(x)^j with G = x^m or T_m
                for (double x : { -1.0, -0.3, 0.0, 0.55, 1.0 })
                {
                    double want = 0, got = 0, norm = 0;
                    for (std::size_t e = 0; e <= d; e++)
                        want += c[e] * (basis ? cheb_t(e, x) : std::pow(x, double(e))), norm += std::fabs(c[e]);
                    const double G = basis ? cheb_t(p.m, x) : std::pow(x, double(p.m));
                    for (std::size_t j = p.g; j-- > 0;)
                    {
                        double r = 0;
                        for (std::size_t i = 0; i < p.m; i++)
                            r += p.chunks[j][i] * (basis ? cheb_t(i, x) : std::pow(x, double(i)));
                        got = got * G + r;
                    }
                    // (every division by T_m doubles the quotient's coefficients: a chunk is up to 2^(g-1) times larger)
                    const double tol = 1e-12 * norm * (basis ? std::ldexp(1.0, static_cast<int>(p.g)) : 1.0);
                    CHECK(std::fabs(got - want) <= tol, "chunks d %zu m %zu basis %u x %g: %g vs %g", d, p.m, basis, x, got,
                          want);
                }
            }
        }
    // ---- a zero chunk is not formed, and the giant it would need is not built
    {
        std::vector<double> c(21, 0.5);
        for (int e = 8; e < 12; e++)
            c[e] = 0;
        const Plan p = make_plan(q.data(), 12, s, c.data(), 20, 0, 4, 0.0);
        CHECK(p.g == 6 && p.J.size() == 4 && !p.formed[2] && p.formed[5], "the zero chunk");
        CHECK(p.needed[2] && p.needed[3] && p.needed[4] && p.needed[5], "giants 2 .. 5 are needed (2 builds 4 and 5)");
        for (int r = 0; r < p.inner_level; r++)
            CHECK(p.K[2 * p.inner_level + r] == 0, "rows of a sum that is not formed stay zero");
    }
    // ---- weights beyond 2^64
    {
        // (at scale 2^40 under a 41-bit prime a coefficient of 1e6 gives a weight of 2^61 and constants of 2^80; 1e7 puts the
        //  weight beyond 2^64 as well)
        const double c[4] = { 0.5, 1.0e7, -0.25, 1.0e6 };
        const Plan p = make_plan(q.data(), 12, s, c, 3, 0, 0, 0.0);
        const double w = c[1] * (p.tau[0] * double(q[p.inner_level - 1]) / p.baby[1].scale);
        CHECK(w > std::ldexp(1.0, 64), "the weight is beyond 2^64: %g", w);
        int e = 0;
        const double f = std::frexp(std::nearbyint(w), &e);
        u128 acc = static_cast<u128>(static_cast<u64>(std::ldexp(f, 53))) % q[0];
        for (int i = 0; i < e - 53; i++)
            acc = acc * 2 % q[0];
        CHECK(p.W[0] == static_cast<u64>(acc), "its residue");
    }
    // ---- refusals, in order
    {
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        const double bad[2] = { 1.0, nan }, good[3] = { 1.0, 2.0, 3.0 }, constant[3] = { 5.0, 0.0, 0.0 };
        const auto why = [&](double scale, const double *c, std::size_t degree, unsigned basis, std::size_t n_baby, int k = 12,
                             double scale_out = 0.0) {
            return refusal([&] { make_plan(q.data(), k, scale, c, degree, basis, n_baby, scale_out); });
        };
        CHECK(why(nan, bad, 1, 2, 1).find("scale") != std::string::npos, "scale first");
        CHECK(why(inf, bad, 1, 2, 1).find("scale") != std::string::npos && why(0.0, bad, 1, 2, 1).find("scale") != std::string::npos &&
                  why(s, bad, 1, 2, 1, 12, -1.0).find("scale") != std::string::npos,
              "scales");
        CHECK(why(s, bad, 1, 2, 1).find("not finite") != std::string::npos, "then the coefficients");
        CHECK(why(s, constant, 2, 2, 1).find("basis") != std::string::npos, "then the basis");
        CHECK(why(s, constant, 2, 1, 1).find("constant") != std::string::npos, "then the degree");
        CHECK(why(s, good, 2, 1, 1, 1).find("n_baby") != std::string::npos && why(s, good, 2, 1, 4, 1).find("n_baby") != std::string::npos,
              "then n_baby");
        CHECK(why(s, good, 2, 1, 0, 2).find("chain") != std::string::npos && why(s, good, 2, 1, 0, 3).empty(), "then the chain");
    }
    if (failures)
    {
        std::printf("poly_plan_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("poly_plan_check: OK\n");
    return 0;
}
