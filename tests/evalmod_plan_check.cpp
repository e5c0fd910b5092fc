// evalmod_plan_check.cpp -- gemini-seal_amd/csrc/evalmod_plan.hpp (the planner of sealhip_evaluator_eval_mod, DESIGN.md section
// 24) executed on the host as a program of its own: the very header api.cpp includes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/evalmod_plan_check.cpp -o evalmod_plan_check
// (built and run by tests/test_bootstrap_host.py). Over a chain of 24 primes near 2^50: the coefficients interpolate the
// function at the nodes; for every r in 0 .. 8 and a few degrees and baby-step counts the levels are the polynomial plan's minus
// r, the forward scales follow the primes in the documented order, and s_r returns to the requested scale within
// 2^(r+3) 2^-53; then the refusals. What the sanitizers watch: every index into the primes and the scale lists.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "evalmod_plan.hpp"

using namespace sealhip;
using u64 = unsigned long long;

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

template <class F>
static bool refuses(F &&f, const char *word)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument &err)
    {
        return std::string(err.what()).find(word) != std::string::npos;
    }
    return false;
}

// T_0 .. T_d at x by the recurrence, summed against c
static long double cheb_value(const std::vector<double> &c, long double x)
{
    long double t0 = 1.0L, t1 = x, sum = c[0];
    for (std::size_t i = 1; i < c.size(); i++)
    {
        sum += c[i] * t1;
        const long double t2 = 2.0L * x * t1 - t0;
        t0 = t1;
        t1 = t2;
    }
    return sum;
}

int main()
{
    // odd values near 2^50, alternately above and below (the planner only reads them as doubles and as moduli of residues)
    std::vector<u64> q;
    for (int i = 0; i < 24; i++)
        q.push_back((1ull << 50) + (i % 2 ? -1 : 1) * (1000003ll * (i + 1)) * 2 + 1);
    const long double pi = 3.14159265358979323846264338327950288L;

    // ---- the coefficients interpolate the function at the nodes
    const unsigned cases[4][3] = { { 12, 3, 31 }, { 12, 2, 47 }, { 8, 3, 23 }, { 1, 0, 7 } };
    for (const auto &cs : cases)
    {
        const std::vector<double> c = evalmod::coeffs(cs[0], cs[1], cs[2]);
        CHECK(c.size() == cs[2] + 1, "coefficient count");
        long double worst = 0;
        for (unsigned j = 0; j <= cs[2]; j++)
        {
            const long double x = std::cos(pi * (j + 0.5L) / (cs[2] + 1));
            worst = std::fmax(worst, std::fabs(cheb_value(c, x) - evalmod::target(cs[0], cs[1], x)));
        }
        CHECK(worst < 1e-13L, "K=%u r=%u d=%u: the interpolant misses a node by %Lg", cs[0], cs[1], cs[2], worst);
    }

    // ---- levels and scales
    const int k = 20;
    for (unsigned r = 0; r <= evalmod::kMaxDoublings; r++)
        for (unsigned d : { 7u, 23u, 31u })
            for (std::size_t n_baby : { std::size_t(0), std::size_t(8) })
                for (double s_x : { std::ldexp(1.0, 50), std::ldexp(1.0, 50) * 1.0123 })
                    for (double scale_out : { 0.0, std::ldexp(1.0, 49) * 1.7 })
                    {
                        const evalmod::Plan p = evalmod::make_plan(q.data(), k, s_x, 12, r, d, n_baby, scale_out);
                        const polyplan::Plan shape = polyplan::make_plan(q.data(), k, s_x, p.c.data(), d, 1, n_baby, 0.0, false);
                        CHECK(p.poly_level == shape.out_level && p.out_level == shape.out_level - static_cast<int>(r), "levels");
                        CHECK(p.scales.size() == r + 1 && p.scales[0] == p.t0 && p.poly.scale_out == p.t0, "scale list");
                        CHECK(p.poly.out_level == p.poly_level, "the polynomial's level does not depend on its scale");
                        for (unsigned i = 1; i <= r; i++)
                        {
                            const double sq = p.scales[i - 1] * p.scales[i - 1];
                            CHECK(p.scales[i] == sq / static_cast<double>(q[p.poly_level - i]), "forward scale %u", i);
                        }
                        const double want = scale_out == 0 ? s_x : scale_out;
                        CHECK(std::fabs(p.scales[r] / want - 1.0) <= std::ldexp(1.0, static_cast<int>(r) + 3 - 53),
                              "r=%u: s_r / scale_out - 1 = %g", r, p.scales[r] / want - 1.0);
                        CHECK(p.n_products == p.poly.n_products + r, "products");
                    }

    // ---- refusals
    const double s50 = std::ldexp(1.0, 50);
    CHECK(refuses([&] { evalmod::make_plan(q.data(), 6, s50, 12, 3, 31, 8, 0.0); }, "end of modulus switching chain"),
          "an out level below 1 passes");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, s50, 12, 9, 31, 8, 0.0); }, "r must be at most 8"), "r = 9 passes");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, s50, 0, 3, 31, 8, 0.0); }, "K must be at least 1"), "K = 0 passes");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, s50, 12, 3, 0, 0, 0.0); }, "degree"), "degree 0 passes");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, std::ldexp(1.0, 63), 12, 3, 31, 8, 0.0); }, "scale out of bounds"),
          "a scale far above the primes passes");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, -1.0, 12, 3, 31, 8, 0.0); }, "scale out of bounds"), "a negative scale");
    CHECK(refuses([&] { evalmod::make_plan(q.data(), k, s50, 12, 3, 31, 8, std::nan("")); }, "scale out of bounds"), "NaN");
    if (failures)
    {
        std::printf("evalmod_plan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("evalmod_plan_check: OK\n");
    return 0;
}
