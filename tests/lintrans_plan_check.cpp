// lintrans_plan_check.cpp -- gemini-seal_amd/csrc/lintrans_plan.hpp (the planner of sealhip_linear_transform_*, DESIGN.md
// section 26) executed on the host as a program of its own: the very header api.cpp includes.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/lintrans_plan_check.cpp -o lintrans_plan_check
// (built and run by tests/test_lintrans_host.py). For log2 n = 3 .. 6, every d, every n1 (0 included) and the masks all,
// diagonal 0 alone, one non-zero diagonal, the band {0, 1, d-1}, every other diagonal and 200 seeded random ones: the steps
// are sorted and distinct, every c of D sits in exactly one cell and no cell holds two, the key list is the sorted set of
// the non-zero steps, the default stride minimises nb + 2 ng with ties to the larger one and is 2^ceil((r+1)/2) on a dense
// grid; the host gather puts every entry where the definition says; the occupancy scan; the refusals. With arguments
// `log_n d n1 mask-as-01-string` it prints one plan, for the Python test to compare with its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "lintrans_plan.hpp"

using namespace sealhip::ltplan;

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

static std::uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static std::uint64_t next_u64()
{
    std::uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::size_t cost_of(const std::vector<std::uint8_t> &mask, std::uint32_t n1)
{
    std::set<std::uint32_t> b, g;
    for (std::uint32_t c = 0; c < mask.size(); c++)
        if (mask[c])
        {
            b.insert(c % n1);
            g.insert(c - c % n1);
        }
    b.erase(0);
    g.erase(0);
    return b.size() + 2 * g.size();
}

static void check_plan(std::uint32_t L, const std::vector<std::uint8_t> &mask, std::uint32_t n1, bool dense)
{
    const std::uint32_t d = static_cast<std::uint32_t>(mask.size());
    const Plan p = make_plan(L, d, dense ? nullptr : mask.data(), n1);
    CHECK(p.d == d && p.log_slots == L && is_pow2(p.n1) && p.n1 <= d && (n1 == 0 || p.n1 == n1), "shape d=%u n1=%u", d, n1);
    if (n1 == 0)
    {
        for (std::uint32_t s = 1; s <= d; s <<= 1)
            CHECK(cost_of(mask, p.n1) < cost_of(mask, s) || (cost_of(mask, p.n1) == cost_of(mask, s) && p.n1 >= s),
                  "default stride d=%u chose %u, %u is better", d, p.n1, s);
        if (dense && d >= 2)
        {
            std::uint32_t r = 0;
            while ((1u << r) < d)
                r++;
            CHECK(p.n1 == (1u << ((r + 2) / 2)), "dense default d=%u is %u", d, p.n1);
        }
    }
    for (std::size_t i = 0; i < p.baby.size(); i++)
        CHECK(p.baby[i] >= 0 && static_cast<std::uint32_t>(p.baby[i]) < p.n1 && (i == 0 || p.baby[i - 1] < p.baby[i]), "baby order");
    for (std::size_t i = 0; i < p.giant.size(); i++)
        CHECK(p.giant[i] >= 0 && static_cast<std::uint32_t>(p.giant[i]) < d && p.giant[i] % static_cast<std::int32_t>(p.n1) == 0 &&
                  (i == 0 || p.giant[i - 1] < p.giant[i]),
              "giant order");
    std::vector<int> seen(d, 0);
    std::set<std::uint32_t> steps;
    std::uint32_t in_use = 0;
    for (std::int32_t g : p.giant)
        for (std::int32_t b : p.baby)
        {
            const std::uint32_t c = static_cast<std::uint32_t>(g + b);
            CHECK(c < d, "cell outside the matrix");
            if (c < d)
                seen[c]++;
        }
    for (std::uint32_t c = 0; c < d; c++)
    {
        CHECK(seen[c] <= 1 && (!mask[c] || seen[c] == 1), "diagonal %u of d=%u sits in %d cells", c, d, seen[c]);
        in_use += mask[c] ? 1 : 0;
    }
    for (std::int32_t s : p.baby)
        if (s)
            steps.insert(static_cast<std::uint32_t>(s));
    for (std::int32_t s : p.giant)
        if (s)
            steps.insert(static_cast<std::uint32_t>(s));
    CHECK(p.n_diagonals == in_use, "n_diagonals");
    CHECK(std::vector<std::uint32_t>(steps.begin(), steps.end()) == p.key_steps, "key steps");
    // a baby and a giant occur only where a diagonal needs them
    for (std::int32_t b : p.baby)
    {
        bool used = false;
        for (std::uint32_t c = 0; c < d; c++)
            used = used || (mask[c] && c % p.n1 == static_cast<std::uint32_t>(b));
        CHECK(used, "baby step %d serves no diagonal", b);
    }
    for (std::int32_t g : p.giant)
    {
        bool used = false;
        for (std::uint32_t c = 0; c < d; c++)
            used = used || (mask[c] && c - c % p.n1 == static_cast<std::uint32_t>(g));
        CHECK(used, "giant step %d serves no diagonal", g);
    }
    // the host gather and the scan, on a matrix whose entry (i, j) is i + 1 + (j + 1) i off the masked diagonals
    const std::uint32_t n = 1u << L;
    std::vector<double> M(2 * static_cast<std::size_t>(d) * d, 0.0);
    for (std::uint32_t i = 0; i < d; i++)
        for (std::uint32_t j = 0; j < d; j++)
            if (mask[(j - i) & (d - 1)])
            {
                M[2 * (static_cast<std::size_t>(i) * d + j)] = i + 1.0;
                M[2 * (static_cast<std::size_t>(i) * d + j) + 1] = -(j + 1.0);
            }
    std::vector<std::uint8_t> occ(d, 9);
    CHECK(occupancy_host(d, M.data(), occ.data()), "finite matrix reported as not finite");
    CHECK(occ == mask, "occupancy differs from the mask d=%u", d);
    std::vector<double> values(2 * p.cells() * n, -1.0);
    values_host(p, M.data(), 0.5, values.data());
    for (std::size_t gi = 0; gi < p.giant.size(); gi++)
        for (std::size_t bi = 0; bi < p.baby.size(); bi++)
            for (std::uint32_t q = 0; q < n; q++)
            {
                const std::uint32_t g = static_cast<std::uint32_t>(p.giant[gi]), c = g + static_cast<std::uint32_t>(p.baby[bi]);
                const std::uint32_t i = ((q + n - g) % n) % d, j = ((q + n - g) % n + c) % d;
                const double *v = &values[2 * ((gi * p.baby.size() + bi) * n + q)];
                const double re = mask[c] ? 0.5 * (i + 1.0) : 0.0, im = mask[c] ? -0.5 * (j + 1.0) : 0.0;
                CHECK(v[0] == re && v[1] == im, "value d=%u n1=%u cell %zu,%zu slot %u", d, p.n1, gi, bi, q);
            }
}

template <class F>
static bool refuses(F f)
{
    try
    {
        f();
    }
    catch (const std::invalid_argument &)
    {
        return true;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc == 5)
    {
        const std::uint32_t L = static_cast<std::uint32_t>(std::atoi(argv[1])), d = static_cast<std::uint32_t>(std::atoi(argv[2]));
        const std::uint32_t n1 = static_cast<std::uint32_t>(std::atoi(argv[3]));
        std::vector<std::uint8_t> mask;
        for (const char *c = argv[4]; *c; c++)
            mask.push_back(*c == '1');
        if (mask.size() != d)
            return 2;
        const Plan p = make_plan(L, d, mask.data(), n1);
        std::printf("n1 %u baby", p.n1);
        for (std::int32_t s : p.baby)
            std::printf(" %d", s);
        std::printf(" giant");
        for (std::int32_t s : p.giant)
            std::printf(" %d", s);
        std::printf(" keys");
        for (std::uint32_t s : p.key_steps)
            std::printf(" %u", s);
        std::printf("\n");
        return 0;
    }
    std::size_t plans = 0;
    for (std::uint32_t L = 3; L <= 6; L++)
        for (std::uint32_t d = 1; d <= (1u << L); d <<= 1)
        {
            std::vector<std::vector<std::uint8_t>> masks;
            masks.push_back(std::vector<std::uint8_t>(d, 1));
            masks.push_back(std::vector<std::uint8_t>(d, 0));
            masks.back()[0] = 1;
            if (d > 1)
            {
                masks.push_back(std::vector<std::uint8_t>(d, 0));
                masks.back()[d < 4 ? d - 1 : d / 2 + 1] = 1;
                masks.push_back(std::vector<std::uint8_t>(d, 0));
                masks.back()[0] = masks.back()[1] = masks.back()[d - 1] = 1;
                masks.push_back(std::vector<std::uint8_t>(d, 0));
                for (std::uint32_t c = 0; c < d; c += 2)
                    masks.back()[c] = 1;
            }
            for (int t = 0; t < 200; t++)
            {
                std::vector<std::uint8_t> m(d, 0);
                const std::uint64_t density = next_u64() % 101;
                for (std::uint32_t c = 0; c < d; c++)
                    m[c] = next_u64() % 100 < density;
                if (std::count(m.begin(), m.end(), 1) == 0)
                    m[next_u64() % d] = 1;
                masks.push_back(m);
            }
            for (std::size_t mi = 0; mi < masks.size(); mi++)
            {
                for (std::uint32_t n1 = 0; n1 <= d; n1 = n1 ? n1 << 1 : 1)
                {
                    check_plan(L, masks[mi], n1, mi == 0);
                    plans++;
                }
            }
        }
    // the scan: -0.0 is zero, a single entry on the last diagonal is found, a NaN or an infinity is reported
    {
        const std::uint32_t d = 8;
        std::vector<double> M(2 * d * d, 0.0);
        std::vector<std::uint8_t> occ(d, 9);
        M[2 * (3 * d + 5)] = -0.0;
        M[2 * (1 * d + 0) + 1] = 1e-300; // row 1, column 0: diagonal d - 1
        CHECK(occupancy_host(d, M.data(), occ.data()), "finite");
        for (std::uint32_t c = 0; c < d; c++)
            CHECK(occ[c] == (c == d - 1), "scan of diagonal %u", c);
        M[2 * (2 * d + 2)] = __builtin_nan("");
        CHECK(!occupancy_host(d, M.data(), occ.data()), "NaN");
        M[2 * (2 * d + 2)] = __builtin_inf();
        CHECK(!occupancy_host(d, M.data(), occ.data()), "infinity");
    }
    // refusals
    const std::uint8_t none[8] = { 0 };
    CHECK(refuses([] { make_plan(3, 0, nullptr, 0); }), "d = 0");
    CHECK(refuses([] { make_plan(3, 6, nullptr, 0); }), "d = 6");
    CHECK(refuses([] { make_plan(3, 16, nullptr, 0); }), "d > n");
    CHECK(refuses([] { make_plan(3, 8, nullptr, 3); }), "n1 = 3");
    CHECK(refuses([] { make_plan(3, 8, nullptr, 16); }), "n1 > d");
    CHECK(refuses([&] { make_plan(3, 8, none, 0); }), "empty mask");
    CHECK(!refuses([] { make_plan(3, 8, nullptr, 8); }), "n1 = d");
    CHECK(!refuses([] { make_plan(0, 1, nullptr, 0); }), "d = n = 1");
    if (failures)
    {
        std::printf("lintrans_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("lintrans_plan_check: OK (%zu plans)\n", plans);
    return 0;
}
