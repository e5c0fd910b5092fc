// poly_eval.cpp -- Paterson-Stockmeyer evaluation of a polynomial on a ciphertext batch over the pipelines' dot_product and
// linear_combination (DESIGN.md sections 20 and 21): the BFV plan and driver, the CKKS driver over poly_plan.hpp's plan; the
// argument checks are the ABI entries' (api.cpp). Temporaries are blocks of the context's pool (pool.cpp) held in a Scratch,
// taken and released in stream order on the calling thread's lane: no synchronisation and, once the pool is warm, no allocator
// call. (Not hipMallocAsync: DESIGN.md section 11 -- in a sequence of calls its blocks gave wrong words, each call alone right.)
#include "../../include/sealhip.h"

#include <algorithm>

#include "engine.hpp"
#include "evalmod_plan.hpp"
#include "poly_plan.hpp"

namespace sealhip
{
    BfvPolyPlan bfv_poly_plan(Engine &h, std::uint32_t k, const u64 *coeffs, std::size_t degree, std::size_t n_baby)
    {
        for (std::size_t i = 0; i <= degree; i++)
            if (coeffs[i] >= h.t)
                throw std::invalid_argument("a coefficient is not below the plain modulus");
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
        const std::size_t n_terms = std::min(m, d + 1) - 1, ms = n_terms + 1;
        // inner sum j is identically zero when all of c_{jm} .. c_{jm + m - 1} are
        std::vector<u64> padded(g * ms, 0);
        std::vector<char> live(g, 0);
        for (std::size_t c = 0; c <= d; c++)
        {
            padded[c] = coeffs[c];
            if (coeffs[c])
                live[c / ms] = 1;
        }
        std::vector<std::size_t> outer; // the giant steps j >= 1 whose inner sum survives
        for (std::size_t j = 1; j < g; j++)
            if (live[j])
                outer.push_back(j);
        if (outer.size() > dot_product_max_terms(h, static_cast<int>(k)))
            throw std::invalid_argument("too many giant steps for one floor at this level (sealhip_evaluator_dot_product_max_terms)");
        return BfvPolyPlan{ d, m, g, n_terms, ms, std::move(padded), std::move(outer) };
    }

    void op_evaluate_polynomial(Engine &e, const BfvPolyPlan &plan, std::uint32_t k, const u64 *x, std::size_t count,
                                const KSwitchKey *key, const sealhip_kswitch_key *const *relin_keys, std::uint32_t n_relin_keys,
                                u64 *o, SinkScope &sink)
    {
        const std::size_t d = plan.d, m = plan.m, g = plan.g, n_terms = plan.n_terms, ms = plan.ms;
        const std::size_t poly = static_cast<std::size_t>(k) * e.n, two_words = count * 2 * poly, two = two_words * sizeof(u64);
        Scratch scratch(e);
        u64 *wide = nullptr; // the size-3 scratch of the products, reused in stream order
        auto product = [&](const u64 *a, const u64 *b) {
            if (!wide)
                wide = scratch.take(count * 3 * poly * sizeof(u64));
            return relin_product(e, k, a, b, count, relin_keys, n_relin_keys, wide, scratch.take(two));
        };
        // baby powers B_1 .. B_min(m, d): B_e = B_ceil(e/2) * B_floor(e/2)
        const std::size_t n_powers = std::min(m, d);
        std::vector<const u64 *> B(n_powers + 1, nullptr);
        B[1] = x;
        for (std::size_t p = 2; p <= n_powers; p++)
            B[p] = product(B[(p + 1) / 2], B[p / 2]);
        // giant powers G_1 = B_m, G_j = G_ceil(j/2) * G_floor(j/2): those a surviving term needs, and what they are built from
        std::vector<const u64 *> G(g, nullptr);
        std::vector<char> needed(g, 0);
        for (std::size_t j : plan.outer)
            needed[j] = 1;
        for (std::size_t j = g; j-- > 2;)
            if (needed[j])
                needed[(j + 1) / 2] = needed[j / 2] = 1;
        if (g > 1)
            G[1] = B[m];
        for (std::size_t j = 2; j < g; j++)
            if (needed[j])
                G[j] = product(G[(j + 1) / 2], G[j / 2]);
        // the tables of the inner sums and the inner sums themselves: I_0 goes straight to out when there is no outer sum
        u64 *W = scratch.take(g * n_terms * k * sizeof(u64)), *K = scratch.take(g * k * sizeof(u64));
        check(launch_poly_tables(e, static_cast<int>(k), plan.padded.data(), plan.padded.size(), ms, W, K), "poly_tables");
        if (g == 1)
        {
            sink.begin();
            op_linear_combination(e, static_cast<int>(k), B.data() + 1, n_terms, 2, count, W, K, 1, o);
            return;
        }
        u64 *I = scratch.take(g * two);
        op_linear_combination(e, static_cast<int>(k), B.data() + 1, n_terms, 2, count, W, K, g, I);
        // (g > 1 means d >= m: the inner sum that holds c_d is not zero, so there is an outer sum)
        std::vector<const u64 *> ga, ib;
        for (std::size_t j : plan.outer)
        {
            ga.push_back(G[j]);
            ib.push_back(I + j * two_words);
        }
        u64 *D = scratch.take(two);
        op_dot_product(e, static_cast<int>(k), ga.data(), ib.data(), plan.outer.size(), count, key, D);
        check(launch_ct_linear(e, CtLinearOp::Add, I, 2, D, 2, 0, o, count, e.map_for(static_cast<int>(k), SEALHIP_BASE_Q)), "add");
        sink.read_pass(o, 2, poly, count);
    }

    // Words per item of the pool blocks op_evaluate_polynomial_ckks takes, in the order it takes them (it counts what it
    // takes and refuses to go on if the two ever disagree).
    std::size_t ckks_poly_temp_words(const polyplan::Plan &p, std::size_t N)
    {
        const std::size_t k = static_cast<std::size_t>(p.k), nb = p.baby.size() - 1;
        std::size_t words = 0;
        bool drops = false;
        for (std::size_t e = 2; e <= nb; e++)
        {
            drops = drops || p.baby[(e + 1) / 2].level != p.baby[e / 2].level;
            words += 2 * static_cast<std::size_t>(p.baby[e].level) * N;
        }
        for (std::size_t j = 2; j < p.g; j++)
            if (p.needed[j])
            {
                drops = drops || p.giant[(j + 1) / 2].level != p.giant[j / 2].level;
                words += 2 * static_cast<std::size_t>(p.giant[j].level) * N;
            }
        if (drops)
            words += 2 * k * N; // one shared drop buffer (only the operand at the higher level is copied)
        if (p.basis == 1 && nb >= 2)
            words += 2 * 3 * k * N; // the size-3 product and the size-3 combination of a Chebyshev step
        const std::size_t nf = 1 + p.J.size();
        words += nf * 2 * static_cast<std::size_t>(p.inner_level) * N; // the inner sums before their rescale
        if (!p.J.empty())
        {
            words += nf * 2 * static_cast<std::size_t>(p.sums_level) * N;
            for (std::size_t j : p.J)
            {
                if (p.giant[j].level != p.outer_level)
                    words += 2 * static_cast<std::size_t>(p.outer_level) * N;
                if (p.sums_level != p.outer_level)
                    words += 2 * static_cast<std::size_t>(p.outer_level) * N;
            }
            words += 2 * static_cast<std::size_t>(p.out_level) * N; // the outer sum
        }
        return words;
    }

    void op_evaluate_polynomial_ckks(Engine &e, const polyplan::Plan &p, std::uint32_t k, const u64 *x, std::size_t count,
                                     const KSwitchKey *key, u64 *o, SinkScope &sink)
    {
        const std::size_t N = e.n, out_poly = static_cast<std::size_t>(p.out_level) * N;
        Scratch scratch(e);
        std::size_t taken = 0; // words per item (the table block T is not one of the plan's temporaries)
        const auto temp = [&](std::size_t words_per_item) {
            taken += words_per_item;
            return scratch.take(count * words_per_item * sizeof(u64));
        };
        const auto poly_words = [&](int level) { return static_cast<std::size_t>(level) * N; };

        // ---- every table of the call, gathered on the host and sent through kernel arguments in one pass
        const int Lin = p.inner_level;
        const std::size_t nb = p.baby.size() - 1, nf = 1 + p.J.size(), mi = p.mi;
        std::vector<u64> tab;
        const u64 *q = e.key_moduli.data();
        std::vector<std::size_t> cheb_at(nb + 1, 0); // Chebyshev step e: weights [2][L] (or [1][L]) then the constant [L]
        if (p.basis == 1)
            for (std::size_t el = 2; el <= nb; el++)
            {
                const int L = p.baby[(el + 1) / 2].level;
                cheb_at[el] = tab.size();
                for (int r = 0; r < L; r++)
                    tab.push_back(2 % q[r]);
                for (int r = 0; r < L; r++) // hi != lo: the weight of E_1; hi == lo: the constant
                    tab.push_back(polyplan::rint_residue(-p.cheb_sub[el], q[r]));
            }
        std::vector<std::size_t> sums{ 0 }; // the sums that are formed, in order
        sums.insert(sums.end(), p.J.begin(), p.J.end());
        const std::size_t w_at = tab.size();
        for (std::size_t j : sums)
            tab.insert(tab.end(), p.W.begin() + j * mi * Lin, p.W.begin() + (j + 1) * mi * Lin);
        const std::size_t k_at = tab.size();
        for (std::size_t j : sums)
            tab.insert(tab.end(), p.K.begin() + j * Lin, p.K.begin() + (j + 1) * Lin);
        const std::size_t ones_at = tab.size();
        tab.insert(tab.end(), 2 * static_cast<std::size_t>(p.out_level), 1);
        u64 *T = scratch.take(tab.size() * sizeof(u64));
        check(launch_put_words(e, T, tab.data(), tab.size()), "put_words");

        // ---- products: an operand above the product's level is dropped to it by a copy (tensor_dot reads one row stride)
        u64 *drop_buf = nullptr;
        const auto dropped = [&](const u64 *a, int la, int L) {
            if (la == L)
                return a;
            if (!drop_buf)
                drop_buf = temp(2 * poly_words(static_cast<int>(k)));
            check(launch_copy_rows(e, a, poly_words(la), drop_buf, poly_words(L), count * 2, L), "drop");
            return static_cast<const u64 *>(drop_buf);
        };
        const auto product_rescale = [&](const u64 *a, int la, const u64 *b, int lb, u64 *dst) {
            const int L = std::min(la, lb);
            const u64 *pa = dropped(a, la, L), *pb = dropped(b, lb, L);
            op_dot_product(e, L, &pa, &pb, 1, count, key, dst, true);
        };

        // ---- baby elements
        std::vector<const u64 *> E(nb + 1, nullptr);
        E[1] = x;
        u64 *wide_p = nullptr, *wide_r = nullptr;
        for (std::size_t el = 2; el <= nb; el++)
        {
            const std::size_t hi = (el + 1) / 2, lo = el / 2;
            const int L = p.baby[hi].level;
            u64 *dst = temp(2 * poly_words(p.baby[el].level));
            if (p.basis == 0)
                product_rescale(E[hi], p.baby[hi].level, E[lo], p.baby[lo].level, dst);
            else
            {
                if (!wide_p)
                    wide_p = temp(3 * poly_words(static_cast<int>(k))), wide_r = temp(3 * poly_words(static_cast<int>(k)));
                const u64 *pa = E[hi], *pb = dropped(E[lo], p.baby[lo].level, L);
                op_dot_product(e, L, &pa, &pb, 1, count, nullptr, wide_p, false);
                const u64 *terms[2] = { wide_p, x };
                const uint32_t levels[2] = { static_cast<uint32_t>(L), k }, sizes[2] = { 3, 2 };
                const u64 *W = T + cheb_at[el];
                if (hi == lo) // 2 P - rint(sc(hi) sc(lo))
                    op_linear_combination_levels(e, L, terms, levels, sizes, 1, 3, count, W, W + L, 1, wide_r);
                else // 2 P - rint(sc(hi) sc(lo) / sc(1)) E_1
                    op_linear_combination_levels(e, L, terms, levels, sizes, 2, 3, count, W, nullptr, 1, wide_r);
                op_switch_key_rescale(e, L, wide_r, 3 * poly_words(L), wide_r + 2 * poly_words(L), 3 * poly_words(L), count, *key,
                                      dst);
            }
            E[el] = dst;
        }

        // ---- giant powers: monomial powers of E_m in both bases
        std::vector<const u64 *> Y(p.g, nullptr);
        if (p.g > 1)
            Y[1] = E[p.m];
        for (std::size_t j = 2; j < p.g; j++)
            if (p.needed[j])
            {
                u64 *dst = temp(2 * poly_words(p.giant[j].level));
                product_rescale(Y[(j + 1) / 2], p.giant[(j + 1) / 2].level, Y[j / 2], p.giant[j / 2].level, dst);
                Y[j] = dst;
            }

        // ---- the inner sums: ONE combination over E_1 .. E_mi, each read at its own level, ONE rescale of the batch
        std::vector<uint32_t> levels(mi), sizes(mi, 2);
        for (std::size_t i = 1; i <= mi; i++)
            levels[i - 1] = static_cast<uint32_t>(p.baby[i].level);
        u64 *S = temp(nf * 2 * poly_words(Lin));
        op_linear_combination_levels(e, Lin, E.data() + 1, levels.data(), sizes.data(), mi, 2, count, T + w_at, T + k_at, nf, S);
        if (p.J.empty())
            op_mod_switch_scale(e, Lin, S, 2, count, o, 0);
        else
        {
            const int LI = p.sums_level, Lo = p.outer_level;
            u64 *I = temp(nf * 2 * poly_words(LI));
            op_mod_switch_scale(e, Lin, S, 2, nf * count, I, 0);
            std::vector<const u64 *> ya, ib;
            const auto copy_at = [&](const u64 *a, int la) { // an operand above the outer sum's level: a copy of its own
                if (la == Lo)
                    return a;
                u64 *c = temp(2 * poly_words(Lo));
                check(launch_copy_rows(e, a, poly_words(la), c, poly_words(Lo), count * 2, Lo), "drop");
                return static_cast<const u64 *>(c);
            };
            for (std::size_t s = 1; s < nf; s++)
            {
                const std::size_t j = p.J[s - 1];
                ya.push_back(copy_at(Y[j], p.giant[j].level));
                ib.push_back(copy_at(I + s * count * 2 * poly_words(LI), LI));
            }
            u64 *D = temp(2 * out_poly);
            op_dot_product(e, Lo, ya.data(), ib.data(), ya.size(), count, key, D, true);
            // out = D + I_0, I_0 read in place at the result's level
            const u64 *terms[2] = { D, I };
            const uint32_t lv[2] = { static_cast<uint32_t>(p.out_level), static_cast<uint32_t>(LI) }, sz[2] = { 2, 2 };
            op_linear_combination_levels(e, p.out_level, terms, lv, sz, 2, 2, count, T + ones_at, nullptr, 1, o);
        }
        if (taken != ckks_poly_temp_words(p, N))
            throw std::logic_error("evaluate_polynomial_ckks: the temporaries taken differ from the plan's count");
        sink.read_pass(o, 2, out_poly, count);
    }

    // ---- EvalMod: the planned polynomial, then r double-angle steps between two pool blocks
    std::size_t evalmod_temp_words(const evalmod::Plan &p, std::size_t N)
    {
        std::size_t words = ckks_poly_temp_words(p.poly, N);
        if (p.r >= 1)
            words += 2 * static_cast<std::size_t>(p.poly_level) * N;
        if (p.r >= 2)
            words += 2 * static_cast<std::size_t>(p.poly_level - 1) * N;
        return words;
    }

    void op_eval_mod(Engine &e, const evalmod::Plan &p, std::uint32_t k, const u64 *x, std::size_t count, const KSwitchKey *key,
                     u64 *o, SinkScope &sink)
    {
        if (p.r == 0)
            return op_evaluate_polynomial_ckks(e, p.poly, k, x, count, key, o, sink);
        if (!key)
            throw std::invalid_argument("not enough relinearization keys");
        const std::size_t N = e.n;
        Scratch scratch(e);
        u64 *a = scratch.take(count * 2 * static_cast<std::size_t>(p.poly_level) * N * sizeof(u64));
        u64 *b = p.r >= 2 ? scratch.take(count * 2 * static_cast<std::size_t>(p.poly_level - 1) * N * sizeof(u64)) : nullptr;
        {
            SinkScope quiet(e, 0); // (the polynomial's result is an intermediate: its read pass must not touch the flags)
            quiet.on = false;
            op_evaluate_polynomial_ckks(e, p.poly, k, x, count, key, a, quiet);
        }
        const u64 *cur = a;
        std::vector<u64> constant;
        for (unsigned i = 1; i <= p.r; i++)
        {
            const int level = p.poly_level - static_cast<int>(i) + 1;
            const double s = p.scales[i - 1];
            constant.assign(level, 0);
            for (int r = 0; r < level; r++)
                constant[r] = polyplan::rint_residue(-std::nearbyint(s * s), e.key_moduli[r]);
            u64 *dst = i == p.r ? o : (cur == a ? b : a);
            if (i == p.r)
                sink.begin(); // the last step's key switch stores the result and notes the flags
            op_double_angle(e, level, cur, count, constant.data(), *key, dst);
            cur = dst;
        }
    }
} // namespace sealhip
