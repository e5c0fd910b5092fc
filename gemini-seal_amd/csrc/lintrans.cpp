// lintrans.cpp -- the tables of a matrix-vector product from a caller's matrix: the occupancy scan, the
// plan (lintrans_plan.hpp), and the grid built chunk by chunk -- values (lintrans.hip) -> op_ckks_encode at the key level --
// into n_giant x n_baby x n_key x N words of device memory. The transform itself is the BSGS entry's pipeline, called by
// api.cpp with the tables' steps and plaintexts; the argument checks are the ABI entries'.
#include "../../include/sealhip.h"

#include <cstring>

#include "engine.hpp"
#include "lintrans_plan.hpp"

namespace sealhip
{
    struct LinearTransform
    {
        ltplan::Plan plan;
        double scale = 0, gain = 0;
        int device = -1;
        u64 *plain = nullptr;           // device, [n_giant][n_baby][n_key][N]
        const Engine *engine = nullptr; // the context the tables were made on
        // (no block is taken today -- the transform's temporaries are the BSGS pipeline's, in the lane's arena -- but the
        // tables end as every tables object does: destroy_held_tables, refused during a graph capture)
        mutable HeldWorkspace<Engine> held;
        ~LinearTransform()
        {
            if (plain)
                (void)hipFree(plain);
        }
    };

    namespace
    {
        // the plan's mask and step lists in one pool block, for the gather: staged from the host, so the stream is
        // synchronised before the host copies go away
        struct PlanDev
        {
            Scratch scratch;
            std::uint8_t *mask = nullptr;
            std::int32_t *baby = nullptr, *giant = nullptr;
            PlanDev(Engine &e, const ltplan::Plan &p) : scratch(e)
            {
                const std::size_t mask_bytes = (p.d + 255) & ~static_cast<std::size_t>(255);
                const std::size_t nb = p.baby.size(), ng = p.giant.size();
                char *base = reinterpret_cast<char *>(scratch.take(mask_bytes + (nb + ng) * sizeof(std::int32_t)));
                mask = reinterpret_cast<std::uint8_t *>(base);
                baby = reinterpret_cast<std::int32_t *>(base + mask_bytes);
                giant = baby + nb;
                hipStream_t s = e.lane().stream;
                SEALHIP_CHECK(hipMemcpyAsync(mask, p.mask.data(), p.d, hipMemcpyHostToDevice, s));
                SEALHIP_CHECK(hipMemcpyAsync(baby, p.baby.data(), nb * sizeof(std::int32_t), hipMemcpyHostToDevice, s));
                SEALHIP_CHECK(hipMemcpyAsync(giant, p.giant.data(), ng * sizeof(std::int32_t), hipMemcpyHostToDevice, s));
                SEALHIP_CHECK(hipStreamSynchronize(s));
            }
        };
    } // namespace

    bool op_lintrans_occupancy(Engine &e, const double *matrix, std::uint32_t d, std::uint8_t *occupied)
    {
        Scratch scratch(e);
        std::uint8_t *flags = reinterpret_cast<std::uint8_t *>(scratch.take(d));
        check(launch_lintrans_occupancy(e, matrix, d, flags), "lintrans occupancy");
        SEALHIP_CHECK(hipMemcpyAsync(occupied, flags, d, hipMemcpyDeviceToHost, e.lane().stream));
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
        e.check_fault();
        bool finite = true;
        for (std::uint32_t c = 0; c < d; c++)
        {
            finite = finite && !(occupied[c] & 2);
            occupied[c] &= 1;
        }
        return finite;
    }

    void op_lintrans_values(Engine &e, const ltplan::Plan &p, const double *matrix, double gain, double *values)
    {
        PlanDev dev(e, p);
        check(launch_lintrans_values(e, matrix, p.d, dev.mask, dev.baby, static_cast<std::uint32_t>(p.baby.size()), dev.giant, 0,
                                     p.cells(), gain, values),
              "lintrans values");
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream)); // (the block of PlanDev goes back to the pool)
        e.check_fault();
    }

    LinearTransform *lintrans_create(Engine &e, const double *matrix, std::uint32_t d, std::uint32_t n1, double scale, double gain)
    {
        std::vector<std::uint8_t> occupied(d);
        if (!op_lintrans_occupancy(e, matrix, d, occupied.data()))
            throw std::invalid_argument("the matrix has an entry that is not finite");
        std::unique_ptr<LinearTransform> t(new LinearTransform);
        t->plan = ltplan::make_plan(static_cast<std::uint32_t>(e.logn - 1), d, occupied.data(), n1); // (all zero: refused here)
        t->scale = scale;
        t->gain = gain;
        t->device = e.device;
        t->engine = &e;
        const ltplan::Plan &p = t->plan;
        const std::size_t N = e.n, n = N >> 1, plain_words = static_cast<std::size_t>(e.n_key) * N, cells = p.cells();
        SEALHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&t->plain), cells * plain_words * sizeof(u64)));
        PlanDev dev(e, p);
        // a chunk of cells: its values (a pool block) and the encoder's complex coefficients (the lane's arena) within the
        // arena's cap together -- a full d = N/2 grid is N/2 cells of N/2 complex values
        const std::size_t value_bytes = n * 2 * sizeof(double), coeff_bytes = N * 2 * sizeof(double);
        const std::size_t chunk = arena_chunk_items(e, cells, value_bytes + coeff_bytes);
        Scratch scratch(e);
        double *values = reinterpret_cast<double *>(scratch.take(chunk * value_bytes));
        for (std::size_t off = 0; off < cells; off += chunk)
        {
            const std::size_t m = std::min(chunk, cells - off);
            check(launch_lintrans_values(e, matrix, d, dev.mask, dev.baby, static_cast<std::uint32_t>(p.baby.size()), dev.giant, off,
                                         m, gain, values),
                  "lintrans values");
            op_ckks_encode(e, e.n_key, values, n, m, scale, t->plain + off * plain_words);
        }
        SEALHIP_CHECK(hipStreamSynchronize(e.lane().stream));
        e.check_fault();
        return t.release();
    }

    void lintrans_destroy(LinearTransform *t)
    {
        if (t)
            destroy_held_tables(t, "linear-transform tables cannot be destroyed during a graph capture", [t] { delete t; });
    }

    const Engine *lintrans_engine(const LinearTransform &t)
    {
        return t.engine;
    }

    const ltplan::Plan &lintrans_plan(const LinearTransform &t)
    {
        return t.plan;
    }

    const u64 *lintrans_plain(const LinearTransform &t)
    {
        return t.plain;
    }

    double lintrans_scale(const LinearTransform &t)
    {
        return t.scale;
    }
} // namespace sealhip
