// held_workspace_check.cpp -- gemini-seal_amd/csrc/held_workspace.hpp (the pool blocks the DFT and bootstrap tables hold for
// their calls' temporaries, homdft.cpp and bootstrap.cpp) executed on the host as a program of its own, over a stub pool that
// records what is taken and released.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/held_workspace_check.cpp -o held_workspace_check
// (built and run by tests/test_held_workspace_host.py). Checks: a request that fits the lane's last block gets that block
// without a pool call, also while capturing; a larger one takes a block and the earlier one stays held; growth while
// capturing throws std::logic_error with the owner's text and changes nothing; two lanes keep separate lists; release_all
// gives every block back exactly once, each lane's in the order taken, and a second call releases nothing; when the pool
// throws, no block is recorded. What the sanitizers watch: the stub's blocks are heap blocks, so a double release, a
// missed release (leak check at exit) and a write through a released block are errors.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "held_workspace.hpp"

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

struct StubPool
{
    mutable std::vector<void *> taken, released;
    std::size_t fail_at = ~std::size_t(0); // the alloc with this index throws
};
static void *pool_alloc(const StubPool &pool, std::size_t bytes)
{
    if (pool.taken.size() == pool.fail_at)
        throw std::runtime_error("out of memory");
    void *p = std::malloc(bytes);
    pool.taken.push_back(p);
    return p;
}
static void pool_release(const StubPool &pool, void *p)
{
    pool.released.push_back(p);
    std::free(p);
}
using Held = sealhip::HeldWorkspace<StubPool>;
static const char *const kRefusal = "the owner's workspace would be allocated during a graph capture";

// get() must refuse with the owner's text and leave the pool and the lists as they were
static void refused(Held &h, const StubPool &pool, const void *lane, std::size_t bytes)
{
    const std::size_t taken = pool.taken.size(), held = h.held();
    bool thrown = false;
    try
    {
        h.get(pool, lane, true, bytes, kRefusal);
    }
    catch (const std::logic_error &e)
    {
        thrown = std::strcmp(e.what(), kRefusal) == 0;
    }
    CHECK(thrown, "growth to %zu bytes during a capture was not refused with the owner's text", bytes);
    CHECK(pool.taken.size() == taken && pool.released.empty() && h.held() == held, "a refused request changed the lists");
}

int main()
{
    int lane_a = 0, lane_b = 0; // (only their addresses matter)
    {
        StubPool pool;
        Held h;
        refused(h, pool, &lane_a, 64); // a lane without a block: any request grows
        char *a0 = h.get(pool, &lane_a, false, 100, kRefusal);
        std::memset(a0, 1, 100);
        CHECK(pool.taken.size() == 1 && a0 == pool.taken[0], "the first request did not take one block");
        CHECK(h.get(pool, &lane_a, false, 100, kRefusal) == a0 && h.get(pool, &lane_a, false, 1, kRefusal) == a0 &&
                  h.get(pool, &lane_a, true, 100, kRefusal) == a0 && pool.taken.size() == 1,
              "a request that fits the last block did not reuse it without a pool call");
        refused(h, pool, &lane_a, 101);
        char *a1 = h.get(pool, &lane_a, false, 300, kRefusal);
        std::memset(a1, 2, 300);
        std::memset(a0, 3, 100); // the earlier block is still held: a captured graph may write to it
        CHECK(pool.taken.size() == 2 && a1 == pool.taken[1] && pool.released.empty() && h.held() == 2,
              "a larger request did not take a second block next to the first");
        CHECK(h.get(pool, &lane_a, true, 100, kRefusal) == a1 && h.get(pool, &lane_a, true, 300, kRefusal) == a1,
              "the last block is not the current one");
        // another lane has a list of its own: lane a's 300 bytes do not serve it
        refused(h, pool, &lane_b, 8);
        char *b0 = h.get(pool, &lane_b, false, 8, kRefusal);
        CHECK(pool.taken.size() == 3 && b0 == pool.taken[2] && h.get(pool, &lane_b, true, 8, kRefusal) == b0 &&
                  h.get(pool, &lane_a, true, 300, kRefusal) == a1,
              "two lanes share a list");
        refused(h, pool, &lane_b, 300);
        char *b1 = h.get(pool, &lane_b, false, 16, kRefusal);
        CHECK(pool.taken.size() == 4 && h.held() == 4, "lane b did not grow on its own");
        h.release_all(pool);
        std::vector<void *> of_a, of_b; // the releases of each lane's blocks, in the order they happened
        for (void *p : pool.released)
            (p == a0 || p == a1 ? of_a : of_b).push_back(p);
        CHECK(pool.released.size() == 4 && of_a == (std::vector<void *>{ a0, a1 }) && of_b == (std::vector<void *>{ b0, b1 }),
              "release_all: %zu of 4 blocks released, or a lane's in another order", pool.released.size());
        CHECK(h.held() == 0, "release_all left blocks recorded");
        h.release_all(pool);
        CHECK(pool.released.size() == 4, "a second release_all released something");
        char *again = h.get(pool, &lane_a, false, 4, kRefusal); // usable afterwards; its block goes with the next release_all
        CHECK(pool.taken.size() == 5 && again == pool.taken[4], "a request after release_all did not take a block");
        h.release_all(pool);
        CHECK(pool.released.size() == 5, "the block taken after release_all was not released");
    }
    for (std::size_t at : { 0, 2 }) // the pool throws at take `at`: nothing is recorded for it, the earlier blocks stay
    {
        StubPool pool;
        pool.fail_at = at;
        Held h;
        bool thrown = false;
        try
        {
            for (std::size_t i = 0; i < 4; i++)
                h.get(pool, &lane_a, false, 32 << i, kRefusal);
        }
        catch (const std::runtime_error &)
        {
            thrown = true;
        }
        CHECK(thrown, "the pool's exception did not pass through");
        CHECK(pool.taken.size() == at && h.held() == at, "pool failure at take %zu: %zu blocks recorded", at, h.held());
        if (at)
            CHECK(h.get(pool, &lane_a, true, 32 << (at - 1), kRefusal) == pool.taken[at - 1], "the last good block is not current");
        h.release_all(pool);
        CHECK(pool.released == pool.taken, "pool failure at take %zu: %zu released, or another order", at, pool.released.size());
    }
    if (failures)
        return 1;
    std::printf("held_workspace_check: OK\n");
    return 0;
}
