// pool_scratch_check.cpp -- gemini-seal_amd/csrc/pool_scratch.hpp (the scoped pool temporaries of the polynomial drivers,
// poly_eval.cpp) executed on the host as a program of its own, over a stub pool that records what is taken and released.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I gemini-seal_amd/csrc tests/pool_scratch_check.cpp -o pool_scratch_check
// (built and run by tests/test_pool_scratch_host.py). Checks: on a return and when an exception is thrown between takes -- by the
// caller or by the pool itself -- every block taken is released exactly once, in the order taken, and not before the scope
// ends; an empty scope releases nothing. What the sanitizers watch: the stub's blocks are heap blocks, so a double release, a
// release of a pointer that was not taken, a missed release (leak check at exit) and a write through a released block are errors.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "pool_scratch.hpp"

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

struct Log
{
    std::vector<void *> taken, released;
    std::size_t fail_at = ~std::size_t(0); // the alloc with this index throws
};
struct StubPool
{
    Log *log;
};
static void *pool_alloc(const StubPool &pool, std::size_t bytes)
{
    if (pool.log->taken.size() == pool.log->fail_at)
        throw std::runtime_error("out of memory");
    void *p = std::malloc(bytes);
    pool.log->taken.push_back(p);
    return p;
}
static void pool_release(const StubPool &pool, void *p)
{
    pool.log->released.push_back(p);
    std::free(p);
}
using Scratch = sealhip::PoolScratch<StubPool>;

// takes n blocks, writes every word of each, then returns or throws; nothing may be released while the scope is open
static void run(Log &log, std::size_t n, bool throw_after)
{
    const StubPool pool{ &log };
    Scratch s(pool);
    for (std::size_t i = 0; i < n; i++)
    {
        const std::size_t words = 1 + 3 * i;
        unsigned long long *w = s.take(words * sizeof(unsigned long long));
        for (std::size_t j = 0; j < words; j++)
            w[j] = j;
        CHECK(log.released.empty(), "a block was released while its scope was open (take %zu)", i);
    }
    if (throw_after)
        throw std::logic_error("the operation failed");
}

int main()
{
    {
        Log log;
        run(log, 0, false);
        CHECK(log.taken.empty() && log.released.empty(), "an empty scope touched the pool");
    }
    for (std::size_t n : { 1, 2, 7 })
    {
        Log log;
        run(log, n, false);
        CHECK(log.taken.size() == n && log.released == log.taken, "return: %zu taken, %zu released, or another order",
              log.taken.size(), log.released.size());
    }
    for (std::size_t n : { 0, 1, 5 }) // the caller throws after n takes
    {
        Log log;
        bool thrown = false;
        try
        {
            run(log, n, true);
        }
        catch (const std::logic_error &)
        {
            thrown = true;
        }
        CHECK(thrown, "the exception did not pass through");
        CHECK(log.taken.size() == n && log.released == log.taken, "throw after %zu takes: %zu released, or another order", n,
              log.released.size());
    }
    for (std::size_t at : { 0, 3 }) // the pool throws at take `at` of 6: the blocks before it go back, nothing else does
    {
        Log log;
        log.fail_at = at;
        bool thrown = false;
        try
        {
            run(log, 6, false);
        }
        catch (const std::runtime_error &)
        {
            thrown = true;
        }
        CHECK(thrown, "the pool's exception did not pass through");
        CHECK(log.taken.size() == at && log.released == log.taken, "pool failure at take %zu: %zu released, or another order", at,
              log.released.size());
    }
    if (failures)
        return 1;
    std::printf("pool_scratch_check: OK\n");
    return 0;
}
