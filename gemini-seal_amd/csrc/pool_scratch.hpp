// pool_scratch.hpp -- the pool blocks an operation holds while it runs. take() gets a block; the destructor gives every block
// back in the order it was taken, on a return and when an exception unwinds. Host code without a HIP dependency, over any
// Pool with pool_alloc(pool, bytes) / pool_release(pool, block): the library's is the Engine (Scratch, engine.hpp), the one
// of tests/pool_scratch_check.cpp a recording stub.
#pragma once

#include <cstddef>
#include <vector>

namespace sealhip
{
    template <class Pool>
    class PoolScratch
    {
        const Pool &pool;
        std::vector<void *> owned;
    public:
        explicit PoolScratch(const Pool &p) : pool(p)
        {}
        PoolScratch(const PoolScratch &) = delete;
        unsigned long long *take(std::size_t bytes) // (u64 words)
        {
            void *p = pool_alloc(pool, bytes);
            owned.push_back(p);
            return static_cast<unsigned long long *>(p);
        }
        ~PoolScratch()
        {
            for (void *p : owned)
                pool_release(pool, p);
        }
    };
} // namespace sealhip
