// held_workspace.hpp -- the pool blocks that tables hold for the temporaries of the calls made with them (DESIGN.md section
// 23): per lane, the last block is current and the earlier ones stay held until release_all, because graphs captured on
// them may still be replayed. get() reuses the lane's current block when it is large enough, refuses to take a larger one
// during a graph capture (a pool block cannot be taken or released there), and otherwise takes one from the pool and keeps
// every earlier block: after one call at a batch size the next makes no allocator call and can be captured. Host code
// without a HIP dependency, over any Pool with pool_alloc(pool, bytes) / pool_release(pool, block), like pool_scratch.hpp:
// the library's is the Engine (homdft.cpp, bootstrap.cpp), the one of tests/held_workspace_check.cpp a recording stub.
#pragma once

#include <cstddef>
#include <map>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace sealhip
{
    template <class Pool>
    class HeldWorkspace
    {
        struct Block
        {
            void *p;
            std::size_t bytes;
        };
        std::mutex mu;
        std::map<const void *, std::vector<Block>> blocks; // by lane; a lane lives as long as its context, the owner less
    public:
        // `bytes` for the lane `lane_key`; `what` is the text of the refusal while `capturing`
        char *get(const Pool &pool, const void *lane_key, bool capturing, std::size_t bytes, const char *what)
        {
            std::lock_guard<std::mutex> lock(mu);
            std::vector<Block> &v = blocks[lane_key];
            if (!v.empty() && v.back().bytes >= bytes)
                return static_cast<char *>(v.back().p);
            if (capturing)
                throw std::logic_error(what);
            v.reserve(v.size() + 1); // (so that a block the pool gave cannot fail to be recorded)
            void *p = pool_alloc(pool, bytes);
            v.push_back(Block{ p, bytes });
            return static_cast<char *>(p);
        }
        // every block back to the pool, once: lane by lane, each lane's in the order taken
        void release_all(const Pool &pool)
        {
            std::lock_guard<std::mutex> lock(mu);
            for (auto &lane : blocks)
                for (Block &b : lane.second)
                    pool_release(pool, b.p);
            blocks.clear();
        }
        std::size_t held() const // (for the tests)
        {
            std::size_t n = 0;
            for (const auto &lane : blocks)
                n += lane.second.size();
            return n;
        }
    };
} // namespace sealhip
