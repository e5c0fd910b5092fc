// pool.cpp -- pooled, stream-ordered device memory of a context (sealhip_pool_*, include/sealhip.h). Blocks are hipMalloc'd
// slabs of one size class each, cached on the free list of the lane that released them. hipMallocAsync / hipMemPool are not
// used on purpose (wrong key words with the stream-ordered allocator).
#include <algorithm>

#include "engine.hpp"

namespace sealhip
{
    namespace
    {
        int floor_log2(std::size_t v)
        {
            int r = 0;
            while (v >>= 1)
                r++;
            return r;
        }

        // hipFree of a cached block (the caller holds P.mu and has made sure no stream still uses it)
        void free_cached(DevicePool &P, void *ptr)
        {
            auto it = P.blocks.find(ptr);
            if (it == P.blocks.end())
                return;
            if (it->second.released)
                (void)hipEventDestroy(it->second.released);
            P.cached -= it->second.bytes;
            P.blocks.erase(it);
            SEALHIP_CHECK(hipFree(ptr));
            P.frees++;
        }

        // the calling lane's cached blocks, freed (out-of-memory retry)
        void trim_lane(const Engine &e, Lane &l)
        {
            DevicePool &P = *e.pool;
            auto lists = P.free.find(&l);
            if (lists == P.free.end())
                return;
            SEALHIP_CHECK(hipStreamSynchronize(l.stream));
            for (auto &cls : lists->second)
                for (void *p : cls.second)
                    free_cached(P, p);
            P.free.erase(lists);
        }
    } // namespace

    std::size_t pool_size_class(std::size_t bytes)
    {
        // a multiple of 256 bytes, then the next m * 2^e with m in {4, 5, 6, 7}: less than 25 % over the rounded request
        const std::size_t b = (std::max<std::size_t>(bytes, 1) + 255) & ~static_cast<std::size_t>(255);
        const std::size_t unit = static_cast<std::size_t>(1) << (floor_log2(b) - 2);
        return (b + unit - 1) / unit * unit;
    }

    void *pool_alloc(const Engine &e, std::size_t bytes)
    {
        if (bytes == 0 || bytes > kPoolMaxBytes)
            throw std::invalid_argument("pool block size out of range (1 byte .. 2^46 bytes)");
        const std::size_t cls = pool_size_class(bytes);
        Lane &l = e.lane();
        DevicePool &P = *e.pool;
        std::lock_guard<std::mutex> lock(P.mu);
        // same lane: stream order already protects the block
        auto own = P.free.find(&l);
        if (own != P.free.end())
        {
            auto list = own->second.find(cls);
            if (list != own->second.end() && !list->second.empty())
            {
                void *p = list->second.back();
                list->second.pop_back();
                PoolBlock &b = P.blocks.at(p);
                b.held = true;
                P.cached -= cls;
                P.in_use += cls;
                P.hits++;
                return p;
            }
        }
        // another lane: this lane's stream waits on the event recorded at the release (no host block)
        if (!l.capturing)
            for (auto &lane_lists : P.free)
            {
                if (lane_lists.first == &l)
                    continue;
                auto list = lane_lists.second.find(cls);
                if (list == lane_lists.second.end())
                    continue;
                for (auto it = list->second.begin(); it != list->second.end(); ++it)
                {
                    PoolBlock &b = P.blocks.at(*it);
                    SEALHIP_CHECK(hipStreamWaitEvent(l.stream, b.released, 0));
                    void *p = *it;
                    list->second.erase(it);
                    b.held = true;
                    b.lane = &l;
                    P.cached -= cls;
                    P.in_use += cls;
                    P.hits++;
                    P.cross_lane_hits++;
                    return p;
                }
            }
        if (l.capturing)
            throw std::logic_error("the pool would allocate during a graph capture: run the sequence once before capturing");
        void *p = nullptr;
        hipError_t err = hipMalloc(&p, cls);
        if (err == hipErrorOutOfMemory)
        {
            (void)hipGetLastError();
            trim_lane(e, l); // once, then give up
            err = hipMalloc(&p, cls);
        }
        if (err != hipSuccess)
        {
            (void)hipGetLastError();
            throw HipError(err, (std::string("pool: hipMalloc of ") + std::to_string(cls) + " bytes: " + hipGetErrorString(err)).c_str());
        }
        P.mallocs++;
        P.misses++;
        PoolBlock b;
        b.bytes = cls;
        b.lane = &l;
        b.held = true;
        P.blocks.emplace(p, b);
        P.in_use += cls;
        return p;
    }

    void pool_check_held(const Engine &e, const void *ptr)
    {
        DevicePool &P = *e.pool;
        std::lock_guard<std::mutex> lock(P.mu);
        auto it = P.blocks.find(const_cast<void *>(ptr));
        if (it == P.blocks.end())
            throw std::invalid_argument("the pointer was not handed out by this context's pool");
        if (!it->second.held)
            throw std::invalid_argument("the pool block was already released");
    }

    void pool_release(const Engine &e, void *ptr)
    {
        Lane &l = e.lane();
        DevicePool &P = *e.pool;
        std::lock_guard<std::mutex> lock(P.mu);
        auto it = P.blocks.find(ptr);
        if (it == P.blocks.end() || !it->second.held) // (another thread may have released it since the check)
            throw std::invalid_argument("the pool block was already released");
        // a captured graph may still use the block at every replay: it cannot go back on any free list
        if (l.capturing)
            throw std::logic_error("a pool block cannot be released during a graph capture: release it after the capture");
        PoolBlock &b = it->second;
        if (!b.released)
            SEALHIP_CHECK(hipEventCreateWithFlags(&b.released, hipEventDisableTiming));
        SEALHIP_CHECK(hipEventRecord(b.released, l.stream));
        b.held = false;
        b.lane = &l;
        P.free[&l][b.bytes].push_back(ptr);
        P.in_use -= b.bytes;
        P.cached += b.bytes;
    }

    void pool_trim(const Engine &e)
    {
        e.sync_and_check(true);
        DevicePool &P = *e.pool;
        std::lock_guard<std::mutex> lock(P.mu);
        for (auto &lane_lists : P.free)
            for (auto &cls : lane_lists.second)
                for (void *p : cls.second)
                    free_cached(P, p);
        P.free.clear();
    }

    void pool_free_all(Engine &e)
    {
        // context destruction, after every lane has drained its stream: every block, held ones included
        DevicePool &P = *e.pool;
        std::lock_guard<std::mutex> lock(P.mu);
        for (auto &kv : P.blocks)
        {
            if (kv.second.released)
                (void)hipEventDestroy(kv.second.released);
            (void)hipFree(kv.first);
        }
        P.blocks.clear();
        P.free.clear();
        P.in_use = P.cached = 0;
    }
} // namespace sealhip
