// What the host_adapter_*_check.cpp programs share: the seeded word stream and its fills, FNV-1a digests, the exception
// checks, empty host operands, a seeded key-switch key, the moduli of the command line and the digest line the Python
// tests look for. Include it after evaluator.hpp. Plain host C++17; every program keeps its own shapes, checks and main.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace adapter_check
{
    using namespace sealhip_host;

    // ---- SplitMix64: oracle_lib.SplitMix on the Python side
    static std::uint64_t splitmix(std::uint64_t &s)
    {
        std::uint64_t z = (s += 0x9E3779B97F4A7C15ULL);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    }

    // rows x n words, row r below mods[r % period]: oracle_lib.SplitMix.fill(rows, n, mods[:period] * (rows / period))
    static void fill_rows(std::uint64_t *words, std::size_t rows, std::size_t n, const std::uint64_t *mods, std::size_t period,
                          std::uint64_t &state)
    {
        for (std::size_t r = 0; r < rows; r++)
            for (std::size_t i = 0; i < n; i++)
                words[r * n + i] = splitmix(state) % mods[r % period];
    }

    // nd digits x 2 x nk rows drawn from the stream
    static std::unique_ptr<KSwitchKeys> seeded_key(const Context &ctx, std::size_t nd, std::size_t nk, std::size_t n,
                                                   const std::uint64_t *mods, std::uint64_t &state)
    {
        std::vector<std::uint64_t> w(nd * 2 * nk * n);
        fill_rows(w.data(), nd * 2 * nk, n, mods, nk, state);
        return std::unique_ptr<KSwitchKeys>(new KSwitchKeys(ctx, w.data(), std::uint32_t(nd)));
    }

    // ---- FNV-1a over the bytes in memory order: oracle_lib.fnv on the Python side
    static const std::uint64_t kFnvBasis = 0xcbf29ce484222325ULL;

    static std::uint64_t digest(std::uint64_t h, const unsigned char *p, std::size_t len)
    {
        for (std::size_t i = 0; i < len; i++)
        {
            h ^= p[i];
            h *= 0x100000001b3ULL;
        }
        return h;
    }

    static std::uint64_t digest(std::uint64_t h, const std::uint64_t *w, std::size_t words)
    {
        return digest(h, reinterpret_cast<const unsigned char *>(w), words * 8);
    }

    static std::uint64_t digest(const unsigned char *p, std::size_t len)
    {
        return digest(kFnvBasis, p, len);
    }

    static std::uint64_t digest(const std::uint64_t *w, std::size_t words)
    {
        return digest(kFnvBasis, w, words);
    }

    static std::uint64_t digest(const std::vector<std::uint64_t> &w)
    {
        return digest(kFnvBasis, w.data(), w.size());
    }

    // "<what> digest <16 hex digits> meta <0|1>"
    static void print_digest(const char *what, std::uint64_t h, bool meta)
    {
        std::printf("%s digest %016llx meta %d\n", what, static_cast<unsigned long long>(h), int(meta));
    }

    // ---- f() must throw an E whose message matches msg
    template <class E, class F, class M>
    static bool throws_matching(F &&f, const char *msg, M &&matches)
    {
        try
        {
            f();
        }
        catch (const E &e)
        {
            if (matches(e.what()))
                return true;
            std::printf("wrong message: '%s' (want '%s')\n", e.what(), msg);
            return false;
        }
        catch (const std::exception &e)
        {
            std::printf("wrong exception: '%s' (want '%s')\n", e.what(), msg);
            return false;
        }
        std::printf("no exception (want '%s')\n", msg);
        return false;
    }

    // the message contains msg
    template <class E, class F>
    static bool throws(F &&f, const char *msg)
    {
        return throws_matching<E>(f, msg, [msg](const char *what) { return std::strstr(what, msg) != nullptr; });
    }

    // the message begins with msg
    template <class E, class F>
    static bool throws_prefix(F &&f, const char *msg)
    {
        return throws_matching<E>(f, msg, [msg](const char *what) { return std::strncmp(what, msg, std::strlen(msg)) == 0; });
    }

    // the message is msg
    template <class E, class F>
    static bool throws_exact(F &&f, const char *msg)
    {
        return throws_matching<E>(f, msg, [msg](const char *what) { return std::strcmp(what, msg) == 0; });
    }

    // f() must throw an E, whatever it says
    template <class E, class F>
    static bool throws(F &&f)
    {
        try
        {
            f();
        }
        catch (const E &)
        {
            return true;
        }
        catch (const std::exception &e)
        {
            std::printf("wrong exception: '%s'\n", e.what());
            return false;
        }
        return false;
    }

    // ---- operands with a shape and no content
    static HostCiphertext host_ct(std::size_t size, std::size_t k, std::size_t n, bool ntt, double scale = 1.0)
    {
        HostCiphertext c;
        c.n_ = n;
        c.resize_raw(size, k);
        c.ntt_form_ = ntt;
        c.scale_ = scale;
        return c;
    }

    static HostPlaintext host_plain(std::size_t k, std::size_t n, bool ntt, double scale)
    {
        HostPlaintext p;
        p.words.assign(k * n, 1);
        p.k = k;
        p.ntt_form = ntt;
        p.scale = scale;
        return p;
    }

    // ---- argv[first .. first + count) as decimal moduli
    static void parse_moduli(char **argv, int first, int count, std::uint64_t *mods)
    {
        for (int i = 0; i < count; i++)
            mods[i] = std::strtoull(argv[first + i], nullptr, 10);
    }
} // namespace adapter_check

using namespace adapter_check;
