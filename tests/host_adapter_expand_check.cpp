// The C++ host adapter's oblivious expansion and sums against plaintext rows (gemini-seal_amd/host/evaluator.hpp:
// Evaluator::expand / dot_plain).
// argv[1] = "host": on a host-only context, the checks the adapter makes itself and their exception classes.
// argv[1] = device ordinal, argv[2..5] = four key primes (CKKS, N = 4096, one special prime): digests of the expanded
// ciphertexts and of the sums for seeded inputs, which the Python test compares with the C ABI's output for the same inputs,
// and the exceptions of the refusals that reach the ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    sealhip_params p{ SEALHIP_SCHEME_CKKS, 8, 4, 2, mods, 0ULL, SEALHIP_MODE_STRICT, -1 };
    Context ctx(p);
    Evaluator<HostCiphertext> ev(ctx);
    const std::map<std::uint32_t, const KSwitchKeys *> none;
    bool ok = true;
    DeviceCiphertext d(ctx);
    std::vector<DeviceCiphertext> outs, terms;
    const std::vector<std::vector<const DevicePlaintext *>> no_plains;
    ok &= throws<std::invalid_argument>([&] { ev.expand(d, 4, none, outs); }, "CKKS encrypted must be in NTT form");
    d.is_ntt_form() = true;
    ok &= throws<std::invalid_argument>([&] { ev.expand(d, 4, none, outs); }, "encrypted size must be 2");
    ok &= throws<std::invalid_argument>([&] { ev.dot_plain(terms, no_plains, outs); }, "must not be empty");
    // a term of size 3 among size-2 terms (shapes without words: the checks come before any device work)
    for (std::size_t i = 0; i < 2; i++)
    {
        terms.emplace_back(ctx);
        terms[i].adopt(nullptr, 0, 2 + i, 2);
        terms[i].is_ntt_form() = true;
    }
    const std::vector<std::vector<const DevicePlaintext *>> null_plains{ { nullptr, nullptr } };
    ok &= throws<std::invalid_argument>([&] { ev.dot_plain(terms, null_plains, outs); }, "encrypted parameter mismatch");
    ok &= outs.empty();
    if (!ok)
        return 1;
    std::printf("host-only expand checks ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    try
    {
        if (argc < 2 || std::strcmp(argv[1], "host") == 0)
            return host_checks();
        if (argc < 6)
            return 2;
        const int device = std::atoi(argv[1]);
        std::uint64_t mods[4];
        parse_moduli(argv, 2, 4, mods);
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3, n_out = 4, n_sums = 2;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, 0, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x28E4A;
        HostCiphertext ct = host_ct(2, k, n, true);
        ct.scale_ = 1048576.0;
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        for (std::uint32_t elt : { 2049u, 4097u }) // N / 2 + 1 and N + 1: the expansion into 4
        {
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elt] = keys.back().get();
        }
        std::vector<DevicePlaintext> plains;
        for (std::size_t i = 0; i < n_sums * n_out; i++)
        {
            std::vector<std::uint64_t> w(k * n);
            fill_rows(w.data(), k, n, mods, k, state);
            plains.emplace_back(ctx);
            plains.back().upload(w, true);
            plains.back().scale() = 4.0;
        }
        Evaluator<HostCiphertext> ev(ctx);
        DeviceCiphertext d(ctx);
        d.upload(ct);
        std::vector<DeviceCiphertext> outs;
        ev.expand(d, n_out, gk, outs, true);
        std::uint64_t h = kFnvBasis;
        bool meta = outs.size() == n_out;
        for (DeviceCiphertext &o : outs)
        {
            HostCiphertext back;
            o.download(back);
            h = digest(h, back.words.data(), back.words.size());
            meta &= back.size() == 2 && back.coeff_modulus_size() == k && back.is_ntt_form() && back.scale() == ct.scale();
        }
        print_digest("device expand", h, meta);
        std::vector<std::vector<const DevicePlaintext *>> rows(n_sums);
        for (std::size_t s = 0; s < n_sums; s++)
            for (std::size_t i = 0; i < n_out; i++)
                rows[s].push_back(&plains[s * n_out + i]);
        std::vector<DeviceCiphertext> sums;
        ev.dot_plain(outs, rows, sums);
        h = kFnvBasis;
        meta = sums.size() == n_sums;
        for (DeviceCiphertext &o : sums)
        {
            HostCiphertext back;
            o.download(back);
            h = digest(h, back.words.data(), back.words.size());
            meta &= back.size() == 2 && back.coeff_modulus_size() == k && back.is_ntt_form() && back.scale() == ct.scale() * 4.0;
        }
        print_digest("device dot_plain", h, meta);
        // the refusals: E_INVALIDARG arrives as std::invalid_argument, and a refused call leaves the destinations alone
        bool ok = throws<std::invalid_argument>([&] { ev.expand(d, 8, gk, outs); }, "Galois key not present");
        ok &= throws<std::invalid_argument>([&] { ev.expand(d, 3, gk, outs); }, "power of two");
        rows[1].pop_back();
        ok &= throws<std::invalid_argument>([&] { ev.dot_plain(outs, rows, sums); }, "one plaintext per term");
        ok &= outs.size() == n_out && sums.size() == n_sums;
        std::printf("refusals %s\n", ok ? "ok" : "wrong");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
