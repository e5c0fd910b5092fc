// The C++ host adapter's hoisted rotations (gemini-seal_amd/host/evaluator.hpp: apply_galois_many, rotate_vector_many).
// argv[1] = "host": on host-only contexts, the operand checks and their messages, the missing key, the empty list, and a
// valid call reaching the ABI (which has no CPU fallback). argv[1] = device ordinal, argv[2..5] = four key primes (CKKS,
// N = 4096, one special prime): digests of the results on the host ciphertext type and on DeviceCiphertext for seeded
// inputs, which the Python test compares with the C ABI's output for the same inputs.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../gemini-seal_amd/host/evaluator.hpp"
#include "adapter_check.hpp"

using namespace sealhip_host;

static int host_checks()
{
    const std::uint64_t mods[4] = { 1073738753ULL, 1099511603713ULL, 1152921504606830593ULL, 1152921504606844417ULL };
    const std::size_t n = 256;
    bool ok = true;
    for (std::uint32_t scheme : { SEALHIP_SCHEME_BFV, SEALHIP_SCHEME_CKKS })
    {
        const bool bfv = scheme == SEALHIP_SCHEME_BFV;
        sealhip_params p{ scheme, 8, 4, 2, mods, bfv ? 786433ULL : 0ULL, SEALHIP_MODE_STRICT, -1 };
        Context ctx(p);
        Evaluator<HostCiphertext> ev(ctx);
        const std::map<std::uint32_t, const KSwitchKeys *> none;
        std::vector<HostCiphertext> out(3);
        std::vector<DeviceCiphertext> dout;
        const HostCiphertext good = host_ct(2, 2, n, !bfv), wrong_form = host_ct(2, 2, n, bfv), three = host_ct(3, 2, n, !bfv);
        const char *form = bfv ? "BFV encrypted cannot be in NTT form" : "CKKS encrypted must be in NTT form";
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_many(wrong_form, { 3 }, none, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.rotate_vector_many(wrong_form, { 1 }, none, out); }, form);
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_many(three, { 3 }, none, out); }, "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.rotate_vector_many(three, { 1 }, none, out); }, "encrypted size must be 2");
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_many(good, { 3 }, none, out); }, "Galois key not present");
        ok &= out.size() == 3; // (a refused call leaves the destinations alone)
        // the ABI entry reads a key for every element: the identity is not exempt here
        ok &= throws<std::invalid_argument>([&] { ev.apply_galois_many(good, { 1 }, none, out); }, "Galois key not present");
        // a map entry without a key is left out of rotate_vector_many's lists: the refusal is the missing device's
        const std::map<std::uint32_t, const KSwitchKeys *> null_entry{ { 3, nullptr } };
        ok &= throws<std::logic_error>([&] { ev.rotate_vector_many(good, { 0 }, null_entry, out); }, "host-only");
        ok &= out.size() == 3;
        ev.apply_galois_many(good, {}, none, out);
        ok &= out.empty();
        out.resize(2);
        ev.rotate_vector_many(good, {}, none, out);
        ok &= out.empty();
        // a valid call (step 0 needs no key) reaches the device, which a host-only context does not have
        ok &= throws<std::logic_error>([&] { ev.rotate_vector_many(good, { 0 }, none, out); }, "host-only");
        if (!bfv) // an empty resident ciphertext: coefficient form, size 0
        {
            DeviceCiphertext d(ctx);
            ok &= throws<std::invalid_argument>([&] { ev.rotate_vector_many(d, { 0 }, none, dout); }, form);
        }
        else
        {
            DeviceCiphertext d(ctx);
            ok &= throws<std::invalid_argument>([&] { ev.apply_galois_many(d, { 3 }, none, dout); }, "encrypted size must be 2");
        }
    }
    if (!ok)
        return 1;
    std::printf("host-only hoist checks ok\n");
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
        const std::size_t n = 4096, k = 3, nk = 4, nd = 3;
        sealhip_params p{ SEALHIP_SCHEME_CKKS, 12, 4, 1, mods, 0, SEALHIP_MODE_PARITY, device };
        Context ctx(p);
        std::uint64_t state = 0x4015;
        HostCiphertext ct = host_ct(2, k, n, true);
        ct.scale_ = 1048576.0;
        fill_rows(ct.words.data(), 2 * k, n, mods, k, state);
        std::uint32_t elts[2];
        throw_on(sealhip_galois_elt_from_step(ctx.get(), 1, &elts[0]));
        throw_on(sealhip_galois_elt_from_step(ctx.get(), -2, &elts[1]));
        std::vector<std::unique_ptr<KSwitchKeys>> keys;
        std::map<std::uint32_t, const KSwitchKeys *> gk;
        for (int e = 0; e < 2; e++)
        {
            keys.push_back(seeded_key(ctx, nd, nk, n, mods, state));
            gk[elts[e]] = keys.back().get();
        }
        Evaluator<HostCiphertext> ev(ctx);
        const std::vector<std::uint32_t> ge{ elts[0], elts[1] };
        const std::vector<int> steps{ 1, 0, -2 };
        auto report = [&](const char *what, const std::vector<HostCiphertext> &out) {
            std::uint64_t h = kFnvBasis;
            bool meta = true;
            for (auto &c : out)
            {
                h = digest(h, c.data(), c.words.size());
                meta = meta && c.size() == 2 && c.coeff_modulus_size() == k && c.is_ntt_form() && c.scale() == ct.scale();
            }
            std::printf("%s digest %016llx count %zu meta %d\n", what, static_cast<unsigned long long>(h), out.size(), int(meta));
        };
        std::vector<HostCiphertext> out;
        ev.apply_galois_many(ct, ge, gk, out);
        report("host apply_galois_many", out);
        ev.rotate_vector_many(ct, steps, gk, out);
        report("host rotate_vector_many", out);
        DeviceCiphertext d(ctx);
        d.upload(ct);
        std::vector<DeviceCiphertext> dout;
        auto down = [&](const char *what) {
            std::vector<HostCiphertext> back(dout.size());
            for (std::size_t i = 0; i < dout.size(); i++)
                dout[i].download(back[i]);
            report(what, back);
        };
        ev.apply_galois_many(d, ge, gk, dout);
        down("device apply_galois_many");
        ev.rotate_vector_many(d, steps, gk, dout);
        down("device rotate_vector_many");
        // the deferred transparency check: a resident operand with c1 = 0 gives transparent results, reported at the
        // next host-visible point
        HostCiphertext z = ct;
        std::fill(z.words.begin() + k * n, z.words.end(), 0);
        DeviceCiphertext dz(ctx);
        dz.upload(z);
        ev.apply_galois_many(dz, ge, gk, dout);
        const bool late = throws<std::logic_error>([&] { ev.synchronize(); }, "result ciphertext is transparent");
        std::printf("deferred transparency %s\n", late ? "ok" : "missing");
    }
    catch (const std::exception &e)
    {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
