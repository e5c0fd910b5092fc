// evaluator.hpp -- C++ host adapter with seal::Evaluator's method names over the sealhip C ABI.
//
// seal::Evaluator is non-virtual and non-copyable (native/src/seal/evaluator.h:1316-1322), so this is not a
// subclass: it is a class with the same method names and argument meaning for the hot-path operations
// (evaluator.h:246-298 multiply/square, :344-371 relinearize, :396-430 mod_switch_to_next, :479-502 mod_switch_to, :565-583
// rescale_to_next, :606-629 rescale_to, :183 add_many, :902-947 transform_to/from_ntt, :984-1021 apply_galois, :1057-1103
// rotate_rows, :1131-1173 rotate_columns, :1201-1239 rotate_vector, :1269-1308 complex_conjugate, :859-900 transform_to_ntt
// and :430-548 mod_switch_to(_next) of plaintexts, and every destination-taking variant), doing
// the same metadata checks on the host and forwarding raw pointers to the ABI. It is a template over the
// ciphertext type so that it compiles both against seal::Ciphertext (where the reference headers exist) and
// against the plain sealhip::HostCiphertext of adapter_core.hpp (everywhere else, e.g. the GPU box).
//
// Required of CT: data() -> uint64_t*, size(), coeff_modulus_size(), poly_modulus_degree(), is_ntt_form()
// (assignable), resize_raw(size, coeff_modulus_size). For seal::Ciphertext the last one is
//   ct.resize(context, parms_id_of_level, size)  -- see INTEGRATION.md.
//
// Exceptions mirror the reference: std::invalid_argument / std::logic_error (evaluator.cpp:238-271).
//
// This is the one header to include. The Evaluator is here; what it stands on (Context, the resident types, the key and
// table handles) is in adapter_core.hpp, and Decryptor, Encryptor and KeyGenerator are in crypto.hpp.
#pragma once

#include "adapter_core.hpp"
#include "crypto.hpp"

namespace sealhip_host
{
    template <class CT>
    class Evaluator
    {
    public:
        explicit Evaluator(const Context &context) : ctx_(context) {}
        ~Evaluator() { ctx_.drop_transparency(this); }

        // Every method on CT has an overload on DeviceCiphertext (the same template): the same host checks and messages,
        // the same ABI entries, but the operands are used in place in their pool blocks. Once the pool is warm a resident
        // call makes no hipMalloc / hipFree, no host<->device copy and no synchronisation; a result that grows or moves to
        // another level gets a pool block and the old one is released stream-ordered. Resident results are also checked
        // for transparency as under SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT (after exactly the operations the reference
        // checks), but LATE: the std::logic_error("result ciphertext is transparent") arrives at the calling thread's next
        // host-visible point -- DeviceCiphertext::download / save, Evaluator::synchronize(), or a full ring of flags. The
        // host overloads do not check (as before). Plaintext operands are host words, staged through the pool per call.
        template <class C>
        using IfCt = typename std::enable_if<std::is_same<C, CT>::value || std::is_same<C, DeviceCiphertext>::value, int>::type;
        // a plaintext operand: host words (staged through the pool per call) or a DevicePlaintext (used in place)
        template <class P>
        using IfPlain = typename std::enable_if<std::is_convertible<P, const std::uint64_t *>::value ||
                                                    std::is_same<P, DevicePlaintext>::value,
                                                int>::type;

        // waits for this thread's work on the context; a host-visible point of the deferred transparency check
        void synchronize()
        {
            throw_on(sealhip_synchronize(ctx_.get()));
            ctx_.check_transparency();
        }

        // Evaluator::multiply_inplace (evaluator.cpp:235-272)
        template <class C, IfCt<C> = 0>
        void multiply_inplace(C &encrypted1, const C &encrypted2)
        {
            check_multiply(encrypted1, encrypted2);
            const std::size_t k = encrypted1.coeff_modulus_size(), n = ctx_.n();
            const std::size_t s1 = encrypted1.size(), s2 = encrypted2.size(), dest = s1 + s2 - 1;
            Dev a = dev_in(encrypted1, s1 * k * n), b = dev_in(encrypted2, s2 * k * n), o = dev_out(dest * k * n);
            Check chk = checked(encrypted1);
            throw_on(sealhip_evaluator_multiply(ctx_.get(), std::uint32_t(k), a.ptr(), std::uint32_t(s1), b.ptr(),
                                                std::uint32_t(s2), 1, o.ptr()));
            chk.done();
            commit(encrypted1, o, dest, k); // :324 / :484
        }

        // Evaluator::square_inplace (evaluator.cpp:529-558) on its own entry (bfv_square / ckks_square, :560-770): the same
        // canonical residues as multiply_inplace(encrypted, encrypted)
        template <class C, IfCt<C> = 0>
        void square_inplace(C &encrypted)
        {
            check_multiply(encrypted, encrypted);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), s = encrypted.size(), dest = 2 * s - 1;
            Dev a = dev_in(encrypted, s * k * n), o = dev_out(dest * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_square(ctx_.get(), std::uint32_t(k), a.ptr(), std::uint32_t(s), 1, o.ptr()));
            chk.done();
            commit(encrypted, o, dest, k);
        }

        // Evaluator::relinearize_inplace (evaluator.cpp:772-827); relin_keys[i] = key of get_index(i + 2)
        template <class C, IfCt<C> = 0>
        void relinearize_inplace(C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            if (size < 2)
                throw std::invalid_argument("encrypted is not valid for encryption parameters");
            if (relin_keys.size() + 2 < size)
                throw std::invalid_argument("not enough relinearization keys"); // :793-796
            if (size == 2)
                return;
            const std::vector<const sealhip_kswitch_key *> raw = raw_relin_keys(relin_keys);
            Dev c = dev_in(encrypted, size * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_relinearize(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1,
                                                   raw.data(), std::uint32_t(raw.size())));
            chk.done();
            dev_back(encrypted, c, size * k * n);
            shrink(encrypted, 2); // :819
        }

        // Evaluator::mod_switch_to_next_inplace (evaluator.cpp:996-1036)
        template <class C, IfCt<C> = 0>
        void mod_switch_to_next_inplace(C &encrypted) { switch_level(encrypted, false); }
        // Evaluator::rescale_to_next_inplace (evaluator.cpp:1090-1126); the caller updates scale() /= q_last (:889-890)
        template <class C, IfCt<C> = 0>
        void rescale_to_next_inplace(C &encrypted) { switch_level(encrypted, true); }

        template <class C, IfCt<C> = 0>
        void transform_to_ntt_inplace(C &encrypted)
        {
            if (encrypted.is_ntt_form())
                throw std::invalid_argument("encrypted is already in NTT form"); // :1759-1762
            transform(encrypted, true);
            encrypted.is_ntt_form() = true;
        }
        template <class C, IfCt<C> = 0>
        void transform_from_ntt_inplace(C &encrypted_ntt)
        {
            if (!encrypted_ntt.is_ntt_form())
                throw std::invalid_argument("encrypted_ntt is not in NTT form"); // :1807-1810
            transform(encrypted_ntt, false);
            encrypted_ntt.is_ntt_form() = false;
        }

        // Evaluator::apply_galois_inplace (evaluator.cpp:1841-1943)
        template <class C, IfCt<C> = 0>
        void apply_galois_inplace(C &encrypted, std::uint32_t galois_elt, const KSwitchKeys &galois_key)
        {
            if (encrypted.size() > 2)
                throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n();
            Dev c = dev_in(encrypted, 2 * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_apply_galois(ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elt,
                                                    galois_key.get()));
            chk.done();
            dev_back(encrypted, c, 2 * k * n);
        }

        // Evaluator::rotate_vector_inplace (evaluator.h:1201-1211): CKKS only, then rotate_internal
        template <class C, IfCt<C> = 0>
        void rotate_vector_inplace(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // :1205-1208
            rotate_vector_like(encrypted, steps, galois_keys);
        }
        // rotate_internal (evaluator.cpp:1945-2000): one automorphism when its key is present, else the NAF of the step count
        template <class C, IfCt<C> = 0>
        void rotate_vector_like(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (steps == 0)
                return;
            std::uint32_t elt = 0;
            throw_on(sealhip_galois_elt_from_step(ctx_.get(), steps, &elt));
            auto it = galois_keys.find(elt);
            if (it != galois_keys.end())
                return apply_galois_inplace(encrypted, elt, *it->second);
            std::vector<int> naf; // util/numth.h:22-42
            bool neg = steps < 0;
            int v = neg ? -steps : steps;
            for (int i = 0; v; i++)
            {
                int zi = (v % 2) ? 2 - (v % 4) : 0;
                v = (v - zi) / 2;
                if (zi)
                    naf.push_back((neg ? -zi : zi) * (1 << i));
            }
            if (naf.size() == 1)
                throw std::invalid_argument("Galois key not present"); // :1985-1988
            for (int s : naf)
                if (std::size_t(s < 0 ? -s : s) != (ctx_.n() >> 1))
                    rotate_vector_like(encrypted, s, galois_keys);
        }

        // Evaluator::rotate_rows_inplace (evaluator.h:1057-1067): BFV only, then rotate_internal like rotate_vector
        template <class C, IfCt<C> = 0>
        void rotate_rows_inplace(C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            require_scheme(SEALHIP_SCHEME_BFV); // :1061-1064
            rotate_vector_like(encrypted, steps, galois_keys);
        }
        // Evaluator::rotate_columns_inplace (evaluator.h:1131-1139): BFV only; conjugate_internal = apply_galois with
        // get_elt_from_step(0) = 2N - 1 (:1343-1363)
        template <class C, IfCt<C> = 0>
        void rotate_columns_inplace(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            require_scheme(SEALHIP_SCHEME_BFV); // :1134-1137
            conjugate_internal(encrypted, galois_keys);
        }
        // Evaluator::complex_conjugate_inplace (evaluator.h:1269-1277): CKKS only, the same automorphism
        template <class C, IfCt<C> = 0>
        void complex_conjugate_inplace(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // :1272-1275
            conjugate_internal(encrypted, galois_keys);
        }

        // Hoisted rotation (sealhip_evaluator_apply_galois_many): `encrypted` under every element of
        // galois_elts with one decomposition of its second polynomial; destinations[i] is the result of galois_elts[i], with
        // the operand's scale / NTT form (and, for a host type, its parms_id). The reference has no such method: each result
        // decrypts like apply_galois's, with noise of the same bound, but is not the same words. An element without its key
        // in galois_keys -> std::invalid_argument("Galois key not present"). BFV needs a STRICT context.
        // The ABI writes all results back to back into one block. A resident destination owns a pool block of its own, so
        // every result but a single one is copied once more on the device (2 k N words each, stream-ordered); and the
        // deferred transparency check takes one ring slot per result, so a resident call takes at most 256 elements
        // (std::invalid_argument("too many results for one checked operation")): split longer lists. Host destinations
        // have neither: they are downloaded straight from the one block, and not checked.
        template <class C, IfCt<C> = 0>
        void apply_galois_many(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                               const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, std::vector<C> &destinations)
        {
            check_galois_operand(encrypted);
            // (the ABI entry reads a key for every element: the identity is not exempt here)
            const std::vector<const sealhip_kswitch_key *> raw = keys_of(galois_elts, galois_keys, false);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), count = galois_elts.size(), words = 2 * k * n;
            if (count == 0)
                return destinations.clear();
            Dev c = dev_in(encrypted, words), o = dev_out(count * words);
            Check chk = checked(encrypted, count);
            throw_on(sealhip_evaluator_apply_galois_many(ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elts.data(), raw.data(),
                                                         std::uint32_t(count), o.ptr()));
            chk.done();
            scatter(encrypted, o, count, words, destinations);
        }
        // The same by rotation steps (sealhip_evaluator_rotate_vector_many): rotate_vector's steps for CKKS, rotate_rows'
        // for BFV; a step of 0 copies the operand; no non-adjacent-form fallback (a chain cannot share a decomposition)
        template <class C, IfCt<C> = 0>
        void rotate_vector_many(const C &encrypted, const std::vector<int> &steps,
                                const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, std::vector<C> &destinations)
        {
            check_galois_operand(encrypted);
            const KeyLists keys = key_lists(galois_keys);
            std::vector<std::int32_t> st(steps.begin(), steps.end());
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), count = st.size(), words = 2 * k * n;
            if (count == 0)
                return destinations.clear();
            Dev c = dev_in(encrypted, words), o = dev_out(count * words);
            Check chk = checked(encrypted, count);
            throw_on(sealhip_evaluator_rotate_vector_many(ctx_.get(), std::uint32_t(k), c.ptr(), 1, st.data(), std::uint32_t(count),
                                                          keys.elts.data(), keys.raw.data(), std::uint32_t(keys.elts.size()),
                                                          o.ptr()));
            chk.done();
            scatter(encrypted, o, count, words, destinations);
        }

        // Ring packing (sealhip_evaluator_extract_lwe / _pack_lwes), on resident ciphertexts. The
        // reference has no such methods. extract_lwe: the LWE samples of the coefficients `indices` (each below N, any
        // order, repeats allowed) of a size-2 ciphertext, which is not modified. pack_lwes: n = 2^l samples into one
        // ciphertext, sample j at coefficient (N / n) j, times n -- times N with `trace`, which also clears every other
        // coefficient, times 1 with `normalize`; galois_keys holds the elements of sealhip_pack_lwes_galois_elts (an absent
        // one -> std::invalid_argument("Galois key not present")); the destination gets the samples' level and scale and
        // the scheme's form, and one deferred transparency slot. BFV needs a STRICT context.
        void extract_lwe(const DeviceCiphertext &encrypted, const std::vector<std::uint32_t> &indices, LweSamples &destination)
        {
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2");
            const std::size_t k = encrypted.coeff_modulus_size();
            LweSamples next(ctx_);
            next.reset(indices.size(), k);
            throw_on(sealhip_evaluator_extract_lwe(ctx_.get(), std::uint32_t(k), encrypted.data(), 1, indices.data(), indices.size(),
                                                   next.a_out(), next.b_out()));
            next.scale() = encrypted.scale();
            destination = std::move(next);
        }
        void pack_lwes(const LweSamples &samples, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       DeviceCiphertext &destination, bool trace = false, bool normalize = false)
        {
            if (!samples.a())
                throw std::invalid_argument("samples are empty");
            const KeyLists keys = key_lists(galois_keys);
            const std::size_t k = samples.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev o = dev_out(words);
            Check chk = checked(destination);
            throw_on(sealhip_evaluator_pack_lwes(ctx_.get(), std::uint32_t(k), samples.a(), samples.b(), samples.size(), 1,
                                                 keys.elts.data(), keys.raw.data(), std::uint32_t(keys.elts.size()), trace ? 1 : 0,
                                                 normalize ? 1 : 0, o.ptr()));
            chk.done();
            destination.adopt(o.st->release(), words, 2, k);
            destination.is_ntt_form() = ctx_.scheme() == SEALHIP_SCHEME_CKKS;
            destination.scale() = samples.scale();
        }

        // Oblivious expansion (sealhip_evaluator_expand): `encrypted`, whose phase carries n = 2^l values
        // in its first n coefficients, into n ciphertexts; destinations[i] holds n times coefficient i of the phase as its
        // constant coefficient (1 times with `normalize`), with the operand's level, scale and form (and, for a host type,
        // its parms_id). galois_keys holds the elements of sealhip_expand_galois_elts (an absent one ->
        // std::invalid_argument("Galois key not present")). The reference has no such method. BFV needs a STRICT context.
        // One block from the ABI, then one pool block and one deferred transparency slot per result, as apply_galois_many's:
        // a resident call takes at most 256 results (std::invalid_argument("too many results for one checked operation")).
        template <class C, IfCt<C> = 0>
        void expand(const C &encrypted, std::size_t n, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                    std::vector<C> &destinations, bool normalize = false)
        {
            check_galois_operand(encrypted);
            if (n == 0)
                throw std::invalid_argument("n must be a power of two between 1 and N");
            const KeyLists keys = key_lists(galois_keys);
            const std::size_t k = encrypted.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev c = dev_in(encrypted, words), o = dev_out(n * words);
            Check chk = checked(encrypted, n);
            throw_on(sealhip_evaluator_expand(ctx_.get(), std::uint32_t(k), c.ptr(), 1, n, keys.elts.data(), keys.raw.data(),
                                              std::uint32_t(keys.elts.size()), normalize ? 1 : 0, o.ptr()));
            chk.done();
            scatter(encrypted, o, n, words, destinations);
        }

        // Sums against plaintext rows (sealhip_evaluator_dot_plain) on resident operands:
        // destinations[s] = sum_i terms[i] (.) plains[s][i], everything in NTT form at one level: the ciphertexts of one size
        // and (CKKS) one scale, the plaintexts k x N words in NTT form and (CKKS) of one scale. Each result has the terms'
        // size, level and form and, for CKKS, the scale terms[0].scale() * plains[0][0].scale(). The ABI reads the terms and
        // the plaintexts from one block each: they are gathered on the device (stream-ordered copies). One pool block and
        // one deferred transparency slot per sum. std::invalid_argument: no terms or no sums, terms that differ in size,
        // level or scale or are not in NTT form, a ragged plaintext matrix, a plaintext of another level, form or scale.
        void dot_plain(const std::vector<DeviceCiphertext> &terms, const std::vector<std::vector<const DevicePlaintext *>> &plains,
                       std::vector<DeviceCiphertext> &destinations)
        {
            if (terms.empty() || plains.empty())
                throw std::invalid_argument("the term list and the sums must not be empty");
            const bool ckks = ctx_.scheme() == SEALHIP_SCHEME_CKKS;
            const std::size_t size = terms[0].size(), k = terms[0].coeff_modulus_size(), n = ctx_.n();
            const std::size_t pw = k * n, words = size * pw, n_terms = terms.size(), n_sums = plains.size();
            for (const DeviceCiphertext &t : terms)
            {
                if (!t.is_ntt_form())
                    throw std::invalid_argument("encrypted must be in NTT form");
                if (t.size() != size || t.coeff_modulus_size() != k || t.size() < 2)
                    throw std::invalid_argument("encrypted parameter mismatch");
                if (ckks && t.scale() != terms[0].scale())
                    throw std::invalid_argument("scale mismatch");
            }
            for (const auto &row : plains)
            {
                if (row.size() != n_terms)
                    throw std::invalid_argument("plains must hold one plaintext per term in every sum");
                for (const DevicePlaintext *p : row)
                {
                    if (!p || !p->is_ntt_form() || p->coeff_modulus_size() != k || p->words() != pw)
                        throw std::invalid_argument("plain must be in NTT form at the terms' level");
                    if (ckks && p->scale() != plains[0][0]->scale())
                        throw std::invalid_argument("scale mismatch");
                }
            }
            Staged x(ctx_, n_terms * words), w(ctx_, n_sums * n_terms * pw);
            for (std::size_t i = 0; i < n_terms; i++)
                throw_on(sealhip_memcpy_d2d(ctx_.get(), x.ptr() + i * words, terms[i].data(), words * 8));
            for (std::size_t s = 0; s < n_sums; s++)
                for (std::size_t i = 0; i < n_terms; i++)
                    plain_to(plain_view(*plains[s][i]), w.ptr() + (s * n_terms + i) * pw, pw);
            Dev o = dev_out(n_sums * words);
            Check chk = checked(terms[0], n_sums);
            throw_on(sealhip_evaluator_dot_plain(ctx_.get(), std::uint32_t(k), x.ptr(), std::uint32_t(n_terms), std::uint32_t(size), 1,
                                                 w.ptr(), std::uint32_t(n_sums), o.ptr()));
            chk.done();
            const double scale = terms[0].scale() * plains[0][0]->scale(); // (the destinations may be the terms)
            scatter(terms[0], o, n_sums, words, destinations, k, size);
            for (DeviceCiphertext &d : destinations)
                if (ckks)
                    d.scale() = scale;
        }

        // Plaintext-weighted sums of rotations (sealhip_evaluator_apply_galois_dot_plain):
        // destinations[s] = sum_i plains[s][i] * sigma_{galois_elts[i]}(encrypted), with one decomposition of the operand's
        // second polynomial and one mod-down per sum. plains[s][i] is a plaintext in KEY-LEVEL NTT form (n_key x N words:
        // what CKKSEncoder::encode and transform_to_ntt give at the key level): a DevicePlaintext, or a host plaintext of
        // HostPlaintext's shape (words, k, ntt_form, scale). Element 1 needs no key. Each result has the operand's level
        // and NTT form and, for CKKS, the scale encrypted.scale() * plain.scale (all plaintexts must share one scale).
        // std::invalid_argument: a plaintext that is not key-level NTT form, a ragged plaintext matrix (a row whose length
        // is not galois_elts.size()), CKKS plaintexts of unequal scale, an element other than 1 without its key ("Galois
        // key not present"). The reference has no such method; the words are those of the ABI entry, not of the
        // composition. Resident destinations: one pool block and one deferred transparency slot per sum, as
        // apply_galois_many's.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_dot_plain(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                                    const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                    const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            dot_plain_internal(encrypted, galois_elts, galois_keys, plains, destinations, false);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_apply_galois_dot_plain_rescale,
        // DESIGN.md section 19): CKKS only; the unmerged method's checks, and "end of modulus switching chain reached" at the
        // last level. Each result is one level down with the scale encrypted.scale() * plain.scale / q_{k-1}.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_dot_plain_rescale(const C &encrypted, const std::vector<std::uint32_t> &galois_elts,
                                            const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                            const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            dot_plain_internal(encrypted, galois_elts, galois_keys, plains, destinations, true);
        }
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_dot_plain_rescale(const C &encrypted, const std::vector<int> &steps,
                                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                             const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // evaluator.h:1205-1208
            dot_plain_internal(encrypted, elts_of_steps(steps), galois_keys, plains, destinations, true);
        }
        // The same by rotation steps (sealhip_evaluator_rotate_vector_dot_plain): CKKS rotate_vector's steps; step 0 is the
        // identity; no non-adjacent-form fallback
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_dot_plain(const C &encrypted, const std::vector<int> &steps,
                                     const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                     const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // evaluator.h:1205-1208
            apply_galois_dot_plain(encrypted, elts_of_steps(steps), galois_keys, plains, destinations);
        }
        // ... and BFV rotate_rows' steps
        template <class C, class P, IfCt<C> = 0>
        void rotate_rows_dot_plain(const C &encrypted, const std::vector<int> &steps,
                                   const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                   const std::vector<std::vector<P>> &plains, std::vector<C> &destinations)
        {
            require_scheme(SEALHIP_SCHEME_BFV); // evaluator.h:1061-1064
            apply_galois_dot_plain(encrypted, elts_of_steps(steps), galois_keys, plains, destinations);
        }

        // Baby-step/giant-step matrix-vector product (sealhip_evaluator_apply_galois_bsgs_plain):
        // destination = sum_j sigma_{giant_elts[j]}( sum_i plains[j][i] * sigma_{baby_elts[i]}(encrypted) ), the giant steps
        // accumulated in the extended basis and ONE full mod-down. plains[giant][baby]: key-level NTT form, DevicePlaintext
        // or host plaintexts, as apply_galois_dot_plain's; element 1 needs no key on either axis; one set of keys serves
        // both. The result has the operand's level and NTT form and, for CKKS, the scale encrypted.scale() * plain.scale.
        // std::invalid_argument as apply_galois_dot_plain (a row whose length is not baby_elts.size(), a matrix without
        // giant_elts.size() rows). The words are those of the ABI entry, not of the composition.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_bsgs_plain(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                     const std::vector<std::uint32_t> &giant_elts,
                                     const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                     const std::vector<std::vector<P>> &plains, C &destination)
        {
            bsgs_plain_internal(encrypted, baby_elts, giant_elts, galois_keys, plains, destination, false);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_apply_galois_bsgs_plain_rescale,
        // DESIGN.md section 19): CKKS only; the unmerged method's checks, and "end of modulus switching chain reached" at the
        // last level. The result is one level down with the scale encrypted.scale() * plain.scale / q_{k-1}.
        template <class C, class P, IfCt<C> = 0>
        void apply_galois_bsgs_plain_rescale(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                             const std::vector<std::uint32_t> &giant_elts,
                                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                             const std::vector<std::vector<P>> &plains, C &destination)
        {
            bsgs_plain_internal(encrypted, baby_elts, giant_elts, galois_keys, plains, destination, true);
        }
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_bsgs_plain_rescale(const C &encrypted, const std::vector<int> &baby_steps,
                                              const std::vector<int> &giant_steps,
                                              const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                              const std::vector<std::vector<P>> &plains, C &destination)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // evaluator.h:1205-1208
            bsgs_plain_internal(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains, destination,
                                true);
        }

        // CoeffToSlot in one call (sealhip_evaluator_coeffs_to_slots): slot j of destination_re /
        // destination_im holds coefficient bitrev(j) / bitrev(j) + N/2 of the operand's message over its scale. The results
        // are dft.out_level() primes long at the operand's scale. galois_keys: element -> key, with the keys of
        // dft.key_steps() and of element 2N - 1.
        template <class C, IfCt<C> = 0>
        void coeffs_to_slots(const C &encrypted, const HomomorphicDFT &dft,
                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination_re,
                             C &destination_im)
        {
            check_dft_operand(encrypted, dft, SEALHIP_DFT_COEFFS_TO_SLOTS);
            const KeyLists keys = key_lists(galois_keys);
            const std::size_t n = ctx_.n(), words = 2 * dft.in_level() * n, out_words = 2 * dft.out_level() * n;
            Dev c = dev_in(encrypted, words), o = dev_out(2 * out_words);
            Check chk = checked(encrypted, 2);
            throw_on(sealhip_evaluator_coeffs_to_slots(ctx_.get(), dft.get(), c.ptr(), 1, keys.elts.data(), keys.raw.data(),
                                                       std::uint32_t(keys.elts.size()), o.ptr(), o.ptr() + out_words));
            chk.done();
            std::vector<C> two;
            scatter(encrypted, o, 2, out_words, two, dft.out_level());
            destination_re = std::move(two[0]);
            destination_im = std::move(two[1]);
        }
        // SlotToCoeff in one call (sealhip_evaluator_slots_to_coeffs): the inverse of coeffs_to_slots, from its slot order
        template <class C, IfCt<C> = 0>
        void slots_to_coeffs(const C &encrypted_re, const C &encrypted_im, const HomomorphicDFT &dft,
                             const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            check_dft_operand(encrypted_re, dft, SEALHIP_DFT_SLOTS_TO_COEFFS);
            check_dft_operand(encrypted_im, dft, SEALHIP_DFT_SLOTS_TO_COEFFS);
            if (encrypted_re.scale() != encrypted_im.scale())
                throw std::invalid_argument("scale mismatch");
            const KeyLists keys = key_lists(galois_keys);
            Dev im = dev_in(encrypted_im, 2 * dft.in_level() * ctx_.n());
            to_size2(encrypted_re, 2, dft.out_level(), destination, nullptr, [&](const std::uint64_t *re, std::uint64_t *o) {
                return sealhip_evaluator_slots_to_coeffs(ctx_.get(), dft.get(), re, im.ptr(), 1, keys.elts.data(), keys.raw.data(),
                                                         std::uint32_t(keys.elts.size()), o);
            });
        }

        // The matrix of `lt` applied to the slots of `encrypted` (sealhip_evaluator_linear_transform),
        // at the operand's level; with rescale the result is one level down. The result's scale is encrypted.scale() *
        // lt.scale(), divided by q_{k-1} with rescale. galois_keys: element -> key, with the keys of lt.key_steps(); a step
        // whose key is absent throws std::invalid_argument("Galois key not present").
        template <class C, IfCt<C> = 0>
        void linear_transform(const C &encrypted, const LinearTransform &lt,
                              const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination, bool rescale = false)
        {
            check_ckks_operand(encrypted); // (CKKS, the scheme's form, size 2)
            if (rescale)
                check_rescale_operand(encrypted);
            const KeyLists keys = key_lists(galois_keys);
            const std::size_t k = encrypted.coeff_modulus_size();
            const double scale = encrypted.scale() * lt.scale() / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
            to_size2(encrypted, 2, rescale ? k - 1 : k, destination, &scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_linear_transform(ctx_.get(), lt.get(), std::uint32_t(k), c, 1, keys.elts.data(),
                                                          keys.raw.data(), std::uint32_t(keys.elts.size()), rescale ? 1 : 0, o);
            });
        }

        // The same by rotation steps (sealhip_evaluator_rotate_vector_bsgs_plain): CKKS rotate_vector's steps; step 0 is the
        // identity; no non-adjacent-form fallback
        template <class C, class P, IfCt<C> = 0>
        void rotate_vector_bsgs_plain(const C &encrypted, const std::vector<int> &baby_steps, const std::vector<int> &giant_steps,
                                      const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                      const std::vector<std::vector<P>> &plains, C &destination)
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // evaluator.h:1205-1208
            apply_galois_bsgs_plain(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains,
                                    destination);
        }
        // ... and BFV rotate_rows' steps
        template <class C, class P, IfCt<C> = 0>
        void rotate_rows_bsgs_plain(const C &encrypted, const std::vector<int> &baby_steps, const std::vector<int> &giant_steps,
                                    const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                    const std::vector<std::vector<P>> &plains, C &destination)
        {
            require_scheme(SEALHIP_SCHEME_BFV); // evaluator.h:1061-1064
            apply_galois_bsgs_plain(encrypted, elts_of_steps(baby_steps), elts_of_steps(giant_steps), galois_keys, plains,
                                    destination);
        }

        // Evaluator::mod_switch_to_inplace (evaluator.cpp:1038-1060) / rescale_to_inplace (:1128-1165). The ABI names a level by
        // its number of primes k (the chain drops one prime per level, context.cpp:423-431); for seal::Ciphertext the
        // binding maps the parms_id argument to it.
        template <class C, IfCt<C> = 0>
        void mod_switch_to_inplace(C &encrypted, std::size_t target_coeff_modulus_size)
        {
            if (target_coeff_modulus_size < 1)
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1047-1050
            if (encrypted.coeff_modulus_size() < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1051-1054
            while (encrypted.coeff_modulus_size() != target_coeff_modulus_size)
                mod_switch_to_next_inplace(encrypted); // :1056-1059
        }
        template <class C, IfCt<C> = 0>
        void rescale_to_inplace(C &encrypted, std::size_t target_coeff_modulus_size)
        {
            if (target_coeff_modulus_size < 1)
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1137-1140
            if (encrypted.coeff_modulus_size() < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1141-1144
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::invalid_argument("unsupported operation for scheme type"); // :1146-1162
            while (encrypted.coeff_modulus_size() != target_coeff_modulus_size)
                rescale_to_next_inplace(encrypted);
        }
        // Evaluator::add_many (evaluator.cpp:153-172)
        template <class C, IfCt<C> = 0>
        void add_many(const std::vector<C> &encrypteds, C &destination)
        {
            if (encrypteds.empty())
                throw std::invalid_argument("encrypteds cannot be empty"); // :155-158
            for (const C &c : encrypteds)
                if (&c == &destination)
                    throw std::invalid_argument("encrypteds must be different from destination"); // :159-165
            destination = encrypteds[0];
            for (std::size_t i = 1; i < encrypteds.size(); i++)
                add_inplace(destination, encrypteds[i]);
        }

        // ---- destination-taking variants (evaluator.h:121-126, :156-168, :214-226, :268-284, :317-322, :371-376, :396-430,
        // :565-583, :916-947, :1021-1027, :1097-1103, :1167-1173, :1239-1245, :1302-1308): copy, then the in-place form
        template <class C, IfCt<C> = 0>
        void negate(const C &encrypted, C &destination) { destination = encrypted; negate_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void add(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // (:160-163: addition commutes, the alias is kept valid)
                add_inplace(destination, encrypted1);
            else
            {
                destination = encrypted1;
                add_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void sub(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // :216-222: destination = -(encrypted2 - encrypted1)
            {
                sub_inplace(destination, encrypted1);
                negate_inplace(destination);
            }
            else
            {
                destination = encrypted1;
                sub_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void multiply(const C &encrypted1, const C &encrypted2, C &destination)
        {
            if (&encrypted2 == &destination) // :272-275
                multiply_inplace(destination, encrypted1);
            else
            {
                destination = encrypted1;
                multiply_inplace(destination, encrypted2);
            }
        }
        template <class C, IfCt<C> = 0>
        void square(const C &encrypted, C &destination) { destination = encrypted; square_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void relinearize(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            destination = encrypted;
            relinearize_inplace(destination, relin_keys);
        }
        template <class C, IfCt<C> = 0>
        void mod_switch_to_next(const C &encrypted, C &destination) { destination = encrypted; mod_switch_to_next_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void rescale_to_next(const C &encrypted, C &destination) { destination = encrypted; rescale_to_next_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void mod_switch_to(const C &encrypted, std::size_t target_coeff_modulus_size, C &destination)
        {
            destination = encrypted;
            mod_switch_to_inplace(destination, target_coeff_modulus_size);
        }
        template <class C, IfCt<C> = 0>
        void rescale_to(const C &encrypted, std::size_t target_coeff_modulus_size, C &destination)
        {
            destination = encrypted;
            rescale_to_inplace(destination, target_coeff_modulus_size);
        }
        template <class C, IfCt<C> = 0>
        void transform_to_ntt(const C &encrypted, C &destination_ntt) { destination_ntt = encrypted; transform_to_ntt_inplace(destination_ntt); }
        template <class C, IfCt<C> = 0>
        void transform_from_ntt(const C &encrypted_ntt, C &destination) { destination = encrypted_ntt; transform_from_ntt_inplace(destination); }
        template <class C, IfCt<C> = 0>
        void apply_galois(const C &encrypted, std::uint32_t galois_elt, const KSwitchKeys &galois_key, C &destination)
        {
            destination = encrypted;
            apply_galois_inplace(destination, galois_elt, galois_key);
        }
        template <class C, IfCt<C> = 0>
        void rotate_vector(const C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_vector_inplace(destination, steps, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void rotate_rows(const C &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_rows_inplace(destination, steps, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void rotate_columns(const C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            rotate_columns_inplace(destination, galois_keys);
        }
        template <class C, IfCt<C> = 0>
        void complex_conjugate(const C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys, C &destination)
        {
            destination = encrypted;
            complex_conjugate_inplace(destination, galois_keys);
        }
        template <class C, class P, IfCt<C> = 0>
        void multiply_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            multiply_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, class P, IfCt<C> = 0>
        void add_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            add_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, class P, IfCt<C> = 0>
        void sub_plain(const C &encrypted, const P &plain, bool plain_is_ntt_form, C &destination)
        {
            destination = encrypted;
            sub_plain_inplace(destination, plain, plain_is_ntt_form);
        }
        template <class C, IfCt<C> = 0>
        void exponentiate(const C &encrypted, std::uint64_t exponent, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            destination = encrypted; // :719-726
            exponentiate_inplace(destination, exponent, relin_keys);
        }

        // Ciphertext inner product (sealhip_evaluator_dot_product): destination = sum_i
        // encrypteds1[i] * encrypteds2[i] over size-2 ciphertexts, the tensor products summed in NTT form, ONE floor (BFV,
        // STRICT contexts only) and, in the overload with a relinearization key, ONE relinearization (size 2; size 3
        // without). Every term is checked like multiply's operands and against the first: same level, and for CKKS one
        // scale on each side (the products must be addable); the result has the terms' level and form and, for CKKS, the
        // scale encrypteds1[0].scale() * encrypteds2[0].scale(). An object may appear in several terms and on both sides.
        // The reference has no such method; for BFV the words are those of the ABI entry, not of the composition.
        template <class C, IfCt<C> = 0>
        void dot_product(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, nullptr, destination);
        }
        template <class C, IfCt<C> = 0>
        void dot_product(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, const KSwitchKeys &relin_key,
                         C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, &relin_key, destination);
        }
        // ... followed by rescale_to_next, in one call and with one rounding (sealhip_evaluator_dot_product_rescale, DESIGN.md
        // section 19): CKKS only; dot_product's checks, and "end of modulus switching chain reached" at the last level. The
        // result has size 2, one level down, with the scale encrypteds1[0].scale() * encrypteds2[0].scale() / q_{k-1}. With
        // one term it is multiply + relinearize + rescale_to_next.
        template <class C, IfCt<C> = 0>
        void dot_product_rescale(const std::vector<C> &encrypteds1, const std::vector<C> &encrypteds2, const KSwitchKeys &relin_key,
                                 C &destination)
        {
            dot_product_internal(encrypteds1, encrypteds2, &relin_key, destination, true);
        }
        // Linear combination with scalar weights (sealhip_evaluator_linear_combination): destination =
        // sum_i weights[i] * terms[i], one streaming pass over the terms -- no transforms, no plaintext objects. Every term is
        // checked like add's operands and against the first: same size (>= 2), same level, the scheme's form. An object may
        // appear in several terms. The reference has no such method; the words are those of multiply_plain with a constant
        // plaintext per term and add over the products.
        // BFV: weights are scalars mod t (a weight >= t is refused); the product uses the residue multiply_plain uses for a
        // one-coefficient plaintext, (c - t [c >= (t + 1) / 2]) mod q_r.
        template <class C, IfCt<C> = 0>
        void linear_combination(const std::vector<C> &terms, const std::vector<std::uint64_t> &weights, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_BFV)
                throw std::invalid_argument("integer weights are for BFV; CKKS takes doubles and a scale");
            check_lincomb_terms(terms, weights.size());
            const std::size_t k = terms[0].coeff_modulus_size();
            const std::uint64_t t = ctx_.plain_modulus(), half = (t + 1) >> 1;
            std::vector<std::uint64_t> w(weights.size() * k);
            for (std::size_t i = 0; i < weights.size(); i++)
            {
                if (weights[i] >= t)
                    throw std::invalid_argument("a weight is not below the plain modulus");
                for (std::size_t r = 0; r < k; r++)
                {
                    const std::uint64_t q = ctx_.key_modulus(r);
                    w[i * k + r] = weights[i] >= half ? (weights[i] % q + (q - t % q)) % q : weights[i] % q;
                }
            }
            linear_combination_internal(terms, w, destination, terms[0].scale());
        }
        // CKKS: weights are doubles with ONE scale; the residues are those of encode(double value, scale)'s constant,
        // round(weight * scale) reduced per prime (ckks.h:405-470), |weight * scale| >= 2^62 is refused. Terms are checked for
        // one scale; the result's scale is terms[0].scale() * scale.
        template <class C, IfCt<C> = 0>
        void linear_combination(const std::vector<C> &terms, const std::vector<double> &weights, double scale, C &destination)
        {
            if (ctx_.scheme() != SEALHIP_SCHEME_CKKS)
                throw std::invalid_argument("weights with a scale are for CKKS; BFV takes scalars mod t");
            check_lincomb_terms(terms, weights.size());
            if (!(scale > 0))
                throw std::invalid_argument("scale out of bounds"); // ckks.h:420-424
            const std::size_t k = terms[0].coeff_modulus_size();
            std::vector<std::uint64_t> w(weights.size() * k);
            for (std::size_t i = 0; i < weights.size(); i++)
            {
                const double v = std::round(weights[i] * scale);
                if (!(std::fabs(v) < 4611686018427387904.0)) // 2^62 (also refuses NaN)
                    throw std::invalid_argument("encoded value is too large");
                const std::uint64_t mag = static_cast<std::uint64_t>(std::fabs(v));
                for (std::size_t r = 0; r < k; r++)
                {
                    const std::uint64_t q = ctx_.key_modulus(r), res = mag % q;
                    w[i * k + r] = std::signbit(v) && res ? q - res : res;
                }
            }
            linear_combination_internal(terms, w, destination, terms[0].scale() * scale);
        }

        // Evaluator-style polynomial evaluation (sealhip_evaluator_evaluate_polynomial): destination =
        // sum_e coeffs[e] * encrypted^e by Paterson-Stockmeyer, BFV on STRICT contexts, a size-2 operand in coefficient form,
        // coefficients below t (lowest degree first), relin_keys as relinearize_inplace takes them (index 0 is read; none is
        // needed for degree one). The reference has no such method; the words are those of tests/poly_eval_ref.py.
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial(const C &encrypted, const std::vector<std::uint64_t> &coeffs,
                                 const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            require_scheme(SEALHIP_SCHEME_BFV);
            check_galois_operand(encrypted);
            if (coeffs.empty())
                throw std::invalid_argument("coeffs must not be empty");
            const std::size_t k = encrypted.coeff_modulus_size();
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_evaluate_polynomial(ctx_.get(), std::uint32_t(k), c, 1, coeffs.data(),
                                                             std::uint32_t(coeffs.size() - 1), 0, raw ? &raw : nullptr, raw ? 1u : 0u, o);
            });
        }
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial_inplace(C &encrypted, const std::vector<std::uint64_t> &coeffs,
                                         const std::vector<const KSwitchKeys *> &relin_keys)
        {
            evaluate_polynomial(encrypted, coeffs, relin_keys, encrypted);
        }

        // CKKS: destination = p(encrypted) with planned levels and scales (sealhip_evaluator_evaluate_polynomial_ckks, DESIGN.md
        // section 21). coeffs are doubles, lowest degree first, in the monomial basis (basis 0) or the Chebyshev basis of
        // the first kind (basis 1, for messages in [-1, 1]); a size-2 operand in NTT form; relin_keys as above. The
        // destination gets the plan's level (sealhip_evaluator_polynomial_plan_ckks: "end of modulus switching chain
        // reached" when the operand's level is too low for the degree) and the scale scale_out, or the operand's scale when
        // scale_out is 0 -- exactly, by construction. The words are those of tests/poly_eval_ckks_ref.py.
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial(const C &encrypted, const std::vector<double> &coeffs,
                                 const std::vector<const KSwitchKeys *> &relin_keys, C &destination, std::uint32_t basis = 0,
                                 double scale_out = 0.0)
        {
            check_ckks_operand(encrypted);
            if (coeffs.empty())
                throw std::invalid_argument("coeffs must not be empty");
            const std::size_t k = encrypted.coeff_modulus_size();
            sealhip_poly_plan plan{};
            throw_on(sealhip_evaluator_polynomial_plan_ckks(ctx_.get(), std::uint32_t(k), encrypted.scale(), coeffs.data(),
                                                            std::uint32_t(coeffs.size() - 1), basis, 0, scale_out, &plan, nullptr,
                                                            nullptr));
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, plan.out_level, destination, &plan.out_scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_evaluate_polynomial_ckks(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), coeffs.data(),
                                                                  std::uint32_t(coeffs.size() - 1), basis, 0, scale_out,
                                                                  raw ? &raw : nullptr, raw ? 1u : 0u, o, nullptr, nullptr);
            });
        }
        template <class C, IfCt<C> = 0>
        void evaluate_polynomial_inplace(C &encrypted, const std::vector<double> &coeffs,
                                         const std::vector<const KSwitchKeys *> &relin_keys, std::uint32_t basis = 0,
                                         double scale_out = 0.0)
        {
            evaluate_polynomial(encrypted, coeffs, relin_keys, encrypted, basis, scale_out);
        }

        // relinearize + rescale_to_next in one call and with one rounding (sealhip_evaluator_relinearize_rescale, DESIGN.md
        // section 19): CKKS only, a size-3 operand in NTT form, relin_keys as relinearize_inplace takes them (index 0 is
        // read); "end of modulus switching chain reached" at the last level. The result has size 2, one level down, with
        // the scale encrypted.scale() / q_{k-1}.
        template <class C, IfCt<C> = 0>
        void relinearize_rescale(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            if (encrypted.size() != 3)
                throw std::invalid_argument("encrypted size must be 3");
            check_rescale_operand(encrypted);
            const sealhip_kswitch_key *raw = first_relin_key(relin_keys);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n();
            const double scale = encrypted.scale() / double(ctx_.key_modulus(k - 1));
            to_size2(encrypted, 3, k - 1, destination, &scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_relinearize_rescale(ctx_.get(), std::uint32_t(k), c, 3, 3 * k * n, 1, &raw, 1, o);
            });
        }

        // ---- CKKS bootstrapping and its parts; size-2 operands in NTT form
        // ModRaise (sealhip_evaluator_mod_raise): the centred coefficients of the operand modulo q_0 re-read modulo the
        // first k_out primes. Only the operand's q_0 rows are read; the destination decrypts to m + q_0 I and keeps the
        // operand's scale (the caller re-declares it, e.g. as q_0 K ahead of coeffs_to_slots).
        template <class C, IfCt<C> = 0>
        void mod_raise(const C &encrypted, std::size_t k_out, C &destination)
        {
            check_ckks_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            if (k_out < 2)
                throw std::invalid_argument("k_out must be at least 2");
            to_size2(encrypted, 2, k_out, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_mod_raise(ctx_.get(), std::uint32_t(k), c, 1, std::uint32_t(k_out), o);
            });
        }
        // destination = 2 encrypted^2 - 1, one level down, at the scale scale^2 / q_(k-1) (sealhip_evaluator_double_angle)
        template <class C, IfCt<C> = 0>
        void double_angle(const C &encrypted, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            check_ckks_operand(encrypted);
            const sealhip_kswitch_key *raw = first_relin_key(relin_keys);
            const std::size_t k = encrypted.coeff_modulus_size();
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached");
            double scale = 0.0; // (the entry reports it)
            to_size2(encrypted, 2, k - 1, destination, &scale, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_double_angle(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), &raw, 1, o, &scale);
            });
        }
        // EvalMod (sealhip_evaluator_eval_mod): slots x = c / (q_0 K) in [-1, 1] become sin(2 pi K x); the destination gets
        // the plan's level and scale (sealhip_evaluator_evalmod_plan), scale_out or the operand's scale up to rounding
        template <class C, IfCt<C> = 0>
        void eval_mod(const C &encrypted, std::uint32_t K, std::uint32_t r, std::uint32_t degree,
                      const std::vector<const KSwitchKeys *> &relin_keys, C &destination, std::uint32_t n_baby = 0,
                      double scale_out = 0.0)
        {
            check_ckks_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            sealhip_evalmod_plan plan{};
            throw_on(sealhip_evaluator_evalmod_plan(ctx_.get(), std::uint32_t(k), encrypted.scale(), K, r, degree, n_baby, scale_out,
                                                    &plan));
            const sealhip_kswitch_key *raw = first_relin_key_or_null(relin_keys);
            to_size2(encrypted, 2, plan.out_level, destination, &plan.scales[plan.r], [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_eval_mod(ctx_.get(), std::uint32_t(k), c, 1, encrypted.scale(), K, r, degree, n_baby,
                                                  scale_out, raw ? &raw : nullptr, raw ? 1u : 0u, o, nullptr, nullptr);
            });
        }
        // The bootstrap in one call (sealhip_evaluator_bootstrap): the destination is at boot.out_level() with the operand's
        // scale. galois_keys: element -> key, with the keys of boot.key_steps() and of element 2N - 1.
        template <class C, IfCt<C> = 0>
        void bootstrap(const C &encrypted, const Bootstrapper &boot, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            bootstrap_internal(encrypted, boot, galois_keys, relin_keys, nullptr, nullptr, destination);
        }
        // The same with ModRaise alone under a sparse secret (sealhip_evaluator_bootstrap_encapsulated):
        // to_sparse = KeyGenerator(sparse secret).switching_keys(dense secret, 1, 1)[0], to_dense =
        // KeyGenerator(dense secret).switching_keys(sparse secret, 1)[0]; the operand, the destination and every other key
        // are under the dense secret
        template <class C, IfCt<C> = 0>
        void bootstrap(const C &encrypted, const Bootstrapper &boot, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                       const std::vector<const KSwitchKeys *> &relin_keys, const KSwitchKeys &to_sparse, const KSwitchKeys &to_dense,
                       C &destination)
        {
            bootstrap_internal(encrypted, boot, galois_keys, relin_keys, to_sparse.get(), to_dense.get(), destination);
        }
        // Re-encryption under another secret (sealhip_evaluator_switch_secret): destination = (c_0, 0) + switch_key(c_1), the
        // operand under the key's source secret, the destination under its target secret (KeyGenerator::switching_keys)
        template <class C, IfCt<C> = 0>
        void switch_secret(const C &encrypted, const KSwitchKeys &key, C &destination)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_switch_secret(ctx_.get(), std::uint32_t(k), c, 1, key.get(), o);
            });
        }

        // The external product (sealhip_evaluator_external_product): destination = base + encrypted (x)
        // rgsw, the phase of `encrypted` times the small polynomial the RGSW encrypts, with additive noise; base (optional)
        // has the operand's size, level and form. The destination (which may be an operand) takes the metadata of
        // `encrypted`. The reference has no such method. CKKS in NTT form; BFV in coefficient form on a STRICT context.
        template <class C, IfCt<C> = 0>
        void external_product(const C &encrypted, const RgswCiphertext &rgsw, C &destination, const C *base = nullptr)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev b;
            if (base)
            {
                check_rgsw_pair(encrypted, *base);
                b = dev_in(*base, words);
            }
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_external_product(ctx_.get(), std::uint32_t(k), c, 1, rgsw.get(), b.ptr(), o);
            });
        }
        // CMux (sealhip_evaluator_cmux): destination = encrypted0 + (encrypted1 - encrypted0) (x) rgsw, i.e. encrypted1 where
        // the RGSW encrypts 1 and encrypted0 where it encrypts 0; the metadata is encrypted0's
        template <class C, IfCt<C> = 0>
        void cmux(const C &encrypted0, const C &encrypted1, const RgswCiphertext &rgsw, C &destination)
        {
            check_galois_operand(encrypted0);
            check_rgsw_pair(encrypted0, encrypted1);
            const std::size_t k = encrypted0.coeff_modulus_size(), words = 2 * k * ctx_.n();
            Dev c1 = dev_in(encrypted1, words);
            to_size2(encrypted0, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_cmux(ctx_.get(), std::uint32_t(k), c, c1.ptr(), 1, rgsw.get(), o);
            });
        }
        // Selection (sealhip_evaluator_select): destination = encrypteds[index] for the index whose bit t (least significant
        // first) rgsw_bits[t] encrypts: a CMux tree over 2^l ciphertexts of one size, level and form, l = rgsw_bits.size()
        // (another count -> std::invalid_argument). The metadata is encrypteds[0]'s. The operands are gathered into one
        // block for the call.
        template <class C, IfCt<C> = 0>
        void select(const std::vector<C> &encrypteds, const std::vector<const RgswCiphertext *> &rgsw_bits, C &destination)
        {
            if (rgsw_bits.size() > 16 || encrypteds.size() != (std::size_t(1) << rgsw_bits.size()))
                throw std::invalid_argument("select needs 2^l ciphertexts for l RGSW bits");
            check_galois_operand(encrypteds[0]);
            const std::size_t k = encrypteds[0].coeff_modulus_size(), words = 2 * k * ctx_.n();
            std::vector<const sealhip_rgsw *> raw;
            for (const RgswCiphertext *g : rgsw_bits)
            {
                if (!g)
                    throw std::invalid_argument("rgsw_bits holds a null entry");
                raw.push_back(g->get());
            }
            Dev all = dev_out(encrypteds.size() * words), o = dev_out(words);
            for (std::size_t i = 0; i < encrypteds.size(); i++)
            {
                check_rgsw_pair(encrypteds[0], encrypteds[i]);
                gather_words(encrypteds[i], all.ptr() + i * words, words);
            }
            Check chk = checked(encrypteds[0]);
            throw_on(sealhip_evaluator_select(ctx_.get(), std::uint32_t(k), all.ptr(), 1, std::uint32_t(raw.size()),
                                              raw.empty() ? nullptr : raw.data(), o.ptr()));
            chk.done();
            const C first = meta_of(encrypteds[0]); // (the destination may be one of the operands)
            take_meta(destination, first);
            commit(destination, o, 2, k);
        }

        // The monomial product (sealhip_evaluator_multiply_monomial): destination = X^exponent encrypted,
        // or (X^exponent - 1) encrypted with minus_one; the exponent is taken modulo 2N with X^N = -1. The destination (which
        // may be the operand) takes the operand's metadata. CKKS in NTT form; BFV in coefficient form on a STRICT context.
        template <class C, IfCt<C> = 0>
        void multiply_monomial(const C &encrypted, std::uint32_t exponent, C &destination, bool minus_one = false)
        {
            check_galois_operand(encrypted);
            const std::size_t k = encrypted.coeff_modulus_size();
            Staged e(ctx_, 1);
            const std::uint64_t word = exponent;
            e.up(&word, 1);
            to_size2(encrypted, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_multiply_monomial(ctx_.get(), std::uint32_t(k), c, 1, 1,
                                                           reinterpret_cast<const std::uint32_t *>(e.ptr()), 1, minus_one ? 1 : 0, o);
            });
        }
        // Blind rotation (sealhip_evaluator_blind_rotate): destination = X^(exponents[0]) test_vector, then for every step t
        // the accumulator plus ((X^(exponents[t]) - 1) accumulator) (x) keys[t - 1]. exponents holds 1 + keys.n_steps() words,
        // one row of what sealhip_lwe_mod_switch writes (another count -> std::invalid_argument). The metadata is the test
        // vector's.
        template <class C, IfCt<C> = 0>
        void blind_rotate(const C &test_vector, const std::vector<std::uint32_t> &exponents, const BlindRotationKeys &keys,
                          C &destination)
        {
            if (exponents.size() != 1 + keys.n_steps())
                throw std::invalid_argument("blind_rotate needs one exponent and one more per key");
            check_galois_operand(test_vector);
            const std::size_t k = test_vector.coeff_modulus_size();
            std::vector<std::uint64_t> packed((exponents.size() + 1) / 2, 0);
            std::memcpy(packed.data(), exponents.data(), exponents.size() * sizeof(std::uint32_t));
            Staged e(ctx_, packed.size());
            e.up(packed.data(), packed.size());
            to_size2(test_vector, 2, k, destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                return sealhip_evaluator_blind_rotate(ctx_.get(), std::uint32_t(k), c, 1, 1,
                                                      reinterpret_cast<const std::uint32_t *>(e.ptr()),
                                                      std::uint32_t(keys.n_steps()), keys.get(), o);
            });
        }

        // Evaluator::multiply_many (evaluator.cpp:1180-1255): destination = product of all, relinearized after every step
        template <class C, IfCt<C> = 0>
        void multiply_many(const std::vector<C> &encrypteds, const std::vector<const KSwitchKeys *> &relin_keys, C &destination)
        {
            if (encrypteds.empty())
                throw std::invalid_argument("encrypteds vector must not be empty"); // :1185-1188
            for (const C &c : encrypteds)
                if (&c == &destination)
                    throw std::invalid_argument("encrypteds must be different from destination"); // :1193-1199
            const std::size_t k = encrypteds[0].coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n;
            std::vector<Dev> dev;
            std::vector<const std::uint64_t *> ptrs;
            for (const C &c : encrypteds)
            {
                if (c.size() != 2 || c.coeff_modulus_size() != k || c.poly_modulus_degree() != n)
                    throw std::invalid_argument("encrypteds is not valid for encryption parameters");
                dev.push_back(dev_in(c, words));
                ptrs.push_back(dev.back().ptr());
            }
            const std::vector<const sealhip_kswitch_key *> raw = raw_relin_keys(relin_keys);
            Dev o = dev_out(words);
            Check chk = checked(destination); // the composite entry leaves the sink alone: the read pass notes the product
            throw_on(sealhip_evaluator_multiply_many(ctx_.get(), std::uint32_t(k), ptrs.data(), std::uint32_t(ptrs.size()), 1,
                                                     raw.data(), std::uint32_t(raw.size()), o.ptr()));
            chk.note(k, o.ptr(), 2);
            chk.done();
            take_meta(destination, encrypteds[0]);
            commit(destination, o, 2, k);
        }
        // Evaluator::exponentiate_inplace (evaluator.cpp:1257-1288)
        template <class C, IfCt<C> = 0>
        void exponentiate_inplace(C &encrypted, std::uint64_t exponent, const std::vector<const KSwitchKeys *> &relin_keys)
        {
            if (exponent == 0)
                throw std::invalid_argument("exponent cannot be 0"); // :1275-1278
            if (exponent == 1)
                return; // :1281-1284
            const std::vector<C> copies(static_cast<std::size_t>(exponent), encrypted);
            multiply_many(copies, relin_keys, encrypted);
        }

        // ---- batches: what `for (auto &ct : cts) evaluator.multiply_inplace(ct, other)` does in the reference, as one call
        // that pipelines the separately allocated ciphertexts through the device (sealhip_evaluator_multiply_host).
        // encrypted1[i] *= encrypted2[i]; with relin_keys the products come back relinearized (size 2).
        void multiply_inplace(std::vector<CT *> &encrypted1, const std::vector<const CT *> &encrypted2,
                              const std::vector<const KSwitchKeys *> *relin_keys = nullptr)
        {
            const std::size_t count = encrypted1.size();
            if (count != encrypted2.size())
                throw std::invalid_argument("encrypted1 and encrypted2 batch size mismatch");
            if (!count)
                return;
            const std::size_t k = encrypted1[0]->coeff_modulus_size(), s1 = encrypted1[0]->size(), s2 = encrypted2[0]->size();
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            for (std::size_t i = 0; i < count; i++)
            {
                check_pair(*encrypted1[i], *encrypted2[i]);
                if (encrypted1[i]->coeff_modulus_size() != k || encrypted1[i]->size() != s1 || encrypted2[i]->size() != s2)
                    throw std::invalid_argument("a batch must be uniform in level and size");
                if (bfv && (encrypted1[i]->is_ntt_form() || encrypted2[i]->is_ntt_form()))
                    throw std::invalid_argument("encrypted1 or encrypted2 cannot be in NTT form");
                if (!bfv && !(encrypted1[i]->is_ntt_form() && encrypted2[i]->is_ntt_form()))
                    throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form");
            }
            const std::size_t dest = s1 + s2 - 1, out_size = relin_keys && dest > 2 ? 2 : dest;
            std::vector<const sealhip_kswitch_key *> raw;
            if (relin_keys)
                raw = raw_relin_keys(*relin_keys);
            // the results land in fresh buffers of the final size, then replace the operands' storage
            std::vector<std::vector<std::uint64_t>> res(count, std::vector<std::uint64_t>(out_size * k * ctx_.n()));
            std::vector<const std::uint64_t *> pa(count), pb(count);
            std::vector<std::uint64_t *> po(count);
            for (std::size_t i = 0; i < count; i++)
            {
                pa[i] = encrypted1[i]->data();
                pb[i] = encrypted2[i]->data();
                po[i] = res[i].data();
            }
            throw_on(sealhip_evaluator_multiply_host(ctx_.get(), std::uint32_t(k), pa.data(), std::uint32_t(s1), pb.data(),
                                                     std::uint32_t(s2), count, po.data(), relin_keys ? raw.data() : nullptr,
                                                     std::uint32_t(raw.size())));
            for (std::size_t i = 0; i < count; i++)
            {
                encrypted1[i]->resize_raw(out_size, k);
                std::copy(res[i].begin(), res[i].end(), encrypted1[i]->data());
            }
        }
        void rotate_vector_inplace(std::vector<CT *> &encrypted, int steps, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            if (encrypted.empty() || steps == 0)
                return;
            const std::size_t k = encrypted[0]->coeff_modulus_size();
            std::vector<std::uint64_t *> p;
            for (CT *ct : encrypted)
            {
                if (ct->size() != 2 || ct->coeff_modulus_size() != k)
                    throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
                p.push_back(ct->data());
            }
            // (an entry without a key stays on the lists: the ABI refuses its element, it does not fall back on the
            // non-adjacent form)
            const KeyLists keys = key_lists(galois_keys, true);
            throw_on(sealhip_evaluator_rotate_vector_host(ctx_.get(), std::uint32_t(k), p.data(), p.size(), steps, keys.elts.data(),
                                                          keys.raw.data(), std::uint32_t(keys.elts.size())));
        }

        // The vector entries above read / write the ciphertexts' own buffers; a pool block (mempool.cpp:45,145) pinned here
        // once lets the DMA engine do that in place (sealhip_host_register). Unregister before freeing.
        void register_pool_block(void *ptr, std::size_t bytes)
        {
            throw_on(sealhip_host_register(ctx_.get(), ptr, bytes));
        }
        void unregister_pool_block(void *ptr)
        {
            throw_on(sealhip_host_unregister(ctx_.get(), ptr));
        }

        // ---- the rest of the Evaluator surface
        // Evaluator::negate_inplace (evaluator.cpp:65-88)
        template <class C, IfCt<C> = 0>
        void negate_inplace(C &encrypted)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            Dev c = dev_in(encrypted, size * k * n);
            Check chk = checked(encrypted);
            throw_on(sealhip_evaluator_negate(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, c.ptr()));
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        // Evaluator::add_inplace (evaluator.cpp:90-151) / sub_inplace (:174-233)
        template <class C, IfCt<C> = 0>
        void add_inplace(C &encrypted1, const C &encrypted2) { add_sub(encrypted1, encrypted2, false); }
        template <class C, IfCt<C> = 0>
        void sub_inplace(C &encrypted1, const C &encrypted2) { add_sub(encrypted1, encrypted2, true); }
        // Evaluator::multiply_plain_inplace (evaluator.cpp:1438-1473). plain: NTT form -> k*N words (multiply_plain_ntt,
        // :1605-1646), coefficient form -> N coefficients below t (multiply_plain_normal, :1475-1603). Host words; the
        // resident overloads stage them through a pool block too.
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void multiply_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            if (encrypted.is_ntt_form() != plain_is_ntt_form)
                throw std::invalid_argument("NTT form mismatch"); // :1449-1452
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            const std::size_t pw = plain_is_ntt_form ? k * n : n;
            Dev c = dev_in(encrypted, size * k * n), p = dev_plain(plain, pw, plain_is_ntt_form);
            Check chk = checked(encrypted);
            throw_on((plain_is_ntt_form ? sealhip_evaluator_multiply_plain_ntt : sealhip_evaluator_multiply_plain)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, p.ptr(), 0));
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        // Evaluator::add_plain_inplace (evaluator.cpp:1290-1362) / sub_plain_inplace (:1364-1435). BFV: plain = N
        // coefficients below t, ciphertext in coefficient form; CKKS: plain = k*N words in NTT form, same level.
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void add_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            plain_linear(encrypted, plain, plain_is_ntt_form, false);
        }
        template <class C, class P, IfCt<C> = 0, IfPlain<P> = 0>
        void sub_plain_inplace(C &encrypted, const P &plain, bool plain_is_ntt_form)
        {
            plain_linear(encrypted, plain, plain_is_ntt_form, true);
        }
        // the resident plaintext names its own form
        void multiply_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            multiply_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        void add_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            add_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        void sub_plain_inplace(DeviceCiphertext &encrypted, const DevicePlaintext &plain)
        {
            sub_plain_inplace(encrypted, plain, plain.is_ntt_form());
        }
        // transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744) on a resident coefficient-form plaintext
        void transform_to_ntt(const DevicePlaintext &plain, std::size_t k, DevicePlaintext &destination_ntt)
        {
            if (plain.is_ntt_form())
                throw std::invalid_argument("plain is already in NTT form"); // :1662-1665
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context"); // :1657-1661
            const std::size_t n = ctx_.n();
            Staged o(ctx_, k * n);
            throw_on(sealhip_evaluator_transform_plain_to_ntt(ctx_.get(), std::uint32_t(k), plain.data(), plain.words(), 0, 1,
                                                              o.ptr()));
            destination_ntt.adopt(o.release(), k * n, k * n, k, true);
        }
        void transform_to_ntt_inplace(DevicePlaintext &plain, std::size_t k) { transform_to_ntt(plain, k, plain); }
        // mod_switch_to(Plaintext &, parms_id) (evaluator.cpp:1062-1088) / mod_switch_to_next (:959-994), resident
        void mod_switch_to_inplace(DevicePlaintext &plain, std::size_t target_coeff_modulus_size)
        {
            const std::size_t k = plain.coeff_modulus_size();
            if (target_coeff_modulus_size < 1 || target_coeff_modulus_size > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1071-1074
            if (!plain.is_ntt_form())
                throw std::invalid_argument("plain is not in NTT form"); // :1075-1078
            if (k < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1079-1082
            if (k == target_coeff_modulus_size)
                return;
            const std::size_t n = ctx_.n(), words = target_coeff_modulus_size * n;
            Staged o(ctx_, words);
            throw_on(sealhip_evaluator_mod_switch_plain_to(ctx_.get(), std::uint32_t(k), plain.data(), 1,
                                                           std::uint32_t(target_coeff_modulus_size), o.ptr()));
            plain.adopt(o.release(), words, words, target_coeff_modulus_size, true);
        }
        void mod_switch_to(const DevicePlaintext &plain, std::size_t target_coeff_modulus_size, DevicePlaintext &destination)
        {
            destination = plain;
            mod_switch_to_inplace(destination, target_coeff_modulus_size);
        }
        void mod_switch_to_next_inplace(DevicePlaintext &plain)
        {
            if (!plain.is_ntt_form())
                throw std::invalid_argument("plain is not in NTT form"); // :963-966
            if (plain.coeff_modulus_size() < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :967-970
            mod_switch_to_inplace(plain, plain.coeff_modulus_size() - 1);
        }
        // Evaluator::transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744), BFV, with or without fast plain lift.
        // plain: coeff_count coefficients in coefficient form (Plaintext::coeff_count()); destination_ntt: k*N words, the
        // plaintext at level k (k primes) in NTT form, ready for multiply_plain on an NTT-form ciphertext of that level.
        void transform_to_ntt(const std::uint64_t *plain, std::size_t coeff_count, std::size_t k, std::uint64_t *destination_ntt)
        {
            check_plain(plain, coeff_count);
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context"); // :1657-1661
            const std::size_t n = ctx_.n();
            Staged p(ctx_, coeff_count ? coeff_count : 1), o(ctx_, k * n);
            if (coeff_count)
                p.up(plain, coeff_count);
            throw_on(sealhip_evaluator_transform_plain_to_ntt(ctx_.get(), std::uint32_t(k), p.ptr(), coeff_count, 0, 1, o.ptr()));
            o.down(destination_ntt, k * n);
        }
        // transform_to_ntt_inplace(Plaintext &, parms_id): plain holds plain.size() coefficients and is resized to k*N words
        // like Plaintext::resize (:1682-1683); is_ntt_form plays Plaintext::is_ntt_form() and is set on success.
        void transform_to_ntt_inplace(std::vector<std::uint64_t> &plain, std::size_t k, bool &is_ntt_form)
        {
            check_plain(plain.data(), plain.size());
            if (k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for the current context");
            if (is_ntt_form)
                throw std::invalid_argument("plain is already in NTT form"); // :1662-1665
            std::vector<std::uint64_t> out(k * ctx_.n());
            transform_to_ntt(plain.data(), plain.size(), k, out.data());
            plain.swap(out);
            is_ntt_form = true;
        }
        // Evaluator::mod_switch_to_inplace(Plaintext &, parms_id) (evaluator.cpp:1062-1088) on an NTT-form plaintext of
        // plain.size() / N primes: the leading target_coeff_modulus_size rows stay (mod_switch_drop_to_next, :959-994).
        void mod_switch_to_inplace(std::vector<std::uint64_t> &plain, bool is_ntt_form, std::size_t target_coeff_modulus_size)
        {
            const std::size_t k = plain_level(plain);
            if (target_coeff_modulus_size < 1 || target_coeff_modulus_size > ctx_.n_key())
                throw std::invalid_argument("parms_id is not valid for encryption parameters"); // :1071-1074
            if (!is_ntt_form)
                throw std::invalid_argument("plain is not in NTT form"); // :1075-1078
            if (k < target_coeff_modulus_size)
                throw std::invalid_argument("cannot switch to higher level modulus"); // :1079-1082
            if (k == target_coeff_modulus_size)
                return;
            const std::size_t n = ctx_.n();
            Staged in(ctx_, k * n), out(ctx_, target_coeff_modulus_size * n);
            in.up(plain.data(), k * n);
            throw_on(sealhip_evaluator_mod_switch_plain_to(ctx_.get(), std::uint32_t(k), in.ptr(), 1,
                                                           std::uint32_t(target_coeff_modulus_size), out.ptr()));
            plain.resize(target_coeff_modulus_size * n);
            out.down(plain.data(), target_coeff_modulus_size * n);
        }
        void mod_switch_to(const std::vector<std::uint64_t> &plain, bool is_ntt_form, std::size_t target_coeff_modulus_size,
                           std::vector<std::uint64_t> &destination)
        {
            destination = plain;
            mod_switch_to_inplace(destination, is_ntt_form, target_coeff_modulus_size);
        }
        // Evaluator::mod_switch_to_next_inplace(Plaintext &) (evaluator.h:430-438, evaluator.cpp:959-994)
        void mod_switch_to_next_inplace(std::vector<std::uint64_t> &plain, bool is_ntt_form)
        {
            const std::size_t k = plain_level(plain);
            if (!is_ntt_form)
                throw std::invalid_argument("plain is not in NTT form"); // :963-966
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :967-970
            mod_switch_to_inplace(plain, true, k - 1);
        }
        void mod_switch_to_next(const std::vector<std::uint64_t> &plain, bool is_ntt_form, std::vector<std::uint64_t> &destination)
        {
            destination = plain;
            mod_switch_to_next_inplace(destination, is_ntt_form);
        }
        // Ciphertext::is_transparent (ciphertext.h:471-476) evaluated on the device copy
        template <class C, IfCt<C> = 0>
        bool is_transparent(const C &encrypted)
        {
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            Dev c = dev_in(encrypted, size * k * n);
            std::uint8_t flag = 0;
            throw_on(sealhip_is_transparent(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, &flag));
            return flag != 0;
        }

    private:
        // A method is: the checks of this section, in the reference's order; the key lists; the operands as Dev; a Check around
        // the ABI entry; and the result delivered by commit / to_size2 / scatter. A new method calls these helpers; it does
        // not restate them.

        // ---- checks
        void require_scheme(std::uint32_t scheme) const
        {
            if (ctx_.scheme() != scheme)
                throw std::logic_error("unsupported scheme");
        }
        // the scheme's form of a ciphertext operand (evaluator.cpp:1304-1311)
        template <class C>
        void check_form(const C &encrypted) const
        {
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            if (bfv && encrypted.is_ntt_form())
                throw std::invalid_argument("BFV encrypted cannot be in NTT form");
            if (!bfv && !encrypted.is_ntt_form())
                throw std::invalid_argument("CKKS encrypted must be in NTT form");
        }
        // apply_galois_inplace's checks on the operand (evaluator.cpp:1848-1887)
        template <class C>
        void check_galois_operand(const C &encrypted) const
        {
            check_form(encrypted);
            if (encrypted.size() != 2)
                throw std::invalid_argument("encrypted size must be 2"); // :1884-1887
        }
        // what every *_rescale method adds to the unmerged method's checks
        template <class C>
        void check_rescale_operand(const C &encrypted) const
        {
            require_scheme(SEALHIP_SCHEME_CKKS); // (rescale_to_next: evaluator.cpp:1098-1101)
            check_form(encrypted);
            if (encrypted.coeff_modulus_size() < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :1005-1008
        }
        // a size-2 operand of a CKKS-only method
        template <class C>
        void check_ckks_operand(const C &encrypted) const
        {
            require_scheme(SEALHIP_SCHEME_CKKS);
            check_galois_operand(encrypted);
        }
        template <class C>
        void check_dft_operand(const C &encrypted, const HomomorphicDFT &dft, std::uint32_t direction) const
        {
            check_ckks_operand(encrypted);
            if (dft.direction() != direction)
                throw std::invalid_argument("the DFT tables were made for the other direction");
            if (encrypted.coeff_modulus_size() != dft.in_level())
                throw std::invalid_argument("encrypted is not at the level of the DFT tables");
        }

        // ---- key lists, as the ABI takes them
        using GaloisKeyMap = std::map<std::uint32_t, const KSwitchKeys *>;
        struct KeyLists
        {
            std::vector<std::uint32_t> elts;
            std::vector<const sealhip_kswitch_key *> raw;
        };
        // every key of the map as parallel (element, handle) lists; an entry without a key is left out, or kept with a null
        // handle
        static KeyLists key_lists(const GaloisKeyMap &galois_keys, bool keep_null = false)
        {
            KeyLists keys;
            for (const auto &kv : galois_keys)
                if (kv.second || keep_null)
                {
                    keys.elts.push_back(kv.first);
                    keys.raw.push_back(kv.second ? kv.second->get() : nullptr);
                }
            return keys;
        }
        // the key of each listed element; identity_exempt: element 1 needs no key and gets a null handle
        static std::vector<const sealhip_kswitch_key *> keys_of(const std::vector<std::uint32_t> &galois_elts,
                                                                const GaloisKeyMap &galois_keys, bool identity_exempt)
        {
            std::vector<const sealhip_kswitch_key *> raw;
            for (std::uint32_t elt : galois_elts)
            {
                const bool exempt = identity_exempt && elt == 1;
                auto it = galois_keys.find(elt);
                if (!exempt && (it == galois_keys.end() || !it->second))
                    throw std::invalid_argument("Galois key not present"); // evaluator.cpp:1871-1874
                raw.push_back(exempt ? nullptr : it->second->get());
            }
            return raw;
        }
        // relin_keys[i] = key of get_index(i + 2), or null
        static std::vector<const sealhip_kswitch_key *> raw_relin_keys(const std::vector<const KSwitchKeys *> &relin_keys)
        {
            std::vector<const sealhip_kswitch_key *> raw;
            for (auto *rk : relin_keys)
                raw.push_back(rk ? rk->get() : nullptr);
            return raw;
        }

        // ---- operands and results on the device
        // The words of an operand on the device for one call: a host ciphertext is staged through a pool block (up, and
        // down again for an in-place result), a resident one is its own block.
        struct Dev
        {
            std::unique_ptr<Staged> st;
            std::uint64_t *p = nullptr;
            std::uint64_t *ptr() const { return p; }
        };
        Dev dev_out(std::size_t words) // a fresh pool block
        {
            Dev d;
            d.st.reset(new Staged(ctx_, words));
            d.p = d.st->ptr();
            return d;
        }
        Dev dev_staged(const std::uint64_t *host, std::size_t words) // ... holding the host words
        {
            Dev d = dev_out(words);
            d.st->up(host, words);
            return d;
        }
        static Dev dev_resident(const std::uint64_t *device) { return Dev{ nullptr, const_cast<std::uint64_t *>(device) }; }
        Dev dev_in(const CT &c, std::size_t words) { return dev_staged(c.data(), words); }
        Dev dev_in(const DeviceCiphertext &c, std::size_t) { return dev_resident(c.data()); }
        Dev dev_plain(const std::uint64_t *plain, std::size_t words, bool) { return dev_staged(plain, words); }
        Dev dev_plain(const DevicePlaintext &plain, std::size_t words, bool ntt_form)
        {
            if (plain.is_ntt_form() != ntt_form || plain.words() != words)
                throw std::invalid_argument("plain is not valid for encryption parameters");
            return dev_resident(plain.data());
        }
        void dev_back(CT &c, Dev &d, std::size_t words) { d.st->down(c.data(), words); }
        void dev_back(DeviceCiphertext &, Dev &, std::size_t) {}
        // the result of `size` polynomials at level k in `o` replaces the operand's words
        void commit(CT &c, Dev &o, std::size_t size, std::size_t k)
        {
            c.resize_raw(size, k);
            o.st->down(c.data(), size * k * ctx_.n());
        }
        void commit(DeviceCiphertext &c, Dev &o, std::size_t size, std::size_t k)
        {
            const std::size_t words = o.st->words();
            c.adopt(o.st->release(), words, size, k);
        }
        // the destination takes the metadata of `src` (host: as the whole object, like before)
        void take_meta(CT &dst, const CT &src) { dst = src; }
        void take_meta(DeviceCiphertext &dst, const DeviceCiphertext &src) { dst.copy_meta(src); }
        // fewer polynomials at the same level, the leading words kept (relinearize)
        void shrink(CT &c, std::size_t size) { c.resize_raw(size, c.coeff_modulus_size()); }
        void shrink(DeviceCiphertext &c, std::size_t size) { c.set_size(size); }

        // The deferred transparency check of one resident result (see the class comment): a slot of this Evaluator's ring
        // is the lane's sink while the operation runs; none is left installed afterwards. Inert for host operands.
        class Check
        {
        public:
            Check() = default;
            Check(const Context &c, const void *owner, std::size_t count = 1) : c_(&c), owner_(owner), count_(count)
            {
                std::uint32_t *slot = c.transparency_slot(owner, count);
                const long hr = sealhip_transparency_sink(c.get(), slot, count);
                if (hr != SEALHIP_S_OK)
                {
                    c.transparency_unslot(owner, count);
                    c_ = nullptr;
                    throw_on(hr);
                }
            }
            Check(const Check &) = delete;
            Check &operator=(const Check &) = delete;
            // entries that leave the sink alone: the read pass over their result
            void note(std::size_t k, const std::uint64_t *ct, std::size_t size)
            {
                if (c_)
                    throw_on(sealhip_transparency_note(c_->get(), std::uint32_t(k), ct, std::uint32_t(size), 1));
            }
            void done() { ok_ = true; }
            ~Check()
            {
                if (!c_)
                    return;
                (void)sealhip_transparency_sink(c_->get(), nullptr, 0);
                if (!ok_)
                    c_->transparency_unslot(owner_, count_);
            }

        private:
            const Context *c_ = nullptr;
            const void *owner_ = nullptr;
            std::size_t count_ = 1;
            bool ok_ = false;
        };
        Check checked(const CT &, std::size_t = 1) { return Check(); }
        Check checked(const DeviceCiphertext &, std::size_t count = 1) { return Check(ctx_, this, count); }

        // the second operand of an RGSW operation: the first one's size, level and form
        template <class C>
        void check_rgsw_pair(const C &first, const C &other) const
        {
            if (other.size() != 2 || other.coeff_modulus_size() != first.coeff_modulus_size() ||
                other.is_ntt_form() != first.is_ntt_form())
                throw std::invalid_argument("encrypted operands differ in size, level or form");
        }
        // an operand's words into a block that gathers several
        void gather_words(const CT &c, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_h2d(ctx_.get(), dst, c.data(), words * 8));
        }
        void gather_words(const DeviceCiphertext &c, std::uint64_t *dst, std::size_t words)
        {
            throw_on(sealhip_memcpy_d2d(ctx_.get(), dst, c.data(), words * 8));
        }
        // an operand's metadata, detached from its words (a host ciphertext is its own metadata)
        CT meta_of(const CT &c) { return c; }
        DeviceCiphertext meta_of(const DeviceCiphertext &c)
        {
            DeviceCiphertext m(ctx_);
            m.copy_meta(c);
            return m;
        }

        // One operand of in_size polynomials in, one size-2 result at level k_out out: call(in, out) is the ABI entry over
        // the two device blocks. The destination (which may be the operand) takes the operand's metadata, the result's
        // words and, where `scale` is not null, that scale, read after the call.
        template <class C, class Call>
        void to_size2(const C &encrypted, std::size_t in_size, std::size_t k_out, C &destination, const double *scale, Call call)
        {
            const std::size_t n = ctx_.n();
            Dev c = dev_in(encrypted, in_size * encrypted.coeff_modulus_size() * n), o = dev_out(2 * k_out * n);
            Check chk = checked(encrypted);
            throw_on(call(c.ptr(), o.ptr()));
            chk.done();
            take_meta(destination, encrypted);
            commit(destination, o, 2, k_out);
            if (scale)
                destination.scale() = *scale;
        }

        template <class C>
        void bootstrap_internal(const C &encrypted, const Bootstrapper &boot,
                                const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys,
                                const std::vector<const KSwitchKeys *> &relin_keys, const sealhip_kswitch_key *to_sparse,
                                const sealhip_kswitch_key *to_dense, C &destination)
        {
            check_ckks_operand(encrypted);
            const sealhip_kswitch_key *relin = first_relin_key(relin_keys);
            const KeyLists keys = key_lists(galois_keys);
            const std::uint32_t k = std::uint32_t(encrypted.coeff_modulus_size()), n_keys = std::uint32_t(keys.elts.size());
            to_size2(encrypted, 2, boot.out_level(), destination, nullptr, [&](const std::uint64_t *c, std::uint64_t *o) {
                if (to_sparse)
                    return sealhip_evaluator_bootstrap_encapsulated(ctx_.get(), boot.get(), k, c, 1, keys.elts.data(),
                                                                    keys.raw.data(), n_keys, &relin, 1, to_sparse, to_dense, o);
                return sealhip_evaluator_bootstrap(ctx_.get(), boot.get(), k, c, 1, keys.elts.data(), keys.raw.data(), n_keys,
                                                   &relin, 1, o);
            });
        }

        // relin_keys as relinearize_inplace takes them, of which index 0 is read: required (:793-796), or null without one
        static const sealhip_kswitch_key *first_relin_key(const std::vector<const KSwitchKeys *> &relin_keys)
        {
            if (relin_keys.empty() || !relin_keys[0])
                throw std::invalid_argument("not enough relinearization keys");
            return relin_keys[0]->get();
        }
        static const sealhip_kswitch_key *first_relin_key_or_null(const std::vector<const KSwitchKeys *> &relin_keys)
        {
            return !relin_keys.empty() && relin_keys[0] ? relin_keys[0]->get() : nullptr;
        }

        // the n results of a hoisted rotation, back to back in `o`, become the destinations (metadata of the operand)
        // (k: the level of the results when it is not the operand's -- the *_rescale methods; size: their polynomials)
        void scatter(const CT &src, Dev &o, std::size_t n, std::size_t words, std::vector<CT> &dst, std::size_t k = 0,
                     std::size_t size = 2)
        {
            dst.assign(n, src);
            for (std::size_t i = 0; k && i < n; i++)
                dst[i].resize_raw(size, k);
            for (std::size_t i = 0; i < n; i++)
                throw_on(sealhip_memcpy_d2h(ctx_.get(), dst[i].data(), o.ptr() + i * words, words * 8));
        }
        void scatter(const DeviceCiphertext &src, Dev &o, std::size_t n, std::size_t words, std::vector<DeviceCiphertext> &dst,
                     std::size_t k = 0, std::size_t size = 2)
        {
            k = k ? k : src.coeff_modulus_size();
            std::vector<DeviceCiphertext> next;
            next.reserve(n);
            for (std::size_t i = 0; i < n; i++)
            {
                next.emplace_back(ctx_);
                next[i].adopt_result(*o.st, i, n, words, size, k);
                next[i].copy_meta(src);
            }
            dst.swap(next);
        }

        // ---- plaintext operands
        // A plaintext of apply_galois_dot_plain / dot_plain as the checks and the staging read it: a DevicePlaintext, or a host
        // plaintext of HostPlaintext's shape (words, k, ntt_form, scale)
        struct PlainView
        {
            const std::uint64_t *data;
            std::size_t words, k;
            bool ntt_form;
            double scale;
            bool on_device;
        };
        static PlainView plain_view(const DevicePlaintext &p)
        {
            return { p.data(), p.words(), p.coeff_modulus_size(), p.is_ntt_form(), p.scale(), true };
        }
        template <class P>
        static PlainView plain_view(const P &p)
        {
            return { p.words.data(), p.words.size(), p.k, p.ntt_form, p.scale, false };
        }
        void plain_to(const PlainView &p, std::uint64_t *dst, std::size_t words)
        {
            throw_on((p.on_device ? sealhip_memcpy_d2d : sealhip_memcpy_h2d)(ctx_.get(), dst, p.data, words * 8));
        }
        // every plains[s] has n_elts plaintexts in key-level NTT form; returns their common scale (CKKS; 1.0 if none)
        template <class P>
        double check_dot_plains(const std::vector<std::vector<P>> &plains, std::size_t n_elts) const
        {
            const std::size_t n_key = ctx_.n_key(), n = ctx_.n();
            bool first = true;
            double scale = 1.0;
            for (const auto &row : plains)
            {
                if (row.size() != n_elts)
                    throw std::invalid_argument("plains must hold one plaintext per Galois element in every sum");
                for (const P &plain : row)
                {
                    const PlainView p = plain_view(plain);
                    if (!p.ntt_form || p.k != n_key || p.words != n_key * n)
                        throw std::invalid_argument("plain must be in NTT form at the key level");
                    if (ctx_.scheme() == SEALHIP_SCHEME_CKKS && !first && p.scale != scale)
                        throw std::invalid_argument("scale mismatch");
                    if (first)
                        scale = p.scale;
                    first = false;
                }
            }
            return scale;
        }
        std::vector<std::uint32_t> elts_of_steps(const std::vector<int> &steps) const
        {
            std::vector<std::uint32_t> elts(steps.size(), 1);
            for (std::size_t i = 0; i < steps.size(); i++)
                if (steps[i] != 0)
                    throw_on(sealhip_galois_elt_from_step(ctx_.get(), steps[i], &elts[i]));
            return elts;
        }

        // ---- the methods behind several public names
        template <class C, class P>
        void dot_plain_internal(const C &encrypted, const std::vector<std::uint32_t> &galois_elts, const GaloisKeyMap &galois_keys,
                                const std::vector<std::vector<P>> &plains, std::vector<C> &destinations, bool rescale)
        {
            check_galois_operand(encrypted);
            if (rescale)
                check_rescale_operand(encrypted);
            const std::vector<const sealhip_kswitch_key *> raw = keys_of(galois_elts, galois_keys, true);
            const std::size_t n_elts = galois_elts.size(), n_sums = plains.size();
            const double scale = check_dot_plains(plains, n_elts);
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n, pw = ctx_.n_key() * n;
            const std::size_t k_out = rescale ? k - 1 : k, out_words = 2 * k_out * n;
            Dev c = dev_in(encrypted, words), o = dev_out((n_sums ? n_sums : 1) * out_words);
            Staged w(ctx_, n_sums * n_elts ? n_sums * n_elts * pw : 1);
            for (std::size_t s = 0; s < n_sums; s++)
                for (std::size_t i = 0; i < n_elts; i++)
                    plain_to(plain_view(plains[s][i]), w.ptr() + (s * n_elts + i) * pw, pw);
            Check chk = checked(encrypted, n_sums ? n_sums : 1);
            throw_on((rescale ? sealhip_evaluator_apply_galois_dot_plain_rescale : sealhip_evaluator_apply_galois_dot_plain)(
                ctx_.get(), std::uint32_t(k), c.ptr(), 1, galois_elts.data(), raw.data(), std::uint32_t(n_elts), w.ptr(),
                std::uint32_t(n_sums), o.ptr()));
            chk.done();
            scatter(encrypted, o, n_sums, out_words, destinations, k_out);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                for (C &d : destinations)
                    d.scale() = encrypted.scale() * scale / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
        }
        template <class C, class P>
        void bsgs_plain_internal(const C &encrypted, const std::vector<std::uint32_t> &baby_elts,
                                 const std::vector<std::uint32_t> &giant_elts, const GaloisKeyMap &galois_keys,
                                 const std::vector<std::vector<P>> &plains, C &destination, bool rescale)
        {
            check_galois_operand(encrypted);
            if (rescale)
                check_rescale_operand(encrypted);
            const std::vector<const sealhip_kswitch_key *> bk = keys_of(baby_elts, galois_keys, true),
                                                           gk = keys_of(giant_elts, galois_keys, true);
            const std::size_t n_baby = baby_elts.size(), n_giant = giant_elts.size();
            if (plains.size() != n_giant)
                throw std::invalid_argument("plains must hold one row of plaintexts per giant element");
            const double plain_scale = check_dot_plains(plains, n_baby);
            const std::size_t k = encrypted.coeff_modulus_size(), pw = ctx_.n_key() * ctx_.n();
            Staged w(ctx_, (n_giant && n_baby) ? n_giant * n_baby * pw : 1);
            for (std::size_t j = 0; j < n_giant; j++)
                for (std::size_t i = 0; i < n_baby; i++)
                    plain_to(plain_view(plains[j][i]), w.ptr() + (j * n_baby + i) * pw, pw);
            const bool ckks = ctx_.scheme() == SEALHIP_SCHEME_CKKS;
            const double scale = encrypted.scale() * plain_scale / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
            to_size2(encrypted, 2, rescale ? k - 1 : k, destination, ckks ? &scale : nullptr,
                     [&](const std::uint64_t *c, std::uint64_t *o) {
                         return (rescale ? sealhip_evaluator_apply_galois_bsgs_plain_rescale : sealhip_evaluator_apply_galois_bsgs_plain)(
                             ctx_.get(), std::uint32_t(k), c, 1, baby_elts.data(), bk.data(), std::uint32_t(n_baby),
                             giant_elts.data(), gk.data(), std::uint32_t(n_giant), w.ptr(), o);
                     });
        }

        template <class C>
        void dot_product_internal(const std::vector<C> &a, const std::vector<C> &b, const KSwitchKeys *relin_key, C &destination,
                                  bool rescale = false)
        {
            if (a.empty() || a.size() != b.size())
                throw std::invalid_argument("encrypteds1 and encrypteds2 must hold the same, non-zero number of terms");
            for (std::size_t i = 0; i < a.size(); i++)
            {
                check_multiply(a[i], b[i]);
                if (a[i].size() != 2 || b[i].size() != 2)
                    throw std::invalid_argument("encrypted size must be 2");
                if (a[i].coeff_modulus_size() != a[0].coeff_modulus_size())
                    throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
                if (ctx_.scheme() == SEALHIP_SCHEME_CKKS && (a[i].scale() != a[0].scale() || b[i].scale() != b[0].scale()))
                    throw std::invalid_argument("scale mismatch");
            }
            if (rescale)
                check_rescale_operand(a[0]);
            const std::size_t k = a[0].coeff_modulus_size(), n = ctx_.n(), words = 2 * k * n, size = relin_key ? 2 : 3;
            const std::size_t k_out = rescale ? k - 1 : k;
            const double scale = a[0].scale() * b[0].scale() / (rescale ? double(ctx_.key_modulus(k - 1)) : 1.0);
            std::vector<Dev> staged;
            std::vector<const std::uint64_t *> pa, pb;
            staged.reserve(2 * a.size());
            for (std::size_t i = 0; i < a.size(); i++)
            {
                staged.push_back(dev_in(a[i], words));
                pa.push_back(staged.back().ptr());
                staged.push_back(dev_in(b[i], words));
                pb.push_back(staged.back().ptr());
            }
            Dev o = dev_out(size * k_out * n);
            const sealhip_kswitch_key *raw = relin_key ? relin_key->get() : nullptr;
            Check chk = checked(a[0]);
            throw_on((rescale ? sealhip_evaluator_dot_product_rescale : sealhip_evaluator_dot_product)(
                ctx_.get(), std::uint32_t(k), pa.data(), pb.data(), std::uint32_t(a.size()), 1, relin_key ? &raw : nullptr,
                relin_key ? 1u : 0u, o.ptr()));
            chk.done();
            take_meta(destination, a[0]); // (every term is staged or enqueued by now: the destination may be one of them)
            commit(destination, o, size, k_out);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                destination.scale() = scale;
        }

        // linear_combination's checks on the term list: one size, one level, the scheme's form and, for CKKS, one scale
        template <class C>
        void check_lincomb_terms(const std::vector<C> &terms, std::size_t n_weights) const
        {
            if (terms.empty() || terms.size() != n_weights)
                throw std::invalid_argument("terms and weights must hold the same, non-zero number of entries");
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            for (const C &c : terms)
            {
                check_form(c);
                if (c.size() < 2 || c.size() != terms[0].size())
                    throw std::invalid_argument("terms must have one size of at least 2");
                if (c.coeff_modulus_size() != terms[0].coeff_modulus_size() || c.poly_modulus_degree() != ctx_.n())
                    throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch");
                if (!bfv && c.scale() != terms[0].scale())
                    throw std::invalid_argument("scale mismatch");
            }
        }
        // w: terms.size() x k canonical residues (one sum, no constant)
        template <class C>
        void linear_combination_internal(const std::vector<C> &terms, const std::vector<std::uint64_t> &w, C &destination,
                                         double scale)
        {
            const std::size_t size = terms[0].size(), k = terms[0].coeff_modulus_size(), words = size * k * ctx_.n();
            std::vector<Dev> staged;
            std::vector<const std::uint64_t *> ptrs;
            staged.reserve(terms.size());
            for (const C &c : terms)
            {
                staged.push_back(dev_in(c, words));
                ptrs.push_back(staged.back().ptr());
            }
            Staged dw(ctx_, w.size());
            dw.up(w.data(), w.size());
            Dev o = dev_out(words);
            Check chk = checked(terms[0]);
            throw_on(sealhip_evaluator_linear_combination(ctx_.get(), std::uint32_t(k), ptrs.data(), std::uint32_t(ptrs.size()),
                                                          std::uint32_t(size), 1, dw.ptr(), nullptr, 1, o.ptr()));
            chk.done();
            take_meta(destination, terms[0]); // (every term is staged or enqueued by now: the destination may be one of them)
            commit(destination, o, size, k);
            if (ctx_.scheme() == SEALHIP_SCHEME_CKKS)
                destination.scale() = scale;
        }

        // the host checks of multiply / square (evaluator.cpp:238-249, :276-279, :449-452)
        template <class C>
        void check_multiply(const C &encrypted1, const C &encrypted2) const
        {
            check_pair(encrypted1, encrypted2);
            const bool bfv = ctx_.scheme() == SEALHIP_SCHEME_BFV;
            if (bfv && (encrypted1.is_ntt_form() || encrypted2.is_ntt_form()))
                throw std::invalid_argument("encrypted1 or encrypted2 cannot be in NTT form"); // :276-279
            if (!bfv && !(encrypted1.is_ntt_form() && encrypted2.is_ntt_form()))
                throw std::invalid_argument("encrypted1 or encrypted2 must be in NTT form"); // :449-452
        }

        // conjugate_internal (evaluator.h:1343-1363): the automorphism x -> x^(2N-1), i.e. get_elt_from_step(0)
        template <class C>
        void conjugate_internal(C &encrypted, const std::map<std::uint32_t, const KSwitchKeys *> &galois_keys)
        {
            std::uint32_t elt = 0;
            throw_on(sealhip_galois_elt_from_step(ctx_.get(), 0, &elt));
            keys_of({ elt }, galois_keys, false); // (refuses an absent key: evaluator.cpp:1871-1874)
            apply_galois_inplace(encrypted, elt, *galois_keys.at(elt));
        }
        template <class C, class P>
        void plain_linear(C &encrypted, const P &plain, bool plain_is_ntt_form, bool sub)
        {
            check_form(encrypted); // :1304-1311
            if (encrypted.is_ntt_form() != plain_is_ntt_form)
                throw std::invalid_argument("NTT form mismatch"); // :1312-1315
            const std::size_t k = encrypted.coeff_modulus_size(), n = ctx_.n(), size = encrypted.size();
            const std::size_t pw = plain_is_ntt_form ? k * n : n;
            Dev c = dev_in(encrypted, size * k * n), p = dev_plain(plain, pw, plain_is_ntt_form);
            Check chk = checked(encrypted); // (the entry has no sink: the read pass notes the result)
            throw_on(sealhip_evaluator_add_plain(ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, p.ptr(), pw,
                                                 sub ? 1 : 0));
            chk.note(k, c.ptr(), size);
            chk.done();
            dev_back(encrypted, c, size * k * n);
        }
        template <class C>
        void add_sub(C &a, const C &b, bool sub)
        {
            if (a.poly_modulus_degree() != ctx_.n() || b.poly_modulus_degree() != ctx_.n() || a.size() < 1 || b.size() < 1)
                throw std::invalid_argument("encrypted1 is not valid for encryption parameters"); // :93-100
            if (a.coeff_modulus_size() != b.coeff_modulus_size())
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch"); // :101-104
            if (a.is_ntt_form() != b.is_ntt_form())
                throw std::invalid_argument("NTT form mismatch"); // :105-108
            const std::size_t k = a.coeff_modulus_size(), n = ctx_.n(), sa = a.size(), sb = b.size();
            const std::size_t so = sa > sb ? sa : sb;
            Dev x = dev_in(a, sa * k * n), y = dev_in(b, sb * k * n), o = dev_out(so * k * n);
            Check chk = checked(a);
            throw_on((sub ? sealhip_evaluator_sub : sealhip_evaluator_add)(ctx_.get(), std::uint32_t(k), x.ptr(),
                                                                           std::uint32_t(sa), y.ptr(), std::uint32_t(sb), 1,
                                                                           o.ptr()));
            chk.done();
            commit(a, o, so, k); // :131-132
        }
        // is_valid_for(Plaintext) (valcheck.cpp:236-281) in coefficient form: at most N coefficients, each below t
        // (plain_modulus 0 under CKKS: no non-empty coefficient-form plaintext is valid)
        void check_plain(const std::uint64_t *plain, std::size_t coeff_count) const
        {
            if (coeff_count > ctx_.n())
                throw std::invalid_argument("plain is not valid for encryption parameters");
            for (std::size_t i = 0; i < coeff_count; i++)
                if (plain[i] >= ctx_.plain_modulus())
                    throw std::invalid_argument("plain is not valid for encryption parameters");
        }
        // level (number of primes) of an NTT-form plaintext: k*N words, 1 <= k <= n_key
        std::size_t plain_level(const std::vector<std::uint64_t> &plain) const
        {
            const std::size_t n = ctx_.n(), k = plain.size() / n;
            if (plain.size() % n != 0 || k < 1 || k > ctx_.n_key())
                throw std::invalid_argument("plain is not valid for encryption parameters");
            return k;
        }
        template <class C>
        void check_pair(const C &a, const C &b) const
        {
            if (a.poly_modulus_degree() != ctx_.n() || b.poly_modulus_degree() != ctx_.n() || a.size() < 2 || b.size() < 2)
                throw std::invalid_argument("encrypted1 is not valid for encryption parameters"); // :238-245
            if (a.coeff_modulus_size() != b.coeff_modulus_size())
                throw std::invalid_argument("encrypted1 and encrypted2 parameter mismatch"); // :246-249
        }
        template <class C>
        void switch_level(C &ct, bool rescale)
        {
            const std::size_t k = ct.coeff_modulus_size(), n = ctx_.n(), size = ct.size();
            if (k < 2)
                throw std::invalid_argument("end of modulus switching chain reached"); // :1005-1008
            Dev c = dev_in(ct, size * k * n), o = dev_out(size * (k - 1) * n);
            Check chk = checked(ct);
            throw_on((rescale ? sealhip_evaluator_rescale_to_next : sealhip_evaluator_mod_switch_to_next)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1, o.ptr()));
            chk.done();
            commit(ct, o, size, k - 1); // :879
        }
        template <class C>
        void transform(C &ct, bool to_ntt)
        {
            const std::size_t k = ct.coeff_modulus_size(), n = ctx_.n(), size = ct.size();
            Dev c = dev_in(ct, size * k * n);
            Check chk = checked(ct); // (the transforms have no sink: the read pass notes the result)
            throw_on((to_ntt ? sealhip_evaluator_transform_to_ntt : sealhip_evaluator_transform_from_ntt)(
                ctx_.get(), std::uint32_t(k), c.ptr(), std::uint32_t(size), 1));
            chk.note(k, c.ptr(), size);
            chk.done();
            dev_back(ct, c, size * k * n);
        }
        const Context &ctx_;
    };
} // namespace sealhip_host
