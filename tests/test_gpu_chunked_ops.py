"""The arena-chunked operations that no other test runs over more than one chunk: CKKS rescale_to_next,
divide_and_round_q_last_ntt_inplace, rescale_special_rns_inplace, dot_product_ct_sk (coefficient form, size 3),
invariant_noise_budget, BFV decrypt, encrypt_zero_asymmetric, batch_decode, ckks_encode and ckks_decode. A child process with
the smallest arena the library accepts (SEALHIP_WORKSPACE_MB=64) runs each over a batch that needs a second, ragged chunk
(asserted from the chunk log) and compares the items on both sides of the chunk boundary and at both ends of the batch with
the oracle, word for word; every budget of the noise-budget batch is compared.

Shapes: N = 2^13, 8 ciphertext primes and 1 special prime. An operation's chunk is 64 MiB / (arena bytes per item), so each
batch is just over 64 MiB of temporaries whatever the level; the counts below are one or two items past a whole chunk."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import noise_ref as R
import oracle_lib as O
from support import ARENA_MB, child_main, rows, run_arena_child

pytestmark = pytest.mark.gpu

LOGN, N, T = 13, 1 << 13, 786433


def _item(S, ctx, buf, index, words):
    one = np.empty(words, dtype=np.uint64)
    assert S.lib().sealhip_memcpy_d2h(ctx.handle, one.ctypes.data, buf.ptr + index * words * 8, words * 8) == 0
    return one


def _boundary(ctx, count):
    """the items to compare, from the entry the operation has just appended to the chunk log"""
    log = ctx.chunk_log()
    assert log, "the operation did not walk its batch in chunks"
    logged, chunk = log[-1]
    assert logged == count and chunk < count and count % chunk != 0, log
    return sorted({0, chunk - 1, chunk, count - 1})


def _child():
    import sealhip as S

    assert os.environ.get("SEALHIP_WORKSPACE_MB") == ARENA_MB
    L = O.lib()
    mods = O.coeff_modulus_create(N, [50] * 8 + [60])
    nk, nsp, kf = len(mods), 1, len(mods) - 1
    bfv, ckks = S.Context(S.SCHEME_BFV, LOGN, mods, nsp, T), S.Context(S.SCHEME_CKKS, LOGN, mods, nsp, 0)
    rbfv, rckks = O.RefContext(1, LOGN, mods, nsp=nsp, t=T), O.RefContext(2, LOGN, mods, nsp=nsp)
    rng = np.random.default_rng(64)
    done = []

    # ---- Evaluator::rescale_to_next (CKKS): the log counts polynomials
    k, count = kf, 65
    x = rows(rng, mods[:k], N, (count * 2,)).reshape(count, 2, k, N)
    out = ckks.alloc(count * 2 * (k - 1) * N)
    ckks.chunk_log()
    S.Evaluator(ckks).rescale_to_next(ckks.upload(x), 2, k, count, out)
    for i in sorted({p // 2 for p in _boundary(ckks, count * 2)}):
        exp = np.zeros((2, k - 1, N), dtype=np.uint64)
        assert L.ref_mod_switch_scale_to_next(C.byref(rckks.c), k, O.ptr(x[i]), 2, O.ptr(exp)) == 0
        assert np.array_equal(_item(S, ckks, out, i, exp.size), exp.reshape(-1)), ("rescale_to_next", i)
    out.free()
    done.append("rescale_to_next")

    # ---- divide_and_round_q_last_ntt_inplace
    k, count = kf, 147
    x = rows(rng, mods[:k], N, (count,))
    d = ckks.upload(x)
    ckks.chunk_log()
    ckks.divide_and_round_q_last_ntt_inplace(k, d, count)
    for i in _boundary(ckks, count):
        exp = x[i].copy()
        L.ref_divide_and_round_q_last_ntt_inplace(rckks.rns_tool(k), O.ptr(exp), rckks.c.key_tables, 0)
        got = _item(S, ckks, d, i, k * N).reshape(k, N)
        assert np.array_equal(got[: k - 1], exp[: k - 1]), ("divide_and_round_q_last_ntt_inplace", i)
    d.free()
    done.append("divide_and_round_q_last_ntt_inplace")

    # ---- rescale_special_rns_inplace (BFV: the q rows go back to coefficient form)
    k, count = kf, 129
    x = rows(rng, mods, N, (count,))
    d = bfv.upload(x)
    bfv.chunk_log()
    bfv.rescale_special_rns_inplace(k, d, count)
    for i in _boundary(bfv, count):
        exp = x[i].copy()
        L.ref_rescale_special_rns_inplace(O.ptr(exp), 0, N, k, nsp, rbfv.c.key_mod, nk, rbfv.c.key_tables, 0)
        got = _item(S, bfv, d, i, nk * N).reshape(nk, N)
        assert np.array_equal(got[:k], exp[:k]), ("rescale_special_rns_inplace", i)
    d.free()
    done.append("rescale_special_rns_inplace")

    # ---- Decryptor::dot_product_ct_sk_array, coefficient form, size 3, below the first level
    k, size, count = 5, 3, 103
    pw = R.random_sk_powers(mods, LOGN, size - 1, rng)
    dpw = bfv.upload(pw)
    x = rows(rng, mods[:k], N, (count * size,)).reshape(count, size, k, N)
    out = bfv.alloc(count * k * N)
    d = bfv.upload(x)
    bfv.chunk_log()
    bfv.dot_product_ct_sk(d, size, k, count, dpw, False, out)
    for i in _boundary(bfv, count):
        exp = np.zeros((k, N), dtype=np.uint64)
        L.ref_dot_product_ct_sk(C.byref(rbfv.c), k, O.ptr(x[i]), size, 0, O.ptr(pw), O.ptr(exp))
        assert np.array_equal(_item(S, bfv, out, i, k * N), exp.reshape(-1)), ("dot_product_ct_sk", i)
    d.free()
    out.free()
    done.append("dot_product_ct_sk")

    # ---- Decryptor::invariant_noise_budget and BFV decrypt on one batch: random c_1, c_0 chosen so that t (c_0 + c_1 s) is a
    # small random polynomial plus one coefficient of magnitude 2^(12 + 5 i) at item i's own position -- every item has its
    # own budget, known from the planted norm alone (noise_ref.planted_budget); the boundary items also go through the
    # oracle's dot product and the restatement
    k, size, count = kf, 2, 65
    tables = [O.Tables(LOGN, p) for p in mods[:k]]
    x = np.empty((count, size, k, N), dtype=np.uint64)
    want = []
    for i in range(count):
        small = rng.integers(-1000, 1000, size=N)
        big = {(i * 7919) % N: (-1 if i & 1 else 1) << (12 + 5 * i)}
        x[i] = R.ciphertext_with_dot(R.planted_rows(small, big, mods[:k], T), size, pw, mods, LOGN, rng, tables=tables)
        want.append(R.planted_budget(small, big, mods[:k]))
    assert len(set(want)) == count and min(want) > 0
    d = bfv.upload(x)
    bfv.chunk_log()
    budgets = bfv.invariant_noise_budget(d, size, k, count, dpw)
    items = _boundary(bfv, count)
    assert list(budgets) == want, (list(budgets), want)
    plain = bfv.alloc(count * N)
    bfv.decrypt(d, size, k, count, dpw, False, plain)
    assert _boundary(bfv, count) == items
    for i in items:
        dot = np.zeros((k, N), dtype=np.uint64)
        L.ref_dot_product_ct_sk(C.byref(rbfv.c), k, O.ptr(x[i]), size, 0, O.ptr(pw), O.ptr(dot))
        assert int(budgets[i]) == R.ref_noise_budget(dot, mods[:k], T), ("invariant_noise_budget", i)
        exp = np.zeros(N, dtype=np.uint64)
        assert L.ref_decrypt_scale_and_round(C.byref(rbfv.c), k, O.ptr(dot), O.ptr(exp)) == 0
        assert np.array_equal(_item(S, bfv, plain, i, N), exp), ("decrypt", i)
    d.free()
    plain.free()
    done += ["invariant_noise_budget", "decrypt"]

    # ---- util::encrypt_zero_asymmetric, both forms of the result
    n_rows, count = kf, 129
    pk = rows(rng, mods[:n_rows], N, (2,))
    u = rng.integers(-1, 2, size=(count, N)).astype(np.int32)
    e = rng.integers(-19, 20, size=(count, 2, N)).astype(np.int32)
    dpk, du, de = bfv.upload(pk), bfv.upload_i32(u), bfv.upload_i32(e)
    out = bfv.alloc(count * 2 * n_rows * N)
    for ntt_form in (False, True):
        bfv.chunk_log()
        bfv.encrypt_zero_asymmetric(n_rows, ntt_form, dpk, du, de, count, out)
        for i in _boundary(bfv, count):
            exp = np.zeros((2, n_rows, N), dtype=np.uint64)
            L.ref_encrypt_zero_asymmetric_given(C.byref(rbfv.c), n_rows, O.ptr(pk), 1 if ntt_form else 0, O.ptr(u[i]),
                                                O.ptr(e[i]), O.ptr(exp))
            assert np.array_equal(_item(S, bfv, out, i, exp.size), exp.reshape(-1)), ("encrypt_zero_asymmetric", ntt_form, i)
    out.free()
    done.append("encrypt_zero_asymmetric")

    # ---- BatchEncoder::decode
    count = 1025
    tb = O.Tables(LOGN, T)
    x = rng.integers(0, T, size=(count, N), dtype=np.uint64)
    d, out = bfv.upload(x), bfv.alloc(count * N)
    bfv.chunk_log()
    bfv.batch_decode(d, count, out)
    for i in _boundary(bfv, count):
        exp = np.zeros(N, dtype=np.uint64)
        L.ref_batch_decode(C.byref(tb.t), O.ptr(x[i]), N, O.ptr(exp))
        assert np.array_equal(_item(S, bfv, out, i, N), exp), ("batch_decode", i)
    d.free()
    out.free()
    done.append("batch_decode")

    # ---- CKKSEncoder::encode and decode
    ck = O.CkksRef(rckks)
    k, count, scale = 2, 513, 2.0 ** 40
    v = rng.integers(-(1 << 30), 1 << 30, size=(count, N // 2)) + 1j * rng.integers(-(1 << 30), 1 << 30, size=(count, N // 2))
    ckks.chunk_log()
    plain = ckks.ckks_encode(v, k, scale)
    for i in _boundary(ckks, count):
        rc, exp = ck.encode(v[i], k, scale)
        assert rc == 0 and np.array_equal(_item(S, ckks, plain, i, k * N), exp.reshape(-1)), ("ckks_encode", i)
    plain.free()
    done.append("ckks_encode")
    count = 257
    x = rows(rng, mods[:k], N, (count,))
    d = ckks.upload(x)
    ckks.chunk_log()
    dec = ckks.ckks_decode(d, k, count, scale)
    for i in _boundary(ckks, count):
        assert np.array_equal(dec[i].view(np.uint64), ck.decode(x[i], scale).view(np.uint64)), ("ckks_decode", i)  # the same bits
    d.free()
    done.append("ckks_decode")
    print("CHUNKED_OK " + " ".join(done))


def test_ops_span_arena_chunks():
    run_arena_child(__file__, "CHUNKED_OK", timeout=600)


if __name__ == "__main__" and "--child" in sys.argv:
    child_main(_child)
