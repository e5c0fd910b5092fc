#!/usr/bin/env python3
"""Encryption on one MI355X: prints one JSON line per measurement.
    python tools/encrypt_bench.py [--reps R] [--count C] [--only cfg3,cfg4,cfg5]
For each config and path (public key; secret key; secret key seeded, BFV only) it times, with host clocks around a
synchronise after one warm-up call, medians over --reps windows:
  fused:    the new entry (sealhip_encryptor_encrypt / sealhip_encryptor_encrypt_symmetric) on C ciphertexts;
  composed: the existing entries chained on the device on the same samples, without any host round trip:
            public key  encrypt_zero_asymmetric over k + 1 rows, divide_and_round_q_last(_ntt)_inplace, then the plaintext
                        step (multiply_add_plain_with_scaling_variant / evaluator_add_plain) on a k-row buffer (the row copy
                        between them is left out, which favours the composition);
            secret key  expand_seed, encrypt_zero_symmetric, then the plaintext step;
  the two are alternated in the same process, window by window;
  oracle:   the oracle's composition on one CPU thread for --oracle-items items, scaled to C.
Per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

import sealhip as S
from bench import CFG3_PRIMES, CFG4_PRIMES, CFG5_PRIMES


def timed(ctx, fn):
    ctx.synchronize()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return time.perf_counter() - t0


def alternate(ctx, a, b, reps):
    timed(ctx, a)
    timed(ctx, b)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(ctx, a))
        tb.append(timed(ctx, b))
    return float(np.median(ta)), float(np.median(tb))


def oracle_time(scheme, logn, mods, t, items, asym, u, e, seeds, es, plains, k):
    """the oracle's composition per item on one thread (oracle_lib entries), seconds per item"""
    import oracle_lib as O

    L = O.lib()
    n, n_key = 1 << logn, len(mods)
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=t)
    cl = O.Client(ref, seed=3)
    pk = np.zeros((2, n_key, n), dtype=np.uint64)
    L.ref_encrypt_zero_symmetric(C.byref(ref.c), n_key, O.ptr(cl.sk), 1, C.byref(cl.state), O.ptr(pk))
    R = k + 1
    pkr = np.ascontiguousarray(pk[:, :R])
    ntt = 1 if scheme == 2 else 0
    t0 = time.perf_counter()
    for i in range(items):
        if asym:
            big = np.zeros((2, R, n), dtype=np.uint64)
            L.ref_encrypt_zero_asymmetric_given(C.byref(ref.c), R, O.ptr(pkr), ntt, np.ascontiguousarray(u[i]).ctypes.data,
                                                np.ascontiguousarray(e[i]).ctypes.data, O.ptr(big))
            tool = ref.rns_tool(R)
            for j in range(2):
                if ntt:
                    L.ref_divide_and_round_q_last_ntt_inplace(tool, O.ptr(big[j]), ref.c.key_tables, 0)
                else:
                    L.ref_divide_and_round_q_last_inplace(tool, O.ptr(big[j]))
            ct = np.ascontiguousarray(big[:, :k])
        else:
            a = np.ascontiguousarray(O.expand_seed(seeds[i], mods[:k], n))
            ct = np.zeros((2, k, n), dtype=np.uint64)
            L.ref_encrypt_zero_symmetric_given(C.byref(ref.c), k, O.ptr(cl.sk), ntt, O.ptr(a),
                                               np.ascontiguousarray(es[i]).ctypes.data, O.ptr(ct))
        if scheme == 1:
            L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(plains[i])), 0,
                                                          O.ptr(ct[0]))
        else:
            for r in range(k):
                L.ref_add_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(np.ascontiguousarray(plains[i][r])), n,
                                        C.byref(ref.c.key_mod[r]), O.ptr(ct[0, r]))
    return (time.perf_counter() - t0) / items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--oracle-items", type=int, default=2)
    ap.add_argument("--only", default="cfg3,cfg4,cfg5")
    a = ap.parse_args()
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {
        "cfg3": (S.SCHEME_BFV, 15, CFG3_PRIMES, 786433),
        "cfg4": (S.SCHEME_CKKS, 15, CFG4_PRIMES, 0),
        "cfg5": (S.SCHEME_BFV, 16, CFG5_PRIMES, 786433),
    }
    rng = np.random.default_rng(1)
    for name in a.only.split(","):
        scheme, logn, mods, t = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k, R, count = n_key - 1, n_key, a.count
        ctx = S.Context(scheme, logn, mods, 1, t)
        sk = ctx.upload(np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]))
        pk_h = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]) for _ in range(2)])
        pk = ctx.upload(pk_h)
        pk_r = ctx.upload(np.ascontiguousarray(pk_h[:, :R]))
        u_h = rng.integers(-1, 2, size=(count, n), dtype=np.int32)
        e_h = rng.integers(-41, 42, size=(count, 2, n), dtype=np.int32)
        es_h = rng.integers(-41, 42, size=(count, n), dtype=np.int32)
        seeds = rng.integers(0, 2**64, size=(count, 8), dtype=np.uint64)
        if scheme == 1:
            pl_h = rng.integers(0, t, size=(count, n), dtype=np.uint64)
        else:
            pl_h = np.stack([rng.integers(0, q, size=(count, n), dtype=np.uint64) for q in mods[:k]], axis=1)
        u, e, es, pl = ctx.upload_i32(u_h), ctx.upload_i32(e_h), ctx.upload_i32(es_h), ctx.upload(pl_h)
        pstride = n if scheme == 1 else k * n
        ct = ctx.alloc(count * 2 * k * n)
        big = ctx.alloc(count * 2 * R * n)
        a_buf = ctx.alloc(count * k * n)

        def plain_step(buf):
            if scheme == 1:
                ctx.multiply_add_plain_with_scaling_variant(k, pl, buf, 2, count)
            else:
                S._check(S.lib().sealhip_evaluator_add_plain(ctx.handle, k, buf.ptr, 2, count, pl.ptr, pstride, 0))

        def fused_asym():
            ctx.encrypt(k, pk, pl, u, e, count, ct, plain_item_stride=pstride)

        def composed_asym():
            ctx.encrypt_zero_asymmetric(R, scheme == 2, pk_r, u, e, count, big)
            if scheme == 1:
                ctx.divide_and_round_q_last_inplace(R, big, count * 2)
            else:
                ctx.divide_and_round_q_last_ntt_inplace(R, big, count * 2)
            plain_step(ct)

        def fused_sym(seeded=False):
            ctx.encrypt_symmetric(k, sk, pl, seeds, es, count, ct, save_seed=seeded, plain_item_stride=pstride)

        def composed_sym():
            ctx.expand_seeds(k, seeds, a_buf)
            ctx.encrypt_zero_symmetric(k, scheme == 2, a_buf, es, sk, count, ct)
            plain_step(ct)

        rows = [("asym", fused_asym, composed_asym), ("sym", fused_sym, composed_sym)]
        if scheme == 1:
            rows.append(("sym_seeded", lambda: fused_sym(True), None))
        for what, fused, composed in rows:
            if composed is not None:
                tf, tc = alternate(ctx, fused, composed, a.reps)
            else:
                tf, _ = alternate(ctx, fused, fused, a.reps)
                tc = None
            to = None
            if what != "sym_seeded" and a.oracle_items > 0:
                to = oracle_time(scheme, logn, mods, t, a.oracle_items, what == "asym", u_h, e_h, seeds, es_h, pl_h, k)
            print(json.dumps({"config": name, "what": what, "count": count, "k": k, "fused_ms": tf * 1e3,
                              "composed_ms": None if tc is None else tc * 1e3,
                              "fused_over_composed": None if tc is None else tf / tc,
                              "oracle_one_thread_ms_scaled": None if to is None else to * count * 1e3}), flush=True)
        del ct, big, a_buf


if __name__ == "__main__":
    main()
