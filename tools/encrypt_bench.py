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
Per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool.
With --sampling it measures instead, per C items:
  sample:        sealhip_sample_polys (1, 2) and (0, 1) alone;
  device:        each encrypt path with its samples drawn on the device (sample_polys_split + encrypt; sample_polys (0, 1)
                 + encrypt_symmetric), next to the same path with the samples handed in (the figure above);
  host:          sealhip_sample_polys_host (1, 2) on one thread and on 16, for --host-items items scaled to C, and the
                 host-to-device copy of C items' samples: what a caller's own sampler costs at best;
  reference-style: samples per second of tests/sample_law_check.cpp (normal_distribution, redraw, truncate) on one thread;
  leaf:          the engine's event timing (sealhip_profile) of seed_leaf and sample_leaf in this run, per leaf."""
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


def law_check_rate():
    """samples per second of tests/sample_law_check.cpp on one thread (None without a compiler)"""
    import subprocess
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sample_law_check")
        try:
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "sample_law_check.cpp")])
            out = subprocess.run([exe, "22"], capture_output=True, text=True, timeout=120).stdout
        except (OSError, subprocess.SubprocessError):
            return None
    for line in out.splitlines():
        if line.startswith("samples_per_second"):
            return float(line.split()[1])
    return None


def sampling(a, name, scheme, logn, mods, t, rng):
    from concurrent.futures import ThreadPoolExecutor

    n, n_key = 1 << logn, len(mods)
    k, count = n_key - 1, a.count
    ctx = S.Context(scheme, logn, mods, 1, t)
    sk = ctx.upload(np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]))
    pk = ctx.upload(np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]) for _ in range(2)]))
    seeds = rng.integers(0, 2**64, size=(count, 8), dtype=np.uint64)
    seeds2 = rng.integers(0, 2**64, size=(count, 8), dtype=np.uint64)
    if scheme == 1:
        pl = ctx.upload(rng.integers(0, t, size=(count, n), dtype=np.uint64))
    else:
        pl = ctx.upload(np.stack([rng.integers(0, q, size=(count, n), dtype=np.uint64) for q in mods[:k]], axis=1))
    pstride = n if scheme == 1 else k * n
    ct = ctx.alloc(count * 2 * k * n)
    all3, u, e, es = ctx.alloc(count * 3 * n // 2), ctx.alloc(count * n // 2), ctx.alloc(count * n), ctx.alloc(count * n // 2)

    def median(fn):
        timed(ctx, fn)
        return float(np.median([timed(ctx, fn) for _ in range(a.reps)]))

    def emit(what, seconds, **more):
        print(json.dumps(dict({"config": name, "what": what, "count": count, "k": k, "ms": seconds * 1e3}, **more)), flush=True)

    def asym_device():
        ctx.sample_polys_split(seeds, 1, 2, u, e)
        ctx.encrypt(k, pk, pl, u, e, count, ct, plain_item_stride=pstride)

    def sym_device():
        ctx.sample_polys(seeds2, 0, 1, es)
        ctx.encrypt_symmetric(k, sk, pl, seeds, es, count, ct, plain_item_stride=pstride)

    t12 = median(lambda: ctx.sample_polys(seeds, 1, 2, all3))
    t01 = median(lambda: ctx.sample_polys(seeds, 0, 1, es))
    emit("sample_polys_1_2", t12)
    emit("sample_polys_0_1", t01)
    ta_dev = median(asym_device)
    ta_in = median(lambda: ctx.encrypt(k, pk, pl, u, e, count, ct, plain_item_stride=pstride))
    emit("asym_device_samples", ta_dev, samples_handed_in_ms=ta_in * 1e3, sampling_over_call=t12 / ta_dev)
    ts_dev = median(sym_device)
    ts_in = median(lambda: ctx.encrypt_symmetric(k, sk, pl, seeds, es, count, ct, plain_item_stride=pstride))
    emit("sym_device_samples", ts_dev, samples_handed_in_ms=ts_in * 1e3, sampling_over_call=t01 / ts_dev)
    # the engine's own event timing of the two leaf kernels, per leaf (units = leaves)
    ctx.profile_enable(True)
    for _ in range(a.reps):
        ctx.sample_polys(seeds, 1, 2, all3)
        ctx.expand_seeds(k, seeds, ct)
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    per_leaf = {tag: prof[tag]["ms"] * 1e6 / prof[tag]["units"] for tag in ("seed_leaf", "sample_leaf") if tag in prof}
    if len(per_leaf) == 2:
        print(json.dumps({"config": name, "what": "leaf", "seed_leaf_ns_per_leaf": per_leaf["seed_leaf"],
                          "sample_leaf_ns_per_leaf": per_leaf["sample_leaf"],
                          "sample_over_seed": per_leaf["sample_leaf"] / per_leaf["seed_leaf"],
                          "sample_leaf_ms_per_call": prof["sample_leaf"]["ms"] / a.reps,
                          "seed_leaf_ms_per_call": prof["seed_leaf"]["ms"] / a.reps}), flush=True)
    # a caller's sampler at best: the same rule on the host, then the copy
    items = min(count, a.host_items)
    host = S.Context(scheme, logn, mods, 1, t, device=-1)
    t0 = time.perf_counter()
    one = host.sample_polys_host(seeds[:items], 1, 2)
    t1 = (time.perf_counter() - t0) / items * count
    with ThreadPoolExecutor(16) as pool:
        t0 = time.perf_counter()
        list(pool.map(lambda i: host.sample_polys_host(seeds[i : i + 1], 1, 2), range(16 * items)))
        t16 = (time.perf_counter() - t0) / (16 * items) * count
    block = np.ascontiguousarray(np.tile(one, (count // items + 1, 1))[:count])
    th2d = median(lambda: all3.upload(block.view(np.uint64)))
    emit("host_sampler_1_2", t1, threads=1, scaled_from_items=items)
    emit("host_sampler_1_2", t16, threads=16, scaled_from_items=16 * items, h2d_copy_ms=th2d * 1e3)
    rate = law_check_rate()
    if rate:
        emit("reference_style_sampler_1_2", count * 3 * n / rate, threads=1, samples_per_second=rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--oracle-items", type=int, default=2)
    ap.add_argument("--only", default="cfg3,cfg4,cfg5")
    ap.add_argument("--sampling", action="store_true", help="measure the device sampler and the paths fed by it instead")
    ap.add_argument("--host-items", type=int, default=4, help="--sampling: items the host sampler runs (scaled to --count)")
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
        if a.sampling:
            sampling(a, name, scheme, logn, mods, t, rng)
            continue
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
