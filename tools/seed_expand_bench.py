#!/usr/bin/env python3
"""Seed expansion on one MI355X (DESIGN.md "Seed expansion"): prints one JSON line per measurement.
    python tools/seed_expand_bench.py [--reps R] [--only name,...]
Times are host clocks around calls that end in a device synchronisation (every timed window ends in ctx.synchronize() or
in an entry that synchronises itself), after one warm-up call of the same shape; medians over --reps windows.
"gbps" = expanded words (8 bytes each) per second. Per-kernel times come from a separate rocprofv3 --kernel-trace --stats
run of this tool; clocks and VALU counters from a counters-only run (profiles/seed_expand/README.md)."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

import sealhip as S
from bench import CFG3_PRIMES, CFG4_PRIMES, CFG5_PRIMES


def wire():
    import importlib.util

    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(ROOT, "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    return W


def median_time(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def key_stream(W, key_id, n, n_key, digits, rng):
    body = struct.pack("<4Q", *key_id) + struct.pack("<Q", 1) + struct.pack("<Q", digits)
    for _ in range(digits):
        c0 = rng.integers(0, 2**50, size=n_key * n, dtype=np.uint64)
        body += W.save_ciphertext(key_id, True, 2, n, n_key, 1.0, c0, seed=rng.bytes(64))
    return W.header(16 + len(body)) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    want = lambda name: not a.only or name in a.only.split(",")
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    W = wire()
    rng = np.random.default_rng(1)
    out = []
    n3, k3 = 1 << 15, 7
    ctx3 = S.Context(S.SCHEME_BFV, 15, CFG3_PRIMES, 1, 786433)
    sync3 = ctx3.synchronize
    words3 = k3 * n3
    if want("host"):
        seed = [int(x) for x in rng.integers(0, 2**63, size=8)]
        t = median_time(lambda: ctx3.expand_seed(k3, seed), a.reps, lambda: None)
        out.append({"what": "host expand_seed_host, one thread, cfg3 k=7", "ms": t * 1e3, "gbps": words3 * 8 / t / 1e9})
    if want("load"):
        pid = (1, 2, 3, 4)
        ctx3.set_parms_id(k3, pid)
        raw = W.save_ciphertext(pid, True, 2, n3, k3, 1.0, rng.integers(0, 2**50, size=words3, dtype=np.uint64),
                                seed=rng.bytes(64))
        dst = ctx3.alloc(2 * words3)
        rbuf = (C.c_char * len(raw)).from_buffer_copy(raw)
        info = S.CiphertextInfo()
        t = median_time(lambda: S._check(S.lib().sealhip_ciphertext_load(ctx3.handle, C.addressof(rbuf), len(raw),
                                                                         C.addressof(info), dst.ptr, 2 * words3)),
                        a.reps, sync3)
        out.append({"what": "one seeded cfg3 ciphertext through sealhip_ciphertext_load, end to end", "ms": t * 1e3})
        count = 1024
        raws = [W.save_ciphertext(pid, True, 2, n3, k3, 1.0, rng.integers(0, 2**50, size=words3, dtype=np.uint64),
                                  seed=rng.bytes(64)) for _ in range(count)]
        dstm = ctx3.alloc(count * 2 * words3)
        bufs = [(C.c_char * len(r)).from_buffer_copy(r) for r in raws]  # as the binding holds them: not timed
        ptrs = (C.c_void_p * count)(*[C.addressof(b) for b in bufs])
        lens = (C.c_size_t * count)(*[len(r) for r in raws])
        infos = (S.CiphertextInfo * count)()
        t = median_time(lambda: S._check(S.lib().sealhip_ciphertext_load_many(
            ctx3.handle, C.addressof(ptrs), C.addressof(lens), count, C.addressof(infos), dstm.ptr, 2 * words3)),
            max(2, a.reps // 2), sync3)
        out.append({"what": "1024 seeded cfg3 streams through sealhip_ciphertext_load_many, end to end", "ms": t * 1e3,
                    "streams_per_s": count / t})
        del dstm
    if want("expand"):
        for count in (1, 64, 1024):
            seeds = rng.integers(0, 2**63, size=(count, 8), dtype=np.uint64)
            o = ctx3.alloc(count * words3)
            t = median_time(lambda: ctx3.expand_seeds(k3, seeds, o), a.reps, sync3)
            out.append({"what": "sealhip_expand_seed, cfg3 k=7", "seeds": count, "ms": t * 1e3,
                        "gbps": count * words3 * 8 / t / 1e9})
            del o
    for name, logn, primes, nsp in (("cfg4", 15, CFG4_PRIMES, 1), ("cfg5", 16, CFG5_PRIMES, 1)):
        if not want(name):
            continue
        n, n_key = 1 << logn, len(primes)
        ctx = S.Context(S.SCHEME_CKKS, logn, primes, nsp, 0)
        key_id = (9, 9, 9, 9)
        ctx.set_parms_id(n_key, key_id)
        digits = n_key - nsp
        raw = key_stream(W, key_id, n, n_key, digits, rng)
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)  # the stream as a binding holds it: not part of the timing

        def load():
            h, slots = C.c_void_p(), C.c_uint64(0)
            S._check(S.lib().sealhip_kswitch_key_load_stream(ctx.handle, C.addressof(buf), len(raw), 0, C.byref(h),
                                                             C.byref(slots)))
            S.lib().sealhip_kswitch_key_destroy(ctx.handle, h.value)

        t = median_time(load, a.reps, ctx.synchronize)
        out.append({"what": "one seeded %s-shaped Galois key (%d digits x %d primes, N=2^%d) through "
                            "sealhip_kswitch_key_load_stream, end to end" % (name, digits, n_key, logn),
                    "ms": t * 1e3, "expanded_mb": digits * n_key * n * 8 / 1e6})
    for line in out:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
