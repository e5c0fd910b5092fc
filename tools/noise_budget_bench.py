#!/usr/bin/env python3
"""Decryptor::invariant_noise_budget on one MI355X: prints one JSON line per measurement.
    python tools/noise_budget_bench.py [--reps R] [--only cfg3,cfg5] [--counts 1,64,1024]
Times are host clocks around sealhip_decryptor_invariant_noise_budget (it ends in a device synchronisation), after one
warm-up call of the same shape; medians over --reps calls. Next to each: the BFV decrypt of the same batch (stream-ordered,
timed with a synchronisation after it). Ciphertexts are uniform words of size 2 at the first data level; the budget does not
depend on the values. Per-kernel times come from a separate rocprofv3 --kernel-trace --stats run of this tool."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

import sealhip as S
from bench import CFG3_PRIMES, CFG5_PRIMES


def median_time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="cfg3,cfg5")
    ap.add_argument("--counts", default="1,64,1024")
    a = ap.parse_args()
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg3": (15, CFG3_PRIMES), "cfg5": (16, CFG5_PRIMES)}
    rng = np.random.default_rng(1)
    for name in a.only.split(","):
        logn, mods = cfgs[name]
        n, k = 1 << logn, len(mods) - 1
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, 786433)
        pw = ctx.upload(np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]))
        one = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods[:k]]) for _ in range(2)])
        counts = [int(c) for c in a.counts.split(",")]
        ct = ctx.alloc(max(counts) * one.size)
        for i in range(max(counts)):  # the same ciphertext in every slot
            S._check(S.lib().sealhip_memcpy_h2d(ctx.handle, ct.ptr + i * one.nbytes, one.ctypes.data, one.nbytes))
        plain = ctx.alloc(max(counts) * n)
        for count in counts:
            t_nb = median_time(lambda: ctx.invariant_noise_budget(ct, 2, k, count, pw), a.reps)

            def dec():
                ctx.decrypt(ct, 2, k, count, pw, False, plain)
                ctx.synchronize()

            t_dec = median_time(dec, a.reps)
            print(json.dumps({"config": name, "log_n": logn, "k": k, "count": count,
                              "noise_budget_ms": t_nb * 1e3, "decrypt_ms": t_dec * 1e3,
                              "noise_budget_ct_per_s": count / t_nb}), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
