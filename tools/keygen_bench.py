#!/usr/bin/env python3
"""Key generation on one MI355X (DESIGN.md "Key generation"): prints one JSON line per measurement.
    python tools/keygen_bench.py [--reps R] [--only cfg3,cfg4,cfg5] [--what relin1,galois1,all]
Times are host clocks around calls that synchronise themselves (sealhip_generate_*_keys and sealhip_kswitch_key_load_stream
end in a device synchronisation), after one warm-up call of the same shape; medians over --reps windows. Keys are destroyed
outside the timed windows. Next to every generation: the load of the seeded stream of the same keys
(sealhip_kswitch_key_load_stream, which expands the seeds on the device), and the host PRNG of the same digits on one
thread (sealhip_expand_seed_host: the part of a host composition that no host implementation avoids). Per-kernel times
come from a separate rocprofv3 --kernel-trace --stats run of this tool."""
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

PID = (1, 2, 3, 4)


def median_time(fn, reps, after=lambda r: None):
    after(fn())
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
        after(r)
    return float(np.median(ts))


def get_elts_all(logn):
    """GaloisTool::get_elts_all (galois.cpp:102-127): 2N - 1, then 5^(2^i) and 5^(-2^i) for i < log N - 1. The last pair is
    one element (5^(N/4) has order 2), which galois_keys() makes once: 2 (log N - 1) keys."""
    n, m = 1 << logn, 2 << logn
    out = [m - 1]
    for i in range(logn - 1):
        for e in (pow(5, 1 << i, m), pow(5, n // 2 - (1 << i), m)):
            if e not in out:
                out.append(e)
    return out


def destroy(keys):
    for k in keys:
        k.__del__()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="cfg3,cfg4,cfg5")
    ap.add_argument("--what", default="relin1,galois1,all")
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
        ctx = S.Context(scheme, logn, mods, 1, t)
        ctx.set_parms_id(n_key, PID)
        d = n_key - 1
        sk = ctx.upload(np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods]))
        for what in a.what.split(","):
            elts = {"relin1": None, "galois1": [3], "all": get_elts_all(logn)}[what]
            n_keys = 1 if elts is None else len(elts)
            seeds = rng.integers(0, 2**64, size=(n_keys, d, 8), dtype=np.uint64)
            noise = ctx.upload_i32(rng.integers(-41, 42, size=(n_keys, d, n), dtype=np.int32))

            def gen(keep=False):
                if elts is None:
                    return ctx.generate_relin_keys(sk, 1, seeds, noise, keep_seeds=keep)
                return ctx.generate_galois_keys(sk, elts, seeds, noise, keep_seeds=keep)

            t_gen = median_time(gen, a.reps, destroy)
            keys = gen(True)
            raw = S.save_kswitch_keys_seeded(ctx, keys)
            destroy(keys)
            buf = (C.c_char * len(raw)).from_buffer_copy(raw)

            def load():
                out = []
                for i in range(n_keys):
                    h, slots = C.c_void_p(), C.c_uint64(0)
                    S._check(S.lib().sealhip_kswitch_key_load_stream(ctx.handle, C.addressof(buf), len(raw), i, C.byref(h),
                                                                     C.byref(slots)))
                    out.append(S.KSwitchKeys._adopt(ctx, h.value))
                return out

            t_load = median_time(load, a.reps, destroy)
            seed0 = [int(x) for x in seeds[0, 0]]
            t_host_digit = median_time(lambda: ctx.expand_seed(n_key, seed0), max(1, a.reps // 2))
            key_bytes = d * 2 * n_key * n * 8
            print(json.dumps({"config": name, "what": what, "keys": n_keys, "digits": d, "key_mb": key_bytes / 1e6,
                              "generate_ms": t_gen * 1e3, "load_seeded_stream_ms": t_load * 1e3,
                              "host_prng_one_thread_ms": t_host_digit * d * n_keys * 1e3,
                              "generate_gbps_key_bytes": n_keys * key_bytes / t_gen / 1e9}), flush=True)
            del noise


if __name__ == "__main__":
    main()
