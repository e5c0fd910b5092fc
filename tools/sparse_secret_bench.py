#!/usr/bin/env python3
"""The fixed-weight sampler on one MI355X: prints one JSON line per measurement.
    python tools/sparse_secret_bench.py [--logn 15,16] [--counts 1,64] [--min-seconds 0.3]
sealhip_sample_fixed_weight (h = 64) next to sealhip_sample_polys(1, 0) -- the yardstick: the same PRNG words, mapped one by
one instead of ranked -- alternating in the same process, five rounds each; device events around at least --min-seconds of
back-to-back calls after two warm-up calls. The ratio of the medians is the cost of ranking; the difference of the medians
over N^2 compares per polynomial gives the rank kernel's compares per second (the raw leaf kernel writes twice the bytes
of the mapped one, which the difference also carries). There is no bar: nothing like this existed to compare against."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", default="15,16")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    a = ap.parse_args()
    import torch

    import oracle_lib as O
    import sealhip as S

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    rng = np.random.default_rng(25)
    for logn in [int(v) for v in a.logn.split(",")]:
        n = 1 << logn
        ctx = S.Context(S.SCHEME_CKKS, logn, O.get_primes(n, 50, 2), 1, 0)
        stream = torch.cuda.Stream()
        ctx.set_stream(stream.cuda_stream)

        def timed(call):
            call()
            call()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            ctx.synchronize()
            reps = max(1, int(a.min_seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
            e0.record(stream)
            for _ in range(reps):
                call()
            e1.record(stream)
            ctx.synchronize()
            return e0.elapsed_time(e1) / reps

        for count in [int(v) for v in a.counts.split(",")]:
            seeds = rng.integers(0, 2**64, size=(count, 8), dtype=np.uint64)
            out = ctx.alloc(count * n // 2)
            fixed, ternary = [], []
            for _ in range(5):
                fixed.append(timed(lambda: ctx.sample_fixed_weight(seeds, 64, out)))
                ternary.append(timed(lambda: ctx.sample_polys(seeds, 1, 0, out)))
            f, t = float(np.median(fixed)), float(np.median(ternary))
            print(json.dumps({"what": "sample_fixed_weight", "logn": logn, "count": count, "h": 64,
                              "fixed_weight_ms": [round(v, 4) for v in fixed], "sample_polys_1_0_ms": [round(v, 4) for v in ternary],
                              "ratio": round(f / t, 2), "rank_compares_per_second": round(count * float(n) * n / ((f - t) * 1e-3), 0),
                              "spread_fixed_weight": round((max(fixed) - min(fixed)) / f, 4),
                              "spread_sample_polys": round((max(ternary) - min(ternary)) / t, 4)}), flush=True)
            out.free()
        ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
