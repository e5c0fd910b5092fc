#!/usr/bin/env python3
"""transform_to_ntt(Plaintext) throughput (sealhip_evaluator_transform_plain_to_ntt) at three shapes, 1024 plaintexts each:
config 3's eight 55-bit primes at N=2^15, config 4's 50-bit primes (FP64 instance) at 2^15 and config 5's sixteen primes at
2^16, each at the first ciphertext level. Per shape, kernel time from sealhip_profile_fetch after a warm-up:
  entry     the entry as shipped: the streaming lift into the destination, then the canonical transform in place
  in-place  sealhip_ntt_negacyclic_harvey on the same count x k rows, already lifted: the lower bound of that composition
The compulsory bytes of the entry are 8N read + 8kN written per plaintext (the in-place transform moves 16N per row);
fractions are against 8 TB/s. (The fused-lift A/B that decided the composition is profiles/r05/plain_ntt.txt.)
    python tools/plain_ntt_bench.py [--count 1024] [--reps 5] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gemini-seal_amd"))
import numpy as np

import sealhip as S

P15_55 = [36028797010444289, 36028797012606977, 36028797013000193, 36028797013327873, 36028797014376449,
          36028797014573057, 36028797014704129, 36028797017456641]
P15_50 = [1125899885412353, 1125899885740033, 1125899886395393, 1125899887312897, 1125899896160257, 1125899899174913,
          1125899901665281, 1125899902124033, 1125899903107073, 1125899903500289, 1125899903827969, 1125899904679937]
P16 = [1125899864506369, 1125899865948161, 1125899870011393, 1125899870404609, 1125899877875713, 1125899879710721,
       1125899882987521, 1125899883380737, 1125899883642881, 1125899884036097, 1125899884167169, 1125899885740033,
       1125899886395393, 1125899887312897, 1125899902124033, 1125899903827969]
SHAPES = [("cfg3 N=2^15 8 x 55-bit (k=7)", 15, P15_55), ("cfg4 N=2^15 12 x 50-bit (k=11, FP64)", 15, P15_50),
          ("cfg5 N=2^16 16 x 50-bit (k=15, FP64)", 16, P16)]
T = 786433


def kernel_ms(ctx, fn, reps):
    fn()
    ctx.synchronize()
    ctx.profile_enable(True)
    for _ in range(reps):
        fn()
    ctx.synchronize()
    prof = ctx.profile_fetch()
    ctx.profile_enable(False)
    return sum(v["ms"] for v in prof.values()) / reps, prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for name, logn, mods in SHAPES:
        n, k, count = 1 << logn, len(mods) - 1, a.count
        ctx = S.Context(S.SCHEME_BFV, logn, mods, 1, T, device=0)
        ev = S.Evaluator(ctx)
        rng = np.random.default_rng(logn + k)
        plain = ctx.upload(rng.integers(0, T, count * n, dtype=np.uint64))
        out = ctx.alloc(count * k * n)
        entry_ms, _ = kernel_ms(ctx, lambda: ev.transform_plain_to_ntt(plain, n, k, count, out), a.reps)
        inplace_ms, _ = kernel_ms(ctx, lambda: ctx.ntt_negacyclic_harvey(out, count, k), a.reps)
        compulsory = count * (8 * n + 8 * k * n)
        line = ("%s, %d plaintexts: entry (lift + transform) %.3f ms = %.0f plaintexts/s, %.1f %% HBM (compulsory 8N + 8kN B) | "
                "in-place transform of the lifted rows %.3f ms (%.1f %% at 16N B/row) | entry / in-place = %.3f" % (
                    name, count, entry_ms, count / (entry_ms / 1e3), compulsory / (entry_ms / 1e3) / 8e12 * 100,
                    inplace_ms, count * k * 16 * n / (inplace_ms / 1e3) / 8e12 * 100, entry_ms / inplace_ms))
        print(line, flush=True)
        lines.append(line)
        for buf in (plain, out):
            buf.free()
        ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# tools/plain_ntt_bench.py --count %d --reps %d, one MI355X, one process\n" % (a.count, a.reps))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
