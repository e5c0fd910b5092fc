#!/usr/bin/env python3
"""Baby-step/giant-step matrix-vector products on one MI355X: prints one JSON line per measurement.
    python tools/bsgs_bench.py --baseline-lib PATH [--only cfg4,cfg5] [--counts 1,64] [--cells 2x2,4x4,8x8,4x16]
                               [--rounds 3] [--min-seconds 0.5]
A cell is n_giant x n_baby; the first element of each axis is the identity (rotation step 0), as in a BSGS product.
candidate: ONE sealhip_evaluator_apply_galois_bsgs_plain call (this tree's library);
baseline:  the composition it replaces, with the library of the PARENT commit (--baseline-lib is its libsealhip.so, built
           from a checkout of the parent next to this tree): one sealhip_evaluator_apply_galois_dot_plain for the n_giant
           inner sums, then one sealhip_evaluator_apply_galois and one sealhip_evaluator_add per non-identity giant.
Each side runs in a process of its own per round (--rounds of them, candidate and baseline alternated); a process warms
every shape up, then times it with device events around at least --min-seconds of back-to-back calls. The driver reports the
median and the spread (max - min) over the rounds and the ratio fused / composed; every record carries the library's launch
profile of one call. The bar: at 4x4 and 8x8 the fused median is no slower than the composed one.
Shapes: config 4 (CKKS, N = 2^15, 12 primes) and config 5's ring (N = 2^16, 16 primes, run as CKKS)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_apply_galois_bsgs_plain", "sealhip_evaluator_rotate_vector_bsgs_plain")


def worker(a):
    import torch

    import sealhip as S
    from bench import CFG4_PRIMES, CFG5_PRIMES

    baseline = a.role == "composed"
    if baseline:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg4": (15, CFG4_PRIMES), "cfg5": (16, CFG5_PRIMES)}
    counts = [int(v) for v in a.counts.split(",")]
    cells = [tuple(int(v) for v in c.split("x")) for c in a.cells.split(",")]
    rng = np.random.default_rng(4)
    stream = torch.cuda.Stream()
    L = S.lib()
    for name in a.only.split(","):
        logn, mods = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k = n_key - 1
        nd = k
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0)
        ctx.set_stream(stream.cuda_stream)
        ev = S.Evaluator(ctx)
        max_e = max(max(c) for c in cells) - 1
        elts = [ctx.galois_elt_from_step(s + 1) for s in range(2 * max_e)]
        one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
        keys = []
        for _ in range(2 * max_e):  # (timing does not depend on the key words: one random slice, rolled)
            one = np.roll(one, 1, axis=1)
            keys.append(S.KSwitchKeys(ctx, np.broadcast_to(one, (nd, 2, n_key, n)).copy()))
        for count in counts:
            item = 2 * k * n
            src_h = np.stack([rng.integers(0, q, size=(count * 2, n), dtype=np.uint64) for q in mods[:k]], axis=1)
            src = ctx.upload(src_h)
            for n_giant, n_baby in cells:
                w_h = np.stack([rng.integers(0, q, size=(n_giant * n_baby, n), dtype=np.uint64) for q in mods], axis=1)
                plains = ctx.upload(w_h)
                baby, bkeys = [1] + elts[:n_baby - 1], [None] + keys[:n_baby - 1]
                giant, gkeys = [1] + elts[max_e:max_e + n_giant - 1], [None] + keys[max_e:max_e + n_giant - 1]
                out = ctx.alloc(count * item)
                inner = ctx.alloc(n_giant * count * item) if baseline else None
                if baseline:

                    def call():
                        ev.apply_galois_dot_plain(src, k, count, baby, bkeys, plains, n_giant, inner)
                        for j in range(1, n_giant):
                            term = inner.ptr + j * count * item * 8
                            ev.apply_galois_inplace(term, k, count, giant[j], gkeys[j])
                            S._check(L.sealhip_evaluator_add(ctx.handle, k, inner.ptr, 2, term, 2, count, inner.ptr))
                else:

                    def call():
                        ev.apply_galois_bsgs_plain(src, k, count, baby, bkeys, giant, gkeys, plains, out)

                call()
                call()
                ctx.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                ctx.synchronize()
                reps = max(1, int(a.min_seconds * 1e3 / max(t0.elapsed_time(t1), 1e-3)) + 1)
                t0.record(stream)
                for _ in range(reps):
                    call()
                t1.record(stream)
                ctx.synchronize()
                ms = t0.elapsed_time(t1) / reps
                rec = {"config": name, "role": a.role, "count": count, "n_giant": n_giant, "n_baby": n_baby, "k": k,
                       "reps": reps, "ms_per_call": ms}
                ctx.profile_enable(True)
                call()
                prof = ctx.profile_fetch()
                ctx.profile_enable(False)
                rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
                print(json.dumps(rec), flush=True)
                for b in (out, inner, plains):
                    if b is not None:
                        b.free()
            src.free()
        del keys, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--only", default="cfg4,cfg5")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--cells", default="2x2,4x4,8x8,4x16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        return worker(a)
    assert os.path.exists(a.baseline_lib), "the parent commit's libsealhip.so is needed for the baseline"
    base = [sys.executable, os.path.abspath(__file__), "--baseline-lib", a.baseline_lib, "--only", a.only, "--counts", a.counts,
            "--cells", a.cells, "--min-seconds", str(a.min_seconds)]
    got = {}
    for rnd in range(a.rounds):
        for role in ("fused", "composed"):  # alternated: every round runs each side once, a process each
            out = subprocess.run(base + ["--role", role], capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                return 1
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
                got.setdefault((rec["config"], rec["count"], rec["n_giant"], rec["n_baby"], role), []).append(rec)
    for (cfg, count, n_giant, n_baby, role), recs in sorted(got.items()):
        if role != "fused":
            continue
        comp = got[(cfg, count, n_giant, n_baby, "composed")]
        f = [r["ms_per_call"] for r in recs]
        c = [r["ms_per_call"] for r in comp]
        print(json.dumps({"summary": cfg, "count": count, "n_giant": n_giant, "n_baby": n_baby,
                          "fused_ms_median": float(np.median(f)), "fused_ms_spread": max(f) - min(f),
                          "composed_ms_median": float(np.median(c)), "composed_ms_spread": max(c) - min(c),
                          "fused_over_composed": float(np.median(f) / np.median(c)),
                          "no_slower_than_composed": bool(np.median(f) <= np.median(c))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
