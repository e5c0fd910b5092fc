#!/usr/bin/env python3
"""Ciphertext inner products on one MI355X: prints one JSON line per measurement.
    python tools/dot_ct_bench.py --baseline-lib PATH [--only cfg3,cfg4] [--counts 1,64] [--terms 2,4,8,16]
                                 [--rounds 3] [--min-seconds 0.5]
candidate:  ONE sealhip_evaluator_dot_product call with a relinearization key (this tree's library);
baselines:  the compositions it replaces, with the library of the PARENT commit (--baseline-lib is its libsealhip.so, built
            from a checkout of the parent next to this tree):
            composed_a: multiply per term, add of the size-3 products, one relinearize (the best composition there);
            composed_b: multiply + relinearize per term, then add of the size-2 results.
Each side runs in a process of its own per round (--rounds of them, the three sides alternated); a process warms every shape
up, then times it with device events around at least --min-seconds of back-to-back calls. The driver reports the median and
the spread (max - min) over the rounds and the ratios dot / composed; every record carries the library's launch profile of
one call. The bar: at 8 terms and 64 items the single call's median is no slower than composed_a's at both shapes.
Shapes: config 3's ring in STRICT mode (BFV, N = 2^15, k = 7) and config 4 (CKKS, N = 2^15, k = 11)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_dot_product", "sealhip_evaluator_dot_product_max_terms")
ROLES = ("dot", "composed_a", "composed_b")


def worker(a):
    import torch

    import sealhip as S
    from bench import CFG3_PRIMES, CFG4_PRIMES, PLAIN_T

    baseline = a.role != "dot"
    if baseline:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg3": (S.SCHEME_BFV, 15, CFG3_PRIMES, PLAIN_T), "cfg4": (S.SCHEME_CKKS, 15, CFG4_PRIMES, 0)}
    counts = [int(v) for v in a.counts.split(",")]
    term_counts = [int(v) for v in a.terms.split(",")]
    rng = np.random.default_rng(18)
    stream = torch.cuda.Stream()
    dev = torch.device("cuda:0")
    L = S.lib()
    for name in a.only.split(","):
        scheme, logn, mods, t = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k = n_key - 1
        ctx = S.Context(scheme, logn, mods, 1, t, mode=S.MODE_STRICT)
        ctx.set_stream(stream.cuda_stream)
        ev = S.Evaluator(ctx)
        one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
        key = S.KSwitchKeys(ctx, np.broadcast_to(one, (k, 2, n_key, n)).copy())  # (timing does not depend on the key words)
        low = int(min(mods[:k]))
        for count in counts:
            item = k * n
            # canonical residues of every prime (below the smallest one); the values play no part in the timing
            ops = [torch.randint(0, low, (count * 2 * item,), dtype=torch.int64, device=dev) for _ in range(2 * max(term_counts))]
            out = ctx.alloc(count * 3 * item)
            prod = ctx.alloc(count * 3 * item) if baseline else None
            for n_terms in term_counts:
                xs, ys = ops[:n_terms], ops[max(term_counts):max(term_counts) + n_terms]
                if a.role == "dot":

                    def call():
                        ev.dot_product(xs, ys, k, count, out, [key])
                elif a.role == "composed_a":

                    def call():
                        ev.multiply(xs[0], 2, ys[0], 2, k, count, out)
                        for i in range(1, n_terms):
                            ev.multiply(xs[i], 2, ys[i], 2, k, count, prod)
                            S._check(L.sealhip_evaluator_add(ctx.handle, k, out.ptr, 3, prod.ptr, 3, count, out.ptr))
                        ev.relinearize_inplace(out, 3, k, count, [key])
                else:

                    def call():
                        # (relinearize leaves the size-2 result in the leading polynomials of each size-3 item: the add walks
                        #  the items as size 3 and the third polynomial's sums are not used)
                        ev.multiply(xs[0], 2, ys[0], 2, k, count, out)
                        ev.relinearize_inplace(out, 3, k, count, [key])
                        for i in range(1, n_terms):
                            ev.multiply(xs[i], 2, ys[i], 2, k, count, prod)
                            ev.relinearize_inplace(prod, 3, k, count, [key])
                            S._check(L.sealhip_evaluator_add(ctx.handle, k, out.ptr, 3, prod.ptr, 3, count, out.ptr))

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
                rec = {"config": name, "role": a.role, "count": count, "n_terms": n_terms, "k": k, "reps": reps, "ms_per_call": ms}
                ctx.profile_enable(True)
                call()
                prof = ctx.profile_fetch()
                ctx.profile_enable(False)
                rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
                print(json.dumps(rec), flush=True)
            out.free()
            if prod is not None:
                prod.free()
            del ops
            torch.cuda.empty_cache()
        del key, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--only", default="cfg3,cfg4")
    ap.add_argument("--counts", default="1,64")
    ap.add_argument("--terms", default="2,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        return worker(a)
    assert os.path.exists(a.baseline_lib), "the parent commit's libsealhip.so is needed for the baselines"
    base = [sys.executable, os.path.abspath(__file__), "--baseline-lib", a.baseline_lib, "--only", a.only, "--counts", a.counts,
            "--terms", a.terms, "--min-seconds", str(a.min_seconds)]
    got = {}
    for rnd in range(a.rounds):
        for role in ROLES:  # alternated: every round runs each side once, a process each
            out = subprocess.run(base + ["--role", role], capture_output=True, text=True, timeout=1500)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                return 1
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
                got.setdefault((rec["config"], rec["count"], rec["n_terms"], role), []).append(rec)
    for (cfg, count, n_terms, role), recs in sorted(got.items()):
        if role != "dot":
            continue
        d = [r["ms_per_call"] for r in recs]
        ca = [r["ms_per_call"] for r in got[(cfg, count, n_terms, "composed_a")]]
        cb = [r["ms_per_call"] for r in got[(cfg, count, n_terms, "composed_b")]]
        print(json.dumps({"summary": cfg, "count": count, "n_terms": n_terms,
                          "dot_ms_median": float(np.median(d)), "dot_ms_spread": max(d) - min(d),
                          "composed_a_ms_median": float(np.median(ca)), "composed_a_ms_spread": max(ca) - min(ca),
                          "composed_b_ms_median": float(np.median(cb)), "composed_b_ms_spread": max(cb) - min(cb),
                          "dot_over_composed_a": float(np.median(d) / np.median(ca)),
                          "dot_over_composed_b": float(np.median(d) / np.median(cb)),
                          "no_slower_than_composed_a": bool(np.median(d) <= np.median(ca))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
