#!/usr/bin/env python3
"""The key switch's mod-down merged with the CKKS rescale on one MI355X: one JSON line per measurement.
    python tools/ks_rescale_bench.py --baseline-lib PATH [--only cfg4,nsp3] [--ops relinearize,dot_product,dot_plain,bsgs]
                                     [--rounds 3] [--min-seconds 0.5]
merged:    ONE sealhip_evaluator_*_rescale call (this tree's library);
composed:  the same operation followed by sealhip_evaluator_rescale_to_next (its _strided form after relinearize), with the
           library of the PARENT commit (--baseline-lib is its libsealhip.so, built from a checkout of the parent next to
           this tree).
Each side runs in a process of its own per round (--rounds of them, the two sides alternated); a process warms every shape
up, then times it with device events around at least --min-seconds of back-to-back calls. The driver reports the median and
the spread (max - min) over the rounds and the ratio merged / composed; every record carries the library's launch profile of
one call. The bar: at 64 items no merged entry's median is slower than its composition's.
Shapes: config 4's ring (CKKS, N = 2^15, k = 11, one special prime) at 1 and 64 ciphertexts, and a ring with three special
primes (N = 2^14, k = 9, 50-bit primes) at 16. dot_product sums 4 terms; dot_plain forms 2 sums over 4 elements (one the
identity); bsgs walks 2 x 2 steps with the identity on each axis."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

NEW = ("sealhip_evaluator_relinearize_rescale", "sealhip_evaluator_dot_product_rescale",
       "sealhip_evaluator_apply_galois_dot_plain_rescale", "sealhip_evaluator_rotate_vector_dot_plain_rescale",
       "sealhip_evaluator_apply_galois_bsgs_plain_rescale", "sealhip_evaluator_rotate_vector_bsgs_plain_rescale")
ROLES = ("merged", "composed")
OPS = ("relinearize", "dot_product", "dot_plain", "bsgs")


def worker(a):
    import torch

    import oracle_lib as O
    import sealhip as S
    from bench import CFG4_PRIMES

    merged = a.role == "merged"
    if not merged:
        S.LIB_PATH = os.path.abspath(a.baseline_lib)
        for name in NEW:  # (the parent's library does not have them)
            S.SYMBOLS.pop(name, None)
    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    cfgs = {"cfg4": (15, list(CFG4_PRIMES), 1, (1, 64)),
            "nsp3": (14, [int(q) for q in O.coeff_modulus_create(1 << 14, [50] * 9 + [51] * 3)], 3, (16,))}
    rng = np.random.default_rng(19)
    stream = torch.cuda.Stream()
    dev = torch.device("cuda:0")
    for name in a.only.split(","):
        logn, mods, nsp, counts = cfgs[name]
        n, n_key = 1 << logn, len(mods)
        k = n_key - nsp
        nd = (k + nsp - 1) // nsp
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, nsp, 0)
        ctx.set_stream(stream.cuda_stream)
        ev = S.Evaluator(ctx)
        one = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in mods])
        key_words = np.broadcast_to(one, (nd, 2, n_key, n)).copy()  # (timing does not depend on the key words)
        relin = S.KSwitchKeys(ctx, key_words)
        elts = [3, 1, 5, 7]
        gkeys = {g: S.KSwitchKeys(ctx, key_words) for g in (3, 5, 7)}
        low = int(min(mods))
        item, item_out = k * n, (k - 1) * n
        plains = torch.randint(0, low, (2 * 4 * n_key * n,), dtype=torch.int64, device=dev)
        for count in counts:
            # canonical residues of every prime (below the smallest one); the values play no part in the timing
            ops = [torch.randint(0, low, (count * 3 * item,), dtype=torch.int64, device=dev) for _ in range(8)]
            out = ctx.alloc(2 * count * 2 * item_out)
            tmp = ctx.alloc(2 * count * 2 * item)

            def relinearize():
                if merged:
                    ev.relinearize_rescale(ops[0], k, count, [relin], out)
                else:
                    ev.relinearize_inplace(ops[0], 3, k, count, [relin])
                    ev.rescale_to_next(ops[0], 2, k, count, out, item_stride=3 * item)

            def dot_product():
                if merged:
                    ev.dot_product_rescale(ops[:4], ops[4:], k, count, out, [relin])
                else:
                    ev.dot_product(ops[:4], ops[4:], k, count, tmp, [relin])
                    ev.rescale_to_next(tmp, 2, k, count, out)

            def dot_plain():
                keys = [gkeys.get(g) for g in elts]
                if merged:
                    ev.apply_galois_dot_plain_rescale(ops[0], k, count, elts, keys, plains, 2, out)
                else:
                    ev.apply_galois_dot_plain(ops[0], k, count, elts, keys, plains, 2, tmp)
                    ev.rescale_to_next(tmp, 2, k, 2 * count, out)

            def bsgs():
                baby, giant = [1, 3], [5, 1]
                bk, gk = [gkeys.get(g) for g in baby], [gkeys.get(g) for g in giant]
                if merged:
                    ev.apply_galois_bsgs_plain_rescale(ops[0], k, count, baby, bk, giant, gk, plains, out)
                else:
                    ev.apply_galois_bsgs_plain(ops[0], k, count, baby, bk, giant, gk, plains, tmp)
                    ev.rescale_to_next(tmp, 2, k, count, out)

            for op in a.ops.split(","):
                call = {"relinearize": relinearize, "dot_product": dot_product, "dot_plain": dot_plain, "bsgs": bsgs}[op]
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
                rec = {"config": name, "role": a.role, "op": op, "count": count, "k": k, "nsp": nsp, "reps": reps,
                       "ms_per_call": ms}
                ctx.profile_enable(True)
                call()
                prof = ctx.profile_fetch()
                ctx.profile_enable(False)
                rec["kernels_ms"] = {tag: round(v["ms"], 4) for tag, v in prof.items()}
                print(json.dumps(rec), flush=True)
            out.free()
            tmp.free()
            del ops
            torch.cuda.empty_cache()
        del relin, gkeys, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--only", default="cfg4,nsp3")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--role", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role:
        return worker(a)
    assert os.path.exists(a.baseline_lib), "the parent commit's libsealhip.so is needed for the compositions"
    base = [sys.executable, os.path.abspath(__file__), "--baseline-lib", a.baseline_lib, "--only", a.only, "--ops", a.ops,
            "--min-seconds", str(a.min_seconds)]
    got = {}
    for rnd in range(a.rounds):
        for role in ROLES:  # alternated: every round runs each side once, a process each
            out = subprocess.run(base + ["--role", role], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                return 1
            for line in out.stdout.splitlines():
                rec = json.loads(line)
                rec["round"] = rnd
                print(json.dumps(rec), flush=True)
                got.setdefault((rec["config"], rec["count"], rec["op"], role), []).append(rec)
    for (cfg, count, op, role), recs in sorted(got.items()):
        if role != "merged":
            continue
        m = [r["ms_per_call"] for r in recs]
        c = [r["ms_per_call"] for r in got[(cfg, count, op, "composed")]]
        print(json.dumps({"summary": cfg, "op": op, "count": count,
                          "merged_ms_median": float(np.median(m)), "merged_ms_spread": max(m) - min(m),
                          "composed_ms_median": float(np.median(c)), "composed_ms_spread": max(c) - min(c),
                          "merged_over_composed": float(np.median(m) / np.median(c)),
                          "no_slower_than_composed": bool(np.median(m) <= np.median(c))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
