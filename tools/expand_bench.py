#!/usr/bin/env python3
"""Oblivious expansion and the sums against plaintext rows on one MI355X: one JSON line per
measurement.
    python tools/expand_bench.py [--what expand,dot_plain] [--terms 4096] [--sums 4]
Ring: N = 2^13, two 50-bit primes and one 60-bit special prime, STRICT, random keys and operands (timing does not depend on
the words). Every figure is the median of three synchronised calls after a warm-up call, on the host clock.
  expand     sealhip_evaluator_expand with the normalisation at (n = 8192, count = 1) and (n = 64, count = 128), both
             schemes, against the same batched sequence of sealhip_evaluator_apply_galois calls (count * 2^t ciphertexts
             under N / 2^(t-1) + 1 for t = 1 .. l): the key switches and the automorphisms without the monomial products,
             the sums and the fan-out. The launch profile (sealhip_profile_fetch) of one further call is split into the step
             launches and everything else (the key switches).
  dot_plain  sealhip_evaluator_dot_plain, `terms` terms x `sums` sums, one item, CKKS, against the loop of multiply_plain
             (NTT form) into a temporary and add into the sum, per term and per sum. Bytes: every ciphertext and plaintext
             word read once and every sum written once -- what the call must move -- over the measured time, against 8 TB/s.
There is no bar: nothing like this existed to compare against."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "gemini-seal_amd")):
    sys.path.insert(0, p)
import numpy as np

HBM_BYTES_PER_S = 8e12


def median_ms(ctx, call):
    call()
    ctx.synchronize()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="expand,dot_plain")
    ap.add_argument("--terms", type=int, default=4096)
    ap.add_argument("--sums", type=int, default=4)
    a = ap.parse_args()
    import oracle_lib as O
    import sealhip as S

    assert S.num_devices() >= 1, "no HIP device: nothing to measure"
    logn, n, k = 13, 1 << 13, 2
    mods = O.coeff_modulus_create(n, [50, 50, 60])
    rng = np.random.default_rng(28)

    def words(lead):
        out = np.empty(tuple(lead) + (k, n), dtype=np.uint64)
        for r in range(k):
            out[..., r, :] = rng.integers(0, mods[r], size=tuple(lead) + (n,), dtype=np.uint64)
        return out

    for scheme, name in ((S.SCHEME_CKKS, "ckks"), (S.SCHEME_BFV, "bfv")):
        if "expand" not in a.what.split(","):
            break
        ctx = S.Context(scheme, logn, mods, 1, 65537 if scheme == S.SCHEME_BFV else 0, mode=S.MODE_STRICT)
        ev = S.Evaluator(ctx)
        key = np.stack([rng.integers(0, q, size=(k, 2, n), dtype=np.uint64) for q in mods], axis=2)  # [nd][2][n_key][N]
        keys = {g: S.KSwitchKeys(ctx, np.roll(key, i, axis=3)) for i, g in enumerate(ctx.expand_galois_elts(n))}
        for n_out, count in ((8192, 1), (64, 128)):
            l = n_out.bit_length() - 1
            ct = ctx.upload(words((count, 2)))
            out = ctx.alloc(count * n_out * 2 * k * n)

            def expand():
                ev.expand(ct, k, count, n_out, keys, out, normalize=True)

            def sequence():  # in place over the front of `out`: the batches the expansion's key switches see
                for t in range(1, l + 1):
                    g = (n >> (t - 1)) + 1
                    ev.apply_galois_inplace(out, k, count << t, g, keys[g])

            ms = median_ms(ctx, expand)
            ctx.profile_enable(True)
            expand()
            ctx.synchronize()
            prof = ctx.profile_fetch()
            ctx.profile_enable(False)
            step_ms = sum(v["ms"] for tag, v in prof.items() if tag == "expand_step")
            all_ms = sum(v["ms"] for v in prof.values())
            seq_ms = median_ms(ctx, sequence)
            # the step launches read each source once and write two results and two targets: 2 + 4 + 2 polynomials per source
            step_bytes = 8 * (n_out - 1) * count * k * n * 8
            print(json.dumps({"what": "expand", "scheme": name, "n": n_out, "count": count, "k": k, "logn": logn,
                              "expand_ms": round(ms, 3), "apply_galois_sequence_ms": round(seq_ms, 3),
                              "profile_step_ms": round(step_ms, 3), "profile_other_ms": round(all_ms - step_ms, 3),
                              "step_share": round(step_ms / all_ms, 4) if all_ms else None,
                              "step_bytes_derived": step_bytes,
                              "step_bytes_per_s": round(step_bytes / (step_ms * 1e-3)) if step_ms else None,
                              "step_roofline_share": round(step_bytes / (step_ms * 1e-3) / HBM_BYTES_PER_S, 4) if step_ms else None}),
                  flush=True)
            ct.free()
            out.free()

    if "dot_plain" in a.what.split(","):
        ctx = S.Context(S.SCHEME_CKKS, logn, mods, 1, 0, mode=S.MODE_STRICT)
        ev = S.Evaluator(ctx)
        n_terms, n_sums, size = a.terms, a.sums, 2
        item = size * k * n
        cts = ctx.alloc(n_terms * item)
        plain = ctx.alloc(n_sums * n_terms * k * n)
        block = 256  # uploads in blocks: the host never holds the whole table
        for i in range(0, n_terms, block):
            m = min(block, n_terms - i)
            ctx.memcpy_d2d(cts.ptr + i * item * 8, ctx.upload(words((m, size))), m * item)
        for i in range(0, n_sums * n_terms, block):
            m = min(block, n_sums * n_terms - i)
            ctx.memcpy_d2d(plain.ptr + i * k * n * 8, ctx.upload(words((m,))), m * k * n)
        ctx.synchronize()
        out = ctx.alloc(n_sums * item)
        ref = ctx.alloc(n_sums * item)
        tmp = ctx.alloc(item)

        def dot():
            ev.dot_plain(cts, plain, k, 1, n_terms, n_sums, out)

        def loop():
            for s in range(n_sums):
                acc = ref.ptr + s * item * 8
                for i in range(n_terms):
                    dst = acc if i == 0 else tmp.ptr
                    ctx.memcpy_d2d(dst, cts.ptr + i * item * 8, item)
                    ev.multiply_plain_inplace(dst, size, k, 1, plain.ptr + (s * n_terms + i) * k * n * 8, ntt_form=True)
                    if i:
                        ev.add(acc, size, tmp, size, k, 1, acc)

        ms = median_ms(ctx, dot)
        loop_ms = median_ms(ctx, loop)
        same = bool(np.array_equal(out.download(), ref.download()))
        moved = (n_terms * item + n_sums * n_terms * k * n + n_sums * item) * 8
        print(json.dumps({"what": "dot_plain", "terms": n_terms, "sums": n_sums, "size": size, "k": k, "logn": logn,
                          "dot_plain_ms": round(ms, 3), "multiply_plain_add_loop_ms": round(loop_ms, 3),
                          "same_words": same, "bytes_derived": moved, "bytes_per_s": round(moved / (ms * 1e-3)),
                          "roofline_share": round(moved / (ms * 1e-3) / HBM_BYTES_PER_S, 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
