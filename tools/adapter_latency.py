"""Builds and runs tools/adapter_latency.cpp on N = 4096 / 8192 / 16384 with CoeffModulus::BFVDefault's primes (modulus.h)
and on BASELINE configs 3 (BFV) and 4 (CKKS), adds the one-thread CPU oracle column for the same operations on words of
the same shapes, and writes profiles/r05/adapter_latency.txt. Columns in ms, each the mean of 10 calls after warm-up:
host overload (pageable), resident overload (DeviceCiphertext), raw ABI (pool blocks), CPU oracle (one thread).
    python tools/adapter_latency.py [--out PATH] [--device 0]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402

T = 786433
DEFAULT_BITS = {12: [36, 36, 37], 13: [43, 43, 44, 44, 44], 14: [48, 48, 48, 49, 49, 49, 49, 49, 49]}


def shapes():
    dig = json.load(open(os.path.join(ROOT, "tests", "golden", "survey_digests.json")))
    rows = {r["cfg"]: r for r in dig["end_to_end"]}
    out = [("BFV N=%d BFVDefault" % (1 << lg), 1, lg, bits, T) for lg, bits in DEFAULT_BITS.items()]
    out.append(("cfg3 BFV N=32768 k=7", 1, 15, rows[3]["bits"], T))
    out.append(("cfg4 CKKS N=32768 k=11", 2, 15, rows[4]["bits"], 0))
    return out


def oracle_ms(scheme, logn, mods, ops):
    """one-thread CPU oracle, mean of 10 (3 for the slow key switches at N = 32768) after one warm-up"""
    L = O.lib()
    n, nk = 1 << logn, len(mods)
    k = nk - 1
    ref = O.RefContext(scheme, logn, mods, nsp=1, t=T if scheme == 1 else 0)
    rng = np.random.default_rng(logn)
    q = np.array(mods, dtype=np.uint64)

    def ct(size):
        return (rng.integers(0, 1 << 62, size=(size, k, n), dtype=np.uint64) % q[None, :k, None]).copy()

    x, y = ct(2), ct(2)
    x3 = np.zeros((3, k, n), dtype=np.uint64)
    mul = L.ref_bfv_multiply if scheme == 1 else L.ref_ckks_multiply
    mul(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(y), 2, O.ptr(x3))
    key = (rng.integers(0, 1 << 62, size=(k, 2, nk, n), dtype=np.uint64) % q[None, None, :, None]).copy()
    keys = (C.c_void_p * 1)(key.ctypes.data)
    plain = rng.integers(0, T, size=n, dtype=np.uint64)
    out3, out2 = np.zeros((3, k, n), dtype=np.uint64), np.zeros((2, k, n), dtype=np.uint64)
    sq = L.ref_bfv_square if scheme == 1 else L.ref_ckks_square
    e1, e0 = L.ref_galois_elt_from_step(n, 1, None), L.ref_galois_elt_from_step(n, 0, None)

    def relin():
        t = x3.copy()
        L.ref_relinearize(C.byref(ref.c), k, O.ptr(t), 3, keys)

    def mulrelin():
        t = np.zeros((3, k, n), dtype=np.uint64)
        mul(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(y), 2, O.ptr(t))
        L.ref_relinearize(C.byref(ref.c), k, O.ptr(t), 3, keys)

    out2k = np.zeros((2, k - 1, n), dtype=np.uint64)
    fns = {
        "add": lambda: L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(y), 2, O.ptr(out2)),
        "multiply": lambda: mul(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(y), 2, O.ptr(out3)),
        "multiply_plain": lambda: L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(out2), 2, O.ptr(plain)),
        "square": lambda: sq(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(out3)),
        "relinearize": relin,
        "rescale": lambda: L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(x), 2, O.ptr(out2k)),
        "rotate_rows": lambda: L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(out2), e1, O.ptr(key)),
        "rotate_vector": lambda: L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(out2), e1, O.ptr(key)),
        "rotate_columns": lambda: L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(out2), e0, O.ptr(key)),
        "complex_conjugate": lambda: L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(out2), e0, O.ptr(key)),
        "multiply+relinearize": mulrelin,
    }
    out2[:] = x
    res = {}
    for op in ops:
        fn = fns[op]
        fn()
        reps = 3 if logn >= 15 and op in ("relinearize", "multiply+relinearize", "rotate_rows", "rotate_vector",
                                          "rotate_columns", "complex_conjugate") else 10
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        res[op] = (time.perf_counter() - t0) * 1000 / reps
        print("  oracle", op, "%.2f ms" % res[op], flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "adapter_latency.txt"))
    ap.add_argument("--device", default="0")
    ap.add_argument("--exe", default=os.path.join(ROOT, "tools", "adapter_latency"))
    a = ap.parse_args()
    libdir = os.path.join(ROOT, "gemini-seal_amd", "lib")
    if not os.path.exists(a.exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", a.exe, os.path.join(ROOT, "tools", "adapter_latency.cpp"),
                               "-L" + libdir, "-lsealhip", "-Wl,-rpath," + libdir])
    lines = ["# adapter latency, ms per call, mean of 10 after warm-up (tools/adapter_latency.py)",
             "# host = Evaluator<HostCiphertext> on pageable words; resident = the DeviceCiphertext overload (ends with",
             "# Evaluator::synchronize); raw = the same sealhip_evaluator_* entries on pool blocks; oracle = CPU, one thread",
             "# the destination-taking rows (add, multiply, square, relinearize, rescale) copy the operand into the destination",
             "# first, as the reference's destination variants do; the in-place rows (multiply_plain, rotations) do not"]
    for name, scheme, logn, bits, t in shapes():
        mods = O.coeff_modulus_create(1 << logn, bits)
        print(name, flush=True)
        out = subprocess.run([a.exe, a.device, str(scheme), str(logn), "1", str(t)] + [str(m) for m in mods],
                             capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit(out.stdout + out.stderr)
        rows = [ln.split() for ln in out.stdout.strip().split("\n")]
        orc = oracle_ms(scheme, logn, mods, [r[0] for r in rows])
        lines.append("")
        lines.append("## %s (%d primes, k = %d)" % (name, len(mods), len(mods) - 1))
        lines.append("%-22s %10s %10s %10s %10s %14s" % ("op", "host", "resident", "raw_abi", "oracle_1t", "resident/raw"))
        for op, h, d, r in rows:
            lines.append("%-22s %10s %10s %10s %10.2f %14.3f" % (op, h, d, r, orc[op], float(d) / float(r)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
