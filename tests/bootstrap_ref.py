"""Restatements for DESIGN.md section 24 (towards CKKS bootstrapping): ModRaise over the oracle's transforms with Python
integers, and the EvalMod plan over tests/poly_eval_ckks_ref.py's plan. Nothing here calls the library under test."""
import math

import numpy as np

import oracle_lib as O
import poly_eval_ckks_ref as PC


def centre(x, q0):
    """x for x <= (q0 - 1) / 2, x - q0 above"""
    return x if x <= (q0 - 1) // 2 else x - q0


def mod_raise(ref, ct, k_out):
    """ct: (count, 2, k_in, N) uint64 in NTT form -> (count, 2, k_out, N): row 0 is the input's row 0; row i >= 1 is
    NTT_i(centre(INTT_0(row 0)) mod q_i), canonical. ref: oracle_lib.RefContext."""
    L = O.lib()
    count, n = ct.shape[0], ct.shape[3]
    q = [int(p) for p in ref.key_moduli]
    out = np.zeros((count, 2, k_out, n), dtype=np.uint64)
    for c in range(count):
        for j in range(2):
            out[c, j, 0] = ct[c, j, 0]
            coef = np.ascontiguousarray(ct[c, j, 0]).copy()
            L.ref_ntt_inverse(O.ptr(coef), ref.tables(0))
            centred = [centre(int(v), q[0]) for v in coef]
            for i in range(1, k_out):
                row = np.array([v % q[i] for v in centred], dtype=np.uint64)
                L.ref_ntt_forward(O.ptr(row), ref.tables(i), 0)
                out[c, j, i] = row
    return out


# ------------------------------------------------------------------ EvalMod: coefficients and plan
def evalmod_function(K, r, x):
    """cos((2 pi K x - pi / 2) / 2^r): r double-angle steps y -> 2 y^2 - 1 turn it into sin(2 pi K x)"""
    return math.cos((2.0 * math.pi * K * x - math.pi / 2.0) / 2.0 ** r)


def double_angle_scale(s, q_dropped):
    """the scale after one step at scale s whose rescale drops the prime q_dropped: s * s / dbl(q), in that order"""
    return s * s / float(q_dropped)


def evalmod_plan(q, k, s_x, coeffs, r, n_baby=0, scale_out=0.0):
    """q: the data primes of the first level; coeffs: the Chebyshev coefficients (only their zero pattern and degree matter
    here). L_0 is the polynomial plan's out level for (k, d, n_baby); step i = 1..r runs at level L_0 - i + 1. Backward:
    t_r = scale_out (0: s_x), t_(i-1) = sqrt(t_i dbl(q_(L_0 - i))); the polynomial is evaluated with scale_out = t_0; forward:
    s_0 = t_0, s_i = s_(i-1) s_(i-1) / dbl(q_(L_0 - i)). Returns a dict: poly_level L_0, out_level L_0 - r, t0,
    scales [s_0 .. s_r], n_products, poly (the polynomial's plan at scale_out = t_0)."""
    q = [int(p) for p in q]
    shape = PC.plan(q, k, float(s_x), coeffs, basis=1, n_baby=n_baby, scale_out=0.0)
    L0 = shape["out_level"]
    if L0 - r < 1:
        raise ValueError("end of modulus switching chain reached")
    t = float(scale_out) if scale_out else float(s_x)
    for i in range(r, 0, -1):
        t = math.sqrt(t * float(q[L0 - i]))
    scales = [t]
    for i in range(1, r + 1):
        scales.append(double_angle_scale(scales[-1], q[L0 - i]))
    poly = PC.plan(q, k, float(s_x), coeffs, basis=1, n_baby=n_baby, scale_out=t)
    return dict(poly_level=L0, out_level=L0 - r, t0=t, scales=scales, n_products=shape["n_products"] + r, poly=poly)
