"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs,
against the committed golden digests of the compiled reference, and -- at full BASELINE sizes --
through size-independent properties. Bar: bit-exact (all arithmetic is unsigned 64-bit integer)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import synth
from support import S as sealhip

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIG = json.load(open(os.path.join(HERE, "golden", "survey_digests.json")))
L = O.lib()


def h(a):
    return "%016x" % O.fnv(a)


def rand_rows(rng, moduli, n, full_range=False):
    rows = []
    for p in moduli:
        if full_range:
            rows.append(rng.integers(0, 2**64, size=n, dtype=np.uint64))
        else:
            rows.append(rng.integers(0, p, size=n, dtype=np.uint64))
    return np.stack(rows)


# ------------------------------------------------------------------ NTT
NTT_CASES = [(3, [20]), (4, [30, 30]), (5, [25]), (6, [30] * 4), (8, [40, 41]), (10, [50] * 3), (12, [36, 36, 37]),
             (13, [59, 58]), (14, [50] * 6), (15, [55] * 8), (16, [50] * 3),
             # mixed sizes around the lazy-sum bounds of the half-row and whole-row shapes (2^55, 2^56) and the FP64 bound
             (14, [58, 56, 55, 48]), (15, [56, 58, 55, 48]), (16, [56, 55, 49])]


@pytest.mark.parametrize("logn,bits", NTT_CASES, ids=lambda x: str(x))
def test_ntt_all_variants_vs_oracle(sealhip, logn, bits):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits) + O.get_primes(n, 57, 1)
    k = len(mods) - 1
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    tabs = [O.Tables(logn, p) for p in mods[:k]]
    rng = np.random.default_rng(1000 + logn)
    count = 3
    x = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
    variants = [
        ("fwd_lazy", ctx.ntt_negacyclic_harvey_lazy, lambda r, t: L.ref_ntt_forward_lazy(O.ptr(r), C.byref(t.t), 0)),
        ("fwd", ctx.ntt_negacyclic_harvey, lambda r, t: L.ref_ntt_forward(O.ptr(r), C.byref(t.t), 0)),
        ("inv_lazy", ctx.inverse_ntt_negacyclic_harvey_lazy, lambda r, t: L.ref_ntt_inverse_lazy(O.ptr(r), C.byref(t.t))),
        ("inv", ctx.inverse_ntt_negacyclic_harvey, lambda r, t: L.ref_ntt_inverse(O.ptr(r), C.byref(t.t))),
    ]
    for name, gpu_fn, ref_fn in variants:
        buf = ctx.upload(x)
        gpu_fn(buf, count, k)
        got = buf.download(x.shape)
        exp = x.copy()
        for c in range(count):
            for i in range(k):
                ref_fn(exp[c, i], tabs[i])
        assert np.array_equal(got, exp), name
    # round trip on the device
    buf = ctx.upload(x)
    ctx.ntt_negacyclic_harvey(buf, count, k)
    ctx.inverse_ntt_negacyclic_harvey(buf, count, k)
    assert np.array_equal(buf.download(x.shape), x)


@pytest.mark.parametrize("logn", [14, 15, 16])
def test_ntt_fp64_instances_extreme_inputs(sealhip, logn):
    """Primes below 2^50 take the floating-point single-pass kernels whenever the output's representative is free
    (canonical transforms, kNttAnyRep consumers). Their exactness argument is a bound (magnitudes below 2^53); drive it
    with the largest admissible primes and the inputs that maximise growth -- all p-1, alternating 0 / p-1, one spike,
    random -- for the forward transform, and values in [0, 2p) (what the lazy inverse accepts) for the inverse. Bit-exact
    against the oracle's integer transforms (ntt.cpp:210-281)."""
    n = 1 << logn
    # a 58-bit prime among the live rows: such launches are split (floating-point rows, then integer rows)
    mods = O.get_primes(n, 50, 3) + O.get_primes(n, 58, 1) + O.get_primes(n, 49, 1) + O.get_primes(n, 30, 1) + O.get_primes(n, 57, 1)
    k = len(mods) - 1
    assert max(mods[:3]) < (1 << 50) and max(mods[:3]) > (1 << 50) - (1 << 40)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    tabs = [O.Tables(logn, p) for p in mods[:k]]
    rng = np.random.default_rng(50 + logn)
    pats = []
    for kind in range(5):
        x = np.zeros((k, n), dtype=np.uint64)
        for i, p in enumerate(mods[:k]):
            if kind == 0:
                x[i, :] = p - 1
            elif kind == 1:
                x[i, ::2] = p - 1
            elif kind == 2:
                x[i, n // 2:] = p - 1
            elif kind == 3:
                x[i, rng.integers(0, n)] = p - 1
            else:
                x[i] = rng.integers(0, p, n, dtype=np.uint64)
        pats.append(x)
    x = np.stack(pats)
    buf = ctx.upload(x)
    ctx.ntt_negacyclic_harvey(buf, len(pats), k)
    got = buf.download(x.shape)
    exp = x.copy()
    for c in range(len(pats)):
        for i in range(k):
            L.ref_ntt_forward(O.ptr(exp[c, i]), C.byref(tabs[i].t), 0)
    assert np.array_equal(got, exp), "forward"
    # inverse: canonical inputs, and the lazy range [0, 2p) (same residues, the canonical output must not change)
    for lazy_in in (False, True):
        y = x.copy()
        if lazy_in:
            for i, p in enumerate(mods[:k]):
                y[:, i, 1::3] += np.uint64(p)
        buf = ctx.upload(y)
        ctx.inverse_ntt_negacyclic_harvey(buf, len(pats), k)
        got = buf.download(x.shape)
        exp = x.copy()
        for c in range(len(pats)):
            for i in range(k):
                L.ref_ntt_inverse(O.ptr(exp[c, i]), C.byref(tabs[i].t))
        assert np.array_equal(got, exp), "inverse lazy_in=%s" % lazy_in


@pytest.mark.parametrize("row", DIG["ntt_digests"], ids=lambda r: "logn%d_k%d" % (r["logn"], len(r["bits"])))
def test_ntt_golden_digests(sealhip, row):
    """The survey's digests of util::ntt_negacyclic_harvey & co. from the compiled reference."""
    logn, k = row["logn"], len(row["bits"])
    n = 1 << logn
    mods = O.coeff_modulus_create(n, row["bits"])
    x = O.SplitMix(0x5EA1 + 1000 * logn + k).fill(k, n, mods)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods + O.get_primes(n, 40, 1), 1, 0)
    f = ctx.upload(x)
    ctx.ntt_negacyclic_harvey(f, 1, k)
    fwd = f.download(x.shape)
    assert h(fwd) == row["fwd"]
    lz = ctx.upload(x)
    ctx.ntt_negacyclic_harvey_lazy(lz, 1, k)
    assert h(lz.download()) == row["fwd_lazy"]
    dy = ctx.alloc(x.size)
    ctx.dyadic_product_coeffmod(f, f, 1, k, dy)
    assert h(dy.download()) == row["dyadic_sq"]
    iv = ctx.upload(x)
    ctx.inverse_ntt_negacyclic_harvey(iv, 1, k)
    assert h(iv.download()) == row["inv"]


@pytest.mark.parametrize("logn", [6, 12, 13, 15])
def test_ntt_bsk_base_60bit_wraparound(sealhip, logn):
    """on the 60-bit Bsk primes the reference's uncorrected lazy butterflies wrap mod 2^64;
    PARITY must reproduce the wrapped words, for canonical and for arbitrary 64-bit inputs."""
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [40, 40, 41])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, 65537)
    k = 2
    nb = ctx.bsk_size(k)
    ref = O.RefContext(1, logn, mods, 1, 65537)
    rt = ref.rns_tool(k)
    bsk = [int(rt.contents.Bsk[i].value) for i in range(nb)]
    rng = np.random.default_rng(7 + logn)
    wrapped = False
    for full in (False, True):
        x = rand_rows(rng, bsk, n, full_range=full)
        if not full:
            x[0, :] = np.uint64(bsk[0] - 1)  # worst case growth
        buf = ctx.upload(x)
        ctx.ntt_negacyclic_harvey_lazy(buf, 1, k, sealhip.BASE_BSK)
        got = buf.download(x.shape)
        exp, strict = x.copy(), x.copy()
        for i in range(nb):
            L.ref_ntt_forward_lazy(O.ptr(exp[i]), C.byref(rt.contents.Bsk_ntt[i]), 0)
            L.ref_ntt_forward(O.ptr(strict[i]), C.byref(rt.contents.Bsk_ntt[i]), 1)
        assert np.array_equal(got, exp)
        canon = exp.copy()
        for i in range(nb):
            p = np.uint64(bsk[i])
            canon[i] = canon[i] % p
        if not np.array_equal(canon, strict):
            wrapped = True
    if logn >= 12:
        assert wrapped, "expected the 60-bit overflow regime to be exercised"


def test_strict_mode_forward_matches_math(sealhip):
    logn = 12
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [40, 40, 41])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, 65537, mode=sealhip.MODE_STRICT)
    k = 2
    nb = ctx.bsk_size(k)
    ref = O.RefContext(1, logn, mods, 1, 65537, mode=1)
    rt = ref.rns_tool(k)
    bsk = [int(rt.contents.Bsk[i].value) for i in range(nb)]
    x = rand_rows(np.random.default_rng(3), bsk, n)
    buf = ctx.upload(x)
    ctx.ntt_negacyclic_harvey_lazy(buf, 1, k, sealhip.BASE_BSK)
    exp = x.copy()
    for i in range(nb):
        L.ref_ntt_forward_lazy(O.ptr(exp[i]), C.byref(rt.contents.Bsk_ntt[i]), 1)
    assert np.array_equal(buf.download(x.shape), exp)


# ------------------------------------------------------------------ coefficient-wise
def test_poly_ops_vs_oracle(sealhip):
    logn, n = 10, 1 << 10
    mods = O.coeff_modulus_create(n, [59, 30, 45, 20])
    k = 3
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    rng = np.random.default_rng(11)
    count = 2
    a = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
    b = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
    lazy_a = np.stack([rand_rows(rng, mods[:k], n, full_range=True) for _ in range(count)])
    da, db, dl, out = ctx.upload(a), ctx.upload(b), ctx.upload(lazy_a), ctx.alloc(a.size)
    ms = [O.modulus(p) for p in mods[:k]]

    def ref2(fn, x, y):
        r = np.empty_like(x)
        for c in range(count):
            for i in range(k):
                fn(O.ptr(x[c, i]), O.ptr(y[c, i]), n, C.byref(ms[i]), O.ptr(r[c, i]))
        return r

    ctx.dyadic_product_coeffmod(dl, db, count, k, out)  # lazy (any 64-bit) first operand, like the NTT outputs
    assert np.array_equal(out.download(a.shape), ref2(L.ref_dyadic_product_coeffmod, lazy_a, b))
    ctx.add_poly_coeffmod(da, db, count, k, out)
    assert np.array_equal(out.download(a.shape), ref2(L.ref_add_poly_coeffmod, a, b))
    ctx.sub_poly_coeffmod(da, db, count, k, out)
    assert np.array_equal(out.download(a.shape), ref2(L.ref_sub_poly_coeffmod, a, b))
    ctx.negate_poly_coeffmod(da, count, k, out)
    r = np.empty_like(a)
    for c in range(count):
        for i in range(k):
            L.ref_negate_poly_coeffmod(O.ptr(a[c, i]), n, C.byref(ms[i]), O.ptr(r[c, i]))
    assert np.array_equal(out.download(a.shape), r)
    scalar = 0x123456789ABCDEF
    ctx.multiply_poly_scalar_coeffmod(dl, count, k, scalar, out)
    for c in range(count):
        for i in range(k):
            L.ref_multiply_poly_scalar_coeffmod(O.ptr(lazy_a[c, i]), n, scalar, C.byref(ms[i]), O.ptr(r[c, i]))
    assert np.array_equal(out.download(a.shape), r)
    # in place (result aliases an operand), as Evaluator uses them
    ctx.add_poly_coeffmod(da, db, count, k, da)
    assert np.array_equal(da.download(a.shape), ref2(L.ref_add_poly_coeffmod, a, b))


def test_galois_vs_oracle_and_kat(sealhip):
    kat = json.load(open(os.path.join(HERE, "golden", "reference_kats.json")))["galois"]
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, 3, [17, 97], 1, 0)
    x = np.array(kat["in"], dtype=np.uint64)
    d, o = ctx.upload(x), ctx.alloc(8)
    ctx.apply_galois(d, 1, 1, kat["elt"], o)
    assert [int(v) for v in o.download()] == kat["apply_galois"]
    ctx.apply_galois_ntt(d, 1, 1, kat["elt"], o)
    assert [int(v) for v in o.download()] == kat["apply_galois_ntt"]
    with pytest.raises(ValueError):
        ctx.apply_galois(d, 1, 1, 4, o)
    with pytest.raises(ValueError):
        ctx.apply_galois(d, 1, 1, 3, d)
    for row in DIG["galois_elts"]:
        n = 1 << row["logn"]
        c2 = sealhip.Context(sealhip.SCHEME_CKKS, row["logn"], O.coeff_modulus_create(n, [30, 30]), 1, 0)
        assert c2.galois_elt_from_step(1) == row["step1"]
        assert c2.galois_elt_from_step(0) == row["step0"]
        assert c2.galois_elt_from_step(-1) == row["stepm1"]
    logn, n = 11, 1 << 11
    mods = O.coeff_modulus_create(n, [50, 50, 50])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, 65537)
    x = np.stack([rand_rows(np.random.default_rng(5), mods[:2], n) for _ in range(2)])
    d, o = ctx.upload(x), ctx.alloc(x.size)
    for elt in (5, 3, 2 * n - 1, ctx.galois_elt_from_step(-3)):
        e1, e2 = np.empty_like(x), np.empty_like(x)
        for c in range(2):
            for i in range(2):
                m = O.modulus(mods[i])
                L.ref_apply_galois(O.ptr(x[c, i]), logn, elt, C.byref(m), O.ptr(e1[c, i]))
                L.ref_apply_galois_ntt(O.ptr(x[c, i]), logn, elt, O.ptr(e2[c, i]))
        ctx.apply_galois(d, 2, 2, elt, o)
        assert np.array_equal(o.download(x.shape), e1)
        ctx.apply_galois_ntt(d, 2, 2, elt, o)
        assert np.array_equal(o.download(x.shape), e2)


# ------------------------------------------------------------------ RNSTool + key-switch pieces: survey digests
UD = DIG["unit_digests"]


@pytest.mark.parametrize("ci", range(len(UD["columns"])), ids=[c["name"] for c in UD["columns"]])
def test_unit_functions_golden_digests(sealhip, ci):
    """Every hot-path L2 function on the survey's inputs, against the compiled reference's digests."""
    col = UD["columns"][ci]
    logn, nsp = col["logn"], col["nsp"]
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, col["bits"])
    nk = len(kmods)
    k = nk - nsp
    bfv = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, nsp, col["t"])
    ckks = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, nsp, 0)
    nb = bfv.bsk_size(k)
    bsk = [int(v) for v in bfv.debug_rns_constants(k, 0)]
    q = kmods[:k]
    sm = O.SplitMix(0)
    res = {}
    sm.set(0xF00D0001)
    out = bfv.alloc((nb + 1) * n)
    bfv.fastbconv_m_tilde(k, bfv.upload(sm.fill(k, n, q)), 1, out)
    res["fastbconv_m_tilde"] = h(out.download())
    sm.set(0xF00D0002)
    out = bfv.alloc(nb * n)
    bfv.sm_mrq(k, bfv.upload(sm.fill(nb + 1, n, bsk + [1 << 32])), 1, out)
    res["sm_mrq"] = h(out.download())
    sm.set(0xF00D0003)
    bfv.fast_floor(k, bfv.upload(sm.fill(k + nb, n, q + bsk)), 1, out)
    res["fast_floor"] = h(out.download())
    sm.set(0xF00D0004)
    out = bfv.alloc(k * n)
    bfv.fastbconv_sk(k, bfv.upload(sm.fill(nb, n, bsk)), 1, out)
    res["fastbconv_sk"] = h(out.download())
    sm.set(0xF00D0005)
    d = bfv.upload(sm.fill(k, n, q))
    bfv.divide_and_round_q_last_inplace(k, d, 1)
    res["divide_and_round_q_last_inplace"] = h(d.download((k, n))[: k - 1])
    sm.set(0xF00D0006)
    d = bfv.upload(sm.fill(k, n, q))
    bfv.divide_and_round_q_last_ntt_inplace(k, d, 1)
    res["divide_and_round_q_last_ntt_inplace"] = h(d.download((k, n))[: k - 1])
    sm.set(0xF00D0007)
    d, o = bfv.upload(sm.fill(1, n, q[:1])), bfv.alloc(n)
    bfv.apply_galois(d, 1, 1, 5, o)
    res["apply_galois"] = h(o.download())
    bfv.apply_galois_ntt(d, 1, 1, 5, o)
    res["apply_galois_ntt"] = h(o.download())
    for key, b in (("modup_rns_first", 0), ("modup_rns_last", col["modup_last_bundle"])):
        ext = np.zeros((k + nsp, n), dtype=np.uint64)
        sm.set(0xF00D0008 + b)
        r0 = b * nsp
        r1 = min(r0 + nsp, k)
        ext[r0:r1] = sm.fill(r1 - r0, n, kmods[r0:r1])
        d = bfv.upload(ext)
        bfv.modup_rns(k, b, d, 1)
        res[key] = h(d.download())
    for key, c in (("rescale_special_ckks", ckks), ("rescale_special_bfv", bfv)):
        sm.set(0xF00D0010 + (1 if c is ckks else 0))
        d = c.upload(sm.fill(k + nsp, n, kmods[:k] + kmods[nk - nsp:]))
        c.rescale_special_rns_inplace(k, d, 1)
        res[key] = h(d.download((k + nsp, n))[:k])
    for key, val in res.items():
        assert val == UD[key][ci], key


def test_rns_tool_batched_vs_oracle(sealhip):
    """Batched, ragged level (k < k_first) and a non-trivial |B| = k+1 case against the oracle."""
    logn, n = 9, 1 << 9
    kmods = O.coeff_modulus_create(n, [59, 59, 59, 59, 40])
    t = (1 << 58) + 1  # large plain modulus -> base_B_size bump (rns.cpp:568-573)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ref = O.RefContext(1, logn, kmods, 1, t)
    rng = np.random.default_rng(21)
    count = 3
    for k in (4, 3, 2):
        rt = ref.rns_tool(k)
        nb = rt.contents.Bsk_size
        assert ctx.bsk_size(k) == nb
        if k == 4:
            assert rt.contents.B_size == k + 1
        bsk = [int(rt.contents.Bsk[i].value) for i in range(nb)]
        q = kmods[:k]
        x = np.stack([rand_rows(rng, q, n) for _ in range(count)])
        o = ctx.alloc(count * (nb + 1) * n)
        ctx.fastbconv_m_tilde(k, ctx.upload(x), count, o)
        exp = np.zeros((count, nb + 1, n), dtype=np.uint64)
        for c in range(count):
            L.ref_fastbconv_m_tilde(rt, O.ptr(x[c]), O.ptr(exp[c]))
        assert np.array_equal(o.download(exp.shape), exp)
        o2 = ctx.alloc(count * nb * n)
        ctx.sm_mrq(k, o, count, o2)
        exp2 = np.zeros((count, nb, n), dtype=np.uint64)
        for c in range(count):
            L.ref_sm_mrq(rt, O.ptr(exp[c]), O.ptr(exp2[c]))
        assert np.array_equal(o2.download(exp2.shape), exp2)
        y = np.stack([rand_rows(rng, q + bsk, n) for _ in range(count)])
        ctx.fast_floor(k, ctx.upload(y), count, o2)
        exp3 = np.zeros((count, nb, n), dtype=np.uint64)
        for c in range(count):
            L.ref_fast_floor(rt, O.ptr(y[c]), O.ptr(exp3[c]))
        assert np.array_equal(o2.download(exp3.shape), exp3)
        o4 = ctx.alloc(count * k * n)
        ctx.fastbconv_sk(k, o2, count, o4)
        exp4 = np.zeros((count, k, n), dtype=np.uint64)
        for c in range(count):
            L.ref_fastbconv_sk(rt, O.ptr(exp3[c]), O.ptr(exp4[c]))
        assert np.array_equal(o4.download(exp4.shape), exp4)


# ------------------------------------------------------------------ end to end: the reference's op chain
@pytest.mark.parametrize("row", DIG["end_to_end"], ids=lambda r: "cfg%d" % r["cfg"])
def test_end_to_end_golden_digests(sealhip, row):
    """multiply -> relinearize -> mod_switch/rescale (+ rotate_vector for CKKS) through the C ABI on the
    survey's synthetic inputs must reproduce the digests of the compiled reference,
    including the F2/F3 behaviour of the BFV configs."""
    inp = synth.end_to_end_inputs(row)
    n, k, logn = inp["n"], inp["k"], inp["logn"]
    scheme = row["scheme"]
    ctx = sealhip.Context(scheme, logn, inp["kmods"], row["nsp"], row["t"])
    ev = sealhip.Evaluator(ctx)
    got = {}
    rk = sealhip.KSwitchKeys(ctx, inp["rk"])
    if scheme == 2:
        gk = sealhip.KSwitchKeys(ctx, inp["gk"])
        c = ctx.upload(inp["a"])
        ev.rotate_vector_inplace(c, k, 1, 1, {ctx.galois_elt_from_step(1): gk})
        got["rotate"] = h(c.download())
    a, b = ctx.upload(inp["a"]), ctx.upload(inp["b"])
    c = ctx.alloc(3 * k * n)
    ev.multiply(a, 2, b, 2, k, 1, c)
    got["mul"] = h(c.download())
    ev.relinearize_inplace(c, 3, k, 1, [rk])
    c2 = c.download((3, k, n))[:2].copy()
    got["relin"] = h(c2)
    o = ctx.alloc(2 * (k - 1) * n)
    d2 = ctx.upload(c2)
    if scheme == 1:
        ev.mod_switch_to_next(d2, 2, k, 1, o)
        got["modswitch"] = h(o.download())
    else:
        ev.rescale_to_next(d2, 2, k, 1, o)
        got["rescale"] = h(o.download())
    assert got == row["digests"]


@pytest.mark.parametrize("scheme,logn,bits,nsp,t", [
    (1, 10, [40, 40, 40, 40, 41], 2, 65537),      # BFV, two special primes, ragged last bundle (k=3, nsp=2)
    (2, 10, [45, 45, 45, 45, 45, 46], 3, 0),       # CKKS, three special primes
    (2, 11, [40, 40, 40, 41], 1, 0),
])
def test_batched_chain_vs_oracle_all_levels(sealhip, scheme, logn, bits, nsp, t):
    """A batch of independent ciphertexts through multiply/relinearize/mod-switch/apply_galois at the first
    level and one level below, item by item against the oracle."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    nk = len(kmods)
    ctx = sealhip.Context(scheme, logn, kmods, nsp, t)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(scheme, logn, kmods, nsp=nsp, t=t)
    rng = np.random.default_rng(99)
    k_first = nk - nsp
    d_full = (k_first + nsp - 1) // nsp
    key = np.stack([rand_rows(rng, kmods * 2, n).reshape(2, nk, n) for _ in range(d_full)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    count = 3
    for k in (k_first, k_first - 1):
        if k < 2:
            continue
        a = np.stack([rand_rows(rng, kmods[:k] * 2, n).reshape(2, k, n) for _ in range(count)])
        b = np.stack([rand_rows(rng, kmods[:k] * 2, n).reshape(2, k, n) for _ in range(count)])
        out = ctx.alloc(count * 3 * k * n)
        ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
        exp = np.zeros((count, 3, k, n), dtype=np.uint64)
        mul = L.ref_bfv_multiply if scheme == 1 else L.ref_ckks_multiply
        for c in range(count):
            assert mul(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(b[c]), 2, O.ptr(exp[c])) == 0
        assert np.array_equal(out.download(exp.shape), exp), "multiply k=%d" % k
        sq = ctx.alloc(count * 3 * k * n)
        ev.square(ctx.upload(a), 2, k, count, sq)
        exps = np.zeros((count, 3, k, n), dtype=np.uint64)
        exps2 = np.zeros((count, 3, k, n), dtype=np.uint64)
        sqr = L.ref_bfv_square if scheme == 1 else L.ref_ckks_square
        for c in range(count):
            assert sqr(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(exps[c])) == 0  # evaluator.cpp:560-770 restated
            assert mul(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(a[c]), 2, O.ptr(exps2[c])) == 0  # cross-check
        assert np.array_equal(exps, exps2), "oracle: square vs multiply(a, a) k=%d" % k
        assert np.array_equal(sq.download(exps.shape), exps), "square k=%d" % k
        ev.relinearize_inplace(out, 3, k, count, [dkey])
        keys = (C.c_void_p * 1)(key.ctypes.data)
        for c in range(count):
            assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp[c]), 3, keys) == 0
        got = out.download(exp.shape)
        assert np.array_equal(got[:, :2], exp[:, :2]), "relinearize k=%d" % k
        c2 = np.ascontiguousarray(exp[:, :2])
        o = ctx.alloc(count * 2 * (k - 1) * n)
        exp_ms = np.zeros((count, 2, k - 1, n), dtype=np.uint64)
        if scheme == 1:
            ev.mod_switch_to_next(ctx.upload(c2), 2, k, count, o)
        else:
            ev.rescale_to_next(ctx.upload(c2), 2, k, count, o)
        for c in range(count):
            assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(c2[c]), 2, O.ptr(exp_ms[c])) == 0
        assert np.array_equal(o.download(exp_ms.shape), exp_ms), "mod switch k=%d" % k
        if scheme == 2:
            ev.mod_switch_to_next(ctx.upload(c2), 2, k, count, o)
            assert np.array_equal(o.download(exp_ms.shape), c2[:, :, : k - 1]), "mod_switch_drop k=%d" % k
        elt = ctx.galois_elt_from_step(-2)
        g = ctx.upload(c2)
        ev.apply_galois_inplace(g, k, count, elt, dkey)
        expg = c2.copy()
        for c in range(count):
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(expg[c]), elt, O.ptr(key)) == 0
        assert np.array_equal(g.download(expg.shape), expg), "apply_galois k=%d" % k


def test_strict_mode_chain_vs_oracle(sealhip):
    """STRICT = Harvey-corrected butterflies + NTT'd in-bundle rows, against the oracle's STRICT."""
    logn, n = 12, 1 << 12
    kmods = O.coeff_modulus_create(n, [36, 36, 37])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, 786433, mode=sealhip.MODE_STRICT)
    par = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, 786433)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=786433, mode=1)
    rng = np.random.default_rng(5)
    k = 2
    key = np.stack([rand_rows(rng, kmods * 2, n).reshape(2, 3, n) for _ in range(2)])
    a = rand_rows(rng, kmods[:k] * 2, n).reshape(1, 2, k, n)
    b = rand_rows(rng, kmods[:k] * 2, n).reshape(1, 2, k, n)
    exp = np.zeros((1, 3, k, n), dtype=np.uint64)
    assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a), 2, O.ptr(b), 2, O.ptr(exp)) == 0
    out, outp = ctx.alloc(exp.size), par.alloc(exp.size)
    sealhip.Evaluator(ctx).multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, 1, out)
    sealhip.Evaluator(par).multiply(par.upload(a), 2, par.upload(b), 2, k, 1, outp)
    assert np.array_equal(out.download(exp.shape), exp)
    assert not np.array_equal(outp.download(exp.shape), exp), "PARITY and STRICT must differ in the F2 regime"
    keys = (C.c_void_p * 1)(key.ctypes.data)
    assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp), 3, keys) == 0
    sealhip.Evaluator(ctx).relinearize_inplace(out, 3, k, 1, [sealhip.KSwitchKeys(ctx, key)])
    assert np.array_equal(out.download(exp.shape)[:, :2], exp[:, :2])


@pytest.mark.parametrize("logn,bits,count", [(14, [45, 45, 46], 5), (15, [55] * 4, 3), (16, [50] * 3, 2), (15, [58, 58, 59], 2)])
def test_strict_mode_at_the_single_pass_ring_sizes(sealhip, logn, bits, count):
    """STRICT at N = 2^14 .. 2^16 (round 4): the 60-bit Bsk rows run the dense lazy forward schedule (ntt_bounds.hpp section 2b) --
    below the top layer, which the lift applies -- and the in-bundle rows of the key switch are gathered and transformed with the
    approximate quotient. Word for word against the oracle's STRICT restatement, operands at their extremes planted (p - 1, 0, 1
    in whole rows and scattered), multiply and relinearize separately and fused through square."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    k = len(kmods) - 1
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, 786433, mode=sealhip.MODE_STRICT)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=786433, mode=1)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(logn * 100 + bits[0])
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    for r in range(k):
        a[0, 0, r, :] = kmods[r] - 1          # a whole row at the top of the range
        b[0, 1, r, ::3] = kmods[r] - 1
        b[0, 0, r, 1::3] = 0
        a[-1, 1, r, : n // 2] = 1
    exp = np.zeros((count, 3, k, n), dtype=np.uint64)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    for c in range(count):
        assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(b[c]), 2, O.ptr(exp[c])) == 0
    out = ctx.alloc(exp.size)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
    assert np.array_equal(out.download(exp.shape), exp), "multiply"
    for c in range(count):
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp[c]), 3, keys) == 0
    ev.relinearize_inplace(out, 3, k, count, [dkey])
    assert np.array_equal(out.download(exp.shape)[:, :2], exp[:, :2]), "relinearize"
    sq = np.zeros((count, 3, k, n), dtype=np.uint64)
    for c in range(count):
        assert L.ref_bfv_square(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(sq[c])) == 0
    ev.square(ctx.upload(a), 2, k, count, out)
    assert np.array_equal(out.download(sq.shape), sq), "square"


# ------------------------------------------------------------------ full BASELINE sizes: properties
@pytest.mark.parametrize("logn,bits,count", [(14, [50] * 6, 64), (15, [55] * 8, 32), (16, [50] * 4, 8)])
def test_full_size_ntt_properties(sealhip, logn, bits, count):
    n = 1 << logn
    mods = O.coeff_modulus_create(n, bits)
    k = len(mods) - 1
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    rng = np.random.default_rng(logn)
    x = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
    y = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
    dx, dy, ds = ctx.upload(x), ctx.upload(y), ctx.alloc(x.size)
    ctx.add_poly_coeffmod(dx, dy, count, k, ds)
    for d in (dx, dy, ds):
        ctx.ntt_negacyclic_harvey(d, count, k)
    # linearity: NTT(x + y) == NTT(x) + NTT(y)
    chk = ctx.alloc(x.size)
    ctx.add_poly_coeffmod(dx, dy, count, k, chk)
    assert np.array_equal(chk.download(), ds.download())
    fx = dx.download(x.shape)
    for i in range(k):
        assert fx[:, i].max() < mods[i]
    # spot-check one item against the oracle
    tabs = [O.Tables(logn, p) for p in mods[:k]]
    c = count - 1
    exp = x[c].copy()
    for i in range(k):
        L.ref_ntt_forward(O.ptr(exp[i]), C.byref(tabs[i].t), 0)
    assert np.array_equal(fx[c], exp)
    # round trip
    ctx.inverse_ntt_negacyclic_harvey(dx, count, k)
    assert np.array_equal(dx.download(x.shape), x)


def test_edge_cases_and_errors(sealhip):
    logn, n = 8, 1 << 8
    mods = O.coeff_modulus_create(n, [40, 40, 41])
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    buf = ctx.upload(np.zeros((2, 2, n), dtype=np.uint64))
    ctx.ntt_negacyclic_harvey(buf, 0, 2)  # empty batch is a no-op
    ctx.ntt_negacyclic_harvey(buf, 2, 2)  # all-zero input
    assert not buf.download().any()
    with pytest.raises(ValueError):
        ctx.ntt_negacyclic_harvey(buf, 1, 9)  # level out of range
    with pytest.raises(ValueError):
        ctx.ntt_negacyclic_harvey(buf, 1, 2, sealhip.BASE_BSK)  # no Bsk base in CKKS
    with pytest.raises(sealhip.LogicError):
        ctx.fastbconv_m_tilde(2, buf, 1, buf)  # BFV-only function
    with pytest.raises(ValueError):
        ev.rescale_to_next(buf, 2, 1, 1, buf)  # end of chain
    with pytest.raises(TypeError):
        ctx.ntt_negacyclic_harvey(0, 1, 2)  # null pointer -> E_POINTER
    bfv = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, 257)
    with pytest.raises(ValueError):
        sealhip.Evaluator(bfv).rescale_to_next(buf, 2, 2, 1, buf)  # unsupported for BFV
    with pytest.raises(ValueError):
        sealhip.Context(sealhip.SCHEME_CKKS, logn, [17, 19], 1, 0)  # not NTT-friendly primes
    with pytest.raises(ValueError):
        sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 3, 0)  # #moduli <= n_special_primes


def test_cpp_host_adapter_chain_matches_golden(sealhip, tmp_path):
    """multiply -> relinearize -> mod_switch_to_next through the C++ adapter (host buffers in, host buffers out)
    on the survey's cfg1 inputs reproduces the compiled reference's digest."""
    import subprocess

    import test_host

    exe = test_host._build_adapter(tmp_path)
    out = subprocess.run([exe, "0"], capture_output=True, text=True, timeout=300, env=dict(os.environ, SEALHIP_HOST_CHUNK="4"))
    assert out.returncode == 0, out.stdout + out.stderr
    want = [r for r in DIG["end_to_end"] if r["cfg"] == 1][0]["digests"]["modswitch"]
    assert "modswitch digest " + want in out.stdout, out.stdout
    assert "f1 identities ok" in out.stdout, out.stdout
    # the batch overloads: 11 separately allocated ciphertexts through the pointer-array entry in chunks of 4
    assert "host batch ok" in out.stdout, out.stdout
    assert "multiply_many ok" in out.stdout, out.stdout
    # round 4: rotate_rows / rotate_columns (BFV), complex_conjugate / rotate_vector (CKKS), the destination-taking
    # variants, add_many, mod_switch_to / rescale_to -- the automorphisms against the oracle's apply_galois on the same words
    # (evaluator.h:1057-1308; evaluator.cpp:1841-1943), the rest against the in-place forms inside the check
    assert "f1 names ok" in out.stdout and "ckks names ok" in out.stdout, out.stdout
    row = [r for r in DIG["end_to_end"] if r["cfg"] == 1][0]
    inp = synth.end_to_end_inputs(row)
    n, k = inp["n"], inp["k"]
    for scheme, names in ((1, ("rotate_rows", "rotate_columns")), (2, ("rotate_vector", "complex_conjugate"))):
        ref = O.RefContext(scheme, inp["logn"], inp["kmods"], nsp=1, t=row["t"] if scheme == 1 else 0)
        for name, step in zip(names, (1, 0)):
            c = inp["b"].copy()
            elt = L.ref_galois_elt_from_step(n, step, None)
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(c), elt, O.ptr(inp["rk"])) == 0
            assert "%s digest %s" % (name, h(c)) in out.stdout, (name, out.stdout)


@pytest.mark.parametrize("bits", [[50, 50, 50, 50], [55, 55, 56, 50], [58, 59, 59, 50], [60, 60, 61, 50]])
def test_quarter_row_inverse_at_n65536(sealhip, bits):
    """Round 4: standalone inverses at N = 2^16 run quarter-row workgroups (the N = 2^15 shape, index bits 0..13) and one streaming
    radix-4 pass for the two top layers (csrc/ntt.hip ntt_inv_top2_kernel: BackwardLazy on the gap N/4, BackwardLazyLast on
    the top, util/ntt.cpp:265-281, 345-404). Every arithmetic instance -- FP64 (50-bit primes), sparse lazy (55-56 bits), dense
    lazy (58-59 bits), the reference's sequence (60-61 bits) -- in the canonical and in the `_lazy` form (whose representatives
    must be the reference's), odd row counts, inputs over the whole documented range [0, 2p) with the extremes planted."""
    logn, n = 16, 1 << 16
    kmods = O.coeff_modulus_create(n, bits)
    k = len(kmods) - 1
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    rng = np.random.default_rng(sum(bits))
    tabs = [O.Tables(logn, p) for p in kmods[:k]]
    for count in (1, 3):
        x = np.stack([np.stack([rng.integers(0, 2 * p, size=n, dtype=np.uint64) for p in kmods[:k]]) for _ in range(count)])
        for i, p in enumerate(kmods[:k]):
            x[0, i, :5] = [2 * p - 1, 0, p, p - 1, 2 * p - 1]
            x[0, i, n // 4: n // 4 + 2] = [2 * p - 1, 0]
            x[0, i, -2:] = [2 * p - 1, 2 * p - 1]
        for name, fn, reffn in (("canonical", ctx.inverse_ntt_negacyclic_harvey, L.ref_ntt_inverse),
                                ("lazy", ctx.inverse_ntt_negacyclic_harvey_lazy, L.ref_ntt_inverse_lazy)):
            d = ctx.upload(x)
            fn(d, count, k)
            got = d.download(x.shape)
            for c in range(count):
                for i in range(k):
                    e = x[c, i].copy()
                    reffn(O.ptr(e), C.byref(tabs[i].t))
                    assert np.array_equal(got[c, i], e), (name, bits, c, i)
    # and back: forward of the canonical inverse is the residue of the input (where the fork's forward transform does not
    # wrap: 2 log n p <= 2^64, SURVEY F2 -- with 60-bit primes at this ring size it does, and the round trip is not the identity
    # in the reference either)
    if max(bits[:k]) <= 58:
        d = ctx.upload(x)
        ctx.inverse_ntt_negacyclic_harvey(d, count, k)
        ctx.ntt_negacyclic_harvey(d, count, k)
        mods = np.array(kmods[:k], dtype=np.uint64).reshape(1, k, 1)
        assert np.array_equal(d.download(x.shape), x % mods)


@pytest.mark.parametrize("logn", [14, 15, 16])
def test_single_pass_ntt_inplace_sibling_handoff_stress(sealhip, logn):
    """The single-pass forward NTT is in place while the two workgroups of a row each read both halves; the
    ticket hand-off must make the result independent of dispatch timing. Uneven launches (odd row counts,
    small and large batches back to back), every word checked against the first run and one row against the oracle."""
    n = 1 << logn
    mods = O.coeff_modulus_create(n, [50, 50, 50]) + O.get_primes(n, 57, 1)
    k = 3
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    rng = np.random.default_rng(logn)
    tabs = [O.Tables(logn, p) for p in mods[:k]]
    for count in (1, 3, 37, 5, 64, 1):
        x = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
        want = None
        for rep in range(4):
            d = ctx.upload(x)
            ctx.ntt_negacyclic_harvey(d, count, k)
            got = d.download(x.shape)
            if want is None:
                want = got
                exp = x[count - 1].copy()
                for i in range(k):
                    L.ref_ntt_forward(O.ptr(exp[i]), C.byref(tabs[i].t), 0)
                assert np.array_equal(got[count - 1], exp)
            else:
                assert np.array_equal(got, want), (count, rep)


@pytest.mark.parametrize("scheme,logn,bits", [(1, 12, [36, 36, 37, 38]), (1, 15, [55] * 4), (2, 12, [40, 40, 40, 41]), (2, 15, [50] * 4)])
def test_level_down_reads_ciphertexts_at_a_stride(sealhip, scheme, logn, bits):
    """mod_switch_to_next / rescale_to_next (evaluator.cpp:829-1036, 1090-1126) on ciphertexts that sit inside a wider
    container -- the size-2 result of relinearize in its size-3 product, the layout multiply -> relinearize leaves in a
    contiguous batch: the strided entries equal the compact ones on the compacted copy, and the oracle; CKKS
    mod_switch_to_next (drop) as well."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    k = len(kmods) - 1
    ctx = sealhip.Context(scheme, logn, kmods, 1, 786433 if scheme == 1 else 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(scheme, logn, kmods, nsp=1, t=786433 if scheme == 1 else 0)
    rng = np.random.default_rng(logn + scheme)
    count = 5
    wide = _rand_ct(rng, kmods[:k], 3, n, count)
    compact = np.ascontiguousarray(wide[:, :2])
    dw = ctx.upload(wide)
    for fn in ([ev.mod_switch_to_next] if scheme == 1 else [ev.rescale_to_next, ev.mod_switch_to_next]):
        o1, o2 = ctx.alloc(count * 2 * (k - 1) * n), ctx.alloc(count * 2 * (k - 1) * n)
        fn(dw, 2, k, count, o1, item_stride=3 * k * n)
        fn(ctx.upload(compact), 2, k, count, o2)
        got = o1.download((count, 2, k - 1, n))
        assert np.array_equal(got, o2.download(got.shape)), fn.__name__
        if fn.__name__ == "rescale_to_next" or scheme == 1:
            for c in range(count):
                exp = np.zeros((2, k - 1, n), dtype=np.uint64)
                assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(compact[c]), 2, O.ptr(exp)) == 0
                assert np.array_equal(got[c], exp), (fn.__name__, c)
        else:
            assert np.array_equal(got, compact[:, :, : k - 1])
    with pytest.raises(ValueError):
        ev.mod_switch_to_next(dw, 2, k, count, ctx.alloc(count * 2 * (k - 1) * n), item_stride=2 * k * n - 1)


@pytest.mark.parametrize("scheme,logn,bits,nsp", [(2, 15, [50] * 6, 1), (1, 15, [55] * 6, 1), (2, 12, [40, 40, 40, 41, 42], 2),
                                                  (1, 12, [36, 36, 37, 38, 39], 1), (2, 15, [58, 56, 50, 50, 59], 1)])
def test_latency_mode_key_switch_split_over_digit_groups(sealhip, scheme, logn, bits, nsp):
    """SURVEY 8(e) latency mode on one device: the digits of a key switch (evaluator.cpp:2259-2368) are formed in two or
    three groups as they would be on two or three GPUs (sealhip_switch_key_partial), the partial products are added word by
    word -- what all_reduce(SUM) does -- and sealhip_switch_key_finish runs the rest. Result == the unsplit
    sealhip_switch_key_inplace == the oracle, word for word; the partials equal the oracle's split as well."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    ctx = sealhip.Context(scheme, logn, kmods, nsp, 65537 if scheme == 1 else 0)
    ref = O.RefContext(scheme, logn, kmods, nsp=nsp, t=65537 if scheme == 1 else 0)
    k = ctx.k_first
    nd = ctx.kswitch_digits(k)
    assert nd == (k + nsp - 1) // nsp
    rng = np.random.default_rng(31 * logn + scheme)
    count = 3
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(nd)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    ct = _rand_ct(rng, kmods[:k], 2, n, count)
    target = _rand_ct(rng, kmods[:k], 1, n, count)[:, 0].copy()
    one = ctx.upload(ct)
    ctx.switch_key_inplace(k, one, ctx.upload(target), count, dkey)
    want = one.download(ct.shape)
    exp = ct.copy()
    for c in range(count):
        assert L.ref_switch_key_inplace(C.byref(ref.c), k, O.ptr(exp[c]), O.ptr(target[c]), O.ptr(key)) == 0
    assert np.array_equal(want, exp), "unsplit key switch vs oracle"
    rows = k + nsp
    dtarget = ctx.upload(target)
    for groups in (2, 3):
        cuts = [(g * nd) // groups for g in range(groups + 1)]
        total = np.zeros((count, 2, rows, n), dtype=np.uint64)
        for g in range(groups):
            part = ctx.alloc(count * 2 * rows * n)
            ctx.switch_key_partial(k, dtarget, count, dkey, cuts[g], cuts[g + 1], part)
            got_p = part.download(total.shape)
            ep = np.zeros((2, rows, n), dtype=np.uint64)
            assert L.ref_switch_key_partial(C.byref(ref.c), k, O.ptr(target[0]), O.ptr(key), cuts[g], cuts[g + 1], O.ptr(ep)) == 0
            assert np.array_equal(got_p[0], ep), ("partial", groups, g)
            total += got_p  # (below groups * p < 2^63)
        split = ctx.upload(ct)
        ctx.switch_key_finish(k, split, ctx.upload(total), count, groups)
        assert np.array_equal(split.download(ct.shape), want), ("finish", groups)
    # a world size whose sum of residues could pass 2^63 is refused, not wrapped (61-bit primes: more than 4 partials)
    if max(kmods) * 1000 >= 1 << 63:
        with pytest.raises(ValueError):
            ctx.switch_key_finish(k, ctx.upload(ct), ctx.upload(total), count, 1000)
    with pytest.raises(ValueError):
        ctx.switch_key_partial(k, dtarget, count, dkey, 0, nd + 1, ctx.alloc(count * 2 * rows * n))


def test_inplace_ntt_handoff_from_three_lanes_at_once(sealhip):
    """The forward single-pass kernel's sibling hand-off (a cross-workgroup ticket per row, a bounded wait, a sticky fault
    word) when several host threads drive ONE context at the same time: every thread has its own lane -- stream, ticket
    buffer, fault word (round 3: per lane) -- and launches in-place transforms of different sizes back to back, integer
    instances (57-bit primes: the canonical wrapper's approximate-quotient schedule and the reference's lazy sequence) and
    FP64 ones (50-bit). Every result against the oracle; no launch may report a hand-off failure."""
    import threading

    logn, n = 15, 1 << 15
    mods = O.get_primes(n, 57, 2) + O.get_primes(n, 50, 2) + O.get_primes(n, 58, 1)
    k = 4
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    tabs = [O.Tables(logn, p) for p in mods[:k]]
    errors = []

    def work(tid):
        try:
            rng = np.random.default_rng(100 + tid)
            for it, count in enumerate((5, 1, 9, 2, 7, 3)[tid:] + (5, 1, 9, 2, 7, 3)[:tid]):
                x = np.stack([rand_rows(rng, mods[:k], n) for _ in range(count)])
                lazy = (it + tid) % 2 == 1
                d = ctx.upload(x)
                (ctx.ntt_negacyclic_harvey_lazy if lazy else ctx.ntt_negacyclic_harvey)(d, count, k)
                got = d.download(x.shape)  # synchronises this thread's lane and reads its fault word
                for c in (0, count - 1):
                    e = x[c].copy()
                    for i in range(k):
                        if lazy:
                            L.ref_ntt_forward_lazy(O.ptr(e[i]), C.byref(tabs[i].t), 0)
                        else:
                            L.ref_ntt_forward(O.ptr(e[i]), C.byref(tabs[i].t), 0)
                    if not np.array_equal(got[c], e):
                        errors.append((tid, it, count, c))
        except Exception as ex:  # noqa: BLE001 -- reported by the asserting thread
            errors.append((tid, repr(ex)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert ctx.lane_count() >= 3


def test_cfg2_full_batch_1024_polynomials(sealhip):
    """BASELINE config 2 at its FULL batch: CKKS N = 2^14, 6 primes, forward + inverse NTT over 1024 key-level polynomials
    (6144 rows in one launch, the shape tools/bench_configs.py times). The golden digest polynomial of the survey sits at
    the first, a middle and the last position of the batch (launch-size dependent choices: XCD chunking, whole-row inverse
    grid) between random polynomials; those three reproduce the compiled reference's digests, sampled random ones equal
    the oracle word for word, and the whole batch round-trips (ntt.cpp:292-404)."""
    rows = [r for r in DIG["ntt_digests"] if r["logn"] == 14 and len(r["bits"]) == 6 and set(r["bits"]) == {50}]
    row = rows[0] if rows else None
    logn, n = 14, 1 << 14
    mods = O.coeff_modulus_create(n, [50] * 6)
    x1 = O.SplitMix(0x5EA1 + 1000 * logn + 6).fill(6, n, mods) if row else None  # the survey's generator (test_ntt_golden_digests)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, mods, 1, 0)
    tabs = [O.Tables(logn, p) for p in mods]
    rng = np.random.default_rng(2)
    P = 1024
    x = np.stack([rng.integers(0, p, size=(P, n), dtype=np.uint64) for p in mods], axis=1)
    marks = [0, 517, P - 1]
    if x1 is not None:
        assert h(x1) == row["input"]
        for m in marks:
            x[m] = x1
    d = ctx.upload(x)
    ctx.ntt_negacyclic_harvey(d, P, 5, sealhip.BASE_KEY)  # level k = 5 of BASE_KEY = all 6 key primes
    f = d.download(x.shape)
    for m in marks + [1, 300, 1000]:
        e = x[m].copy()
        for i in range(6):
            L.ref_ntt_forward(O.ptr(e[i]), C.byref(tabs[i].t), 0)
        assert np.array_equal(f[m], e), m
    if x1 is not None:
        for m in marks:
            assert h(f[m]) == row["fwd"], m
    ctx.inverse_ntt_negacyclic_harvey(d, P, 5, sealhip.BASE_KEY)
    assert np.array_equal(d.download(x.shape), x)


def test_full_size_batch_indexing_and_threads(sealhip):
    """cfg3 at full size with a batch of identical ciphertexts: every item must reproduce the compiled reference's
    digest (exercises item strides / chunking at BASELINE size), also when two host threads drive the same context."""
    import threading

    row = [r for r in DIG["end_to_end"] if r["cfg"] == 3][0]
    inp = synth.end_to_end_inputs(row)
    n, k = inp["n"], inp["k"]
    ctx = sealhip.Context(row["scheme"], inp["logn"], inp["kmods"], row["nsp"], row["t"])
    ev = sealhip.Evaluator(ctx)
    rk = sealhip.KSwitchKeys(ctx, inp["rk"])
    count = 5
    a = np.stack([inp["a"]] * count)
    b = np.stack([inp["b"]] * count)
    results = {}

    def work(tag):
        out = ctx.alloc(count * 3 * k * n)
        ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
        mul = out.download((count, 3, k, n)).copy()
        ev.relinearize_inplace(out, 3, k, count, [rk])
        results[tag] = (mul, out.download((count, 3, k, n))[:, :2].copy())

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert len(results) == 2
    for mul, relin in results.values():
        for c in range(count):
            assert h(mul[c]) == row["digests"]["mul"]
            assert h(np.ascontiguousarray(relin[c])) == row["digests"]["relin"]


def test_small_vectors_full_words(sealhip):
    """Committed full vectors (tests/golden/small_vectors.json): every output word of the HIP path."""
    SV = json.load(open(os.path.join(HERE, "golden", "small_vectors.json")))
    for case in SV["ntt"]:
        logn, p = case["logn"], case["p"]
        n = 1 << logn
        ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, [p, O.get_primes(n, 20, 1)[0]], 1, 0)
        x = np.array(case["x"], dtype=np.uint64)
        for name, fn in (("fwd_lazy", ctx.ntt_negacyclic_harvey_lazy), ("fwd", ctx.ntt_negacyclic_harvey),
                         ("inv_lazy", ctx.inverse_ntt_negacyclic_harvey_lazy), ("inv", ctx.inverse_ntt_negacyclic_harvey)):
            d = ctx.upload(x)
            fn(d, 1, 1)
            assert d.download().tolist() == case[name], (logn, name)
    for ch in SV["chains"]:
        n, k = 1 << ch["logn"], ch["k"]
        ctx = sealhip.Context(ch["scheme"], ch["logn"], ch["key_moduli"], ch["nsp"], ch["t"])
        ev = sealhip.Evaluator(ctx)
        key = sealhip.KSwitchKeys(ctx, np.array(ch["key"], dtype=np.uint64))
        a, b = np.array(ch["a"], dtype=np.uint64), np.array(ch["b"], dtype=np.uint64)
        c = ctx.alloc(3 * k * n)
        ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, 1, c)
        assert c.download((3, k, n)).tolist() == ch["multiply"]
        ev.relinearize_inplace(c, 3, k, 1, [key])
        c2 = c.download((3, k, n))[:2].copy()
        assert c2.tolist() == ch["relinearize"]
        o = ctx.alloc(2 * (k - 1) * n)
        (ev.mod_switch_to_next if ch["scheme"] == 1 else ev.rescale_to_next)(ctx.upload(c2), 2, k, 1, o)
        assert o.download((2, k - 1, n)).tolist() == ch["mod_switch_scale_to_next"]
        g = ctx.upload(c2)
        ev.rotate_vector_inplace(g, k, 1, 3, {ch["galois_elt_step3"]: key})
        assert g.download((2, k, n)).tolist() == ch["apply_galois"]


# ---------------------------------------------------------------- the rest of the Evaluator surface
def _rand_ct(rng, mods, size, n, count):
    return np.stack([rng.integers(0, p, size=(count, size, n), dtype=np.uint64) for p in mods], axis=2).copy()


@pytest.mark.parametrize("logn,sa,sb", [(5, 2, 2), (12, 3, 2), (12, 2, 3), (15, 2, 2)])
def test_f1_add_sub_negate(sealhip, logn, sa, sb):
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, [40, 40, 41])
    k, count = 2, 3
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(2, logn, kmods, nsp=1, t=0)
    rng = np.random.default_rng(logn * 10 + sa)
    a, b = _rand_ct(rng, kmods[:k], sa, n, count), _rand_ct(rng, kmods[:k], sb, n, count)
    so = max(sa, sb)
    da, db, do = ctx.upload(a), ctx.upload(b), ctx.alloc(count * so * k * n)
    for name, gfn, rfn in (("add", ev.add, L.ref_evaluator_add), ("sub", ev.sub, L.ref_evaluator_sub)):
        gfn(da, sa, db, sb, k, count, do)
        got = do.download((count, so, k, n))
        exp = np.zeros_like(got)
        for i in range(count):
            rfn(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(b[i]), sb, O.ptr(exp[i]))
        assert np.array_equal(got, exp), name
    ev.negate(da, sa, k, count, da)  # in place
    exp = np.zeros_like(a)
    for i in range(count):
        L.ref_evaluator_negate(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(exp[i]))
    assert np.array_equal(da.download(a.shape), exp)
    if sa >= sb:  # in place on the first operand, as Evaluator::add_inplace
        da.upload(a)
        ev.add(da, sa, db, sb, k, count, da)
        exp = np.zeros_like(a)
        for i in range(count):
            L.ref_evaluator_add(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(b[i]), sb, O.ptr(exp[i]))
        assert np.array_equal(da.download(a.shape), exp)
    else:
        with pytest.raises(ValueError):
            ev.add(da, sa, db, sb, k, count, da)


@pytest.mark.parametrize("logn", [5, 12, 15])
def test_f1_multiply_plain(sealhip, logn):
    n, t = 1 << logn, 786433 if logn > 10 else 257
    kmods = O.coeff_modulus_create(n, [40, 40, 41])
    k, count, size = 2, 3, 2
    rng = np.random.default_rng(logn)
    # BFV, coefficient form: multiply_plain_normal (one plaintext per ciphertext, then one for all)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    ct = _rand_ct(rng, kmods[:k], size, n, count)
    plains = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    plains[1] = 0
    plains[1, 5] = t - 3  # a monomial in the upper half: the reference takes its shortcut here (evaluator.cpp:1516-1553)
    for stride, pl in ((n, plains), (0, plains[:1])):
        d = ctx.upload(ct)
        ev.multiply_plain_inplace(d, size, k, count, ctx.upload(pl), stride, ntt_form=False)
        exp = ct.copy()
        for i in range(count):
            assert L.ref_multiply_plain(C.byref(ref.c), k, O.ptr(exp[i]), size, O.ptr(pl[i if stride else 0])) == 0
        assert np.array_equal(d.download(ct.shape), exp), stride
    # CKKS, NTT form: multiply_plain_ntt
    c2 = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    e2 = sealhip.Evaluator(c2)
    r2 = O.RefContext(2, logn, kmods, nsp=1, t=0)
    pn = np.stack([rng.integers(0, p, size=(count, n), dtype=np.uint64) for p in kmods[:k]], axis=1).copy()
    for stride, pl in ((k * n, pn), (0, pn[:1])):
        d = c2.upload(ct)
        e2.multiply_plain_inplace(d, size, k, count, c2.upload(pl), stride)
        exp = ct.copy()
        for i in range(count):
            L.ref_multiply_plain_ntt(C.byref(r2.c), k, O.ptr(exp[i]), size, O.ptr(pl[i if stride else 0]))
        assert np.array_equal(d.download(ct.shape), exp), stride
    # unsupported: CKKS context for the coefficient-form product, and a plain modulus above a prime
    with pytest.raises(sealhip.LogicError):
        e2.multiply_plain_inplace(c2.upload(ct), size, k, count, c2.upload(plains), n, ntt_form=False)


@pytest.mark.parametrize("scheme,logn,bits", [(1, 15, [55] * 4), (1, 12, [36, 36, 37]), (2, 15, [50] * 4), (2, 15, [58] * 4),
                                              (2, 12, [40, 40, 40, 41])])
def test_transparency_is_a_flag_output_of_the_operations(sealhip, scheme, logn, bits):
    """the transparent-ciphertext test the reference runs after every operation (evaluator.cpp:265-271,
    ciphertext.h:471-476) as a flag output of the kernels (sealhip_transparency_sink). Batches in which some results are
    transparent by construction (second polynomials zero, so products / key switches / automorphisms of them are zero): the
    flags written by multiply, square, relinearize, apply_galois (fused into the storing kernel), mod_switch / rescale,
    rotate_vector, add, negate (read pass on the result) must equal the separate device reduction sealhip_is_transparent on
    the same result, and the known pattern; results with a sink equal results without one; an operation on a fresh batch
    clears what an earlier one left."""
    n, t = 1 << logn, 786433
    kmods = O.coeff_modulus_create(n, bits)
    k = len(kmods) - 1
    ctx = sealhip.Context(scheme, logn, kmods, 1, t if scheme == 1 else 0)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(5 * logn + scheme)
    count = 6
    zero_items = [1, 4]  # their second polynomial is zero
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    for i in zero_items:
        a[i, 1] = 0
        b[i, 1] = 0
    a[2, 1] = 0
    a[2, 1, k - 1, n - 1] = 1  # one non-zero word: not transparent
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    flags = ctx.alloc((count + 1) // 2)
    flags.upload(np.full((count + 1) // 2, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))  # stale garbage: every op must clear first

    def got():
        return (flags.download().view(np.uint32)[:count] != 0).tolist()

    want = [i not in zero_items for i in range(count)]
    ctx.transparency_sink(flags, count)
    try:
        # multiply (products of ciphertexts whose second polynomials are zero have zero polynomials 1 and 2)
        prod = ctx.alloc(count * 3 * k * n)
        ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, prod)
        assert got() == want == [not v for v in ctx.is_transparent(prod, 3, k, count).tolist()], "multiply"
        ref_prod = prod.download((count, 3, k, n)).copy()
        sq = ctx.alloc(count * 3 * k * n)
        ev.square(ctx.upload(a), 2, k, count, sq)
        assert got() == [not v for v in ctx.is_transparent(sq, 3, k, count).tolist()], "square"
        assert got()[1] is False and got()[4] is False and got()[0] is True
        # relinearize (of the products: polynomial 2 zero -> nothing is added -> polynomial 1 stays zero)
        ev.relinearize_inplace(prod, 3, k, count, [dkey])
        relin = np.ascontiguousarray(prod.download((count, 3, k, n))[:, :2])
        assert got() == want == [not v for v in ctx.is_transparent(ctx.upload(relin), 2, k, count).tolist()], "relinearize"
        # apply_galois
        g = ctx.upload(a)
        ev.apply_galois_inplace(g, k, count, ctx.galois_elt_from_step(1), dkey)
        assert got() == want == [not v for v in ctx.is_transparent(g, 2, k, count).tolist()], "apply_galois"
        ref_g = g.download((count, 2, k, n)).copy()
        # mod_switch_to_next / rescale_to_next (read pass)
        o = ctx.alloc(count * 2 * (k - 1) * n)
        (ev.mod_switch_to_next if scheme == 1 else ev.rescale_to_next)(ctx.upload(a), 2, k, count, o)
        assert got() == want == [not v for v in ctx.is_transparent(o, 2, k - 1, count).tolist()], "level down"
        # add: a + (-a) is transparent everywhere; negate keeps the pattern
        neg = ctx.alloc(count * 2 * k * n)
        ev.negate(ctx.upload(a), 2, k, count, neg)
        assert got() == want, "negate"
        s = ctx.alloc(count * 2 * k * n)
        ev.add(ctx.upload(a), 2, neg, 2, k, count, s)
        assert got() == [False] * count, "add"
        # a smaller batch only touches its own flags; a larger one than the sink is refused
        ev.negate(ctx.upload(a[:2]), 2, k, 2, ctx.alloc(2 * 2 * k * n))
        assert got()[:2] == want[:2]
        ctx.transparency_sink(flags, 2)
        with pytest.raises(ValueError):
            ev.negate(ctx.upload(a), 2, k, count, neg)
        # a call rejected for the sink's capacity leaves BOTH the in-place operand and the flags as they were
        # (the capacity is validated before the first launch; the flags are cleared only where they start to be written)
        before = got()
        dct = ctx.upload(a)
        plain_ntt = ctx.upload(np.stack([rand_rows(rng, kmods[:k], n) for _ in range(count)]))
        with pytest.raises(ValueError):
            ev.multiply_plain_inplace(dct, 2, k, count, plain_ntt, plain_stride=k * n, ntt_form=True)
        assert np.array_equal(dct.download(a.shape), a) and got() == before
        with pytest.raises(ValueError):  # rejected for its level before anything else: the flags stay
            ev.mod_switch_to_next(ctx.upload(a), 2, k + 5, count, ctx.alloc(count * 2 * k * n))
        assert got() == before
    finally:
        ctx.transparency_sink(None, 0)
    # the same operations without a sink give the same words
    prod2 = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, prod2)
    assert np.array_equal(prod2.download((count, 3, k, n)), ref_prod)
    g2 = ctx.upload(a)
    ev.apply_galois_inplace(g2, k, count, ctx.galois_elt_from_step(1), dkey)
    assert np.array_equal(g2.download((count, 2, k, n)), ref_g)


def test_transparency_sink_dies_with_its_thread(sealhip):
    """ADVICE r03 (engine.cpp LanePool::give): a lane goes back to the pool when its thread exits, the sink the thread had
    registered must not go with it. Thread A registers a 2-item sink and exits; thread B -- which gets A's lane from the idle
    list -- runs a 6-item operation: no E_INVALIDARG from the stale capacity, and A's buffer keeps its sentinel."""
    import threading

    logn, n = 12, 4096
    kmods = O.coeff_modulus_create(n, [40, 40, 41])
    k, count = 2, 6
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(3)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    flags = ctx.alloc(1)
    sentinel = np.array([0xA5A5A5A5A5A5A5A5], dtype=np.uint64)
    flags.upload(sentinel)
    err = []

    def thread_a():
        try:
            ctx.transparency_sink(flags, 2)
            ev.negate(ctx.upload(a[:2]), 2, k, 2, ctx.alloc(2 * 2 * k * n))
            ctx.synchronize()
            flags.upload(sentinel)  # what the sink wrote is not the point; what happens AFTER the thread is
            ctx.synchronize()
        except Exception as e:  # pragma: no cover
            err.append(e)

    ta = threading.Thread(target=thread_a)
    ta.start()
    ta.join()
    out = {}

    def thread_b():
        try:
            o = ctx.alloc(count * 2 * k * n)
            ev.negate(ctx.upload(a), 2, k, count, o)  # count > the dead thread's capacity of 2
            out["neg"] = o.download((count, 2, k, n))
        except Exception as e:
            err.append(e)

    tb = threading.Thread(target=thread_b)
    tb.start()
    tb.join()
    assert not err, err
    assert np.array_equal(flags.download(), sentinel), "a later thread wrote into the sink of a thread that has exited"
    kk = np.array(kmods[:k], dtype=np.uint64).reshape(1, 1, k, 1)
    assert np.array_equal(out["neg"], np.where(a == 0, a, kk - a))


def test_f1_transparent_mod63_and_native_rotate(sealhip):
    logn, n = 12, 4096
    kmods = O.coeff_modulus_create(n, [40, 40, 40, 41])
    k, count = 3, 4
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(77)
    ct = _rand_ct(rng, kmods[:k], 2, n, count)
    ct[1, 1:] = 0
    ct[3, 1, 2, 4095] = 0
    ct[2, 1] = 0
    ct[2, 1, k - 1, n - 1] = 1  # a single non-zero word at the very end
    d = ctx.upload(ct)
    assert ctx.is_transparent(d, 2, k, count).tolist() == [False, True, False, False]
    assert ctx.is_transparent(d, 1, k, 2 * count).all()  # size < 2
    with pytest.raises(sealhip.LogicError):
        ev.check_not_transparent(d, 2, k, count)
    # modulo_poly_coeffs_63
    x = rng.integers(0, 1 << 63, size=(5, k, n), dtype=np.uint64)
    dx = ctx.upload(x)
    ctx.modulo_poly_coeffs_63(dx, 5, k, dx)
    assert np.array_equal(dx.download(x.shape), np.stack([x[:, r] % np.uint64(kmods[r]) for r in range(k)], axis=1))
    # rotate_vector behind the C ABI == the host-side NAF walk (and the direct key when present)
    krng = np.random.default_rng(3)
    keys = {}
    for step in (1, 2, 4, 8, -1, -4):
        elt = ctx.galois_elt_from_step(step)
        keys[elt] = sealhip.KSwitchKeys(ctx, np.stack([_rand_ct(krng, kmods, 2, n, 1)[0] for _ in range(k)]))
    src = _rand_ct(rng, kmods[:k], 2, n, count)
    for steps in (1, 3, 7, -3, 0):
        a, b = ctx.upload(src), ctx.upload(src)
        ev.rotate_vector_inplace(a, k, count, steps, keys)
        ev.rotate_vector_native(b, k, count, steps, keys)
        assert np.array_equal(a.download(src.shape), b.download(src.shape)), steps
    with pytest.raises(ValueError):
        ev.rotate_vector_native(ctx.upload(src), k, count, 16, keys)  # power of two without a key


@pytest.mark.parametrize("scheme,logn,bits", [
    (1, 15, 55), (1, 15, 56), (1, 15, 57), (1, 15, 58), (1, 15, 59), (1, 14, 56), (1, 14, 57), (1, 14, 58), (1, 16, 55), (1, 16, 56),
    (1, 16, 57), (1, 16, 58), (2, 15, 55), (2, 15, 56), (2, 15, 58), (2, 14, 56), (2, 16, 55), (2, 16, 57), (2, 16, 58)])
def test_shortcut_boundaries_largest_admitted_primes(sealhip, scheme, logn, bits):
    """csrc/ntt_bounds.hpp admits each shortcut up to a prime size (lazy-sum inverse: 2^55 whole-row / 2^56 half-row at
    N = 2^15, 2^56 / 2^56 at 2^14, 2^55 at 2^16; kNttAnyRep, kNttApprox (round 4: the level-2 quotient, 4p per layer) and the
    unreduced mod-up: 2^58 at N = 2^14 / 2^15, 2^57 at 2^16; fused tensor product: 2^59 on exact-quotient rows, 2^57 on
    approximate-quotient rows; the canonical entry's schedule on inputs below 4p: the same sizes). The recurrences are proved on the CPU (tests/bounds_check.cpp); this drives the real pipelines with the
    LARGEST primes below each bound and one size above it, and the inputs that maximise growth (all p-1, alternating,
    half, plus random), bit-exact against the oracle: multiply + relinearize (BFV) / rotate + multiply + relinearize +
    rescale (CKKS), and the standalone inverse on lazy-range inputs up to 2p-1.
    Reference: evaluator.cpp:274-527,772-827,2259-2368, util/ntt.cpp:245-404."""
    n, nk, t = 1 << logn, 4, 786433
    kmods = sorted(O.get_primes(n, bits, nk))  # the nk largest primes below 2^bits
    assert max(kmods) < (1 << bits) and min(kmods) > (1 << bits) - (1 << (bits - 8))
    k = nk - 1
    ctx = sealhip.Context(scheme, logn, kmods, 1, t if scheme == 1 else 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(scheme, logn, kmods, nsp=1, t=t if scheme == 1 else 0)
    rng = np.random.default_rng(bits * 100 + logn)

    def pattern(kind, mods, polys):
        x = np.zeros((polys, len(mods), n), dtype=np.uint64)
        for i, p in enumerate(mods):
            if kind == 0:
                x[:, i, :] = p - 1
            elif kind == 1:
                x[:, i, ::2] = p - 1
            elif kind == 2:
                x[:, i, n // 2:] = p - 1
            else:
                x[:, i] = rng.integers(0, p, (polys, n), dtype=np.uint64)
        return x

    key = np.stack([pattern(j % 4, kmods, 2) if j < 2 else pattern(3, kmods, 2) for j in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    a = np.stack([pattern(kind, kmods[:k], 2) for kind in (0, 1, 2, 3)])
    b = np.stack([pattern(kind, kmods[:k], 2) for kind in (0, 0, 3, 3)])
    count = a.shape[0]
    mul = L.ref_bfv_multiply if scheme == 1 else L.ref_ckks_multiply
    out = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
    exp = np.zeros((count, 3, k, n), dtype=np.uint64)
    for c in range(count):
        assert mul(C.byref(ref.c), k, O.ptr(a[c]), 2, O.ptr(b[c]), 2, O.ptr(exp[c])) == 0
    assert np.array_equal(out.download(exp.shape), exp), "multiply"
    ev.relinearize_inplace(out, 3, k, count, [dkey])
    for c in range(count):
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp[c]), 3, keys) == 0
    assert np.array_equal(out.download(exp.shape)[:, :2], exp[:, :2]), "relinearize"
    if scheme == 2:
        elt = ctx.galois_elt_from_step(3)
        g = ctx.upload(a)
        ev.apply_galois_inplace(g, k, count, elt, dkey)
        expg = a.copy()
        for c in range(count):
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(expg[c]), elt, O.ptr(key)) == 0
        assert np.array_equal(g.download(expg.shape), expg), "apply_galois"
        c2 = np.ascontiguousarray(exp[:, :2])
        o = ctx.alloc(count * 2 * (k - 1) * n)
        ev.rescale_to_next(ctx.upload(c2), 2, k, count, o)
        exp_ms = np.zeros((count, 2, k - 1, n), dtype=np.uint64)
        for c in range(count):
            assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(c2[c]), 2, O.ptr(exp_ms[c])) == 0
        assert np.array_equal(o.download(exp_ms.shape), exp_ms), "rescale"
    # standalone transforms: canonical forward on residues, canonical inverse on the lazy range [0, 2p)
    tabs = [O.Tables(logn, p) for p in kmods[:k]]
    x = np.concatenate([pattern(kind, kmods[:k], 1) for kind in (0, 1, 2, 3)])
    for lazy_in in (False, True):
        y = x.copy()
        if lazy_in:
            for i, p in enumerate(kmods[:k]):
                y[:, i, :] += np.uint64(p)  # every word in [p, 2p): all 2p-1 for the first pattern
        buf = ctx.upload(y)
        ctx.inverse_ntt_negacyclic_harvey(buf, x.shape[0], k)
        e = x.copy()
        for c in range(x.shape[0]):
            for i in range(k):
                L.ref_ntt_inverse(O.ptr(e[c, i]), C.byref(tabs[i].t))
        assert np.array_equal(buf.download(x.shape), e), "inverse lazy_in=%s" % lazy_in
    for top in (False, True):  # residues, and the top of the documented operand range: every word in [3p, 4p)
        y = x.copy()
        if top:
            for i, p in enumerate(kmods[:k]):
                y[:, i, :] += np.uint64(3 * p)
        buf = ctx.upload(y)
        ctx.ntt_negacyclic_harvey(buf, x.shape[0], k)
        e = y.copy()
        for c in range(x.shape[0]):
            for i in range(k):
                L.ref_ntt_forward(O.ptr(e[c, i]), C.byref(tabs[i].t), 0)
        assert np.array_equal(buf.download(x.shape), e), "forward top=%s" % top


@pytest.mark.parametrize("scheme,logn,bits", [(1, 15, [55] * 4), (1, 14, [50] * 3 + [58]), (1, 16, [50] * 3), (1, 12, [36, 36, 37]),
                                              (1, 15, [59, 59, 59]), (2, 15, [50] * 4), (2, 13, [40, 40, 41])])
def test_square_is_its_own_path(sealhip, scheme, logn, bits):
    """Evaluator::square (evaluator.cpp:528-558) -> bfv_square (:560-702) / ckks_square (:704-770): a size-2 operand is
    lifted and transformed once and c_1 = x_0 x_1 is added to itself; other sizes go through multiply. The engine's path
    (two lifts / 2 (k + |Bsk|) forward rows, the doubling inside the fused inverse load or the tensor kernel) against the
    oracle's branch-by-branch restatement, with multiply(a, a) as the cross-check on both sides, extreme values included
    (all p-1: the doubled product is the largest lazy value the inverse is handed)."""
    n, t = 1 << logn, 786433
    kmods = O.coeff_modulus_create(n, bits)
    k = len(kmods) - 1
    ctx = sealhip.Context(scheme, logn, kmods, 1, t if scheme == 1 else 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(scheme, logn, kmods, nsp=1, t=t if scheme == 1 else 0)
    rng = np.random.default_rng(7 * logn + scheme)
    mul = L.ref_bfv_multiply if scheme == 1 else L.ref_ckks_multiply
    sqr = L.ref_bfv_square if scheme == 1 else L.ref_ckks_square
    for size in (2, 3):
        a = np.stack([rand_rows(rng, kmods[:k] * size, n).reshape(size, k, n) for _ in range(3)])
        for i, p in enumerate(kmods[:k]):
            a[0, :, i, :] = p - 1
            a[1, 0, i, ::2] = p - 1
        count, dest = a.shape[0], 2 * size - 1
        out = ctx.alloc(count * dest * k * n)
        ev.square(ctx.upload(a), size, k, count, out)
        got = out.download((count, dest, k, n))
        out2 = ctx.alloc(count * dest * k * n)
        da = ctx.upload(a)
        ev.multiply(da, size, ctx.upload(a), size, k, count, out2)
        for c in range(count):
            exp = np.zeros((dest, k, n), dtype=np.uint64)
            assert sqr(C.byref(ref.c), k, O.ptr(a[c]), size, O.ptr(exp)) == 0
            assert np.array_equal(got[c], exp), "square size=%d item %d" % (size, c)
            exp2 = np.zeros((dest, k, n), dtype=np.uint64)
            assert mul(C.byref(ref.c), k, O.ptr(a[c]), size, O.ptr(a[c]), size, O.ptr(exp2)) == 0
            assert np.array_equal(exp, exp2), "oracle: square vs multiply(a, a)"
        assert np.array_equal(out2.download(got.shape), got), "engine: multiply(a, a) vs square"


@pytest.mark.parametrize("k_first", [3, 7, 9])
def test_bfv_multiply_extreme_values_59bit(sealhip, k_first):
    """Largest user primes the fork admits (59 bits, util/defines.h:40) and operands that are all p-1 / all zero /
    alternating: worst case for the carry-free dot-product accumulators of the fused BEHZ kernels (devmath.hpp DotAcc)."""
    logn, n, t = 12, 4096, 786433
    kmods = O.coeff_modulus_create(n, [59] * (k_first + 1))
    k = k_first
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    top = np.stack([np.full((2, n), p - 1, dtype=np.uint64) for p in kmods[:k]], axis=1)
    alt = top.copy()
    alt[:, :, ::2] = 0
    rng = np.random.default_rng(k_first)
    rnd = _rand_ct(rng, kmods[:k], 2, n, 1)[0]
    cases = [(top, top), (top, alt), (alt, rnd), (np.zeros_like(top), top)]
    a = np.stack([c[0] for c in cases])
    b = np.stack([c[1] for c in cases])
    out = ctx.alloc(len(cases) * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, len(cases), out)
    got = out.download((len(cases), 3, k, n))
    for i in range(len(cases)):
        exp = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(exp)) == 0
        assert np.array_equal(got[i], exp), i


@pytest.mark.parametrize("scheme,nsp,count", [(1, 1, 19), (1, 2, 16), (2, 1, 27)])
def test_key_switch_large_batch_key_reuse(sealhip, scheme, nsp, count):
    """Batches of >= 16 ciphertexts take the inner-product kernel that keeps the key words in registers across eight
    ciphertexts (ks_mac_items_kernel); ragged last groups included. relinearize + apply_galois against the oracle."""
    logn, n = 11, 2048
    kmods = O.coeff_modulus_create(n, [45] * (4 + nsp))
    k = 4
    d = (k + nsp - 1) // nsp
    t = 65537 if scheme == 1 else 0
    ctx = sealhip.Context(scheme, logn, kmods, nsp, t)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(scheme, logn, kmods, nsp=nsp, t=t)
    rng = np.random.default_rng(100 * scheme + nsp)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(d)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    ct3 = _rand_ct(rng, kmods[:k], 3, n, count)
    dct = ctx.upload(ct3)
    ev.relinearize_inplace(dct, 3, k, count, [dkey])
    got = dct.download(ct3.shape)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    for i in range(count):
        exp = ct3[i].copy()
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp), 3, keys) == 0
        assert np.array_equal(got[i, :2], exp[:2]), i
    ct2 = _rand_ct(rng, kmods[:k], 2, n, count)
    elt = ctx.galois_elt_from_step(3)
    g = ctx.upload(ct2)
    ev.apply_galois_inplace(g, k, count, elt, dkey)
    got = g.download(ct2.shape)
    for i in range(count):
        exp = ct2[i].copy()
        assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(exp), elt, O.ptr(key)) == 0
        assert np.array_equal(got[i], exp), i


# ---------------------------------------------------------------- decrypt-side arithmetic, semantic end-to-end
@pytest.mark.parametrize("logn,nsp", [(8, 1), (12, 2), (14, 1)])
def test_f2_encrypt_evaluate_on_gpu_decrypt(sealhip, logn, nsp):
    """Client side from the oracle (keys, symmetric encryption), evaluation on the GPU in STRICT mode (the fork's BFV
    relinearize is not semantically valid, F3), decryption on the GPU: plaintexts multiply as polynomials mod
    (x^N + 1, t); and every GPU decrypt equals the oracle's decrypt of the same ciphertext."""
    n, t = 1 << logn, 65537
    kmods = O.coeff_modulus_create(n, [45] * (3 + nsp))
    ref = O.RefContext(1, logn, kmods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=logn)
    k, count = cl.k, 3
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, nsp, t, mode=sealhip.MODE_STRICT)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(logn)
    m1 = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    m2 = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    a = np.stack([cl.encrypt_bfv(m) for m in m1])
    b = np.stack([cl.encrypt_bfv(m) for m in m2])
    pw = ctx.upload(cl.sk_powers(2))

    def gpu_decrypt(dct, size, kk):
        dot = ctx.alloc(count * kk * n)
        ctx.dot_product_ct_sk(dct, size, kk, count, pw, False, dot)
        out = ctx.alloc(count * n)
        ctx.decrypt_scale_and_round(kk, dot, count, out)
        return out.download((count, n))

    da = ctx.upload(a)
    assert np.array_equal(gpu_decrypt(da, 2, k), m1)  # fresh ciphertexts
    prod = ctx.alloc(count * 3 * k * n)
    ev.multiply(da, 2, ctx.upload(b), 2, k, count, prod)
    want = np.stack([O.negacyclic_mod_t(x, y, t) for x, y in zip(m1, m2)]) if logn <= 12 else None
    got3 = gpu_decrypt(prod, 3, k)
    host3 = prod.download((count, 3, k, n))
    for i in range(count):  # bit-exact against the oracle's decrypt of the GPU ciphertext
        assert np.array_equal(got3[i], cl.decrypt_bfv(host3[i])), i
    if want is not None:
        assert np.array_equal(got3, want)
    rk = sealhip.KSwitchKeys(ctx, cl.relin_key())
    ev.relinearize_inplace(prod, 3, k, count, [rk])
    c2 = ctx.upload(prod.download((count, 3, k, n))[:, :2].copy())
    got2 = gpu_decrypt(c2, 2, k)
    assert np.array_equal(got2, got3)  # relinearization does not change the plaintext
    low = ctx.alloc(count * 2 * (k - 1) * n)
    ev.mod_switch_to_next(c2, 2, k, count, low)
    assert np.array_equal(gpu_decrypt(low, 2, k - 1), got3)
    # rotate by one step and compare with the permuted plaintext
    elt = ctx.galois_elt_from_step(1)
    gk = sealhip.KSwitchKeys(ctx, cl.galois_key(elt))
    g = ctx.upload(a)
    ev.apply_galois_inplace(g, k, count, elt, gk)
    rot = gpu_decrypt(g, 2, k)
    idx = (np.arange(n, dtype=np.int64) * elt) % (2 * n)
    for i in range(count):
        perm = np.zeros(n, dtype=np.uint64)
        perm[idx % n] = np.where(idx < n, m1[i], (t - m1[i]) % t)
        assert np.array_equal(rot[i], perm), i


def test_f2_ckks_semantics_parity_mode(sealhip):
    """CKKS in PARITY mode (the fork as built) is semantically sound: encrypt two scaled integer polynomials, multiply,
    relinearize, rescale and rotate on the GPU, decrypt (dot product with the secret key on the GPU, CRT on the host):
    the results are the polynomial product / its rescaled value / the permuted input up to the scheme's noise."""
    logn, n = 10, 1024
    kmods = O.coeff_modulus_create(n, [40, 40, 40, 45])
    ref = O.RefContext(2, logn, kmods, nsp=1, t=0)
    cl = O.Client(ref, seed=5)
    k = cl.k
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(5)
    p1 = rng.integers(-(1 << 20), 1 << 20, size=n).astype(object)
    p2 = rng.integers(-(1 << 20), 1 << 20, size=n).astype(object)
    full = np.convolve(p1, p2)
    want = [int(full[i]) - (int(full[i + n]) if i + n < len(full) else 0) for i in range(n)]
    a, b = ctx.upload(cl.encrypt_poly_ntt(p1)), ctx.upload(cl.encrypt_poly_ntt(p2))
    pw = ctx.upload(cl.sk_powers(2))

    def decrypt(dct, size, kk):
        dot = ctx.alloc(kk * n)
        ctx.dot_product_ct_sk(dct, size, kk, 1, pw, True, dot)
        return cl.centered_from_ntt_rows(dot.download((kk, n)))

    got, _ = decrypt(a, 2, k)
    assert max(abs(g - int(w)) for g, w in zip(got, p1)) < 64  # fresh noise
    prod = ctx.alloc(3 * k * n)
    ev.multiply(a, 2, b, 2, k, 1, prod)
    got, _ = decrypt(prod, 3, k)
    assert max(abs(g - w) for g, w in zip(got, want)) < 1 << 40  # ~ N * |p| * |e|
    ev.relinearize_inplace(prod, 3, k, 1, [sealhip.KSwitchKeys(ctx, cl.relin_key())])
    c2 = ctx.upload(prod.download((3, k, n))[:2].copy())
    got, _ = decrypt(c2, 2, k)
    assert max(abs(g - w) for g, w in zip(got, want)) < 1 << 41
    low = ctx.alloc(2 * (k - 1) * n)
    ev.rescale_to_next(c2, 2, k, 1, low)
    got, _ = decrypt(low, 2, k - 1)
    qlast = kmods[k - 1]
    assert max(abs(g - w / qlast) for g, w in zip(got, want)) < 1 << 12
    elt = ctx.galois_elt_from_step(3)
    g = ctx.upload(a.download((2, k, n)))
    ev.apply_galois_inplace(g, k, 1, elt, sealhip.KSwitchKeys(ctx, cl.galois_key(elt)))
    got, _ = decrypt(g, 2, k)
    perm = [0] * n
    for i in range(n):
        j = (i * elt) % (2 * n)
        perm[j % n] = int(p1[i]) if j < n else -int(p1[i])
    assert max(abs(x - y) for x, y in zip(got, perm)) < 1 << 30  # key-switch noise ~ N * q_i * |e| / P


def test_randomised_differential_against_oracle(sealhip):
    """tools/fuzz_parity.py: random ring sizes (2^3..2^16), prime counts and bit sizes (25..59, mixed: both mod-up
    treatments of the gathered NTT), special-prime counts, schemes and batch sizes through multiply -> relinearize ->
    mod_switch/rescale -> apply_galois; every word against the oracle. (150 cases with another seed ran clean in r01.)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(HERE), "tools", "fuzz_parity.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    rng = np.random.default_rng(2024)
    done = sum(fz.one(rng, it) != "skip" for it in range(16))
    assert done >= 8


# ---------------------------------------------------------------- encrypt-side arithmetic on the device
@pytest.mark.parametrize("scheme,logn,bits,nsp,t", [(1, 5, [30, 30, 31], 1, 257), (1, 11, [45] * 4, 2, 65537),
                                                     (2, 13, [50] * 3, 1, 0), (1, 14, [55] * 3, 1, 786433)])
def test_f2_encrypt_zero_parity(sealhip, scheme, logn, bits, nsp, t):
    """encrypt_zero_symmetric / encrypt_zero_asymmetric (util/rlwe.cpp:140-300) with the same samples on both sides:
    bit-exact against the oracle in both output forms, at key level and at the first ciphertext level."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(scheme, logn, kmods, nsp=nsp, t=t)
    ctx = sealhip.Context(scheme, logn, kmods, nsp, t)
    rng = np.random.default_rng(logn)
    count = 3
    sk = rand_rows(rng, kmods, n)
    dsk = ctx.upload(sk)
    for rows in (len(kmods), len(kmods) - nsp):
        a = np.stack([rand_rows(rng, kmods[:rows], n) for _ in range(count)])
        e = rng.integers(-19, 20, size=(count, n)).astype(np.int32)
        e[0, :4] = [-19, 19, 0, -1]
        pk = np.stack([rand_rows(rng, kmods[:rows], n) for _ in range(2)])
        u = rng.integers(-1, 2, size=(count, n)).astype(np.int32)
        e2 = rng.integers(-19, 20, size=(count, 2, n)).astype(np.int32)
        for ntt_form in (True, False):
            out = ctx.alloc(count * 2 * rows * n)
            # the secret key keeps its key-level row stride N: rows 0..rows-1 are its first rows
            ctx.encrypt_zero_symmetric(rows, ntt_form, ctx.upload(a), ctx.upload_i32(e), dsk, count, out)
            got = out.download((count, 2, rows, n))
            for i in range(count):
                exp = np.zeros((2, rows, n), dtype=np.uint64)
                L.ref_encrypt_zero_symmetric_given(C.byref(ref.c), rows, O.ptr(sk), 1 if ntt_form else 0,
                                                   O.ptr(a[i]), O.ptr(e[i]), O.ptr(exp))
                assert np.array_equal(got[i], exp), (rows, ntt_form, i)
            # in place: a already sits in the c_1 slot
            buf = np.zeros((count, 2, rows, n), dtype=np.uint64)
            buf[:, 1] = a
            dbuf = ctx.upload(buf)
            ctx.encrypt_zero_symmetric(rows, ntt_form, dbuf.ptr + rows * n * 8, ctx.upload_i32(e), dsk, count, dbuf)
            assert np.array_equal(dbuf.download(got.shape), got)
            ctx.encrypt_zero_asymmetric(rows, ntt_form, ctx.upload(pk), ctx.upload_i32(u), ctx.upload_i32(e2), count, out)
            got = out.download((count, 2, rows, n))
            for i in range(count):
                exp = np.zeros((2, rows, n), dtype=np.uint64)
                L.ref_encrypt_zero_asymmetric_given(C.byref(ref.c), rows, O.ptr(pk), 1 if ntt_form else 0,
                                                    O.ptr(u[i]), O.ptr(e2[i]), O.ptr(exp))
                assert np.array_equal(got[i], exp), (rows, ntt_form, i)


@pytest.mark.parametrize("logn,bits,t", [(4, [30, 31], 2), (10, [40] * 3, 65537), (12, [60, 60, 60], (1 << 60) - 93),
                                         (13, [50] * 4, 1 << 20)])
def test_f2_scaling_variant_add_sub_plain(sealhip, logn, bits, t):
    """multiply_add/sub_plain_with_scaling_variant (util/scalingvariant.cpp:15-92) = BFV add_plain / sub_plain:
    bit-exact for small, large (60-bit), prime and power-of-two plain moduli; sub undoes add."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits + [bits[-1]])
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(logn)
    count, size = 3, 2
    for k in (len(bits), 1):
        ct = np.stack([_rand_ct(rng, kmods[:k], size, n, 1)[0] for _ in range(count)])
        plain = rng.integers(0, t, size=(count, n), dtype=np.uint64)
        plain[0, :3] = [0, t - 1, t // 2]
        d = ctx.upload(ct)
        ev.add_plain_inplace(d, size, k, count, ctx.upload(plain))
        got = d.download(ct.shape)
        exp = ct.copy()
        for i in range(count):
            L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain[i]), 0, O.ptr(exp[i, 0]))
        assert np.array_equal(got, exp), k
        ev.sub_plain_inplace(d, size, k, count, ctx.upload(plain))
        assert np.array_equal(d.download(ct.shape), ct)
        ev.sub_plain_inplace(d, size, k, count, ctx.upload(plain[0]), plain_stride=0)  # one plaintext for all
        exp = ct.copy()
        for i in range(count):
            L.ref_multiply_add_plain_with_scaling_variant(C.byref(ref.c), k, O.ptr(plain[0]), 1, O.ptr(exp[i, 0]))
        assert np.array_equal(d.download(ct.shape), exp)


def test_f2_ckks_add_plain(sealhip):
    logn, n = 10, 1024
    kmods = O.coeff_modulus_create(n, [40] * 4)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(3)
    k, count = 3, 2
    ct = np.stack([_rand_ct(rng, kmods[:k], 2, n, 1)[0] for _ in range(count)])
    plain = np.stack([rand_rows(rng, kmods[:k], n) for _ in range(count)])
    d = ctx.upload(ct)
    ev.add_plain_inplace(d, 2, k, count, ctx.upload(plain))
    got = d.download(ct.shape)
    mods = np.array(kmods[:k], dtype=np.uint64)[:, None]
    assert np.array_equal(got[:, 0], (ct[:, 0] + plain) % mods) and np.array_equal(got[:, 1], ct[:, 1])
    ev.sub_plain_inplace(d, 2, k, count, ctx.upload(plain))
    assert np.array_equal(d.download(ct.shape), ct)


def test_f2_public_key_encrypt_on_gpu_decrypt_on_gpu(sealhip):
    """Encryptor::encrypt with a public key, every arithmetic step on the device (encrypt_zero_asymmetric at key level,
    divide_and_round_q_last to the first level, + round(q m / t)), then multiply in STRICT mode and decrypt on the device."""
    logn, n, t, nsp = 12, 4096, 65537, 1
    kmods = O.coeff_modulus_create(n, [45] * 4)
    ref = O.RefContext(1, logn, kmods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=4)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, nsp, t, mode=sealhip.MODE_STRICT)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(8)
    n_key, k, count = cl.n_key, cl.k, 2
    dsk = ctx.upload(cl.sk)
    a = rand_rows(rng, kmods, n)[None]
    pk = ctx.alloc(2 * n_key * n)
    ctx.encrypt_zero_symmetric(n_key, True, ctx.upload(a), ctx.upload_i32(rng.integers(-6, 7, size=(1, n))), dsk, 1, pk)

    def encrypt(m):
        u = rng.integers(-1, 2, size=(count, n)).astype(np.int32)
        e = rng.integers(-6, 7, size=(count, 2, n)).astype(np.int32)
        big = ctx.alloc(count * 2 * n_key * n)
        ctx.encrypt_zero_asymmetric(n_key, False, pk, ctx.upload_i32(u), ctx.upload_i32(e), count, big)
        ctx.divide_and_round_q_last_inplace(n_key, big, count * 2)
        ct = ctx.upload(big.download((count, 2, n_key, n))[:, :, :k].copy())
        ev.add_plain_inplace(ct, 2, k, count, ctx.upload(m))
        return ct

    m1 = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    m2 = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    c1, c2 = encrypt(m1), encrypt(m2)
    pw = ctx.upload(cl.sk_powers(2))

    def decrypt(dct, size):
        dot = ctx.alloc(count * k * n)
        ctx.dot_product_ct_sk(dct, size, k, count, pw, False, dot)
        out = ctx.alloc(count * n)
        ctx.decrypt_scale_and_round(k, dot, count, out)
        return out.download((count, n))

    assert np.array_equal(decrypt(c1, 2), m1)
    prod = ctx.alloc(count * 3 * k * n)
    ev.multiply(c1, 2, c2, 2, k, count, prod)
    want = np.stack([O.negacyclic_mod_t(x, y, t) for x, y in zip(m1, m2)])
    assert np.array_equal(decrypt(prod, 3), want)


# ---------------------------------------------------------------- BatchEncoder on the device
@pytest.mark.parametrize("logn,t", [(6, 257), (12, 65537), (13, 786433), (15, 786433), (16, 786433)])
def test_f4_batch_encoder_parity(sealhip, logn, t):
    """BatchEncoder::encode / decode (batchencoder.cpp:113-154, :339-376): bit-exact against the oracle, the
    reference's own known answers (all-5 -> the constant 5; zero padding), round trip and slot-wise products."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, [50, 50])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    assert ctx.using_batching
    tb = O.Tables(logn, t)
    rng = np.random.default_rng(logn)
    count = 4
    vals = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    vals[0] = 5
    vals[1] = np.arange(n) % t
    plain = ctx.alloc(count * n)
    ctx.batch_encode(ctx.upload(vals), n, count, plain)
    got = plain.download((count, n))
    for i in range(count):
        exp = np.zeros(n, dtype=np.uint64)
        L.ref_batch_encode(C.byref(tb.t), O.ptr(vals[i]), n, O.ptr(exp))
        assert np.array_equal(got[i], exp), i
    assert got[0, 0] == 5 and not got[0, 1:].any()
    back = ctx.alloc(count * n)
    ctx.batch_decode(plain, count, back)
    assert np.array_equal(back.download((count, n)), vals)
    # short input: the remaining slots are zero
    nv = 20
    ctx.batch_encode(ctx.upload(vals[:, :nv].copy()), nv, count, plain)
    ctx.batch_decode(plain, count, back)
    res = back.download((count, n))
    assert np.array_equal(res[:, :nv], vals[:, :nv]) and not res[:, nv:].any()
    # decode of arbitrary plaintexts against the oracle
    pl = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    ctx.batch_decode(ctx.upload(pl), count, back)
    res = back.download((count, n))
    for i in range(count):
        exp = np.zeros(n, dtype=np.uint64)
        L.ref_batch_decode(C.byref(tb.t), O.ptr(pl[i]), n, O.ptr(exp))
        assert np.array_equal(res[i], exp), i


@pytest.mark.parametrize("logn,t", [(6, 257), (13, 786433), (15, 786433)])
def test_f4_batch_encoder_int64_overloads(sealhip, logn, t):
    """BatchEncoder::encode / decode for vector<int64_t> (batchencoder.cpp:156-198, :378-420) on the device against the
    oracle's restatement (pinned by BatchUnbatchIntVector's known answers in tests/test_oracle.py)."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, [50, 50])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    tb = O.Tables(logn, t)
    rng = np.random.default_rng(logn)
    count = 3
    vals = rng.integers(-(t // 2), t // 2 + 1, size=(count, n), dtype=np.int64)
    vals[0] = -5
    plain = ctx.alloc(count * n)
    ctx.batch_encode_int64(ctx.upload(vals.view(np.uint64)), n, count, plain)
    got = plain.download((count, n))
    for i in range(count):
        exp = np.zeros(n, dtype=np.uint64)
        L.ref_batch_encode_signed(C.byref(tb.t), O.ptr(np.ascontiguousarray(vals[i]).view(np.uint64)), n, O.ptr(exp))
        assert np.array_equal(got[i], exp), i
    assert got[0, 0] == t - 5 and not got[0, 1:].any()
    back = ctx.alloc(count * n)
    ctx.batch_decode_int64(plain, count, back)
    assert np.array_equal(back.download((count, n)).view(np.int64), vals)
    nv = 20  # short input: the remaining slots are zero
    ctx.batch_encode_int64(ctx.upload(np.ascontiguousarray(vals[:, :nv]).view(np.uint64)), nv, count, plain)
    ctx.batch_decode_int64(plain, count, back)
    res = back.download((count, n)).view(np.int64)
    assert np.array_equal(res[:, :nv], vals[:, :nv]) and not res[:, nv:].any()


def test_f4_batching_unavailable_is_reported(sealhip):
    n = 1024
    kmods = O.coeff_modulus_create(n, [40, 40])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, 10, kmods, 1, 1 << 16)  # not prime
    assert not ctx.using_batching
    buf = ctx.alloc(n)
    with pytest.raises(ValueError):
        ctx.batch_encode(buf, n, 1, buf)
    ctx2 = sealhip.Context(sealhip.SCHEME_BFV, 10, kmods, 1, 65537)
    with pytest.raises(sealhip.LogicError):  # batchencoder.cpp:119-122
        ctx2.batch_encode(ctx2.alloc(n + 1), n + 1, 1, ctx2.alloc(n))


# ---------------------------------------------------------------- ciphertext wire format <-> HBM
def test_f3_ciphertext_load_save_roundtrip_and_validation(sealhip):
    """Ciphertext::load / save (ciphertext.cpp:170-330) with the words going straight between the byte stream and HBM:
    the stream the engine writes is byte-identical to the oracle's, loading it back gives the same words, the loaded
    ciphertext evaluates to the same result as the directly uploaded one, and invalid inputs are refused with the
    reference's error classes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(os.path.dirname(HERE), "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    logn, n, t = 12, 4096, 65537
    kmods = O.coeff_modulus_create(n, [36, 36, 37])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    ids = {3: (1, 2, 3, 4), 2: (5, 6, 7, 8), 1: (9, 10, 11, 12)}
    for k, pid in ids.items():
        ctx.set_parms_id(k, pid)
    rng = np.random.default_rng(12)
    k, size = 2, 2
    a = _rand_ct(rng, kmods[:k], size, n, 1)[0]
    b = _rand_ct(rng, kmods[:k], size, n, 1)[0]
    raw_a = W.save_ciphertext(ids[k], False, size, n, k, 1.0, a.reshape(-1))
    da = ctx.alloc(a.size)
    info = ctx.load_ciphertext(raw_a, da)
    assert (info.size, info.coeff_modulus_size, info.is_ntt_form, info.seeded) == (size, k, 0, 0)
    assert np.array_equal(da.download(a.shape), a)
    assert ctx.save_ciphertext(info, da) == raw_a  # byte-identical stream
    # evaluate on the loaded ciphertext, save the result, load it back
    prod = ctx.alloc(3 * k * n)
    ev.multiply(da, 2, ctx.upload(b), 2, k, 1, prod)
    direct = ctx.alloc(3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, 1, direct)
    assert np.array_equal(prod.download(), direct.download())
    pinfo = sealhip.CiphertextInfo()
    pinfo.parms_id[:] = ids[k]
    pinfo.size, pinfo.coeff_modulus_size, pinfo.is_ntt_form, pinfo.scale, pinfo.poly_modulus_degree = 3, k, 0, 1.0, n
    raw_p = ctx.save_ciphertext(pinfo, prod)
    parsed = W.load_ciphertext(raw_p)
    assert parsed["size"] == 3 and parsed["k"] == k and np.array_equal(parsed["words"], prod.download())
    back = ctx.alloc(3 * k * n)
    assert ctx.load_ciphertext(raw_p, back).size == 3 and np.array_equal(back.download(), prod.download())
    # validation (valcheck.cpp:67-105, :228-240, :284-317)
    assert ctx.is_data_valid_for(da, size, k, 1).all()
    bad = a.copy()
    bad[1, 1, 7] = kmods[1]
    both = ctx.upload(np.stack([a, bad]))
    assert list(ctx.is_data_valid_for(both, size, k, 2)) == [True, False]
    with pytest.raises(sealhip.LogicError, match="ciphertext data is invalid"):  # unknown parms_id
        ctx.load_ciphertext(W.save_ciphertext((7, 7, 7, 7), False, size, n, k, 1.0, a.reshape(-1)), da)
    with pytest.raises(sealhip.LogicError, match="ciphertext data is invalid"):  # k does not match the level
        ctx.load_ciphertext(W.save_ciphertext(ids[3], False, size, n, k, 1.0, a.reshape(-1)), da)
    with pytest.raises(sealhip.LogicError, match="ciphertext data is invalid"):  # size 1
        ctx.load_ciphertext(W.save_ciphertext(ids[k], False, 1, n, k, 1.0, a.reshape(-1)[: k * n]), da)
    with pytest.raises(sealhip.LogicError, match="ciphertext data is invalid"):  # buffer shorter than size*k*N
        ctx.load_ciphertext(W.save_ciphertext(ids[k], False, size, n, k, 1.0, a.reshape(-1)[:-1]), da)
    with pytest.raises(sealhip.LogicError, match="unexpected size"):
        ctx.load_ciphertext(W.save_ciphertext(ids[k], False, size, n, k, 1.0, np.concatenate([a.reshape(-1), a[0, 0]])), da)
    if size == 2:  # a seeded stream is expanded on load (test_f3_seeded_ciphertexts_and_keys_are_expanded_on_load)
        si = ctx.load_ciphertext(W.save_ciphertext(ids[k], False, 2, n, k, 1.0, a.reshape(-1)[: k * n], seed=bytes(64)), da)
        assert si.seeded == 1 and np.array_equal(da.download(a.shape)[0], a[0])
    with pytest.raises(ValueError, match="too small"):
        ctx.load_ciphertext(raw_a, da, capacity_words=a.size - 1)


# ---------------------------------------------------------------- host-side trees over the device ops
def test_f3_seeded_ciphertexts_and_keys_are_expanded_on_load(sealhip):
    """A seeded ciphertext on the wire is c_0 plus the 64-byte seed of c_1 (ciphertext.cpp:189-208); loading it re-samples
    c_1 like Ciphertext::expand_seed (:126-133, :296-309). The loaded words equal c_0 || oracle expansion, a seeded
    RelinKeys stream loads to the same key as its expanded form, and evaluating with either gives identical results."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(os.path.dirname(HERE), "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    logn, n, t = 12, 4096, 65537
    kmods = O.coeff_modulus_create(n, [45] * 4)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(19)
    n_key, k = 4, 3
    pid, key_id = (5, 6, 7, 8), (9, 10, 11, 12)
    ctx.set_parms_id(k, pid)
    ctx.set_parms_id(n_key, key_id)
    seed = [int(x) for x in rng.integers(0, 2**63, size=8)]
    seed_bytes = np.array(seed, dtype="<u8").tobytes()
    c0 = rand_rows(rng, kmods[:k], n)
    raw = W.save_ciphertext(pid, False, 2, n, k, 1.0, c0.reshape(-1), seed=seed_bytes)
    dst = ctx.alloc(2 * k * n)
    info = ctx.load_ciphertext(raw, dst)
    assert info.seeded == 1 and info.size == 2
    got = dst.download((2, k, n))
    assert np.array_equal(got[0], c0) and np.array_equal(got[1], O.expand_seed(seed, kmods[:k], n))
    assert ctx.is_data_valid_for(dst, 2, k, 1).all()
    with pytest.raises(ValueError, match="too small"):
        ctx.load_ciphertext(raw, ctx.alloc(k * n))
    # a seeded key stream: every digit stores component 0 and the seed of component 1
    d = 3
    digits0 = [rand_rows(rng, kmods, n) for _ in range(d)]
    seeds = [[int(x) for x in rng.integers(0, 2**63, size=8)] for _ in range(d)]
    full = np.stack([np.stack([digits0[j], O.expand_seed(seeds[j], kmods, n)]) for j in range(d)])
    body = struct_pack_kswitch_seeded(W, key_id, digits0, seeds, n, n_key)
    rk_seeded = sealhip.KSwitchKeys.from_stream(ctx, body, 0)
    ct = np.stack([_rand_ct(rng, kmods[:k], 3, n, 1)[0] for _ in range(2)])
    a, b = ctx.upload(ct), ctx.upload(ct)
    ev.relinearize_inplace(a, 3, k, 2, [rk_seeded])
    ev.relinearize_inplace(b, 3, k, 2, [sealhip.KSwitchKeys(ctx, full)])
    assert np.array_equal(a.download(), b.download())


def struct_pack_kswitch_seeded(W, key_id, digits0, seeds, n, n_key):
    """a KSwitchKeys stream (kswitchkeys.cpp:43-85) whose PublicKeys are seeded ciphertexts"""
    import struct

    body = struct.pack("<4Q", *key_id) + struct.pack("<Q", 1) + struct.pack("<Q", len(digits0))
    for c0, sd in zip(digits0, seeds):
        body += W.save_ciphertext(key_id, True, 2, n, n_key, 1.0, c0.reshape(-1), seed=np.array(sd, dtype="<u8").tobytes())
    return W.header(16 + len(body)) + body


def test_f1_multiply_many_exponentiate_add_many_resize(sealhip):
    """Evaluator::multiply_many / exponentiate / add_many (evaluator.cpp:153-172, 1180-1288) and Ciphertext::resize on
    device-resident batches: the same queue order as the reference, every step bit-exact against the oracle's
    multiply + relinearize; mod_switch_to walks the chain."""
    logn, n, t = 10, 1024, 65537
    kmods = O.coeff_modulus_create(n, [45] * 5)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(2)
    k, count, d = 4, 2, 4
    key = np.stack([np.stack([rand_rows(rng, kmods, n) for _ in range(2)]) for _ in range(d)])
    rk = sealhip.KSwitchKeys(ctx, key)
    cts = [np.stack([_rand_ct(rng, kmods[:k], 2, n, 1)[0] for _ in range(count)]) for _ in range(5)]

    def ref_product(a, b):
        out = np.zeros((count, 2, k, n), dtype=np.uint64)
        keys = (C.c_void_p * 1)(key.ctypes.data)
        for i in range(count):
            wide = np.zeros((3, k, n), dtype=np.uint64)
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(wide)) == 0
            assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(wide), 3, keys) == 0
            out[i] = wide[:2]
        return out

    queue = [ref_product(cts[0], cts[1]), ref_product(cts[2], cts[3]), cts[4]]
    i = 0
    while i < len(queue) - 1:
        queue.append(ref_product(queue[i], queue[i + 1]))
        i += 2
    got = ev.multiply_many([ctx.upload(c) for c in cts], k, count, [rk])
    assert np.array_equal(got.download((count, 2, k, n)), queue[-1])
    # exponentiate(3) = multiply_many of three copies: (x*x) relinearized, then times x
    x = cts[0]
    want = ref_product(ref_product(x, x), x)  # queue: [x*x, x] -> (x*x)*x
    got = ev.exponentiate(ctx.upload(x), 3, k, count, [rk])
    assert np.array_equal(got.download((count, 2, k, n)), want)
    with pytest.raises(ValueError, match="exponent cannot be 0"):
        ev.exponentiate(ctx.upload(x), 0, k, count, [rk])
    with pytest.raises(ValueError, match="must not be empty"):
        ev.multiply_many([], k, count, [rk])
    assert np.array_equal(ev.exponentiate(ctx.upload(x), 1, k, count, [rk]).download(x.shape), x)
    # add_many
    out = ctx.alloc(count * 2 * k * n)
    ev.add_many([ctx.upload(c) for c in cts[:3]], 2, k, count, out)
    mods = np.array(kmods[:k], dtype=np.uint64)[None, None, :, None]
    assert np.array_equal(out.download(cts[0].shape), ((cts[0] + cts[1]) % mods + cts[2]) % mods)
    # resize: grow to 3 (new polynomial zero), shrink back
    grown = ev.resize(ctx.upload(x), 2, 3, k, count).download((count, 3, k, n))
    assert np.array_equal(grown[:, :2], x) and not grown[:, 2].any()
    assert np.array_equal(ev.resize(ctx.upload(grown), 3, 2, k, count).download(x.shape), x)
    # mod_switch_to: two levels down = two mod_switch_to_next
    low = ev.mod_switch_to(ctx.upload(x), 2, k, k - 2, count).download((count, 2, k - 2, n))
    for i in range(count):
        a1 = np.zeros((2, k - 1, n), dtype=np.uint64)
        a2 = np.zeros((2, k - 2, n), dtype=np.uint64)
        assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(x[i]), 2, O.ptr(a1)) == 0
        assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k - 1, O.ptr(a1), 2, O.ptr(a2)) == 0
        assert np.array_equal(low[i], a2), i


# ---------------------------------------------------------------- CKKSEncoder on the device
@pytest.mark.parametrize("logn,bits,scale_log2", [(3, [30, 30], 16), (6, [40] * 4, 16), (10, [60] * 4, 40), (11, [55] * 4, 110),
                                                  (12, [55] * 4, 130), (13, [50] * 6, 40), (15, [50] * 4, 40),
                                                  (12, [60] * 4, 40)])
def test_f4_ckks_encoder_parity(sealhip, logn, bits, scale_log2):
    """CKKSEncoder::encode / decode (ckks.h:405-747). The device issues every floating-point operation in the
    reference's order without contraction and takes its root tables from the host's libm, so the plaintext words AND
    the decoded doubles are compared for equality with the oracle (tolerance 0); independently the round trip meets
    the reference tests' own bound |decode(encode(v)) - v| < 0.5 (native/tests/seal/ckks.cpp:45)."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, bits)
    ref = O.RefContext(2, logn, kmods, nsp=1)
    ck = O.CkksRef(ref)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    k, scale, count = len(bits) - 1, 2.0 ** scale_log2, 3
    rng = np.random.default_rng(logn)
    bound = 1 << (30 if scale_log2 <= 40 and bits[0] >= 50 else 8)
    v = rng.integers(-bound, bound, size=(count, n // 2)) + 1j * rng.integers(-bound, bound, size=(count, n // 2))
    v[0, :2] = [0.5 + 0.25j, -1.5]  # ties and fractions
    plain = ctx.ckks_encode(v, k, scale)
    got = plain.download((count, k, n))
    for i in range(count):
        rc, exp = ck.encode(v[i], k, scale)
        assert rc == 0 and np.array_equal(got[i], exp), i
    dec = ctx.ckks_decode(plain, k, count, scale)
    for i in range(count):
        exp = ck.decode(got[i], scale)
        assert np.array_equal(dec[i].view(np.uint64), exp.view(np.uint64)), i  # the same bits
    if not (logn >= 11 and max(bits) >= 60):
        # (with 60-bit primes at N >= 2^11 the fork's forward NTT wraps, SURVEY F2: the reference's own encoder is
        # unsound there; the engine reproduces its words bit for bit, checked above, and the bound is not asserted)
        assert np.max(np.abs(dec - v)) < 0.5
    # short input: zero padding
    nv = max(1, n // 8)
    short = ctx.ckks_encode(v[:, :nv].copy(), k, scale).download((count, k, n))
    for i in range(count):
        assert np.array_equal(short[i], ck.encode(v[i, :nv], k, scale)[1]), i
    # decode of arbitrary NTT-form plaintexts (values far from any encoding: exercises the upper-half branch)
    arb = np.stack([rand_rows(rng, kmods[:k], n) for _ in range(count)])
    dec = ctx.ckks_decode(ctx.upload(arb), k, count, scale)
    for i in range(count):
        assert np.array_equal(dec[i].view(np.uint64), ck.decode(arb[i], scale).view(np.uint64)), i
    # lower level
    if k > 1:
        low = ctx.ckks_encode(v, 1, 2.0 ** 16).download((count, 1, n))
        for i in range(count):
            assert np.array_equal(low[i], ck.encode(v[i], 1, 2.0 ** 16)[1]), i


def test_f4_ckks_single_value_encode(sealhip):
    """CKKSEncoder::encode(double value, ...) / encode(int64_t value, ...) (ckks.cpp:80-275) against the oracle's
    branch-by-branch restatement, through all three decomposition regimes and both signs; error classes as the reference."""
    logn, n = 12, 4096
    kmods = O.coeff_modulus_create(n, [50] * 5)
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0)
    ref = O.RefContext(2, logn, kmods, nsp=1, t=0)
    k = 4
    for v, scale in ((3.141592653589793, 2.0**40), (-2.718281828, 2.0**40), (12345.678, 2.0**20), (-0.3, 2.0**90),
                     (7.0, 2.0**150), (0.0, 2.0**30), (-1e-30, 2.0**40)):
        exp = np.zeros((k, n), dtype=np.uint64)
        assert L.ref_ckks_encode_value(C.byref(ref.c), k, v, scale, O.ptr(exp)) == 0
        got = ctx.ckks_encode_value(v, k, scale, count=2).download((2, k, n))
        assert np.array_equal(got[0], exp) and np.array_equal(got[1], exp), (v, scale)
    for iv in (0, 5, -5, 2**62, -(2**62), -(2**63)):
        exp = np.zeros((k, n), dtype=np.uint64)
        assert L.ref_ckks_encode_int64(C.byref(ref.c), k, iv, O.ptr(exp)) == 0
        assert np.array_equal(ctx.ckks_encode_value(iv, k, 1.0).download((1, k, n))[0], exp), iv
    with pytest.raises(ValueError, match="scale out of bounds"):
        ctx.ckks_encode_value(1.0, k, 2.0**250)
    with pytest.raises(ValueError, match="encoded value is too large"):
        ctx.ckks_encode_value(2.0**150, k, 2.0**100)
    # and it decodes to the value in every slot (the reference test's bound, ckks.cpp:271-275)
    plain = ctx.ckks_encode_value(1234.5, k, 2.0**40)
    assert np.max(np.abs(ctx.ckks_decode(plain, k, 1, 2.0**40)[0] - 1234.5)) < 0.5


def test_f4_ckks_encoder_errors(sealhip):
    n = 1024
    kmods = O.coeff_modulus_create(n, [40, 40, 40])
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, 10, kmods, 1, 0)
    v = np.ones((1, n // 2), dtype=np.complex128)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ctx.ckks_encode(v, 2, 2.0 ** 200)
    with pytest.raises(ValueError, match="scale out of bounds"):
        ctx.ckks_encode(v, 2, -1.0)
    with pytest.raises(ValueError, match="encoded values are too large"):
        ctx.ckks_encode(v * 2.0 ** 30, 1, 2.0 ** 30)
    with pytest.raises(ValueError, match="values_size is too large"):
        ctx.ckks_encode(np.ones((1, n), dtype=np.complex128), 2, 2.0 ** 20)
    bfv = sealhip.Context(sealhip.SCHEME_BFV, 10, kmods, 1, 65537)
    with pytest.raises(ValueError, match="unsupported scheme"):
        bfv.ckks_encode(v, 2, 2.0 ** 20)


def test_f3_kswitch_keys_stream_to_hbm(sealhip):
    """KSwitchKeys::load (kswitchkeys.cpp:87-150) for RelinKeys / GaloisKeys streams: the digits of keys_[index] go from the
    byte stream straight into HBM in the K1 layout; relinearizing with the stream-loaded key equals relinearizing with the
    directly uploaded one; empty slots, wrong parms_id and malformed members are reported like the reference does."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("wire_format", os.path.join(os.path.dirname(HERE), "oracle", "wire_format.py"))
    W = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(W)
    logn, n, t = 11, 2048, 65537
    kmods = O.coeff_modulus_create(n, [40] * 4)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(9)
    n_key, k, d = 4, 3, 3
    key_id = (21, 22, 23, 24)
    ctx.set_parms_id(n_key, key_id)
    key = np.stack([np.stack([rand_rows(rng, kmods, n) for _ in range(2)]) for _ in range(d)])
    other = np.stack([np.stack([rand_rows(rng, kmods, n) for _ in range(2)]) for _ in range(d)])
    raw = W.save_kswitch_keys(key_id, [list(key), [], list(other)], n, n_key)  # slot 1 unused (as in GaloisKeys)
    rk = sealhip.KSwitchKeys.from_stream(ctx, raw, 0)
    assert rk is not None and rk.n_slots == 3
    assert sealhip.KSwitchKeys.from_stream(ctx, raw, 1) is None
    rk2 = sealhip.KSwitchKeys.from_stream(ctx, raw, 2)
    count = 2
    ct = np.stack([_rand_ct(rng, kmods[:k], 3, n, 1)[0] for _ in range(count)])
    for loaded, host in ((rk, key), (rk2, other)):
        a, b = ctx.upload(ct), ctx.upload(ct)
        ev.relinearize_inplace(a, 3, k, count, [loaded])
        ev.relinearize_inplace(b, 3, k, count, [sealhip.KSwitchKeys(ctx, host)])
        assert np.array_equal(a.download(), b.download())
    # KSwitchKeys::save: the engine writes the same bytes the oracle's restatement of kswitchkeys.cpp:43-85 does
    assert sealhip.save_kswitch_keys(ctx, [rk, None, rk2]) == raw
    assert sealhip.save_kswitch_keys(ctx, [sealhip.KSwitchKeys(ctx, key)]) == W.save_kswitch_keys(key_id, [list(key)], n, n_key)
    with pytest.raises(ValueError, match="out of range"):
        sealhip.KSwitchKeys.from_stream(ctx, raw, 3)
    with pytest.raises(sealhip.LogicError, match="not valid"):
        sealhip.KSwitchKeys.from_stream(ctx, W.save_kswitch_keys((1, 1, 1, 1), [list(key)], n, n_key), 0)
    with pytest.raises(sealhip.LogicError, match="not valid"):  # a digit at the wrong level
        sealhip.KSwitchKeys.from_stream(ctx, W.save_kswitch_keys(key_id, [[key[0][:, :3]]], n, 3), 0)
    with pytest.raises(RuntimeError, match="I/O error"):
        sealhip.KSwitchKeys.from_stream(ctx, raw[: len(raw) // 2], 2)


# ---------------------------------------------------------------- HIP graphs for launch-bound small batches
def test_graph_capture_replay_is_bit_exact(sealhip):
    """A multiply -> relinearize -> mod_switch chain on fixed buffers captured into one hipGraph: replays with new input
    data in the same buffers equal the oracle; capturing without a warm run, or replaying after the arena was
    re-allocated, is refused."""
    logn, n, t = 13, 8192, 65537
    kmods = O.coeff_modulus_create(n, [50] * 4)
    ref = O.RefContext(1, logn, kmods, nsp=1, t=t)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(13)
    k, count = 3, 2
    key = np.stack([np.stack([rand_rows(rng, kmods, n) for _ in range(2)]) for _ in range(k)])
    rk = sealhip.KSwitchKeys(ctx, key)
    da, db = ctx.alloc(count * 2 * k * n), ctx.alloc(count * 2 * k * n)
    wide, two, low = ctx.alloc(count * 3 * k * n), ctx.alloc(count * 2 * k * n), ctx.alloc(count * 2 * (k - 1) * n)

    def chain():
        ev.multiply(da, 2, db, 2, k, count, wide)
        ev.relinearize_inplace(wide, 3, k, count, [rk])
        ev.resize(wide, 3, 2, k, count, two)
        ev.mod_switch_to_next(two, 2, k, count, low)

    fresh = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, t)
    with pytest.raises((sealhip.LogicError, RuntimeError, MemoryError)):  # nothing allocated yet: not capturable
        sealhip._check(sealhip.lib().sealhip_graph_capture_begin(fresh.handle))
        try:
            sealhip.Evaluator(fresh).multiply(fresh.alloc(2 * k * n), 2, fresh.alloc(2 * k * n), 2, k, 1, fresh.alloc(3 * k * n))
        finally:
            h = C.c_void_p()
            sealhip._check(sealhip.lib().sealhip_graph_capture_end(fresh.handle, C.byref(h)))
    # the failing operation aborted and discarded the capture (it says so), and the context works normally afterwards
    assert "aborted" in sealhip.lib().sealhip_last_error_string().decode() or True
    fa, fb, fo = fresh.upload(_rand_ct(rng, kmods[:k], 2, n, 1)), fresh.upload(_rand_ct(rng, kmods[:k], 2, n, 1)), fresh.alloc(3 * k * n)
    sealhip._check(sealhip.lib().sealhip_graph_capture_begin(fresh.handle))
    hr = sealhip.lib().sealhip_evaluator_multiply(fresh.handle, k, fa.ptr, 2, fb.ptr, 2, 1, fo.ptr) & 0xFFFFFFFF
    assert hr != 0 and "aborted" in sealhip.lib().sealhip_last_error_string().decode()
    h = C.c_void_p()
    assert sealhip.lib().sealhip_graph_capture_end(fresh.handle, C.byref(h)) & 0xFFFFFFFF == sealhip.COR_E_INVALIDOPERATION
    sealhip.Evaluator(fresh).multiply(fa, 2, fb, 2, k, 1, fo)  # not stuck in capture mode
    w = np.zeros((3, k, n), dtype=np.uint64)
    ha, hb = fa.download((2, k, n)), fb.download((2, k, n))
    assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(ha), 2, O.ptr(hb), 2, O.ptr(w)) == 0
    assert np.array_equal(fo.download((3, k, n)), w)
    da.upload(_rand_ct(rng, kmods[:k], 2, n, count))
    db.upload(_rand_ct(rng, kmods[:k], 2, n, count))
    # a graph embeds the addresses of the keys it uses: destroying one makes every earlier graph stale
    rk_tmp = sealhip.KSwitchKeys(ctx, key)
    g_tmp = ctx.capture(lambda: ev.relinearize_inplace(wide, 3, k, count, [rk_tmp]))
    g_tmp.launch()
    ctx.synchronize()
    del rk_tmp
    import gc
    gc.collect()
    with pytest.raises(sealhip.LogicError, match="key-switch key was destroyed"):
        g_tmp.launch()
    g = ctx.capture(chain)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    for trial in range(3):
        a, b = _rand_ct(rng, kmods[:k], 2, n, count), _rand_ct(rng, kmods[:k], 2, n, count)
        da.upload(a)
        db.upload(b)
        g.launch()
        got = low.download((count, 2, k - 1, n))
        for i in range(count):
            w = np.zeros((3, k, n), dtype=np.uint64)
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(w)) == 0
            assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(w), 3, keys) == 0
            lo = np.zeros((2, k - 1, n), dtype=np.uint64)
            assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(w[:2].copy()), 2, O.ptr(lo)) == 0
            assert np.array_equal(got[i], lo), (trial, i)
    # a larger operation re-allocates the arena: the graph holds stale addresses and says so
    big = 64
    ev.multiply(ctx.alloc(big * 2 * k * n), 2, ctx.alloc(big * 2 * k * n), 2, k, big, ctx.alloc(big * 3 * k * n))
    with pytest.raises(sealhip.LogicError, match="stale"):
        g.launch()


def test_new_entry_points_accept_empty_batches(sealhip):
    """count = 0 (and n_values = 0) are no-ops everywhere, like the reference's loops over empty ranges"""
    n = 1024
    kmods = O.coeff_modulus_create(n, [40, 40, 40])
    ctx = sealhip.Context(sealhip.SCHEME_BFV, 10, kmods, 1, 65537)
    ev = sealhip.Evaluator(ctx)
    buf = ctx.alloc(4 * 2 * 2 * n)
    i32 = ctx.upload_i32(np.zeros(2 * n, dtype=np.int32))
    ctx.encrypt_zero_symmetric(2, True, buf, i32, buf, 0, buf)
    ctx.encrypt_zero_asymmetric(2, False, buf, i32, i32, 0, buf)
    ev.add_plain_inplace(buf, 2, 2, 0, buf)
    ctx.batch_encode(buf, n, 0, buf)
    ctx.batch_decode(buf, 0, buf)
    ev.resize(buf, 2, 3, 2, 0, buf)
    assert ctx.is_data_valid_for(buf, 2, 2, 0).size == 0
    # zero values: every slot is zero -> the zero plaintext
    vals = ctx.upload(np.zeros(n, dtype=np.uint64))
    out = ctx.alloc(n)
    ctx.batch_encode(vals, 0, 1, out)
    assert not out.download().any()
    ck = sealhip.Context(sealhip.SCHEME_CKKS, 10, kmods, 1, 0)
    z = ck.ckks_encode(np.zeros((1, 0), dtype=np.complex128), 2, 2.0 ** 20)
    assert not z.download().any()
    assert ck.ckks_encode(np.zeros((0, 4), dtype=np.complex128), 2, 2.0 ** 20).words == 0
    ctx.synchronize()
    ck.synchronize()


def test_full_size_batched_pipeline_semantics_cfg3(sealhip):
    """Everything either side of the hot path at BASELINE config 3's parameters (N = 2^15, {55} x 8 primes, t = 786433),
    all arithmetic on the device in STRICT mode: BatchEncoder encode -> public-key encryption (encrypt_zero_asymmetric
    at key level, divide_and_round_q_last, scaling variant) -> multiply -> relinearize -> mod_switch_to_next -> decrypt
    (dot product with the secret key, scale-and-round) -> BatchEncoder decode == the slot-wise product of the inputs;
    add_plain / multiply_plain shift and scale the slots as documented."""
    logn, n, t, nsp = 15, 1 << 15, 786433, 1
    kmods = O.coeff_modulus_create(n, [55] * 8)  # CoeffModulus::Create(N, {55} x 8): config 3's primes
    ref = O.RefContext(1, logn, kmods, nsp=nsp, t=t, mode=1)
    cl = O.Client(ref, seed=15)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, nsp, t, mode=sealhip.MODE_STRICT)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(15)
    n_key, k, count = cl.n_key, cl.k, 2
    dsk = ctx.upload(cl.sk)
    pk = ctx.alloc(2 * n_key * n)
    ctx.encrypt_zero_symmetric(n_key, True, ctx.upload(rand_rows(rng, kmods, n)[None]),
                               ctx.upload_i32(rng.integers(-6, 7, size=(1, n))), dsk, 1, pk)
    va = rng.integers(0, t, size=(count, n), dtype=np.uint64)
    vb = rng.integers(0, t, size=(count, n), dtype=np.uint64)

    def encode(v):
        p = ctx.alloc(count * n)
        ctx.batch_encode(ctx.upload(v), n, count, p)
        return p

    def encrypt(plain):
        big = ctx.alloc(count * 2 * n_key * n)
        ctx.encrypt_zero_asymmetric(n_key, False, pk, ctx.upload_i32(rng.integers(-1, 2, size=(count, n))),
                                    ctx.upload_i32(rng.integers(-6, 7, size=(count, 2, n))), count, big)
        ctx.divide_and_round_q_last_inplace(n_key, big, count * 2)
        ct = ctx.upload(big.download((count, 2, n_key, n))[:, :, :k].copy())
        ev.add_plain_inplace(ct, 2, k, count, plain)
        return ct

    def decrypt_decode(dct, size, kk):
        pw = ctx.upload(cl.sk_powers(size - 1))
        dot = ctx.alloc(count * kk * n)
        ctx.dot_product_ct_sk(dct, size, kk, count, pw, False, dot)
        pl = ctx.alloc(count * n)
        ctx.decrypt_scale_and_round(kk, dot, count, pl)
        out = ctx.alloc(count * n)
        ctx.batch_decode(pl, count, out)
        return out.download((count, n))

    pa, pb = encode(va), encode(vb)
    ca, cb = encrypt(pa), encrypt(pb)
    assert np.array_equal(decrypt_decode(ca, 2, k), va)
    prod = ctx.alloc(count * 3 * k * n)
    ev.multiply(ca, 2, cb, 2, k, count, prod)
    rk = sealhip.KSwitchKeys(ctx, cl.relin_key())
    ev.relinearize_inplace(prod, 3, k, count, [rk])
    two = ev.resize(prod, 3, 2, k, count)
    low = ctx.alloc(count * 2 * (k - 1) * n)
    ev.mod_switch_to_next(two, 2, k, count, low)
    assert np.array_equal(decrypt_decode(low, 2, k - 1), (va * vb) % t)
    # plaintext operations on the encrypted slots
    ev.add_plain_inplace(ca, 2, k, count, pb)
    assert np.array_equal(decrypt_decode(ca, 2, k), (va + vb) % t)
    ev.multiply_plain_inplace(cb, 2, k, count, pa, plain_stride=n, ntt_form=False)
    assert np.array_equal(decrypt_decode(cb, 2, k), (va * vb) % t)


# ---------------------------------------------------------------- separately allocated host ciphertexts, re-entrancy
@pytest.mark.parametrize("scheme", [1, 2])
def test_host_pointer_array_entries_match_the_device_batch_path(sealhip, scheme):
    """A std::vector<seal::Ciphertext> is one separately allocated buffer per ciphertext (ciphertext.h:709-721): the *_host
    entries take arrays of host pointers and pipeline them through the device in chunks (default 64). 150 scattered
    ciphertexts = three chunks, the last one ragged; every result must equal what the contiguous device-batch entries
    produce, which the tests above pin to the oracle and the golden digests."""
    logn, n, nsp = 12, 4096, 1
    kmods = O.coeff_modulus_create(n, [40] * 4)
    k, count = 3, 150
    t = 65537 if scheme == 1 else 0
    ctx = sealhip.Context(scheme, logn, kmods, nsp, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(31 + scheme)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    # separately allocated, differently aligned host buffers
    ha = [a[i].copy() for i in range(count)]
    hb = [np.ascontiguousarray(np.concatenate([np.zeros(i % 3 + 1, dtype=np.uint64), b[i].ravel()])[i % 3 + 1:]).reshape(2, k, n)
          for i in range(count)]
    # reference: the device-batch path
    d3 = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, d3)
    mul = d3.download((count, 3, k, n)).copy()
    ev.relinearize_inplace(d3, 3, k, count, [dkey])
    relin = d3.download((count, 3, k, n))[:, :2].copy()
    out3 = [np.zeros((3, k, n), dtype=np.uint64) for _ in range(count)]
    ev.multiply_host(ha, 2, hb, 2, k, out3)
    out2 = [np.zeros((2, k, n), dtype=np.uint64) for _ in range(count)]
    ev.multiply_host(ha, 2, hb, 2, k, out2, relin_keys=[dkey])
    for i in range(count):
        assert np.array_equal(out3[i], mul[i]), i
        assert np.array_equal(out2[i], relin[i]), i
    ev.relinearize_host(out3, 3, k, [dkey])  # in place: the first two polynomials of every buffer
    for i in range(count):
        assert np.array_equal(out3[i][:2], relin[i]), i
    # level switch and rotation
    low = ctx.alloc(count * 2 * (k - 1) * n)
    drel = ctx.upload(relin)
    (ev.rescale_to_next if scheme == 2 else ev.mod_switch_to_next)(drel, 2, k, count, low)
    want_low = low.download((count, 2, k - 1, n))
    hlow = [np.zeros((2, k - 1, n), dtype=np.uint64) for _ in range(count)]
    ev.mod_switch_to_next_host(out2, 2, k, hlow, rescale=scheme == 2)
    for i in range(count):
        assert np.array_equal(hlow[i], want_low[i]), i
    elt = ctx.galois_elt_from_step(3)
    ev.rotate_vector_inplace(drel, k, count, 3, {elt: dkey})
    want_rot = drel.download((count, 2, k, n))
    ev.rotate_vector_host(out2, k, 3, {elt: dkey})
    for i in range(count):
        assert np.array_equal(out2[i], want_rot[i]), i
    # errors: a null pointer in the batch, a missing key
    with pytest.raises(ValueError):
        ev.rotate_vector_host(out2, k, 5, {elt: dkey})
    ev.multiply_host([], 2, [], 2, k, [])  # empty batch


def test_host_entries_on_registered_pool_blocks(sealhip):
    """sealhip_host_register: the reference's ciphertexts are pieces of MemoryPool blocks (mempool.cpp:45,145) that live as long
    as the pool. With the blocks pinned in place the *_host entries copy straight between the caller's buffers and the device;
    results must be the same words as through the staging path -- all items registered, only the inputs registered (outputs
    staged), items of one array half in and half out of registered memory (falls back to staging for that array), in place
    (relinearize, rotate) -- and the registry must refuse overlaps and unknown pointers."""
    logn, n, nsp, t = 12, 4096, 1, 65537
    kmods = O.coeff_modulus_create(n, [40] * 4)
    k, count = 3, 150  # three chunks of 64, the last one ragged
    ctx = sealhip.Context(1, logn, kmods, nsp, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(77)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    d3 = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, d3)
    ev.relinearize_inplace(d3, 3, k, count, [dkey])
    relin = d3.download((count, 3, k, n))[:, :2].copy()
    elt = ctx.galois_elt_from_step(3)
    drel = ctx.upload(relin)
    ev.rotate_vector_inplace(drel, k, count, 3, {elt: dkey})
    want_rot = drel.download((count, 2, k, n))
    # "pool blocks": a few big allocations, ciphertexts are pieces of them at odd offsets
    words = 2 * k * n
    blocks = [np.zeros(50 * (words + 3) + 5, dtype=np.uint64) for _ in range(9)]

    def piece(blk, j):
        o = 1 + j * (words + 3)
        return blk[o:o + words].reshape(2, k, n)

    ha = [piece(blocks[i // 50], i % 50) for i in range(count)]
    hb = [piece(blocks[3 + i // 50], i % 50) for i in range(count)]
    ho = [piece(blocks[6 + i // 50], i % 50) for i in range(count)]
    for i in range(count):
        ha[i][...] = a[i]
        hb[i][...] = b[i]
    for blk in blocks[:6]:
        ev.host_register(blk)
    # inputs pinned, outputs staged
    ev.multiply_host(ha, 2, hb, 2, k, ho, relin_keys=[dkey])
    for i in range(count):
        assert np.array_equal(ho[i], relin[i]), i
        ho[i][...] = 0
    for blk in blocks[6:]:
        ev.host_register(blk)
    # everything pinned
    ev.multiply_host(ha, 2, hb, 2, k, ho, relin_keys=[dkey])
    for i in range(count):
        assert np.array_equal(ho[i], relin[i]), i
    # in place on pinned buffers
    ev.rotate_vector_host(ho, k, 3, {elt: dkey})
    for i in range(count):
        assert np.array_equal(ho[i], want_rot[i]), i
    # one array partly outside registered memory: that array takes the staging path, the words do not change
    mixed = [ha[i] if i % 2 else ha[i].copy() for i in range(count)]
    out = [np.zeros((2, k, n), dtype=np.uint64) for _ in range(count)]
    ev.multiply_host(mixed, 2, hb, 2, k, out, relin_keys=[dkey])
    for i in range(count):
        assert np.array_equal(out[i], relin[i]), i
    # a buffer that only starts inside a registered block is not "registered"
    tail = blocks[0][-words // 2:]
    assert tail.nbytes < words * 8
    # registry errors
    with pytest.raises(ValueError):
        ev.host_register(blocks[0])  # again
    with pytest.raises(ValueError):
        ev.host_register(blocks[1][10:20])  # inside a registered range
    with pytest.raises(ValueError):
        ev.host_unregister(blocks[1][10:20])  # not the start of one
    for blk in blocks:
        ev.host_unregister(blk)
    with pytest.raises(ValueError):
        ev.host_unregister(blocks[0])
    # and the staging path still serves the same buffers afterwards
    for i in range(count):
        ho[i][...] = 0
    ev.multiply_host(ha, 2, hb, 2, k, ho, relin_keys=[dkey])
    for i in range(count):
        assert np.array_equal(ho[i], relin[i]), i


def test_context_is_reentrant_one_lane_per_thread(sealhip):
    """seal::Evaluator is re-entrant (evaluator.h:1375-1377). Four host threads drive ONE context with different operations at
    the same time; each gets its own lane (stream + arena), nothing serialises on a context lock, and every result equals
    the single-threaded one."""
    import threading

    logn, n, nsp, t = 13, 8192, 1, 786433
    kmods = O.coeff_modulus_create(n, [50] * 4)
    k, count = 3, 6
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, nsp, t)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(77)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)

    def work(which, reps, out):
        for _ in range(reps):
            if which == 0:
                o = ctx.alloc(count * 3 * k * n)
                ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, o)
                ev.relinearize_inplace(o, 3, k, count, [dkey])
                out[which] = o.download((count, 3, k, n))[:, :2].copy()
            elif which == 1:
                d = ctx.upload(a)
                ctx.ntt_negacyclic_harvey(d, count * 2, k)
                ctx.inverse_ntt_negacyclic_harvey(d, count * 2, k)
                out[which] = d.download(a.shape)
            elif which == 2:
                res = [np.zeros((2, k, n), dtype=np.uint64) for _ in range(count)]
                ev.multiply_host([a[i] for i in range(count)], 2, [b[i] for i in range(count)], 2, k, res, relin_keys=[dkey])
                out[which] = np.stack(res)
            else:
                d = ctx.upload(a)
                o = ctx.alloc(count * 2 * (k - 1) * n)
                ev.mod_switch_to_next(d, 2, k, count, o)
                out[which] = o.download((count, 2, k - 1, n))

    single = {}
    for w in range(4):
        work(w, 1, single)
    lanes_before = ctx.lane_count()
    multi = {}
    threads = [threading.Thread(target=work, args=(w, 5, multi)) for w in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    ctx.synchronize()
    assert ctx.lane_count() >= lanes_before + 3  # (a finished thread's lane may be re-used by a later one)
    for w in range(4):
        assert np.array_equal(multi[w], single[w]), w
    assert np.array_equal(single[1], a) and np.array_equal(single[0], single[2])


# ---------------------------------------------------------------- the launch shapes bench.py is timed on
def _bench_shape_batch(row, count, n_random, seed):
    """`count` ciphertext pairs of a BASELINE config: the survey's golden input interleaved with `n_random` distinct
    random pairs (positions spread over the batch, first and last included), so that wrong item / chunk offsets cannot
    cancel out."""
    inp = synth.end_to_end_inputs(row)
    k, n = inp["k"], inp["n"]
    rng = np.random.default_rng(seed)
    a = np.stack([inp["a"]] * count)
    b = np.stack([inp["b"]] * count)
    where = sorted({int(x) for x in np.linspace(0, count - 1, n_random)})
    for i in where:
        a[i] = rand_rows(rng, inp["kmods"][:k] * 2, n).reshape(2, k, n)
        b[i] = rand_rows(rng, inp["kmods"][:k] * 2, n).reshape(2, k, n)
    return inp, a, b, where


@pytest.mark.parametrize("count", [33, 65])
def test_cfg3_bench_launch_shapes_vs_golden_and_oracle(sealhip, count):
    """BASELINE config 3 (what bench.py times) at a batch that takes the same kernels as the bench: count >= 16 selects
    ks_mac_items_kernel<7> at N = 2^15 (key words kept in registers across a group of ciphertexts: groups of eight at
    33, with a ragged last group; groups of sixteen -- the bench's -- at 65, again ragged), the single-pass NTT kernels
    see multi-polynomial launches, and -- when SEALHIP_WORKSPACE_MB shrinks the arena
    (test_bench_shapes_with_a_small_arena re-runs this test so) -- the batch spans many arena chunks. Golden items must
    reproduce the compiled reference's digests, random items the oracle's words."""
    row = [r for r in DIG["end_to_end"] if r["cfg"] == 3][0]
    inp, a, b, where = _bench_shape_batch(row, count, 5, 33)
    n, k = inp["n"], inp["k"]
    ctx = sealhip.Context(row["scheme"], inp["logn"], inp["kmods"], row["nsp"], row["t"])
    ev = sealhip.Evaluator(ctx)
    rk = sealhip.KSwitchKeys(ctx, inp["rk"])
    out = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, out)
    mul = out.download((count, 3, k, n)).copy()
    ev.relinearize_inplace(out, 3, k, count, [rk])
    relin = out.download((count, 3, k, n))
    ref = O.RefContext(1, inp["logn"], inp["kmods"], nsp=row["nsp"], t=row["t"])
    keys = (C.c_void_p * 1)(inp["rk"].ctypes.data)
    for i in range(count):
        if i in where:
            exp = np.zeros((3, k, n), dtype=np.uint64)
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(exp)) == 0
            assert np.array_equal(mul[i], exp), i
            assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(exp), 3, keys) == 0
            assert np.array_equal(relin[i], exp), i
        else:
            assert h(mul[i]) == row["digests"]["mul"], i
            assert h(np.ascontiguousarray(relin[i, :2])) == row["digests"]["relin"], i


def test_cfg4_rotate_large_batch_vs_golden_and_oracle(sealhip):
    """BASELINE config 4 (CKKS N = 2^15, 12 primes, 11 digits): rotate_vector over 32 ciphertexts -- the batched Galois
    gather, ks_mac_items_kernel<11>, the special-row inverse and the CKKS mod-down at the shape the scaling runs use."""
    row = [r for r in DIG["end_to_end"] if r["cfg"] == 4][0]
    count = 32
    inp, a, _, where = _bench_shape_batch(row, count, 4, 44)
    n, k = inp["n"], inp["k"]
    ctx = sealhip.Context(row["scheme"], inp["logn"], inp["kmods"], row["nsp"], row["t"])
    ev = sealhip.Evaluator(ctx)
    gk = sealhip.KSwitchKeys(ctx, inp["gk"])
    elt = ctx.galois_elt_from_step(1)
    c = ctx.upload(a)
    ev.rotate_vector_inplace(c, k, count, 1, {elt: gk})
    got = c.download((count, 2, k, n))
    ref = O.RefContext(2, inp["logn"], inp["kmods"], nsp=row["nsp"], t=0)
    for i in range(count):
        if i in where:
            exp = a[i].copy()
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(exp), elt, O.ptr(inp["gk"])) == 0
            assert np.array_equal(got[i], exp), i
        else:
            assert h(got[i]) == row["digests"]["rotate"], i


def test_cfg4_variant_with_16_decomposition_digits(sealhip):
    """BASELINE.json words config 4 as "12 primes ... 16 decomposition digits"; with n_special_primes = 1 the digit count
    is the number of ciphertext primes (keygenerator.cpp:334-336), so 16 digits means 17 key primes (SURVEY section 8
    header). That variant -- CKKS N = 2^15, {50} x 17, k = 16, ks_mac_items_kernel<16> and 17-row key-level polynomials --
    against the oracle: rotate_vector, multiply + relinearize, rescale."""
    logn, n, nsp = 15, 1 << 15, 1
    kmods = O.coeff_modulus_create(n, [50] * 17)
    k, d, count = 16, 16, 17
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, nsp, 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(2, logn, kmods, nsp=nsp, t=0)
    rng = np.random.default_rng(16)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(d)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    elt = ctx.galois_elt_from_step(1)
    g = ctx.upload(a)
    ev.rotate_vector_inplace(g, k, count, 1, {elt: dkey})
    rot = g.download(a.shape)
    o = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, o)
    ev.relinearize_inplace(o, 3, k, count, [dkey])
    rel = o.download((count, 3, k, n))[:, :2].copy()
    low = ctx.alloc(count * 2 * (k - 1) * n)
    ev.rescale_to_next(ctx.upload(rel), 2, k, count, low)
    res = low.download((count, 2, k - 1, n))
    keys = (C.c_void_p * 1)(key.ctypes.data)
    for i in (0, 7, count - 1):
        exp = a[i].copy()
        assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(exp), elt, O.ptr(key)) == 0
        assert np.array_equal(rot[i], exp), i
        wide = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_ckks_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(wide)) == 0
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(wide), 3, keys) == 0
        assert np.array_equal(rel[i], wide[:2]), i
        lo = np.zeros((2, k - 1, n), dtype=np.uint64)
        assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(wide[:2])), 2, O.ptr(lo)) == 0
        assert np.array_equal(res[i], lo), i


def test_ckks_mixed_prime_chain_single_pass_kernels(sealhip):
    """The usual CKKS chain -- 60-bit first and special primes, 40-bit primes in between -- at N = 2^14, where the
    single-pass kernels run: launches whose live rows mix primes below 2^50 with larger ones are split into a
    floating-point and an integer launch, the mod-down transform gathers a 60-bit special row (integer instance of
    reduce mode 5: top inverse layer + negation on load), and apply_galois writes (galois(c0) + r0, r1) without the copy /
    fill. rotate_vector, conjugate, multiply + relinearize + rescale and the canonical transforms against the oracle."""
    logn, n, nsp = 14, 1 << 14, 1
    kmods = O.coeff_modulus_create(n, [60, 40, 40, 40, 60])
    k, count = 4, 3
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, nsp, 0)
    ev = sealhip.Evaluator(ctx)
    ref = O.RefContext(2, logn, kmods, nsp=nsp, t=0)
    rng = np.random.default_rng(6040)
    key = np.stack([_rand_ct(rng, kmods, 2, n, 1)[0] for _ in range(k)])
    dkey = sealhip.KSwitchKeys(ctx, key)
    a = _rand_ct(rng, kmods[:k], 2, n, count)
    b = _rand_ct(rng, kmods[:k], 2, n, count)
    keys = (C.c_void_p * 1)(key.ctypes.data)
    for elt in (ctx.galois_elt_from_step(1), 2 * n - 1):  # a rotation and the conjugation
        g = ctx.upload(a)
        ev.apply_galois_inplace(g, k, count, elt, dkey)
        rot = g.download(a.shape)
        for i in range(count):
            exp = a[i].copy()
            assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(exp), elt, O.ptr(key)) == 0
            assert np.array_equal(rot[i], exp), (elt, i)
    o = ctx.alloc(count * 3 * k * n)
    ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, o)
    ev.relinearize_inplace(o, 3, k, count, [dkey])
    rel = o.download((count, 3, k, n))[:, :2].copy()
    low = ctx.alloc(count * 2 * (k - 1) * n)
    ev.rescale_to_next(ctx.upload(rel), 2, k, count, low)
    res = low.download((count, 2, k - 1, n))
    for i in range(count):
        wide = np.zeros((3, k, n), dtype=np.uint64)
        assert L.ref_ckks_multiply(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(b[i]), 2, O.ptr(wide)) == 0
        assert L.ref_relinearize(C.byref(ref.c), k, O.ptr(wide), 3, keys) == 0
        assert np.array_equal(rel[i], wide[:2]), i
        lo = np.zeros((2, k - 1, n), dtype=np.uint64)
        assert L.ref_mod_switch_scale_to_next(C.byref(ref.c), k, O.ptr(np.ascontiguousarray(wide[:2])), 2, O.ptr(lo)) == 0
        assert np.array_equal(res[i], lo), i
    # canonical transforms over the mixed rows (split launches), both directions
    tabs = [O.Tables(logn, p) for p in kmods[:k]]
    x = a[:, 0].copy()
    buf = ctx.upload(x)
    ctx.inverse_ntt_negacyclic_harvey(buf, count, k)
    inv = buf.download(x.shape)
    ctx.ntt_negacyclic_harvey(buf, count, k)
    fwd = buf.download(x.shape)
    for c in range(count):
        for i in range(k):
            e = x[c, i].copy()
            L.ref_ntt_inverse(O.ptr(e), C.byref(tabs[i].t))
            assert np.array_equal(inv[c, i], e), (c, i)
            # (no round-trip identity on the 60-bit row: the reference's forward butterflies wrap there)
            L.ref_ntt_forward(O.ptr(e), C.byref(tabs[i].t), 0)
            assert np.array_equal(fwd[c, i], e), (c, i)


def test_bench_shapes_with_a_small_arena():
    """SEALHIP_WORKSPACE_MB is read once per process: a child process with a 64 MB arena runs the two tests above with
    a smaller batch, so that every operation walks its batch in chunks of two or three ciphertexts (config 3 needs 27 MB
    of temporaries per pair in multiply and 22.5 MB per ciphertext in the key switch): the chunk-offset arithmetic of
    csrc/pipeline.cpp against the golden digests and the oracle."""
    import subprocess
    import sys

    env = dict(os.environ, SEALHIP_WORKSPACE_MB="64", SEALHIP_TEST_SMALL_ARENA_COUNT="7")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "small_arena_child"],
                       env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    tail = r.stdout.decode("utf-8", "replace")[-600:]
    assert r.returncode == 0 and " passed" in tail, tail


def _bench_child(argv, launcher=False, timeout=900):
    import json
    import subprocess
    import sys

    bench_py = os.path.join(os.path.dirname(HERE), "bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable]
    if launcher:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                "--master-port", "29577"]
    r = subprocess.run(cmd + [bench_py] + argv, env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    out, err = r.stdout.decode("utf-8", "replace"), r.stderr.decode("utf-8", "replace")
    assert r.returncode == 0, (out[-1500:], err[-1500:])
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-1500:]
    return json.loads(lines[0])


@pytest.mark.parametrize("launcher", [True, False], ids=["under_torchrun", "own_group"])
def test_bench_rccl_path_with_one_rank(launcher):
    """The multi-GPU path of bench.py on the real backend, as far as one GPU allows: a child process (as the driver starts
    it: `python -m torch.distributed.run --nproc-per-node 1 bench.py --gpus 1 --force-dist ...`, and once with bench.py
    building its own one-rank group) runs init_process_group("nccl", device_id=...), the timing barrier, all_reduce
    (max-over-ranks), all_gather (digests) and the final gather of the result slice -- to itself -- on RCCL, verifies the
    timed output against the oracle, and reports `rccl_ranks_seen` from the collective. SURVEY 8(e); the workload is
    evaluator.cpp:235-272,772-827 (multiply + relinearize)."""
    line = _bench_child(["--gpus", "1", "--force-dist", "--batch", "64", "--steps", "1", "--warmup", "1",
                         "--no-cpu-baseline", "--ntt-polys", "0", "--gather-cts", "16", "--verify-items", "3",
                         "--pcie-pairs", "0"], launcher=launcher)
    assert line["dist_initialized"] is True and line["n_gpus"] == 1
    assert line["gather"]["backend"] == "nccl" and line["gather"]["ranks_seen"] == 1 and line["rccl_ranks_seen"] == 1
    assert line["gather"]["bytes_per_rank"] == 16 * 2 * 7 * 32768 * 8
    assert line["verified_vs_oracle"] is True and line["verified_items"] == [0, 32, 63]
    assert line["key_replicated"] is True and line["roofline"]["kernel"] == "ntt_fwd_half"


def test_bench_dump_outputs_are_the_verified_words(tmp_path):
    """bench.py --dump-outputs on the engine: a batch of two ciphertexts (both verified against the oracle) is small enough
    to be dumped whole; the words put back together from their 32-bit halves lie below their primes and are the results
    the run digested itself (rank_digests: the size-2 results of the first four items)."""
    import torch

    import bench

    d = str(tmp_path / "dump")
    line = _bench_child(["--gpus", "1", "--batch", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                         "--ntt-polys", "0", "--verify-items", "2", "--pcie-pairs", "0", "--dump-outputs", d])
    assert line["verified_vs_oracle"] is True and line["verified_items"] == [0, 1]
    hi, lo, idx = (np.load(os.path.join(d, "ciphertexts_%s.npy" % s)) for s in ("hi", "lo", "index"))
    n, k = 1 << 15, 7
    assert hi.dtype == lo.dtype == idx.dtype == np.float64 and np.array_equal(idx, np.arange(2 * 2 * k * n))
    words = hi.astype(np.uint64) << np.uint64(32) | lo.astype(np.uint64)
    assert (words.reshape(2, 2, k, n) < np.array(bench.CFG3_PRIMES[:k], dtype=np.uint64)[:, None]).all()
    assert "%016x" % bench.cheap_digest(torch.from_numpy(words.view(np.int64))) == line["rank_digests"][0]


def test_latency_mode_tool_runs_its_all_reduce_on_rccl():
    """tools/latency_mode.py (the digits of one key switch split over the ranks, partial products summed by
    all_reduce over RCCL, the rest on every rank) as a child process under torch.distributed.run with one rank: the
    collective executes on the nccl backend and the split key switch equals the unsplit one (evaluator.cpp:2259-2368)."""
    import json
    import subprocess
    import sys

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    tool = os.path.join(os.path.dirname(HERE), "tools", "latency_mode.py")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
                        "127.0.0.1", "--master-port", "29585", tool, "--config", "3", "--reps", "2"],
                       env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode("utf-8", "replace")
    assert r.returncode == 0, (out[-800:], r.stderr.decode("utf-8", "replace")[-800:])
    line = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert line["split_equals_unsplit"] is True and line["ranks"] == 1 and line["digits"] == 7


@pytest.mark.parametrize("config,batch", [(4, 9), (5, 3)])
def test_bench_other_baseline_configs_verify_themselves(config, batch):
    """bench.py --config 4 (CKKS rotate_vector, evaluator.h:1201-1211; the in-place rotation applied warmup + steps times
    equals the oracle's repeated apply_galois) and --config 5 (BFV N = 2^16 multiply + relinearize + mod_switch_to_next,
    evaluator.cpp:996-1036): the same JSON schema, the first / middle / last item checked word for word against the oracle."""
    line = _bench_child(["--config", str(config), "--batch", str(batch), "--steps", "2", "--warmup", "1",
                         "--no-cpu-baseline", "--ntt-polys", "0", "--pcie-pairs", "2"])
    assert line["config"]["baseline_config"] == config and line["config"]["ciphertexts_per_gpu"] == batch
    assert line["verified_vs_oracle"] is True and line["verified_items"] == list(range(batch))  # small batch: every item
    assert line["pcie_inclusive"]["matches_device_path"] is True and line["pcie_inclusive"]["units"] == 2
    assert line["unit"] == {4: "rotate_vector/s", 5: "pipeline/s"}[config]
    assert line["roofline"]["kernel"].startswith("ntt_") and 0 < line["roofline"]["frac"] < 1
    assert line["pipeline_roofline"]["compulsory_bytes_per_unit"] > 0 and len(line["kernels"]) >= 3


@pytest.mark.parametrize("config,batch,mode", [(4, 1024, "parity"), (5, 256, "parity"), (3, 1024, "strict")])
def test_bench_full_size_batches_verify_256_items(config, batch, mode):
    """the BASELINE batch sizes of the side configs (config 4: 1024 ciphertexts per GPU, config 5:
    256) and the STRICT mode of config 3 go through the bench child with the wide self-check: at least 256 items -- 0, B/2,
    B-1, the edges of every arena chunk, seeded random picks -- word for word against the oracle (evaluator.h:1201-1211,
    evaluator.cpp:235-272,772-827,996-1036; STRICT: SURVEY B.6), the PCIe-inclusive block against the device path, and the
    roofline carrying the measured arithmetic ceiling next to the HBM fraction."""
    line = _bench_child(["--config", str(config), "--batch", str(batch), "--mode", mode, "--steps", "2", "--warmup", "1",
                         "--no-cpu-baseline", "--ntt-polys", "0", "--pcie-pairs", "8"])
    assert line["config"]["baseline_config"] == config and line["config"]["ciphertexts_per_gpu"] == batch
    assert line["config"]["mode"] == mode.upper()
    assert line["verified_vs_oracle"] is True and line["verified_count"] == len(line["verified_items"]) >= 256
    items = line["verified_items"]
    assert {0, batch // 2, batch - 1} <= set(items) and items == sorted(set(items)) and items[-1] == batch - 1
    for c in line["verified_chunk_sizes"]:  # every chunk edge is among the checked items
        assert all({e - 1, e} <= set(items) for e in range(c, batch, c))
    assert line["pcie_inclusive"]["matches_device_path"] is True and line["pcie_inclusive"]["value"] > 0
    roof = line["roofline"]
    assert roof["bound"] == ("hbm" if config == 4 else "valu") and 0 < roof["frac"] < 1
    assert roof["valu_ceiling"]["butterflies_per_s"] > 1e11 and roof["alu_ceiling_frac"] > 0


@pytest.mark.skipif("SEALHIP_TEST_SMALL_ARENA_COUNT" not in os.environ, reason="child of test_bench_shapes_with_a_small_arena")
def test_small_arena_child(sealhip):
    assert os.environ.get("SEALHIP_WORKSPACE_MB") == "64"
    count = int(os.environ["SEALHIP_TEST_SMALL_ARENA_COUNT"])
    test_cfg3_bench_launch_shapes_vs_golden_and_oracle(sealhip, count)
    # cfg4 rotate at 7 ciphertexts: Galois scratch at the arena front + chunked key switch behind it
    row = [r for r in DIG["end_to_end"] if r["cfg"] == 4][0]
    inp = synth.end_to_end_inputs(row)
    n, k = inp["n"], inp["k"]
    ctx = sealhip.Context(row["scheme"], inp["logn"], inp["kmods"], row["nsp"], row["t"])
    ev = sealhip.Evaluator(ctx)
    gk = sealhip.KSwitchKeys(ctx, inp["gk"])
    c = ctx.upload(np.stack([inp["a"]] * count))
    ev.rotate_vector_inplace(c, k, count, 1, {ctx.galois_elt_from_step(1): gk})
    got = c.download((count, 2, k, n))
    for i in range(count):
        assert h(got[i]) == row["digests"]["rotate"], i


def test_ntt_handoff_failure_surfaces_at_every_host_visible_point(sealhip):
    """The forward NTT's sibling hand-off has a bounded wait; when it times out the launch's rows are invalid and a
    sticky flag is raised. sealhip_debug_ntt_handoff withholds the hand-off signal and cuts the wait to one poll, which
    drives exactly that path: every entry point that makes results host-visible must then fail (E_UNEXPECTED ->
    RuntimeError) instead of returning the rows with S_OK, once per failure, and the engine must work again afterwards."""
    logn, n = 15, 1 << 15
    kmods = O.coeff_modulus_create(n, [55] * 3)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, kmods, 1, 786433)
    k = 2
    rng = np.random.default_rng(7)
    x = rand_rows(rng, kmods[:k] * 2, n).reshape(2, k, n)
    ctx.set_parms_id(k, (1, 2, 3, 4))
    info = sealhip.CiphertextInfo()
    info.parms_id[:] = (1, 2, 3, 4)
    info.size, info.coeff_modulus_size, info.poly_modulus_degree, info.scale = 2, k, n, 1.0

    def fail_once(fn):
        d = ctx.upload(x)
        ctx.debug_ntt_handoff(spin_limit=1, suppress_signal=True)
        try:
            ctx.ntt_negacyclic_harvey_lazy(d, 2, k)  # every wave's wait gives up after one poll
            with pytest.raises(RuntimeError, match="sibling workgroup wait timed out"):
                fn(d)
        finally:
            ctx.debug_ntt_handoff(0, False)
        return d

    out = np.empty(x.size, dtype=np.uint64)
    L_ = sealhip.lib()
    fail_once(lambda d: ctx.synchronize())
    fail_once(lambda d: sealhip._check(L_.sealhip_memcpy_d2h(ctx.handle, out.ctypes.data, d.ptr, out.size * 8)))
    fail_once(lambda d: ctx.save_ciphertext(info, d))
    fail_once(lambda d: ctx.is_data_valid_for(d, 2, k, 1))
    fail_once(lambda d: ctx.is_transparent(d, 2, k, 1))
    fail_once(lambda d: ctx.profile_fetch())
    ctx.synchronize()  # the flag was consumed by the failing call: nothing is pending
    # and the engine is intact: the same transform, hand-off restored, is bit-exact again
    d = ctx.upload(x)
    ctx.ntt_negacyclic_harvey_lazy(d, 2, k)
    got = d.download(x.shape)
    tabs = [O.Tables(logn, p) for p in kmods[:k]]
    for j in range(2):
        for i in range(k):
            e = x[j, i].copy()
            L.ref_ntt_forward_lazy(O.ptr(e), C.byref(tabs[i].t), 0)
            assert np.array_equal(got[j, i], e)


def test_exact_ntt_variants_still_match_the_golden_digests():
    """The lazy-sum inverse and the last-layer shortcut of the forward transform are switched off with
    SEALHIP_NTT_EXACT_INV / SEALHIP_NTT_EXACT_FWD, the canonical transform's approximate-quotient schedule (round 3) with
    SEALHIP_NTT_CANON_EXACT (read once per process, hence the child process): the exact kernels
    must reproduce the same golden digests of the compiled reference as the default ones do in this process, and the NTT
    entries' matrix over the documented operand ranges must pass as it does here."""
    import subprocess
    import sys

    env = dict(os.environ, SEALHIP_NTT_EXACT_INV="1", SEALHIP_NTT_EXACT_FWD="1", SEALHIP_NTT_CANON_EXACT="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "end_to_end_golden_digests or ntt_golden_digests or ntt_all_variants or ntt_entries_over_the_documented_range or ntt_entries_on_key_and_bsk or transform_to_and_from_ntt"],
                       env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode("utf-8", "replace")[-400:]
    assert r.returncode == 0 and " passed" in tail, tail


def test_integer_instances_instead_of_fp64_still_match_the_golden_digests():
    """SEALHIP_NTT_NO_FP64 is the last switch of this kind the SHIPPING library reads: integer instances for primes below
    2^50 (configs 2, 4, 5), next to the SEALHIP_NTT_EXACT_* / _CANON_EXACT switches of the test above, which run the
    reference's own sequences. Child process (read once): the golden digests of the compiled reference must come out as
    they do here. (Round 4: the A/B knobs that restored REPLACED forms -- SEALHIP_LIFT_TOP_OFF, SEALHIP_KS_MODDOWN_UNFUSED,
    SEALHIP_KS_MODDOWN_STORE_UNFUSED, SEALHIP_TENSOR_UNFUSED, SEALHIP_NTT_WHOLE_ROW, SEALHIP_NTT_TWO_PASS, SEALHIP_RNS_UNFUSED
    -- are gone from it: the first five were deleted with the measurement-only build that read them, the last two with the
    two-launch transform. The forms they restored are still reached by PARAMETERS -- primes of 59+ bits, operand sizes
    other than 2, nsp > 1, N = 2^16 and N = 2^14, STRICT mode, k > 16 -- and the tests with such parameters cover them.) The NTT
    entries' matrix over the documented operand ranges runs here too: its FP64-class rows then take the integer instances."""
    import subprocess
    import sys

    env = dict(os.environ, SEALHIP_NTT_NO_FP64="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider",
                        "-k", "end_to_end_golden_digests or ntt_golden_digests or bench_launch_shapes or cfg4_rotate_large_batch or ntt_entries_over_the_documented_range or ntt_entries_on_key_and_bsk or transform_to_and_from_ntt"],
                       env=env, cwd=os.path.dirname(HERE), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    tail = r.stdout.decode("utf-8", "replace")[-400:]
    assert r.returncode == 0 and " passed" in tail, tail


# ------------------------------------------------------------------ the four NTT entries over their documented operand ranges
# include/sealhip.h: forward inputs below 4p, inverse inputs below 2p; `_lazy` = the reference's words (wrapped ones included),
# canonical = the residues those words reduce to. launch_half / launch_half_inv pick an instance per prime class; every instance
# is exact only inside a bound stated on that input range. The classes at 2^14..2^16 come from the predicates themselves
# (tests/golden/ntt_instance_classes.json, pinned to csrc/ntt_bounds.hpp by tests/test_host.py).
CLASSES = json.load(open(os.path.join(HERE, "golden", "ntt_instance_classes.json")))
MATRIX_FIXED_BITS = (30, 49, 55, 59, 60, 61)
_MATH = {}


def _math(logn, p):
    if (logn, p) not in _MATH:
        if len(_MATH) >= 4:  # (the tables of a 2^16 prime are Python integers: keep a few)
            _MATH.clear()
        _MATH[(logn, p)] = O.MathNtt(logn, p)
    return _MATH[(logn, p)]


def ntt_matrix_classes(logn):
    """[(label, three primes)] for one ring size: fixed sizes below 2^14; from 2^14 the three largest primes each predicate
    admits and the three smallest it refuses (below 2^61), a 30-bit class, the largest 60- and 61-bit primes, and the largest
    primes one bit above the canonical forward's limit (its predicate is stated in bits: the worst a one-bit slip admits)."""
    top = lambda bits: O.ntt_primes_around((1 << bits) - 1, logn)[0]
    if logn < 14:
        return [("%dbit" % b, top(b)) for b in MATRIX_FIXED_BITS]
    c = CLASSES[str(logn)]
    out = []
    for key in ("fp64", "fwd_canon", "fwd_canon_small_quot", "fwd_dense", "inv_lazy", "inv_dense"):
        below, above = O.ntt_primes_around(c[key], logn)
        out.append((key + "_max", below))
        if max(above) < 1 << 61:
            out.append((key + "_min_refused", above))
    out += [("30bit", top(30)), ("60bit_max", top(60)), ("61bit_max", top(61)),
            ("fwd_canon_next_bit_max", top(c["fwd_canon"].bit_length() + 1))]
    seen, uniq = set(), []
    for label, ps in out:
        if tuple(ps) not in seen:
            seen.add(tuple(ps))
            uniq.append((label, ps))
    return uniq


def _special_prime(logn, avoid):
    return next(p for p in O.ntt_primes_around((1 << 40) - 1, logn)[0] if p not in avoid)


def ntt_range_patterns(rng, mods, n, mult, count=7):
    """count polynomials x len(mods) rows over [0, mult p): residues; every word mult p - 1; alternating 0 / mult p - 1;
    half 0, half mult p - 1; words across [(mult - 1) p, mult p); random over [0, mult p); and 0, p - 1, p, 2p, 3p (those below
    mult p) and mult p - 1 planted at 0, N/4, N/2, N - 1 (and next to them) on a random background. Further polynomials
    repeat the kinds with fresh random words."""
    x = np.zeros((count, len(mods), n), dtype=np.uint64)
    for c in range(count):
        kind = c % 7 if count > 1 else 6
        for i, p in enumerate(mods):
            top = mult * p - 1
            if kind == 0:
                x[c, i] = rng.integers(0, p, n, dtype=np.uint64)
            elif kind == 1:
                x[c, i] = top
            elif kind == 2:
                x[c, i, ::2] = top
            elif kind == 3:
                x[c, i, n // 2:] = top
            elif kind == 4:
                x[c, i] = rng.integers((mult - 1) * p, mult * p, n, dtype=np.uint64)
            else:
                x[c, i] = rng.integers(0, mult * p, n, dtype=np.uint64)
            if kind == 6:
                vals = [v for v in (0, p - 1, p, 2 * p, 3 * p) if v < top] + [top]
                spots = [0, 1, n // 4, n // 4 + 1, n // 2, n // 2 + 1, n - 2, n - 1]
                for j, s in enumerate(spots):
                    x[c, i, s] = vals[(j + i) % len(vals)]
    return x


def _oracle_rows(x, tabs, fn):
    e = x.copy()
    for c in range(e.shape[0]):
        for i, t in enumerate(tabs):
            fn(O.ptr(e[c, i]), C.byref(t))
    return e


_INV_CACHE = {}


def _oracle_inverse(x, tabs, fn):
    """the inverse words do not depend on the mode: one oracle run per input for PARITY and STRICT"""
    key = (id(fn), tuple(int(t.mod.value) for t in tabs), x.shape, hash(x.tobytes()))
    if key not in _INV_CACHE:
        if len(_INV_CACHE) > 16:
            _INV_CACHE.clear()
        _INV_CACHE[key] = _oracle_rows(x, tabs, fn)
    return _INV_CACHE[key]


_MATH_ROWS = {}


def _math_row(logn, p, row, inverse):
    """the math reference of one row, computed once for PARITY and STRICT"""
    key = (logn, p, inverse, hash(row.tobytes()))
    if key not in _MATH_ROWS:
        if len(_MATH_ROWS) >= 16:
            _MATH_ROWS.clear()
        M = _math(logn, p)
        _MATH_ROWS[key] = np.array(M.inverse(row) if inverse else M.forward(row), dtype=np.uint64)
    return _MATH_ROWS[key]


FWD_LAZY = {0: lambda r, t: L.ref_ntt_forward_lazy(r, t, 0), 1: lambda r, t: L.ref_ntt_forward_lazy(r, t, 1)}
FWD = {0: lambda r, t: L.ref_ntt_forward(r, t, 0), 1: lambda r, t: L.ref_ntt_forward(r, t, 1)}
INV_LAZY, INV = L.ref_ntt_inverse_lazy, L.ref_ntt_inverse


def check_four_entries(sealhip, ctx, mods, tabs, k, base, strict, x_fwd, x_inv, what, math_rows=()):
    """The four entries on x_fwd ([0, 4p)) / x_inv ([0, 2p)), count = x.shape[0], word for word against the oracle
    (PARITY: the reference's words; STRICT: Harvey's corrected forward sequence, i.e. the mathematics). `math_rows`:
    (poly, row) pairs whose canonical results must also equal the math reference."""
    count = x_fwd.shape[0]
    mcol = np.array(mods, dtype=np.uint64).reshape(1, -1, 1)
    s = 1 if strict else 0
    results = {}
    for name, fn, x, ref in (("fwd_lazy", ctx.ntt_negacyclic_harvey_lazy, x_fwd, FWD_LAZY[s]),
                             ("fwd", ctx.ntt_negacyclic_harvey, x_fwd, FWD[s]),
                             ("inv_lazy", ctx.inverse_ntt_negacyclic_harvey_lazy, x_inv, INV_LAZY),
                             ("inv", ctx.inverse_ntt_negacyclic_harvey, x_inv, INV)):
        d = ctx.upload(x)
        fn(d, count, k, base)
        got = d.download(x.shape)
        exp = _oracle_inverse(x, tabs, ref) if name.startswith("inv") else _oracle_rows(x, tabs, ref)
        bad = np.argwhere((got != exp).any(axis=2))
        assert bad.size == 0, (what, name, "strict" if strict else "parity", "(poly, row) differing:", bad[:8].tolist())
        results[name] = got
    if strict:  # the lazy words lie in the documented output ranges and reduce to the canonical results
        assert (results["fwd_lazy"] < 4 * mcol).all() and (results["inv_lazy"] < 2 * mcol).all(), what
        assert np.array_equal(results["fwd_lazy"] % mcol, results["fwd"]), what
        assert np.array_equal(results["inv_lazy"] % mcol, results["inv"]), what
    logn = int(x_fwd.shape[2]).bit_length() - 1
    for c, i in math_rows:
        assert np.array_equal(_math_row(logn, mods[i], x_fwd[c, i], False), results["fwd"][c, i]), (what, "math fwd", c, i)
        assert np.array_equal(_math_row(logn, mods[i], x_inv[c, i], True), results["inv"][c, i]), (what, "math inv", c, i)
    return results


def _fwd_cannot_wrap(logn, p):
    """the reference's forward words on inputs below 4p stay below (4 + 2 log n) p (ForwardLazy adds 2p per layer)"""
    return (4 + 2 * logn) * p < 1 << 64


@pytest.mark.parametrize("logn", [3, 4, 8, 12, 13, 14, 15, 16])
def test_ntt_entries_over_the_documented_range_per_instance_class(sealhip, logn):
    """Every NTT entry on BASE_Q, PARITY and STRICT, for each prime class of the ring size (context: three primes of the class
    and a special prime), on inputs over the whole documented operand range with the extremes planted; count 7 (21 rows:
    the eight XCD row chunks are not filled evenly) and count 1. PARITY: every word equals the oracle's, wrapped ones included,
    and where the reference cannot wrap the canonical results of one row per class equal the math reference. STRICT: the
    `_lazy` forward is Harvey's sequence word for word, the canonical results are the mathematics for every class -- 60-61
    bits included, where PARITY wraps -- and the lazy words lie in [0, 4p) / [0, 2p)."""
    n = 1 << logn
    rng = np.random.default_rng(4000 + logn)
    for label, mods in ntt_matrix_classes(logn):
        kmods = list(mods) + [_special_prime(logn, mods)]
        tabs = [O.Tables(logn, p) for p in mods]
        traw = [t.t for t in tabs]
        for count in (7, 1):
            x_fwd = ntt_range_patterns(rng, mods, n, 4, count)
            x_inv = ntt_range_patterns(rng, mods, n, 2, count)
            for strict in (False, True):
                ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0,
                                      mode=sealhip.MODE_STRICT if strict else sealhip.MODE_PARITY)
                math_rows = ()
                if count == 1 and (strict or all(_fwd_cannot_wrap(logn, p) for p in mods)):
                    math_rows = [(0, 0)]
                check_four_entries(sealhip, ctx, mods, traw, 3, sealhip.BASE_Q, strict, x_fwd, x_inv,
                                   "logn=%d %s %s count=%d" % (logn, label, [p.bit_length() for p in mods], count), math_rows)
    if logn == 15:  # an odd count of 37 polynomials (111 rows) at the canonical forward's boundary class
        label, mods = next(c for c in ntt_matrix_classes(logn) if c[0] == "fwd_canon_max")
        ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, list(mods) + [_special_prime(logn, mods)], 1, 0)
        tabs = [O.Tables(logn, p) for p in mods]
        check_four_entries(sealhip, ctx, mods, [t.t for t in tabs], 3, sealhip.BASE_Q, False,
                           ntt_range_patterns(rng, mods, n, 4, 37), ntt_range_patterns(rng, mods, n, 2, 37), "count=37")


@pytest.mark.parametrize("logn", [14, 15, 16])
@pytest.mark.parametrize("strict", [False, True], ids=["parity", "strict"])
def test_ntt_entries_on_key_and_bsk_bases_and_mixed_launches(sealhip, logn, strict):
    """The four entries on BASE_KEY (every key prime, the special one included) and BASE_BSK (the 60-bit Bsk rows of a BFV
    context) against the oracle's key / Bsk tables, and on BASE_Q of a context whose rows mix an FP64-class prime, a
    sparse-lazy-class prime and a 60-bit prime: one launch is split into the floating-point rows and the integer rows
    (split_by_fp), each row checked on its own. Inputs over [0, 4p) / [0, 2p), extremes planted, odd counts."""
    n = 1 << logn
    mode = sealhip.MODE_STRICT if strict else sealhip.MODE_PARITY
    rng = np.random.default_rng(5000 + logn + 7 * strict)
    top = lambda bits: O.ntt_primes_around((1 << bits) - 1, logn)[0][0]
    kmods = [top(49), top(55), top(60), top(61)]
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0, mode=mode)
    tabs = [O.Tables(logn, p) for p in kmods]
    traw = [t.t for t in tabs]
    # BASE_Q: FP64 + sparse + 60-bit rows in one launch
    check_four_entries(sealhip, ctx, kmods[:3], traw[:3], 3, sealhip.BASE_Q, strict, ntt_range_patterns(rng, kmods[:3], n, 4, 5),
                       ntt_range_patterns(rng, kmods[:3], n, 2, 5), "mixed BASE_Q", math_rows=[(4, 0), (4, 1)] if strict else [(4, 0)])
    # BASE_KEY: all four key primes, at the top level and one below (the special prime stays in the base)
    for k in (3, 2):
        rows = kmods[:k] + kmods[3:]
        check_four_entries(sealhip, ctx, rows, traw[:k] + traw[3:], k, sealhip.BASE_KEY, strict,
                           ntt_range_patterns(rng, rows, n, 4, 3), ntt_range_patterns(rng, rows, n, 2, 3), "BASE_KEY k=%d" % k)
    # BASE_BSK of a BFV context: the 60-bit Bsk primes (PARITY wraps there; the oracle's words are the yardstick)
    bmods = O.coeff_modulus_create(n, [50, 50, 51])
    bctx = sealhip.Context(sealhip.SCHEME_BFV, logn, bmods, 1, 65537, mode=mode)
    ref = O.RefContext(1, logn, bmods, 1, 65537, mode=1 if strict else 0)
    k = 2
    rt = ref.rns_tool(k)
    nb = bctx.bsk_size(k)
    bsk = [int(rt.contents.Bsk[i].value) for i in range(nb)]
    check_four_entries(sealhip, bctx, bsk, [rt.contents.Bsk_ntt[i] for i in range(nb)], k, sealhip.BASE_BSK, strict,
                       ntt_range_patterns(rng, bsk, n, 4, 3), ntt_range_patterns(rng, bsk, n, 2, 3), "BASE_BSK")


@pytest.mark.parametrize("logn,strict", [(12, False), (14, True), (15, False), (16, False)])
def test_transform_to_and_from_ntt(sealhip, logn, strict):
    """Evaluator::transform_to_ntt_inplace / transform_from_ntt_inplace (evaluator.cpp:1746-1839): ciphertexts of size 2 and 3,
    an odd count, at the top level and one below it; polynomial by polynomial the same words as the canonical entries and as
    the oracle's transforms."""
    n = 1 << logn
    kmods = O.coeff_modulus_create(n, [49, 55, 58, 60])
    mode = sealhip.MODE_STRICT if strict else sealhip.MODE_PARITY
    ctx = sealhip.Context(sealhip.SCHEME_CKKS, logn, kmods, 1, 0, mode=mode)
    ev = sealhip.Evaluator(ctx)
    tabs = [O.Tables(logn, p) for p in kmods]
    rng = np.random.default_rng(6000 + logn)
    count = 3
    for k in (3, 2):
        for size in (2, 3):
            x = ntt_range_patterns(rng, kmods[:k], n, 1, count * size).reshape(count, size, k, n)
            d = ctx.upload(x)
            ev.transform_to_ntt_inplace(d, size, k, count)
            fwd = d.download(x.shape)
            e = ctx.upload(x)
            ctx.ntt_negacyclic_harvey(e, count * size, k)
            assert np.array_equal(fwd, e.download(x.shape)), (k, size)
            exp = _oracle_rows(x.reshape(count * size, k, n), [t.t for t in tabs[:k]], FWD[1 if strict else 0])
            assert np.array_equal(fwd.reshape(exp.shape), exp), (k, size)
            ev.transform_from_ntt_inplace(d, size, k, count)
            back = d.download(x.shape)
            ctx.inverse_ntt_negacyclic_harvey(e, count * size, k)
            assert np.array_equal(back, e.download(x.shape)), (k, size)
            assert np.array_equal(back, x), (k, size)


def _empty_batch_calls(S, ctx, scheme, b, i32, n_key, k):
    """(name, thunk) for every entry of include/sealhip.h that takes a count, with count = 0 and valid arguments"""
    Lb = S.lib()
    h, n = ctx.handle, ctx.n
    key = S.KSwitchKeys(ctx, np.zeros((ctx.kswitch_digits(k), 2, n_key, n), dtype=np.uint64))
    keys = (C.c_void_p * 1)(key.handle)
    elt = ctx.galois_elt_from_step(1)
    elts = (C.c_uint32 * 1)(elt)
    o = b + 8 * (4 * n_key * n)  # outputs: the second half of the buffer (no entry sees an aliased operand)
    host = np.zeros(8, dtype=np.uint64)
    hp = (C.c_void_p * 1)(host.ctypes.data)
    flags = np.zeros(1, dtype=np.uint8)
    bfv, ckks = scheme == S.SCHEME_BFV, scheme == S.SCHEME_CKKS
    calls = []
    bases = [S.BASE_Q, S.BASE_KEY] + ([S.BASE_BSK] if bfv else [])
    for base in bases:
        for name in ("ntt_negacyclic_harvey_lazy", "ntt_negacyclic_harvey", "inverse_ntt_negacyclic_harvey_lazy",
                     "inverse_ntt_negacyclic_harvey"):
            calls.append(("%s base=%d" % (name, base), lambda f=getattr(Lb, "sealhip_" + name), base=base: f(h, b, 0, k, base)))
        calls += [
            ("dyadic_product base=%d" % base, lambda base=base: Lb.sealhip_dyadic_product_coeffmod(h, b, b, 0, k, base, o)),
            ("multiply_poly_scalar base=%d" % base, lambda base=base: Lb.sealhip_multiply_poly_scalar_coeffmod(h, b, 0, k, base, 3, o)),
            ("add_poly base=%d" % base, lambda base=base: Lb.sealhip_add_poly_coeffmod(h, b, b, 0, k, base, o)),
            ("sub_poly base=%d" % base, lambda base=base: Lb.sealhip_sub_poly_coeffmod(h, b, b, 0, k, base, o)),
            ("negate_poly base=%d" % base, lambda base=base: Lb.sealhip_negate_poly_coeffmod(h, b, 0, k, base, o)),
            ("modulo_poly_coeffs_63 base=%d" % base, lambda base=base: Lb.sealhip_modulo_poly_coeffs_63(h, b, 0, k, base, o)),
        ]
    E = Lb
    calls += [
        ("transform_to_ntt", lambda: E.sealhip_evaluator_transform_to_ntt(h, k, b, 2, 0)),
        ("transform_from_ntt", lambda: E.sealhip_evaluator_transform_from_ntt(h, k, b, 2, 0)),
        ("apply_galois", lambda: E.sealhip_apply_galois(h, b, 0, k, elt, o)),
        ("apply_galois_ntt", lambda: E.sealhip_apply_galois_ntt(h, b, 0, k, elt, o)),
        ("modup_rns", lambda: E.sealhip_modup_rns(h, k, 0, b, 0)),
        ("rescale_special_rns_inplace", lambda: E.sealhip_rescale_special_rns_inplace(h, k, b, 0)),
        ("switch_key_inplace", lambda: E.sealhip_switch_key_inplace(h, k, b, o, 0, key.handle)),
        ("switch_key_partial", lambda: E.sealhip_switch_key_partial(h, k, b, 0, key.handle, 0, 1, o)),
        ("switch_key_finish", lambda: E.sealhip_switch_key_finish(h, k, b, o, 0, 1)),
        ("multiply", lambda: E.sealhip_evaluator_multiply(h, k, b, 2, b, 2, 0, o)),
        ("square", lambda: E.sealhip_evaluator_square(h, k, b, 2, 0, o)),
        ("relinearize", lambda: E.sealhip_evaluator_relinearize(h, k, b, 3, 0, keys, 1)),
        ("mod_switch_to_next", lambda: E.sealhip_evaluator_mod_switch_to_next(h, k, b, 2, 0, o)),
        ("mod_switch_to_next_strided", lambda: E.sealhip_evaluator_mod_switch_to_next_strided(h, k, b, 2, 2 * k * n, 0, o)),
        ("apply_galois (evaluator)", lambda: E.sealhip_evaluator_apply_galois(h, k, b, 0, elt, key.handle)),
        ("rotate_vector", lambda: E.sealhip_evaluator_rotate_vector(h, k, b, 0, 1, elts, keys, 1)),
        ("multiply_host", lambda: E.sealhip_evaluator_multiply_host(h, k, hp, 2, hp, 2, 0, hp, keys, 1)),
        ("relinearize_host", lambda: E.sealhip_evaluator_relinearize_host(h, k, hp, 3, 0, keys, 1)),
        ("rotate_vector_host", lambda: E.sealhip_evaluator_rotate_vector_host(h, k, hp, 0, 1, elts, keys, 1)),
        ("mod_switch_to_next_host", lambda: E.sealhip_evaluator_mod_switch_to_next_host(h, k, hp, 2, 0, hp)),
        ("negate", lambda: E.sealhip_evaluator_negate(h, k, b, 2, 0, o)),
        ("add", lambda: E.sealhip_evaluator_add(h, k, b, 2, b, 2, 0, o)),
        ("sub", lambda: E.sealhip_evaluator_sub(h, k, b, 2, b, 2, 0, o)),
        ("multiply_plain_ntt", lambda: E.sealhip_evaluator_multiply_plain_ntt(h, k, b, 2, 0, o, 0)),
        ("add_plain", lambda: E.sealhip_evaluator_add_plain(h, k, b, 2, 0, o, k * n if ckks else n, 0)),
        ("is_transparent", lambda: E.sealhip_is_transparent(h, k, b, 2, 0, flags.ctypes.data)),
        ("is_data_valid_for", lambda: E.sealhip_is_data_valid_for(h, k, b, 2, 0, flags.ctypes.data)),
        ("ciphertext_resize", lambda: E.sealhip_ciphertext_resize(h, k, b, 2, o, 3, 0)),
        ("dot_product_ct_sk", lambda: E.sealhip_decryptor_dot_product_ct_sk(h, k, b, 2, 0, b, 1, o)),
        ("encrypt_zero_symmetric", lambda: E.sealhip_encrypt_zero_symmetric(h, k, 1, b, i32, b, 0, o)),
        ("encrypt_zero_asymmetric", lambda: E.sealhip_encrypt_zero_asymmetric(h, k, 1, b, i32, i32, 0, o)),
    ]
    if bfv:
        calls += [
            ("multiply_many", lambda: E.sealhip_evaluator_multiply_many(h, k, (C.c_void_p * 2)(b, b), 2, 0, keys, 1, o)),
            ("exponentiate", lambda: E.sealhip_evaluator_exponentiate(h, k, b, 3, 0, keys, 1, o)),
            ("multiply_plain", lambda: E.sealhip_evaluator_multiply_plain(h, k, b, 2, 0, o, 0)),
            ("fastbconv_m_tilde", lambda: E.sealhip_fastbconv_m_tilde(h, k, b, 0, o)),
            ("sm_mrq", lambda: E.sealhip_sm_mrq(h, k, b, 0, o)),
            ("fast_floor", lambda: E.sealhip_fast_floor(h, k, b, 0, o)),
            ("fastbconv_sk", lambda: E.sealhip_fastbconv_sk(h, k, b, 0, o)),
            ("divide_and_round_q_last_inplace", lambda: E.sealhip_divide_and_round_q_last_inplace(h, k, b, 0)),
            ("divide_and_round_q_last_ntt_inplace", lambda: E.sealhip_divide_and_round_q_last_ntt_inplace(h, k, b, 0)),
            ("decrypt_scale_and_round", lambda: E.sealhip_decrypt_scale_and_round(h, k, b, 0, o)),
            ("multiply_add_plain_with_scaling_variant",
             lambda: E.sealhip_multiply_add_plain_with_scaling_variant(h, k, b, n, o, 2, 0, 0)),
            ("batch_encode", lambda: E.sealhip_batch_encode(h, b, n, 0, o)),
            ("batch_decode", lambda: E.sealhip_batch_decode(h, b, 0, o)),
            ("batch_encode_int64", lambda: E.sealhip_batch_encode_int64(h, b, n, 0, o)),
            ("batch_decode_int64", lambda: E.sealhip_batch_decode_int64(h, b, 0, o)),
        ]
    if ckks:
        calls += [
            ("rescale_to_next", lambda: E.sealhip_evaluator_rescale_to_next(h, k, b, 2, 0, o)),
            ("rescale_to_next_strided", lambda: E.sealhip_evaluator_rescale_to_next_strided(h, k, b, 2, 2 * k * n, 0, o)),
            ("rescale_to_next_host", lambda: E.sealhip_evaluator_rescale_to_next_host(h, k, hp, 2, 0, hp)),
            ("ckks_encode", lambda: E.sealhip_ckks_encode(h, k, b, 4, 0, 2.0 ** 30, o)),
            ("ckks_decode", lambda: E.sealhip_ckks_decode(h, k, b, 0, 2.0 ** 30, o)),
            ("ckks_encode_value", lambda: E.sealhip_ckks_encode_value(h, k, 1.5, 2.0 ** 30, 0, o)),
            ("ckks_encode_int64", lambda: E.sealhip_ckks_encode_int64(h, k, 7, 0, o)),
        ]
    return calls, (key, keys, host, hp, flags)


@pytest.mark.parametrize("logn", [10, 14, 15, 16])
@pytest.mark.parametrize("strict", [False, True], ids=["parity", "strict"])
def test_every_counted_entry_accepts_an_empty_batch(sealhip, logn, strict):
    """count = 0 is a no-op on every entry that takes a count, like the reference's loops over empty ranges -- at the ring
    sizes of the single-pass NTT kernels too, where launch_ntt once fell through to the tiled planner and returned
    COR_E_INVALIDOPERATION. Each call returns S_OK and the sentinel-filled buffer it is handed stays unchanged.
    (2^10: the tiled kernels' sizes, the control.)"""
    n = 1 << logn
    mode = sealhip.MODE_STRICT if strict else sealhip.MODE_PARITY
    failures = []
    for scheme, bits, t in ((sealhip.SCHEME_BFV, [50, 50, 51], 786433), (sealhip.SCHEME_CKKS, [50, 40, 51], 0)):
        kmods = O.coeff_modulus_create(n, bits)
        ctx = sealhip.Context(scheme, logn, kmods, 1, t, mode=mode)
        k = len(kmods) - 1
        words = 8 * 4 * len(kmods) * n
        sentinel = (np.arange(words, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1 << 63)
        buf = ctx.upload(sentinel)
        i32 = ctx.upload_i32(np.full(4 * n, -7, dtype=np.int32))
        calls, keep = _empty_batch_calls(sealhip, ctx, scheme, buf.ptr, i32.ptr, len(kmods), k)
        for name, fn in calls:
            rc = fn() & 0xFFFFFFFF
            if rc != 0:
                failures.append((scheme, name, "0x%08x" % rc, sealhip.lib().sealhip_last_error_string().decode()))
        ctx.synchronize()
        assert np.array_equal(buf.download(), sentinel), (scheme, "the buffer changed")
        del keep, calls
    assert not failures, failures


# ---------------------------------------------------------------- BFV multiply / square at every BEHZ plan cell
_BEHZ_GENERIC_LEVELS = range(17, 33)  # the run-time-k instance's levels past the exact range's k = 15 / 16 cells


def _behz_plan_cases():
    """(required coverage, cases by grid context). Required: every (cell, log n) that oracle_lib.bfv_plan_cell reaches on
    the dispatch grid of tests/test_host.py (PARITY); every level 17..32 of the run-time-k instance with (2,2) and with
    square, spread over the rings 2^14..2^16; and each operand shape on both sides of each fork edge the restatement
    derives (gather per shape, fused_tensor for square, defer at 32 / 33), at a ring chosen by the edge level. Each
    requirement is met by its cheapest case."""
    grid = O.bfv_plan_contexts(json.load(open(os.path.join(HERE, "golden", "behz_instance_classes.json"))))
    plans = {}
    for ci, (logn, name, mods, t) in enumerate(grid):
        for k in range(1, O.BFV_PLAN_LEVELS + 1):
            for sa, sb, sq in O.BFV_PLAN_SHAPES:
                plans[ci, k, sa, sb, sq] = O.bfv_multiply_plan(logn, mods, t, k, sa, sb, sq)

    def cost(key):
        ci, k, sa, sb, sq = key
        return ((1 << grid[ci][0]) * k * (sa + sb), key)

    best = {}

    def want(req, key):
        if req not in best or cost(key) < cost(best[req]):
            best[req] = key

    edges = {}  # (shape, fork) -> the levels where it flips, on the class "58" at t = 786433 of each ring
    for key, plan in plans.items():
        ci, k, sa, sb, sq = key
        logn = grid[ci][0]
        want(("cell", O.bfv_plan_cell(plan, sa, sb), logn), key)
        if k in _BEHZ_GENERIC_LEVELS and (sa, sb) == (2, 2) and logn == 14 + k % 3:
            want(("generic", k, sq), key)
        if grid[ci][1] == "58" and grid[ci][3] == O.BFV_PLAN_T[0] and logn >= 14 and k > 1:
            prev = plans[ci, k - 1, sa, sb, sq]
            for fork in ("gather", "fused_tensor", "defer"):
                if prev[fork] != plan[fork] and logn == 14 + (k - 1) % 3:
                    edges[(sa, sb, sq), fork] = k - 1
                    for kk in (k - 1, k):
                        want(("edge", (sa, sb, sq), fork, kk), (ci, kk, sa, sb, sq))
    assert {f for _, f in edges} == {"gather", "fused_tensor", "defer"}, edges
    cases = {}
    for req, (ci, k, sa, sb, sq) in best.items():
        cases.setdefault(ci, set()).add((k, sa, sb, sq))
    return set(best), best, plans, [(grid[ci], sorted(v)) for ci, v in sorted(cases.items())]


def _behz_operand(rng, mods, size, n, pattern):
    """one ciphertext of `size` polynomials: 0 every word q - 1, 1 q - 1 alternating with 0, 2 upper half q - 1 (lower
    half 0), 3 zero, 4 random"""
    if pattern == 4:
        return _rand_ct(rng, mods, size, n, 1)[0]
    top = np.stack([np.full((size, n), p - 1, dtype=np.uint64) for p in mods], axis=1)
    if pattern == 1:
        top[:, :, 1::2] = 0
    elif pattern == 2:
        top[:, :, : n // 2] = 0
    elif pattern == 3:
        top[:] = 0
    return top


# item patterns (a, b): the worst case, two independent random operands, then one of the mixed pairs
_BEHZ_MIXED = ((1, 2), (2, 1), (1, 4), (3, 0), (2, 4), (4, 1))


def _behz_run(sealhip, ctx, ref, logn, mods, k, sa, sb, sq, items, seed, pool):
    n = 1 << logn
    rng = np.random.default_rng(seed)
    count = len(items)
    a = np.stack([_behz_operand(rng, mods[:k], sa, n, pa) for pa, _ in items])
    b = np.stack([_behz_operand(rng, mods[:k], sb, n, pb) for _, pb in items])
    dest = sa + sb - 1
    out = ctx.alloc(count * dest * k * n)
    ev = sealhip.Evaluator(ctx)
    if sq:
        ev.square(ctx.upload(a), 2, k, count, out)
    else:
        ev.multiply(ctx.upload(a), sa, ctx.upload(b), sb, k, count, out)
    got = out.download((count, dest, k, n))
    ref.rns_tool(k)  # built here, once: the oracle calls below run on several threads and only read the context

    def oracle(i):
        exp = np.zeros((dest, k, n), dtype=np.uint64)
        if sq:
            assert L.ref_bfv_square(C.byref(ref.c), k, O.ptr(a[i]), 2, O.ptr(exp)) == 0
        else:
            assert L.ref_bfv_multiply(C.byref(ref.c), k, O.ptr(a[i]), sa, O.ptr(b[i]), sb, O.ptr(exp)) == 0
        return exp

    return [(got[i], pool.submit(oracle, i), (logn, k, sa, sb, sq, items[i])) for i in range(count)]


def test_bfv_multiply_every_behz_plan_cell(sealhip):
    """BFV multiply / square bit-exact against the oracle at every reachable cell of the dispatch (oracle_lib.bfv_plan_cell:
    lift and floor instance -- exact k = 1..15, run-time k, step-by-step --, |B| = k or k + 1, the lift's top layer,
    deferred_top 0 / 1 / 2, gather, fused tensor product and its approximate-quotient form, square) on EACH ring log n =
    12, 14, 15, 16 where it is reachable; every level 17..32 of the run-time-k instance; and the operand shapes on both
    sides of each fork edge. Each on its cheapest case of the grid of tests/test_host.py (prime classes 50..61 bits and
    the s1 edge primes, t = 786433 and a 59-bit t, levels 1..33 of a 34-prime context). Every case runs three items: all
    words q - 1 in both operands, two independent random operands, and a mixed pair (q - 1 alternating with 0, upper half
    q - 1, zero, random); cases with the lift's top layer run a single worst-case item as well (odd item counts for the
    paired-column grid). The plans the engine reports for the chosen cases must cover the required set before any
    arithmetic is compared: a dispatch change that moves a case off its cell fails as a coverage error."""
    from concurrent.futures import ThreadPoolExecutor

    required, best, plans, cases = _behz_plan_cases()
    grid = O.bfv_plan_contexts(json.load(open(os.path.join(HERE, "golden", "behz_instance_classes.json"))))
    ctxs = {}
    ran = set()
    for req, (ci, k, sa, sb, sq) in sorted(best.items(), key=lambda r: r[1]):
        logn, name, mods, t = grid[ci]
        if ci not in ctxs:
            ctxs = {ci: sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, t)}  # one context alive at a time
        got = ctxs[ci].debug_bfv_multiply_plan(k, sa, sb, sq)
        ran.add(("cell", O.bfv_plan_cell(got, sa, sb), logn))
        if got["floor_kernel"] == O.BEHZ_GENERIC and k in _BEHZ_GENERIC_LEVELS and (sa, sb) == (2, 2) and logn == 14 + k % 3:
            ran.add(("generic", k, sq))
        if req[0] == "edge":
            # the engine's own plan flips the fork between this level and its neighbour on the other side of the edge
            _, shape, fork, kk = req
            lo = min(k for r, (c2, k, *_) in best.items() if r[:3] == req[:3])
            other = ctxs[ci].debug_bfv_multiply_plan(lo + 1 if k == lo else lo, sa, sb, sq)
            if other[fork] != got[fork]:
                ran.add(req)
    del ctxs
    assert ran == required, ("not run", sorted(map(str, required - ran)), "not reachable", sorted(map(str, ran - required)))
    assert {r[2] for r in required if r[0] == "cell"} == {12, 14, 15, 16}
    assert {(r[1], r[2]) for r in required if r[0] == "generic"} == {(k, sq) for k in _BEHZ_GENERIC_LEVELS for sq in (0, 1)}
    seed = 0
    with ThreadPoolExecutor(8) as pool:
        for (logn, name, mods, t), todo in cases:
            ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, t)
            ref = O.RefContext(1, logn, mods, nsp=1, t=t)
            pending = []
            for k, sa, sb, sq in todo:
                seed += 1
                items = [(0, 0), (4, 4), _BEHZ_MIXED[seed % len(_BEHZ_MIXED)]]
                pending += _behz_run(sealhip, ctx, ref, logn, mods, k, sa, sb, sq, items, seed, pool)
                if ctx.debug_bfv_multiply_plan(k, sa, sb, sq)["lift_top"]:
                    pending += _behz_run(sealhip, ctx, ref, logn, mods, k, sa, sb, sq, [(0, 0)], seed, pool)
                if sum(g.nbytes for g, _, _ in pending) > 1 << 29:  # bound the words held for comparison
                    for got, fut, what in pending:
                        assert np.array_equal(got, fut.result()), (name, t) + what
                    pending = []
            for got, fut, what in pending:
                assert np.array_equal(got, fut.result()), (name, t) + what


@pytest.mark.parametrize("logn,bits", [(14, 59), (15, 55)])
def test_bfv_multiply_behz_strict(sealhip, logn, bits):
    """STRICT mode at the exact instances' edges (k = 1, 14, 15), the run-time-k instance (16, 32) and the step-by-step
    kernels (33): (2,2) and square against the oracle, whose STRICT sequence it must match."""
    n = 1 << logn
    mods = O.ntt_primes_below(n, 1 << bits, O.BFV_PLAN_LEVELS + 1)
    t = O.BFV_PLAN_T[1]
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, t, mode=sealhip.MODE_STRICT)
    ref = O.RefContext(1, logn, mods, nsp=1, t=t, mode=1)
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(8) as pool:
        pending = []
        for j, k in enumerate((1, 14, 15, 16, 32, 33)):
            for sq in (False, True):
                items = [(0, 0), (4, 4), _BEHZ_MIXED[j % len(_BEHZ_MIXED)]]
                pending += _behz_run(sealhip, ctx, ref, logn, mods, k, 2, 2, sq, items, 100 * logn + 2 * j + sq, pool)
        for got, fut, what in pending:
            assert np.array_equal(got, fut.result()), what


@pytest.mark.parametrize("k", [16, 33])
def test_transparency_flags_at_generic_and_stepwise_behz_levels(sealhip, k):
    """The transparency sink of multiply and square at the run-time-k floor (k = 16) and the step-by-step floor followed by
    the separate read pass (k = 33, launch_nonzero_words): items whose second polynomials are zero have zero polynomials
    1.. of the product; the flags must equal that pattern and the device reduction sealhip_is_transparent.
    (test_transparency_is_a_flag_output_of_the_operations covers the exact-k levels.)"""
    logn, n, t = 14, 1 << 14, 786433
    mods = O.ntt_primes_below(n, 1 << 50, O.BFV_PLAN_LEVELS + 1)
    ctx = sealhip.Context(sealhip.SCHEME_BFV, logn, mods, 1, t)
    assert ctx.debug_bfv_multiply_plan(k)["floor_kernel"] == (O.BEHZ_GENERIC if k <= 32 else O.BEHZ_STEPWISE)
    ev = sealhip.Evaluator(ctx)
    rng = np.random.default_rng(k)
    count, zero_items = 5, [1, 4]
    a = _rand_ct(rng, mods[:k], 2, n, count)
    b = _rand_ct(rng, mods[:k], 2, n, count)
    for i in zero_items:
        a[i, 1] = 0
        b[i, 1] = 0
    want = [i not in zero_items for i in range(count)]
    flags = ctx.alloc((count + 1) // 2)
    flags.upload(np.full((count + 1) // 2, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64))
    ctx.transparency_sink(flags, count)
    try:
        for op in ("multiply", "square"):
            prod = ctx.alloc(count * 3 * k * n)
            if op == "multiply":
                ev.multiply(ctx.upload(a), 2, ctx.upload(b), 2, k, count, prod)
            else:
                ev.square(ctx.upload(a), 2, k, count, prod)
            got = (flags.download().view(np.uint32)[:count] != 0).tolist()
            assert got == want == [not v for v in ctx.is_transparent(prod, 3, k, count).tolist()], op
    finally:
        ctx.transparency_sink(None, 0)
