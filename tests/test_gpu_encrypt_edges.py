"""The encrypt-side kernels on planted words: rlwe_stage_kernel<0..3>, scaling_variant_kernel and batch_permute_kernel
(rlwe.hip), the four fused encrypt_*_finish_kernels (encrypt.hip), and scaling_variant_fix (engine.hpp) as poly_tables_kernel
calls it. Random operands reach none of the branches that decide these kernels' words, so the operands are built:
  * u = (1, 0, .., 0) and pk_j = NTT(target_j) make u (.) pk_j the chosen polynomial; a secret key NTT(target) a^{-1} does the
    same for a (.) s, whatever the seed expands to (tests/encrypt_edge_ref.py, pinned to the oracle by
    tests/test_encrypt_edges_host.py);
  * the targets put x + half either side of q_last, the rows' subtraction at -1, 0 and +1, and c + lift(e) at 0, p - 1 and
    across p; the plaintexts hold the words whose Barrett quotient estimate is one short, and those where it is exact;
  * the planted coefficients are 0, 1, N - 2, N - 1 and a random one, in the first and the last item of three; every other
    word is random.
Every word of every item is compared with Python integers (no tolerance anywhere), and with the oracle's composition where
the oracle has the RNSTool."""
import ctypes as C

import numpy as np
import pytest

import encrypt_edge_ref as E
import oracle_lib as O
import poly_eval_ref as P
from support import S, session_memo

pytestmark = pytest.mark.gpu

L = O.lib()
PID = (0x5151, 0x6262, 0x7373, 0x8484)
COUNT, FIRST, LAST = 3, 0, 2
SIGNS = (1, -1, 1)  # u = delta for the first and the last item, -delta for the one between


class Session:
    """one modulus chain on both sides, at one ring and one plain modulus (0: CKKS)"""

    def __init__(self, S, name, logn, t, mode=0):
        bits, self.nsp = E.CHAINS[name]
        self.scheme = 1 if t else 2
        self.logn, self.n, self.t = logn, 1 << logn, t
        self.mods = O.coeff_modulus_create(self.n, bits)
        self.n_key = len(self.mods)
        self.k_first = self.n_key - self.nsp
        self.ref = O.RefContext(self.scheme, logn, self.mods, nsp=self.nsp, t=t, mode=mode)
        self.ctx = S.Context(self.scheme, logn, self.mods, self.nsp, t, mode=mode)
        for k in range(1, self.n_key + 1):
            self.ctx.set_parms_id(k, (PID[0] + k,) + PID[1:])
        self.ev = S.Evaluator(self.ctx)
        self.rng = np.random.default_rng(1000 * logn + len(name) + t % 997)

    def noise(self, shape):
        return self.rng.integers(-E.SAMPLE_BOUND, E.SAMPLE_BOUND + 1, size=shape).astype(np.int32)

    def plains(self, lead):
        return self.rng.integers(0, self.t, size=tuple(lead) + (self.n,), dtype=np.uint64)

    def tool(self, R):
        return L.ref_context_rns_tool(C.byref(self.ref.c), R)


session = session_memo(Session)


def bfv_cases(every_t=(4,), one_t=(11,)):
    """(chain, ring, t): every plain modulus at the rings `every_t`; one per chain at the rings `one_t` (a prime, a power of
    two, the 60-bit one), where the Python side is the slow one"""
    out = [(name, logn, t) for logn in every_t for t in E.PLAIN_MODULI for name in E.chains_for(t)]
    return out + [c for logn in one_t for c in (("mixed", logn, 786433), ("55", logn, 1 << 20), ("60", logn, (1 << 60) - 93))]


def case_id(c):
    return "%s-n%d-t%s" % (c[0], c[1], c[2] if c[2] < 1 << 21 else "60bit")


def deltas(se, k, plain):
    """[item][N] of ref_delta_m rows, memoising the words"""
    memo = {}
    mods = se.mods[:k]
    return [[memo.setdefault(int(m), E.ref_delta_m(m, mods, se.t)) for m in item] for item in plain]


def small_sum(target, e, mods, sign=1, negate=False):
    """[rows][N]: sign target + lift(e) modulo each row's prime (negated), in Python integers"""
    ev = np.array([int(v) for v in e], dtype=object)
    out = np.empty(target.shape, dtype=np.uint64)
    for r, p in enumerate(mods[:target.shape[0]]):
        v = (sign * target[r] + ev) % int(p)
        out[r] = ((-v) % int(p) if negate else v).astype(np.uint64)
    return out


def pair_columns(p):
    """the planted sample pairs of p by their c: [(c, e for the first item, e for the last item)] -- items that share a
    product polynomial differ in their samples"""
    pairs = E.planted_sample_pairs(p)
    cols = []
    for c in E.unique([c for c, _ in pairs]):
        es = [e for c2, e in pairs if c2 == c]
        cols.append((c, es[0], es[-1]))
    assert {(c, e) for c, a, b in cols for e in (a, b)} == set(pairs)
    return cols


def plant_pairs(se, target, e_first, e_last, rows):
    """target[rows][N] (shared by the first and the last item) and their samples at the planted positions"""
    pos = E.planted_positions(se.n, se.rng)
    for r in range(rows):
        for (c, a, b), i in zip(pair_columns(se.mods[r]), pos):
            target[r, i] = c
            e_first[i], e_last[i] = a, b
    return pos


def assert_sums_reached(words, mods, pos, negated=False):
    """the planted positions of `words` ([rows][N], a sum with a small sample) hold 0 and p - 1 in every row (negated: the sums
    were 0 and p - 1, so the words are 0 -- not p -- and 1)"""
    for r in range(words.shape[0]):
        got = {int(words[r, i]) for i in pos}
        assert 0 in got and (1 if negated else int(mods[r]) - 1) in got, (r, got)


def plant_plain_words(se, k, plain, round_index, used):
    """the planted plaintext words at the planted positions of the first and the last item, a different stretch of the list
    every round"""
    words = E.planted_plain_words(se.mods[:k], se.t)
    slots = E.planted_slots(se.n, se.rng, (FIRST, LAST))
    for s, (i, _, c) in enumerate(slots):
        m = words[(round_index * len(slots) + s) % len(words)]
        plain[i, c] = m
        used.add(m)
    return slots


def assert_estimates_reached(se, k, used):
    """the plaintext words used hold one whose quotient estimate is one short (unless t is a power of two) and an exact one"""
    t = se.t
    kinds = {E.barrett_quotient_estimate(num, t) == num // t for num in (E.numerator(m, se.mods[:k], t) for m in used)}
    assert kinds == ({True} if t & (t - 1) == 0 else {True, False}), (t, kinds)


# ---------------------------------------------------------------- scaling_variant_kernel through the Evaluator and the entry
@pytest.mark.parametrize("case", bfv_cases((4, 11), ()), ids=case_id)
def test_scaling_variant_on_planted_words(S, case):
    """add_plain / sub_plain / multiply_add_plain_with_scaling_variant at k = 1 and k = k_first: c_0 +- Delta m in Python
    integers; c_0 planted so that the sum and the difference are 0 and wrap in every row; sub after add restores"""
    se = session(S, *case)
    ctx, ev, n, t, size = se.ctx, se.ev, se.n, se.t, 2
    for k in sorted({1, se.k_first}):
        mods = se.mods[:k]
        used = set()
        n_words = len(E.planted_plain_words(mods, t))
        for rnd in range(-(-n_words // 10)):
            plain = se.plains((COUNT,))
            slots = plant_plain_words(se, k, plain, rnd, used)
            assert len(slots) == 10
            dm = deltas(se, k, plain)
            d_plain = ctx.upload(plain)
            for shift in range(4):
                ct = E.random_rows(se.rng, mods, n, (COUNT, size))
                for s, (i, _, c) in enumerate(slots):
                    kind = (s + shift) % 4
                    for r, p in enumerate(mods):
                        d = dm[i][c][r]
                        # the sum is 0; the difference is 0; the sum wraps; the difference borrows
                        ct[i, 0, r, c] = [(-d) % p, d, p - 1, 0][kind]
                add, sub = ct.copy(), ct.copy()
                for i in range(COUNT):
                    for r, p in enumerate(mods):
                        col = np.array([dm[i][c][r] for c in range(n)], dtype=object)
                        add[i, 0, r] = (ct[i, 0, r] + col) % p
                        sub[i, 0, r] = (ct[i, 0, r] - col) % p
                ct, add, sub = E.to_u64(ct), E.to_u64(add), E.to_u64(sub)
                for r in range(k):
                    assert not add[:, 0, r].all() and not sub[:, 0, r].all(), (k, r)  # both reach 0 in every row
                d = ctx.upload(ct)
                ev.add_plain_inplace(d, size, k, COUNT, d_plain)
                assert np.array_equal(d.download(ct.shape), add), (k, rnd, shift, "add")
                ev.sub_plain_inplace(d, size, k, COUNT, d_plain)
                assert np.array_equal(d.download(ct.shape), ct), (k, rnd, shift, "sub after add")
                ctx.multiply_add_plain_with_scaling_variant(k, d_plain, d, size, COUNT, subtract=True)
                assert np.array_equal(d.download(ct.shape), sub), (k, rnd, shift, "sub")
                ctx.multiply_add_plain_with_scaling_variant(k, d_plain, d, size, COUNT)
                assert np.array_equal(d.download(ct.shape), ct), (k, rnd, shift, "add after sub")
            # one plaintext for all (plain_stride 0): the first item's, on the last operands
            one = ctx.upload(np.ascontiguousarray(plain[FIRST]))
            want = ct.copy()
            for i in range(COUNT):
                for r, p in enumerate(mods):
                    col = np.array([dm[FIRST][c][r] for c in range(n)], dtype=object)
                    want[i, 0, r] = ((ct[i, 0, r].astype(object) - col) % p).astype(np.uint64)
            ev.sub_plain_inplace(d, size, k, COUNT, one, plain_stride=0)
            assert np.array_equal(d.download(ct.shape), want), (k, rnd, "stride 0")
            ctx.multiply_add_plain_with_scaling_variant(k, one, d, size, COUNT, plain_stride=0)
            assert np.array_equal(d.download(ct.shape), ct), (k, rnd, "stride 0 back")
        assert used >= set(E.planted_plain_words(mods, t))
        assert_estimates_reached(se, k, used)


# ---------------------------------------------------------------- fused public-key encrypt, BFV
def division_scenarios(mods_R):
    """(last-row sum, which planted residue the rows above hold, the sample): every pair of the three occurs"""
    out = []
    for li, x_last in enumerate(E.planted_last_row(mods_R[-1])):
        for kind in range(E.ROW_KINDS):
            out.append((x_last, kind, E.SAMPLE_VALUES[(li + kind) % len(E.SAMPLE_VALUES)]))
    return out


def oracle_asym(se, k, R, pk, u, e, plain):
    """test_gpu_encryptor.py's composition for one item: encrypt_zero_asymmetric_given over R rows, divide_and_round_q_last
    (the oracle's where it has the tool), the first k rows, the plaintext step"""
    c, ntt = se.ref.c, 1 if se.scheme == 2 else 0
    big = np.zeros((2, R, se.n), dtype=np.uint64)
    L.ref_encrypt_zero_asymmetric_given(C.byref(c), R, O.ptr(pk), ntt, O.ptr(u), O.ptr(np.ascontiguousarray(e)), O.ptr(big))
    if R == k + 1:
        tool = se.tool(R)
        for j in range(2):
            if not tool:
                E.divround_restated(big[j], se.mods, R, ntt, c)
            elif ntt:
                L.ref_divide_and_round_q_last_ntt_inplace(tool, O.ptr(big[j]), c.key_tables, 0)
            else:
                L.ref_divide_and_round_q_last_inplace(tool, O.ptr(big[j]))
    ct = np.ascontiguousarray(big[:, :k])
    if plain is not None and se.scheme == 1:
        L.ref_multiply_add_plain_with_scaling_variant(C.byref(c), k, O.ptr(np.ascontiguousarray(plain)), 0, O.ptr(ct[0]))
    elif plain is not None:
        for r in range(k):
            L.ref_add_poly_coeffmod(O.ptr(ct[0, r]), O.ptr(np.ascontiguousarray(plain[r])), se.n, C.byref(c.key_mod[r]),
                                    O.ptr(ct[0, r]))
    return ct


def key_rows(se, pk_R):
    """2 x n_key x N: the R planted rows of each polynomial, random rows behind them"""
    R = pk_R.shape[1]
    pk = E.to_u64(E.random_rows(se.rng, se.mods, se.n, (2,)))
    pk[:, :R] = pk_R
    return pk


def encrypt(se, k, pk, plain, u, e, stride=None):
    ctx = se.ctx
    ct = ctx.alloc(COUNT * 2 * k * se.n)
    ctx.encrypt(k, ctx.upload(pk), ctx.upload(plain) if plain is not None else None, ctx.upload_i32(u), ctx.upload_i32(e),
                COUNT, ct, plain_item_stride=stride)
    return ct.download((COUNT, 2, k, se.n))


def expected_asym_bfv(se, k, R, target, e, dm, traces):
    """[item][2][k][N] from the target, the samples and the Delta m rows, coefficient by coefficient; traces[(i, j, c)]
    receives divround_rows's trace"""
    mods_R = se.mods[:R]
    out = np.zeros((COUNT, 2, k, se.n), dtype=np.uint64)
    for i in range(COUNT):
        for j in range(2):
            for c in range(se.n):
                col = [(SIGNS[i] * target[j, r, c] + int(e[i, j, c])) % p for r, p in enumerate(mods_R)]
                if R == k + 1:
                    col = E.divround_rows(col, mods_R, traces.setdefault((i, j, c), {}))
                if dm is not None and j == 0:
                    col = [(v + d) % p for v, d, p in zip(col, dm[i][c], mods_R)]
                out[i, j, :, c] = col
    return out


@pytest.mark.parametrize("case", bfv_cases(), ids=case_id)
def test_public_key_encrypt_bfv_on_planted_words(S, case):
    """ctx.encrypt at every level without a plaintext (the key level stores the sums: encrypt_asym_bfv_finish_kernel<false>)
    and at k_first with the planted plaintext words, per item and one for all"""
    se = session(S, *case)
    n, t = se.n, se.t
    u = np.stack([E.delta_u(n, s) for s in SIGNS])
    for k in range(1, se.n_key + 1):
        R = k + 1 if k < se.n_key else k
        mods_R = se.mods[:R]
        runs = [False, True] if k == se.k_first else [False]
        for with_plain in runs:
            used, seen = set(), []
            if R == k:
                batches = [None]
            else:
                scen = division_scenarios(mods_R)
                batches = [scen[off:off + 10] for off in range(0, len(scen), 10)]
            for b, batch in enumerate(batches):
                target = E.random_rows(se.rng, mods_R, n, (2,))
                e = se.noise((COUNT, 2, n))
                slots = E.planted_slots(n, se.rng, (FIRST,), polys=2)  # the first and the last item share the target
                if batch is None:
                    pos = [plant_pairs(se, target[j], e[FIRST, j], e[LAST, j], R) for j in range(2)]
                else:
                    for (x_last, kind, ev), (_, j, c) in zip(batch, slots):
                        sums = [E.planted_row(p, E.row_temp(x_last, mods_R, r))[kind] for r, p in enumerate(mods_R[:-1])]
                        for r, v in enumerate(sums + [x_last]):
                            target[j, r, c] = (v - ev) % mods_R[r]
                        e[FIRST, j, c] = e[LAST, j, c] = ev
                plain = dm = None
                if with_plain:
                    plain = se.plains((COUNT,))
                    plant_plain_words(se, k, plain, b, used)
                    dm = deltas(se, k, plain)
                pk = key_rows(se, E.pk_for_targets(se.ref, target))
                traces = {}
                want = expected_asym_bfv(se, k, R, target, e, dm, traces)
                got = encrypt(se, k, pk, plain, u, e)
                assert np.array_equal(got, want), (k, with_plain, b)
                if se.tool(R) or R == k:
                    pk_R = np.ascontiguousarray(pk[:, :R])
                    for i in range(COUNT):
                        pl = plain[i] if with_plain else None
                        assert np.array_equal(want[i], oracle_asym(se, k, R, pk_R, u[i], e[i], pl)), (k, with_plain, b, i)
                if batch is None:
                    for j in range(2):
                        assert_sums_reached(want[FIRST, j], mods_R, pos[j])
                else:
                    seen += [traces[(i, j, c)] for i in (FIRST, LAST) for _, (_, j, c) in zip(batch, slots)]
                if with_plain and b == 0:  # one plaintext for all (plain_item_stride 0): the last item's
                    got = encrypt(se, k, pk, np.ascontiguousarray(plain[LAST]), u, e, stride=0)
                    one = expected_asym_bfv(se, k, R, target, e, [dm[LAST]] * COUNT, {})
                    assert np.array_equal(got, one), (k, "stride 0")
            if R == k + 1:  # the planted coefficients went both ways at every branch
                assert {tr["wrapped"] for tr in seen} == {True, False}
                for r in range(k):
                    assert any(tr["borrow"][r] for tr in seen) and any(tr["zero"][r] for tr in seen), (k, r)
            if with_plain:
                assert used >= set(E.planted_plain_words(se.mods[:k], t))
                assert_estimates_reached(se, k, used)


# ---------------------------------------------------------------- fused public-key encrypt, CKKS
def ntt_sample(n, value):
    """e = value (1, 0, .., 0): its transform is lift(value) in every word"""
    e = np.zeros(n, dtype=np.int32)
    e[0] = value
    return e


def exact_noise(se, row, planted):
    """a noise polynomial with the (position, value) pairs of `planted` whose transform on key prime `row` is exact, so that
    the inverse transform of the last row gives target + e word for word (encrypt_edge_ref.round_trips)"""
    for _ in range(32):
        e = se.noise((se.n,))
        for w, ev in planted:
            e[w] = ev
        if E.round_trips(se.ref, [E.lift(v, se.mods[row]) for v in e], row):
            return e
    raise AssertionError("no noise polynomial with an exact transform")


def plant_ntt_plain(se, v, plain, pos):
    """NTT-form plaintext words at the planted positions of the first and the last item so that v + plain is 0, 1 (after a
    wrap) and p - 1 (just short of one); v: [item][k][N], what the sum starts from"""
    for i in (FIRST, LAST):
        for s, c in enumerate(pos):
            for r in range(v.shape[1]):
                p, x = se.mods[r], int(v[i, r, c])
                plain[i, r, c] = [(-x) % p, (1 - x) % p, (p - 1 - x) % p][(s + r + i) % 3]


def add_ntt_plain(se, v, plain):
    out = v.copy()
    for r in range(v.shape[-2]):
        out[..., r, :] = ((v[..., r, :].astype(object) + plain[..., r, :].astype(object)) % se.mods[r]).astype(np.uint64)
    return out


def assert_plain_sums_reached(se, v, plain, pos):
    sums = add_ntt_plain(se, v, plain)
    for r in range(v.shape[1]):
        got = {int(sums[i, r, c]) for i in (FIRST, LAST) for c in pos}
        assert {0, 1, se.mods[r] - 1} <= got, (r, got)
        assert any(int(v[i, r, c]) + int(plain[i, r, c]) >= se.mods[r] for i in (FIRST, LAST) for c in pos)


@pytest.mark.parametrize("logn", [4, 11])
@pytest.mark.parametrize("name", list(E.CHAINS))
def test_public_key_encrypt_ckks_on_planted_words(S, name, logn):
    """the last row's coefficients planted through pk_last = NTT(target): every level below the key level, up to the first
    level with an NTT-form plaintext whose sum with c_0 is 0 and wraps; the key level (rlwe_stage_kernel<2> alone) on the
    sample pairs"""
    se = session(S, name, logn, 0)
    n, c = se.n, se.ref.c
    u = np.stack([E.delta_u(n, s) for s in SIGNS])
    for k in range(1, se.n_key):
        R = k + 1
        q_last = se.mods[k]
        e = se.noise((COUNT, 2, n))
        target = E.random_rows(se.rng, [q_last], n, (2,))[:, 0]
        slots = E.planted_slots(n, se.rng, (FIRST,), polys=2)
        lasts = E.planted_last_row(q_last)
        for s, (_, j, i) in enumerate(slots):
            target[j, i] = (lasts[s % len(lasts)] - E.SAMPLE_VALUES[s % len(E.SAMPLE_VALUES)]) % q_last
        for i in (FIRST, LAST):
            for j in range(2):
                e[i, j] = exact_noise(se, k, [(w, E.SAMPLE_VALUES[s % len(E.SAMPLE_VALUES)])
                                             for s, (_, jj, w) in enumerate(slots) if jj == j])
        pk = E.to_u64(E.random_rows(se.rng, se.mods, n, (2,)))  # rows 0..k-1: NTT-form words as they come
        for j in range(2):
            pk[j, k] = E.ntt_row(se.ref, target[j], k)
        pk_R = np.ascontiguousarray(pk[:, :R])
        zero = np.zeros((COUNT, 2, k, n), dtype=np.uint64)
        half = q_last >> 1
        wraps = set()
        for i in range(COUNT):
            big = np.zeros((2, R, n), dtype=np.uint64)
            L.ref_encrypt_zero_asymmetric_given(C.byref(c), R, O.ptr(pk_R), 1, O.ptr(u[i]), O.ptr(np.ascontiguousarray(e[i])),
                                                O.ptr(big))
            for j in range(2):
                coeffs = E.divround_restated(big[j], se.mods, R, 1, c)
                if i in (FIRST, LAST):  # the planted sums are what the kernel's last row holds
                    for s, (_, jj, pos) in enumerate(slots):
                        if jj == j:
                            assert coeffs[pos] == lasts[s % len(lasts)], (k, i, j, pos)
                            wraps.add(coeffs[pos] + half >= q_last)
            zero[i] = big[:, :k]
        assert wraps == {True, False}
        got = encrypt(se, k, pk, None, u, e)
        assert np.array_equal(got, zero), (k, "zero")
        if k > se.k_first:
            continue  # (a level between the first and the key level holds no plaintext)
        pos = E.planted_positions(n, se.rng)
        plain = E.to_u64(E.random_rows(se.rng, se.mods[:k], n, (COUNT,)))
        plant_ntt_plain(se, zero[:, 0], plain, pos)
        assert_plain_sums_reached(se, zero[:, 0], plain, pos)
        want = zero.copy()
        want[:, 0] = add_ntt_plain(se, zero[:, 0], plain)
        got = encrypt(se, k, pk, plain, u, e)
        assert np.array_equal(got, want), (k, "plain")
        for i in range(COUNT):
            assert np.array_equal(want[i], oracle_asym(se, k, R, pk_R, u[i], e[i], plain[i])), (k, i)
        got = encrypt(se, k, pk, np.ascontiguousarray(plain[LAST]), u, e, stride=0)
        want[:, 0] = add_ntt_plain(se, zero[:, 0], plain[LAST])
        assert np.array_equal(got, want), (k, "stride 0")
    # the key level: c_j = NTT(e_j) + u (.) pk_j, nothing divided
    for evs in (((1, -1), (E.SAMPLE_BOUND, -E.SAMPLE_BOUND)), ((0, 0), (-1, 1))):
        check_asym_ntt_form(se, se.n_key, evs, lambda pk, uu, ee: encrypt(se, se.n_key, pk, None, uu, ee))


def check_asym_ntt_form(se, rows, evs, run):
    """c_j = lift(e_j) + u (.) pk_j in NTT form with e_j = ev (1, 0, .., 0): evs = (the first item's (ev_0, ev_1), the last
    item's); pk holds every c of the planted pairs at the planted positions"""
    n = se.n
    u = np.stack([E.delta_u(n, s) for s in SIGNS])
    pk = E.random_rows(se.rng, se.mods[:rows], n, (2,))
    pos = E.planted_positions(n, se.rng)
    for j in range(2):
        for r in range(rows):
            for (cv, _, _), i in zip(pair_columns(se.mods[r]), pos):
                pk[j, r, i] = cv
    e = se.noise((COUNT, 2, n))
    for i, pair in zip((FIRST, LAST), evs):
        for j in range(2):
            e[i, j] = ntt_sample(n, pair[j])
    pk64 = E.to_u64(pk)
    got = run(key_rows(se, pk64) if rows < se.n_key else pk64, u, e)
    for i, pair in zip((FIRST, LAST), evs):
        for j in range(2):
            want = small_sum(pk[j], np.full(n, pair[j]), se.mods)
            assert np.array_equal(got[i, j], want), (rows, evs, i, j)
    for i in range(COUNT):
        want = np.zeros((2, rows, n), dtype=np.uint64)
        L.ref_encrypt_zero_asymmetric_given(C.byref(se.ref.c), rows, O.ptr(pk64), 1, O.ptr(u[i]),
                                            O.ptr(np.ascontiguousarray(e[i])), O.ptr(want))
        assert np.array_equal(got[i], want), (rows, evs, i)


# ---------------------------------------------------------------- fused symmetric encrypt
def oracle_sym(se, k, sk, seed, e, plain, seeded):
    """test_gpu_encryptor.py's composition for one item"""
    c = se.ref.c
    sample, a = E.seeded_a(se.ref, seed, se.mods[:k], se.n, seeded)
    a = np.ascontiguousarray(a).copy()
    ct = np.zeros((2, k, se.n), dtype=np.uint64)
    L.ref_encrypt_zero_symmetric_given(C.byref(c), k, O.ptr(sk), 1 if se.scheme == 2 else 0, O.ptr(a),
                                       O.ptr(np.ascontiguousarray(e)), O.ptr(ct))
    if seeded:
        ct[1] = sample
    if plain is not None and se.scheme == 1:
        L.ref_multiply_add_plain_with_scaling_variant(C.byref(c), k, O.ptr(np.ascontiguousarray(plain)), 0, O.ptr(ct[0]))
    elif plain is not None:
        ct[0] = add_ntt_plain(se, ct[0], plain)
    return ct


def encrypt_sym(se, k, sk, plain, seeds, e, save_seed):
    ctx = se.ctx
    ct = ctx.alloc(COUNT * 2 * k * se.n)
    ctx.encrypt_symmetric(k, ctx.upload(sk), ctx.upload(plain) if plain is not None else None, seeds, ctx.upload_i32(e), COUNT,
                          ct, save_seed=save_seed)
    return ct.download((COUNT, 2, k, se.n))


def sym_key(se, k, target, a, target_is_ntt=False):
    """n_key x N: the planting key on the first k rows, ones behind them"""
    sk = E.ones_key(se.mods, se.n)
    sk[:k] = E.sk_for_targets(se.ref, target, a, se.mods, target_is_ntt)
    return sk


@pytest.mark.parametrize("save_seed", [False, True], ids=["unseeded", "seeded"])
@pytest.mark.parametrize("case", bfv_cases(), ids=case_id)
def test_symmetric_encrypt_bfv_on_planted_words(S, case, save_seed):
    """c_0 = -(a s + e) [+ Delta m] with a s planted through the secret key: the first and the last item share the seed, so
    both see the target; the one between has another seed and is compared with the oracle alone"""
    se = session(S, *case)
    n, t = se.n, se.t
    for k in sorted({1, se.k_first, se.n_key}):
        mods = se.mods[:k]
        assert k * n >= 9  # (below that the reference drops save_seed)
        seed = E.pick_seed(se.rng, mods, n, se.ref, save_seed)
        other = se.rng.integers(0, 2**64, size=8, dtype=np.uint64, endpoint=False)
        seeds = np.stack([seed, other, seed])
        sample, a = E.seeded_a(se.ref, seed, mods, n, save_seed)
        assert sample.all() and a.all()
        for with_plain in ([False, True] if k == se.k_first else [False]):
            target = E.random_rows(se.rng, mods, n)
            e = se.noise((COUNT, n))
            pos = plant_pairs(se, target, e[FIRST], e[LAST], k)
            sk = sym_key(se, k, target, a)
            plain = dm = None
            used = set()
            if with_plain:
                plain = se.plains((COUNT,))
                plant_plain_words(se, k, plain, 0, used)
                dm = deltas(se, k, plain)
            got = encrypt_sym(se, k, sk, plain, seeds, e, save_seed)
            for i in (FIRST, LAST):
                c0 = small_sum(target, e[i], mods, negate=True)
                assert_sums_reached(c0, mods, pos, negated=True)
                if with_plain:
                    for r, p in enumerate(mods):
                        col = np.array([dm[i][c][r] for c in range(n)], dtype=object)
                        c0[r] = ((c0[r].astype(object) + col) % p).astype(np.uint64)
                assert np.array_equal(got[i, 0], c0), (k, with_plain, i)
            for i in range(COUNT):
                want = oracle_sym(se, k, sk, seeds[i], e[i], plain[i] if with_plain else None, save_seed)
                assert np.array_equal(got[i], want), (k, with_plain, i, "oracle")
            if with_plain:
                assert used >= set(E.planted_plain_words(mods, t))
                assert_estimates_reached(se, k, used)


@pytest.mark.parametrize("logn", [4, 11])
@pytest.mark.parametrize("name", list(E.CHAINS))
def test_symmetric_encrypt_ckks_on_planted_words(S, name, logn):
    """c_0 = -(NTT(e) + c_1 (.) s) [+ plain]: e = ev (1, 0, .., 0) puts lift(ev) in every word, c_1 (.) s is planted through
    the secret key; the plaintext makes the last sum 0 and wrap"""
    se = session(S, name, logn, 0)
    n = se.n
    b = E.SAMPLE_BOUND
    for k in sorted({1, se.k_first, se.n_key}):
        mods = se.mods[:k]
        seed = E.pick_seed(se.rng, mods, n)
        other = se.rng.integers(0, 2**64, size=8, dtype=np.uint64, endpoint=False)
        seeds = np.stack([seed, other, seed])
        a = E.seeded_a(se.ref, seed, mods, n, False)[1]
        # (the three rounds meet every planted pair: c = p - 1 with +1 and 0, c = 0 with -1 and 0, the three of +-19)
        for ev_first, ev_last in ((1, 0), (-1, 0), (b, -b)):
            target = E.random_rows(se.rng, mods, n)
            pos = E.planted_positions(n, se.rng)
            for r in range(k):
                for (cv, _, _), i in zip(pair_columns(mods[r]), pos):
                    target[r, i] = cv
            e = se.noise((COUNT, n))
            e[FIRST], e[LAST] = ntt_sample(n, ev_first), ntt_sample(n, ev_last)
            sk = sym_key(se, k, target, a, target_is_ntt=True)
            got = encrypt_sym(se, k, sk, None, seeds, e, False)
            zero = np.zeros((COUNT, 2, k, n), dtype=np.uint64)
            for i in range(COUNT):
                zero[i] = oracle_sym(se, k, sk, seeds[i], e[i], None, False)
            for i, ev in ((FIRST, ev_first), (LAST, ev_last)):
                c0 = small_sum(target, np.full(n, ev), mods, negate=True)
                assert np.array_equal(zero[i, 0], c0) and np.array_equal(zero[i, 1], a), (k, ev)
            assert np.array_equal(got, zero), (k, ev_first, ev_last)
            if k == se.n_key:
                continue  # (no plaintext is valid at the key level)
            plain = E.to_u64(E.random_rows(se.rng, mods, n, (COUNT,)))
            plant_ntt_plain(se, zero[:, 0], plain, pos)
            assert_plain_sums_reached(se, zero[:, 0], plain, pos)
            want = zero.copy()
            want[:, 0] = add_ntt_plain(se, zero[:, 0], plain)
            got = encrypt_sym(se, k, sk, plain, seeds, e, False)
            assert np.array_equal(got, want), (k, ev_first, ev_last, "plain")


# ---------------------------------------------------------------- the unfused entries (rlwe_stage_kernel<0..3>)
@pytest.mark.parametrize("t", [786433, 0], ids=["bfv", "ckks"])
@pytest.mark.parametrize("logn", [4, 11])
@pytest.mark.parametrize("name", list(E.CHAINS))
def test_encrypt_zero_entries_on_planted_sums(S, name, logn, t):
    """encrypt_zero_symmetric (a_ntt and sk_ntt = 1 handed in; also in place, a already in the c_1 slot) and
    encrypt_zero_asymmetric, in both output forms, at the key level and the first level"""
    se = session(S, name, logn, t)
    ctx, n, c = se.ctx, se.n, se.ref.c
    b = E.SAMPLE_BOUND
    for rows in (se.n_key, se.k_first):
        mods = se.mods[:rows]
        ones = E.ones_key(se.mods, n)  # (the key keeps its key-level row stride)
        d_ones = ctx.upload(ones)
        # --- symmetric, coefficient form: c_0 = -(target + e), c_1 = target; every item has its own a
        target = E.random_rows(se.rng, mods, n, (COUNT,))
        e = se.noise((COUNT, n))
        pos = plant_pairs(se, target[FIRST], e[FIRST], e[LAST], rows)
        target[LAST] = target[FIRST]
        a = E.ntt_rows(se.ref, target)
        want = np.zeros((COUNT, 2, rows, n), dtype=np.uint64)
        for i in range(COUNT):
            want[i, 0] = small_sum(target[i], e[i], mods, negate=True)
            want[i, 1] = E.to_u64(target[i])
            exp = np.zeros((2, rows, n), dtype=np.uint64)
            L.ref_encrypt_zero_symmetric_given(C.byref(c), rows, O.ptr(ones), 0, O.ptr(a[i]), O.ptr(e[i]), O.ptr(exp))
            assert np.array_equal(want[i], exp), (rows, i)
        for i in (FIRST, LAST):
            assert_sums_reached(want[i, 0], mods, pos, negated=True)
        check_sym_entry(se, rows, False, a, e, d_ones, want)
        # --- symmetric, NTT form: c_0 = -(lift(ev) + a), c_1 = a
        for ev_first, ev_last in ((1, 0), (-1, 0), (b, -b)):
            a = E.random_rows(se.rng, mods, n, (COUNT,))
            e = se.noise((COUNT, n))
            for i, ev in ((FIRST, ev_first), (LAST, ev_last)):
                e[i] = ntt_sample(n, ev)
                for r in range(rows):
                    for (cv, _, _), w in zip(pair_columns(mods[r]), pos):
                        a[i, r, w] = cv
            a64 = E.to_u64(a)
            want = np.zeros((COUNT, 2, rows, n), dtype=np.uint64)
            for i in range(COUNT):
                L.ref_encrypt_zero_symmetric_given(C.byref(c), rows, O.ptr(ones), 1, O.ptr(a64[i]), O.ptr(e[i]),
                                                   O.ptr(want[i]))
            for i, ev in ((FIRST, ev_first), (LAST, ev_last)):
                assert np.array_equal(want[i, 0], small_sum(a[i], np.full(n, ev), mods, negate=True)), (rows, ev)
            check_sym_entry(se, rows, True, a64, e, d_ones, want)
        # --- asymmetric, coefficient form: c_j = +-target_j + e_j
        u = np.stack([E.delta_u(n, s) for s in SIGNS])
        target = E.random_rows(se.rng, mods, n, (2,))
        e = se.noise((COUNT, 2, n))
        for j in range(2):
            pos = plant_pairs(se, target[j], e[FIRST, j], e[LAST, j], rows)
        pk = E.pk_for_targets(se.ref, target)
        out = ctx.alloc(COUNT * 2 * rows * n)
        ctx.encrypt_zero_asymmetric(rows, False, ctx.upload(pk), ctx.upload_i32(u), ctx.upload_i32(e), COUNT, out)
        got = out.download((COUNT, 2, rows, n))
        for i in range(COUNT):
            for j in range(2):
                want = small_sum(target[j], e[i, j], mods, sign=SIGNS[i])
                assert np.array_equal(got[i, j], want), (rows, i, j)
            exp = np.zeros((2, rows, n), dtype=np.uint64)
            L.ref_encrypt_zero_asymmetric_given(C.byref(c), rows, O.ptr(pk), 0, O.ptr(u[i]), O.ptr(np.ascontiguousarray(e[i])),
                                                O.ptr(exp))
            assert np.array_equal(got[i], exp), (rows, i)
        assert_sums_reached(got[FIRST, 1], mods, pos)
        # --- asymmetric, NTT form: c_j = lift(ev_j) +- pk_j

        def run(pk, uu, ee):
            out = ctx.alloc(COUNT * 2 * rows * n)
            ctx.encrypt_zero_asymmetric(rows, True, ctx.upload(np.ascontiguousarray(pk[:, :rows])), ctx.upload_i32(uu),
                                        ctx.upload_i32(ee), COUNT, out)
            return out.download((COUNT, 2, rows, n))

        for evs in (((1, -1), (b, -b)), ((0, 0), (-1, 1))):
            check_asym_ntt_form(se, rows, evs, run)


def check_sym_entry(se, rows, ntt_form, a, e, d_sk, want):
    """encrypt_zero_symmetric into a fresh buffer, and in place with a already in the c_1 slot"""
    ctx, n = se.ctx, se.n
    out = ctx.alloc(COUNT * 2 * rows * n)
    ctx.encrypt_zero_symmetric(rows, ntt_form, ctx.upload(a), ctx.upload_i32(e), d_sk, COUNT, out)
    assert np.array_equal(out.download(want.shape), want), (rows, ntt_form)
    buf = np.zeros(want.shape, dtype=np.uint64)
    buf[:, 1] = a
    dbuf = ctx.upload(buf)
    ctx.encrypt_zero_symmetric(rows, ntt_form, dbuf.ptr + rows * n * 8, ctx.upload_i32(e), d_sk, COUNT, dbuf)
    assert np.array_equal(dbuf.download(want.shape), want), (rows, ntt_form, "in place")


# ---------------------------------------------------------------- scaling_variant_fix inside poly_tables_kernel
def test_polynomial_constant_on_planted_words(S):
    """p(x) = c + x on a BFV ciphertext: the constant added at coefficient 0 of c_0 is Delta c, for a c whose quotient estimate
    is one short and for one whose estimate is exact (tests/poly_eval_ref.py's setup, STRICT)"""
    t = 257
    se = session(S, "55", 11, t, mode=S.MODE_STRICT)
    ctx, ev, n, k = se.ctx, se.ev, se.n, se.k_first
    mods = se.mods[:k]
    short = [m for m in E.planted_plain_words(mods, t)
             if E.barrett_quotient_estimate(E.numerator(m, mods, t), t) == E.numerator(m, mods, t) // t - 1]
    exact = [m for m in E.planted_plain_words(mods, t)
             if m not in short and E.ref_delta_m(m, mods, t) != [0] * k]
    assert short and exact
    ct = E.to_u64(E.random_rows(se.rng, mods, n, (COUNT, 2)))
    for word in (short[0], exact[0], exact[-1]):
        dm = E.ref_delta_m(word, mods, t)
        assert dm == P.bfv_constant(se.ref, k, word)
        out = ctx.alloc(COUNT * 2 * k * n)
        ev.evaluate_polynomial(ctx.upload(ct), [word, 1], k, COUNT, out)
        got = out.download(ct.shape)
        want = ct.copy()
        for r, p in enumerate(mods):
            want[:, 0, r, 0] = [(int(v) + dm[r]) % p for v in ct[:, 0, r, 0]]
        assert np.array_equal(got, want), word
        assert np.array_equal(got[1], P.evaluate_polynomial(se.ref, k, ct[1], [word, 1]))


# ---------------------------------------------------------------- the signed BatchEncoder (batch_permute_kernel)
@pytest.mark.parametrize("t", [257, 786433])
def test_signed_batch_encoder_on_planted_words(S, t):
    """decode: the slot words t >> 1 (the largest non-negative), (t >> 1) + 1 (the most negative), 0 and t - 1 (-1); encode:
    their signed values. Against ref_batch_*_signed and against the values written out by hand."""
    logn, n = 6, 1 << 6
    se = session(S, "55", logn, t)
    ctx = se.ctx
    assert ctx.using_batching
    tb = O.Tables(logn, t)
    half = t >> 1
    words = [half, half + 1, 0, t - 1]
    signed = [half, -half, 0, -1]
    assert [w if w <= half else w - t for w in words] == signed
    slots = se.plains((COUNT,))
    pos = E.planted_positions(n, se.rng)
    for i in (FIRST, LAST):
        for s, c in enumerate(pos):
            slots[i, c] = words[(s + i) % 4]
    by_hand = np.array([[int(v) if int(v) <= half else int(v) - t for v in item] for item in slots], dtype=np.int64)
    # decode: the plaintexts whose slots hold these words (the unsigned encoder of the oracle)
    plain = np.zeros((COUNT, n), dtype=np.uint64)
    for i in range(COUNT):
        L.ref_batch_encode(C.byref(tb.t), O.ptr(slots[i]), n, O.ptr(plain[i]))
    back = ctx.alloc(COUNT * n)
    ctx.batch_decode_int64(ctx.upload(plain), COUNT, back)
    got = back.download((COUNT, n)).view(np.int64)
    assert np.array_equal(got, by_hand)
    for i in range(COUNT):
        exp = np.zeros(n, dtype=np.uint64)
        L.ref_batch_decode_signed(C.byref(tb.t), O.ptr(plain[i]), n, O.ptr(exp))
        assert np.array_equal(got[i], exp.view(np.int64)), i
    for i in (FIRST, LAST):
        assert {int(got[i, c]) for c in pos} >= set(signed)
    # encode: the signed values give the same plaintexts
    dplain = ctx.alloc(COUNT * n)
    ctx.batch_encode_int64(ctx.upload(np.ascontiguousarray(by_hand).view(np.uint64)), n, COUNT, dplain)
    enc = dplain.download((COUNT, n))
    assert np.array_equal(enc, plain)
    for i in range(COUNT):
        exp = np.zeros(n, dtype=np.uint64)
        L.ref_batch_encode_signed(C.byref(tb.t), O.ptr(np.ascontiguousarray(by_hand[i]).view(np.uint64)), n, O.ptr(exp))
        assert np.array_equal(enc[i], exp), i
