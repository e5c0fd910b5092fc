"""The linear layer in plain integers, and operands made of the words at which modular code goes wrong.

References: every coefficient-wise operation, both automorphisms, the Evaluator's add / sub / negate / multiply_plain(_ntt)
and the two validity checks, written from their definitions in Python integers (numpy `object` arrays hold Python integers;
only indices are int64). Nothing here calls the oracle or the library: tests/test_linear_layer_host.py holds the oracle to
these, tests/test_gpu_linear_layer.py the kernels.

Operands: `boundary_words`, `wide_words` and `words_63` are the word sets per prime; `boundary_rows` and `boundary_pairs`
lay them out over batches [item..][row][column] so that every word (every ordered pair of words) meets every row's prime
in both lanes of a 16-byte pair; `plants` and `transparency_plants` are the batches of the validity checks.

"Row" below is an RNS row: the words of one prime over all items of the batch. At N = 8 no single polynomial row can hold a
set of sixteen words, so the builders' guarantees are per prime over the batch, and `lead_for` / `boundary_pairs` choose how
many items that takes."""
import numpy as np

import oracle_lib as O

M64 = (1 << 64) - 1
CORNERS = (0, 1, -2, -1)  # both lanes of the first and of the last 16-byte pair of a row


# ---------------------------------------------------------------- prime chains (four ciphertext primes, one special prime)
def ntt_primes_from(n, count):
    """the smallest `count` primes = 1 (mod 2n)"""
    out, c = [], 2 * n + 1
    while len(out) < count:
        if O.is_prime(c):
            out.append(c)
        c += 2 * n
    return out


def chain(name, logn):
    """P61: the largest primes below 2^61; PMIN: the smallest NTT primes of the ring; PMIX: 61, 20, 45 and 61 bits, so that
    a row's prime is not monotone in the row index. Each is four ciphertext primes followed by one special prime."""
    n = 1 << logn
    if name == "P61":
        return O.ntt_primes_below(n, 1 << 61, 5)
    if name == "PMIN":
        return ntt_primes_from(n, 5)
    assert name == "PMIX", name
    big = O.ntt_primes_below(n, 1 << 61, 3)
    mods = [big[0], O.ntt_primes_below(n, 1 << 20, 1)[0], O.ntt_primes_below(n, 1 << 45, 1)[0], big[1], big[2]]
    assert [p.bit_length() for p in mods] == [61, 20, 45, 61, 61]
    return mods


CHAINS = ("P61", "PMIN", "PMIX")


# ---------------------------------------------------------------- word sets
def boundary_words(p):
    return [0, 1, 2, (p - 1) // 2, (p + 1) // 2, p - 2, p - 1]


def wide_words(p):
    """for operands documented as any 64-bit word"""
    return boundary_words(p) + [p, p + 1, 2 * p - 1, 2 * p, 4 * p - 1, (1 << 63) - 1, 1 << 63, (1 << 64) - p, M64]


def words_63(p):
    """for modulo_poly_coeffs_63: words below 2^63"""
    top = (1 << 63) - 1
    m = top // p
    out = [0, p - 1, p, p + 1, 2 * p - 1, 2 * p, m * p - 1, m * p]
    if m * p + 1 <= top:
        out.append(m * p + 1)
    return out + [top]


def below_p(p):
    return p


def below_2_63(p):
    return 1 << 63


def below_2_64(p):
    return 1 << 64


# ---------------------------------------------------------------- operand builders
def _random_words(rng, bound, size):
    assert bound <= 1 << 63 or bound == 1 << 64
    if bound == 1 << 64:
        return rng.integers(0, M64, size=size, dtype=np.uint64, endpoint=True)
    return rng.integers(0, bound, size=size, dtype=np.uint64)


def lead_for(n, n_words, corners=False):
    """the number of items from which boundary_rows puts every word of a set of n_words into both lanes of every row;
    corners: and at each of the four corner columns as well"""
    planted = (n - 4) // 4  # (even lane, odd lane) pairs of set words among an item's interior columns
    return max(-(-n_words // planted), n_words if corners else 1)


def boundary_rows(mods, n, lead, words, rng, fill=below_p):
    """[lead..][len(mods)][n] uint64 for a unary operand. Per row r (prime p, set W = words(p)), over the items m = 0, 1, ..
    of the batch in order:
      columns 0, 1, n-2, n-1 of item m hold W[m + r], W[m + r + 1], W[m + r + 2], W[m + r + 3] (indices mod |W|): set words
        only, and from |W| items on every word has been at every corner;
      the interior columns, counted j = 0, 1, .. through the batch, hold W[j / 4 + r] in the even lane (j = 0 mod 4) and
        W[j / 4 + r + |W| / 2] in the odd lane (j = 1 mod 4); j = 2, 3 mod 4 are random words below fill(p).
    From lead_for(n, |W|) items on every word is in both lanes of every row."""
    lead = tuple(lead)
    items = int(np.prod(lead)) if lead else 1
    out = np.empty((items, len(mods), n), dtype=np.uint64)
    assert n >= 8 and n % 4 == 0
    for r, p in enumerate(mods):
        p = int(p)
        W = [int(w) for w in words(p)]
        nw = len(W)
        Wa = np.array(W, dtype=np.uint64)
        row = _random_words(rng, fill(p), (items, n))
        m = np.arange(items)
        for ci, col in enumerate(CORNERS):
            row[:, col] = Wa[(m + r + ci) % nw]
        inner = row[:, 2:n - 2].reshape(-1)  # (a copy when not contiguous: written back below)
        j = np.arange(inner.size)
        even, odd = j % 4 == 0, j % 4 == 1
        inner[even] = Wa[(j[even] // 4 + r) % nw]
        inner[odd] = Wa[(j[odd] // 4 + r + nw // 2) % nw]
        row[:, 2:n - 2] = inner.reshape(items, n - 4)
        out[:, r, :] = row
    return out.reshape(lead + (len(mods), n))


def boundary_pairs(mods, n, lead, words_a, words_b, rng, fill_a=below_p, fill_b=below_p, count=None):
    """(a, b), each [count][lead..][len(mods)][n] uint64, for a binary operation. Per row r (prime p) and per index into
    `lead`, the slots (item, column) are counted s = 0, 1, .. through the batch; the first |A| |B| of them hold the ordered
    pairs (A[i], B[j]) of words_a(p) x words_b(p), pair number (s + 3 r) mod |A| |B|, so that a pair's lane and column differ
    from row to row; the slots after them hold random words below fill_a(p), fill_b(p). `count` defaults to the smallest
    batch (at least two items) that holds every ordered pair in every row."""
    lead = tuple(lead)
    inner = int(np.prod(lead)) if lead else 1
    npairs = max(len(words_a(int(p))) * len(words_b(int(p))) for p in mods)
    if count is None:
        count = max(2, -(-npairs // n))
    assert count * n >= npairs, "the batch is too small for every ordered pair"
    a = np.empty((count, inner, len(mods), n), dtype=np.uint64)
    b = np.empty_like(a)
    for r, p in enumerate(mods):
        p = int(p)
        A, B = [int(w) for w in words_a(p)], [int(w) for w in words_b(p)]
        pa = np.array([x for x in A for _ in B], dtype=np.uint64)
        pb = np.array([y for _ in A for y in B], dtype=np.uint64)
        for l in range(inner):
            ra = _random_words(rng, fill_a(p), count * n)
            rb = _random_words(rng, fill_b(p), count * n)
            s = np.arange(len(pa))
            ra[s] = pa[(s + 3 * r) % len(pa)]
            rb[s] = pb[(s + 3 * r) % len(pa)]
            a[:, l, r, :] = ra.reshape(count, n)
            b[:, l, r, :] = rb.reshape(count, n)
    shape = (count,) + lead + (len(mods), n)
    return a.reshape(shape), b.reshape(shape)


def row_words(x, r):
    """the words of RNS row r of a batch [..][rows][n], as [items][n]"""
    return x[..., r, :].reshape(-1, x.shape[-1])


def plants(mods, n, size, extra=()):
    """The batch of is_data_valid_for: ct[items][size][k][n], expected flags and one label per item. For every polynomial j,
    row r and corner column c there is one item with p_r - 1 planted on an otherwise-zero ciphertext (valid) and one with p_r
    (invalid). `extra` = (row, word, valid) triples planted at (polynomial size - 1, row, column 1)."""
    k = len(mods)
    cases = []
    for j in range(size):
        for r in range(k):
            for c in CORNERS:
                cases.append((j, r, c, int(mods[r]) - 1, True))
                cases.append((j, r, c, int(mods[r]), False))
    for r, w, ok in extra:
        cases.append((size - 1, r, 1, int(w), ok))
    ct = np.zeros((len(cases), size, k, n), dtype=np.uint64)
    for i, (j, r, c, w, _) in enumerate(cases):
        ct[i, j, r, c] = w
    return ct, np.array([ok for *_, ok in cases], dtype=bool), ["poly %d row %d col %d word %d" % c[:4] for c in cases]


def transparency_plants(k, n, size):
    """The batch of is_transparent: ct[items][size][k][n] with at most one non-zero word per item, and one label per item.
    Items that must and must not be transparent alternate, so that a flag that bleeds into a neighbour shows."""
    spots = [("all zero", None),
             ("first word of polynomial 1", (1, 0, 0)),
             ("last word of polynomial 0", (0, k - 1, n - 1)),
             ("last word of the last polynomial", (size - 1, k - 1, n - 1)),
             ("first word of polynomial 0", (0, 0, 0)),
             ("second word of polynomial 1", (1, 0, 1)),
             ("all zero again", None),
             ("last word of polynomial 1", (1, k - 1, n - 1))]
    ct = np.zeros((len(spots), size, k, n), dtype=np.uint64)
    for i, (_, at) in enumerate(spots):
        if at is not None:
            ct[(i,) + at] = 1
    return ct, [name for name, _ in spots]


# ---------------------------------------------------------------- exact references
def _obj(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def _u64(x):
    return np.array(x.tolist(), dtype=np.uint64).reshape(x.shape)


def _per_row(fn, mods, *operands):
    """fn(p, row words..) per RNS row of operands [..][rows][n], in Python integers"""
    ops = [_obj(o) for o in operands]
    out = np.empty(ops[0].shape, dtype=object)
    assert ops[0].shape[-2] == len(mods)
    for r, p in enumerate(mods):
        out[..., r, :] = fn(int(p), *[o[..., r, :] for o in ops])
    return _u64(out)


def dyadic_product(a, b, mods):
    return _per_row(lambda p, x, y: (x * y) % p, mods, a, b)


def add(a, b, mods):
    return _per_row(lambda p, x, y: (x + y) % p, mods, a, b)


def sub(a, b, mods):
    return _per_row(lambda p, x, y: (x - y) % p, mods, a, b)


def negate(a, mods):
    return _per_row(lambda p, x: (-x) % p, mods, a)


def modulo(a, mods):
    return _per_row(lambda p, x: x % p, mods, a)


def scalar_product(a, s, mods):
    return _per_row(lambda p, x: (x * int(s)) % p, mods, a)


def apply_galois(x, logn, g, mods):
    """coefficient form: out[(i g) mod N] = (-1)^floor(i g / N) in[i] mod p"""
    n = 1 << logn
    raw = np.arange(n, dtype=np.int64) * int(g)
    idx, flip = raw & (n - 1), ((raw >> logn) & 1).astype(bool)

    def one(p, v):
        out = np.empty(v.shape, dtype=object)
        out[..., idx] = np.where(flip, (-v) % p, v)
        return out

    return _per_row(one, mods, x)


def bitrev(i, logn):
    i = np.asarray(i, dtype=np.int64)
    out = np.zeros_like(i)
    for b in range(logn):
        out |= ((i >> b) & 1) << (logn - 1 - b)
    return out


def galois_ntt_table(logn, g):
    """position i holds the evaluation at psi^(2 bitrev(i) + 1): out[i] = in[bitrev(((g (2 bitrev(i) + 1)) mod 2N - 1) / 2)]"""
    n = 1 << logn
    e = (int(g) * (2 * bitrev(np.arange(n), logn) + 1)) & (2 * n - 1)
    return bitrev((e - 1) >> 1, logn)


def apply_galois_ntt(x, logn, g):
    return np.ascontiguousarray(np.asarray(x, dtype=np.uint64)[..., galois_ntt_table(logn, g)])


def apply_galois_ints(row, logn, g, p):
    """the same two maps on one row, in Python integers and loops only: (coefficient form, NTT form)"""
    n = 1 << logn
    rev = lambda i: int(format(i, "0%db" % logn)[::-1], 2)
    coeff, ntt = [None] * n, [None] * n
    for i in range(n):
        coeff[(i * g) % n] = (int(row[i]) * (-1) ** ((i * g) // n)) % p
        ntt[i] = int(row[rev((((g * (2 * rev(i) + 1)) % (2 * n)) - 1) // 2)])
    return coeff, ntt


def ct_add(a, b, mods, subtract=False):
    """Evaluator add / sub on a[count][sa][k][n], b[count][sb][k][n]: the tail of the longer operand is copied, or negated
    when it is b's and the operation is sub"""
    sa, sb = a.shape[1], b.shape[1]
    lo = min(sa, sb)
    head = (sub if subtract else add)(a[:, :lo], b[:, :lo], mods)
    if sa == sb:
        return head
    tail = a[:, lo:] if sa > sb else negate(b[:, lo:], mods) if subtract else b[:, lo:]
    return np.concatenate([head, tail], axis=1)


def ct_negate(a, mods):
    return negate(a, mods)


def multiply_plain_ntt(ct, plain, mods):
    """ct[count][size][k][n] times plain[count or 1][k][n], the plaintext broadcast over the polynomials"""
    return dyadic_product(ct, np.broadcast_to(plain[:, None], ct.shape), mods)


def centred(plain, t):
    """v - t [v >= (t + 1) / 2] as Python integers"""
    thr = (t + 1) // 2
    return [int(v) - t if int(v) >= thr else int(v) for v in plain]


def _conv(a, b):
    """the integer product of two polynomials with non-negative coefficients: one multiplication of packed integers"""
    slot = (max(a).bit_length() + max(b).bit_length() + len(a).bit_length() + 8) // 8
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(slot, "little") for x in v), "little")
    prod = (pack(a) * pack(b)).to_bytes(slot * 2 * len(a), "little")
    return [int.from_bytes(prod[i * slot:(i + 1) * slot], "little") for i in range(2 * len(a))]


def negacyclic(a, c):
    """a (non-negative integers) times c (signed integers) in Z[x] / (x^n + 1), over the integers"""
    n = len(a)
    a = [int(x) for x in a]
    pos, neg = _conv(a, [max(x, 0) for x in c]), _conv(a, [max(-x, 0) for x in c])
    full = [x - y for x, y in zip(pos, neg)]
    return [full[i] - full[i + n] for i in range(n)]


def multiply_plain(ct, plain, t, mods):
    """BFV coefficient-form multiply_plain: ct[count][size][k][n] times the centred lift of plain[count or 1][n], as a
    negacyclic product over the integers reduced per row"""
    out = np.empty(ct.shape, dtype=np.uint64)
    for i in range(ct.shape[0]):
        c = centred(plain[i if plain.shape[0] > 1 else 0], t)
        for j in range(ct.shape[1]):
            for r, p in enumerate(mods):
                out[i, j, r] = [x % int(p) for x in negacyclic(ct[i, j, r].tolist(), c)]
    return out


def is_data_valid_for(ct, mods):
    """per item: every word is below its row's prime"""
    return np.array([all(int(item[:, r].max()) < int(p) for r, p in enumerate(mods)) for item in ct], dtype=bool)


def is_transparent(ct):
    """per item: fewer than two polynomials, or polynomials 1.. identically zero"""
    return np.array([item.shape[0] < 2 or not item[1:].any() for item in ct], dtype=bool)
