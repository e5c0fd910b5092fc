"""The RNS tool in plain integers, and operands solved so that its rounding decisions sit on their boundaries.

RnsRef restates RNSTool (util/rns.cpp:539-729 for the constants, :731-1126 for the functions csrc/rns.hip cites) in Python
integers: every constant is derived here from the primes alone (m_tilde = 2^32), nothing is read from the engine or the
oracle. The functions work per coefficient column on batches [items][rows][n] (numpy `object` arrays hold the integers),
follow the reference's definitions, return canonical residues as uint64 and, on request, the intermediate that decides the
branch: r_m_tilde, alpha_sk, the rounded last word, v_gamma and r.

The planters fix every other word of a column and solve one word so that the deciding intermediate takes a chosen value;
`spread` lays targets out over a batch the way linear_layer_ref.boundary_rows lays out words (every corner column, both
lanes of interior pairs). tests/test_rns_host.py holds the oracle to these integers and checks what the plants cover;
tests/test_gpu_rns.py holds the kernels to both."""
import numpy as np

import linear_layer_ref as R
import oracle_lib as O

MT = 1 << 32  # m_tilde
R_M_TILDE_TARGETS = (0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1)


class NotPlantable(ValueError):
    """no row of the chain admits every target of this plant"""


def _obj(x):
    return np.asarray(x, dtype=np.uint64).astype(object)


def _u64(x):
    return np.array(x.tolist(), dtype=np.uint64).reshape(x.shape)


def _prod(vals):
    out = 1
    for v in vals:
        out *= int(v)
    return out


def _inv(a, m):
    return pow(int(a) % m, -1, m) if m > 1 else 0


class Conv:
    """BaseConverter (rns.cpp:237-290, 452-523): punctured products of the input base, their inverses modulo their own
    prime, and the punctured products modulo each output modulus"""

    def __init__(self, ibase, obase):
        self.ibase, self.obase = [int(p) for p in ibase], [int(p) for p in obase]
        total = _prod(self.ibase)
        self.punct = [total // p for p in self.ibase]
        self.inv_punct = [_inv(h, p) for h, p in zip(self.punct, self.ibase)]
        self.matrix = [[h % o for h in self.punct] for o in self.obase]

    def scaled(self, rows):
        """x_i (q^_i)^-1 mod q_i per input row (rows: a list of object arrays)"""
        return [rows[i] * self.inv_punct[i] % p for i, p in enumerate(self.ibase)]

    def dot(self, scaled, j):
        """sum_i scaled_i q^_i mod obase[j]"""
        acc = 0
        for s, m in zip(scaled, self.matrix[j]):
            acc = acc + s * m
        return acc % self.obase[j]

    def convert(self, rows):
        s = self.scaled(rows)
        return [self.dot(s, j) for j in range(len(self.obase))]


class RnsRef:
    """the level's primes q[:k], the plain modulus t and the auxiliary primes in the order of oracle_lib.aux_primes
    (m_sk, gamma, B_0, B_1, ..)"""

    def __init__(self, q, t, aux):
        self.q, self.t, self.k = [int(p) for p in q], int(t), len(q)
        self.B_size = O.base_b_size(self.q, self.t)
        assert len(aux) >= self.B_size + 2
        self.m_sk, self.gamma = int(aux[0]), int(aux[1])
        self.B = [int(p) for p in aux[2:2 + self.B_size]]
        self.Bsk = self.B + [self.m_sk]
        self.Bsk_size = len(self.Bsk)
        every = self.q + self.Bsk + [self.gamma]
        assert len(set(every)) == len(every), "the bases must be pairwise distinct primes"
        self.prod_q, self.prod_B = _prod(self.q), _prod(self.B)
        self.q_to_Bsk = Conv(self.q, self.Bsk)
        self.q_to_m_tilde = Conv(self.q, [MT])
        self.B_to_q = Conv(self.B, self.q)
        self.B_to_m_sk = Conv(self.B, [self.m_sk])
        self.q_to_t_gamma = Conv(self.q, [self.t, self.gamma])
        self.prod_B_mod_q = [self.prod_B % p for p in self.q]
        self.prod_q_mod_Bsk = [self.prod_q % b for b in self.Bsk]
        self.inv_prod_q_mod_Bsk = [_inv(self.prod_q, b) for b in self.Bsk]
        self.inv_m_tilde_mod_Bsk = [_inv(MT, b) for b in self.Bsk]
        self.inv_prod_B_mod_m_sk = _inv(self.prod_B, self.m_sk)
        self.inv_prod_q_mod_m_tilde = _inv(self.prod_q, MT)
        self.inv_q_last_mod_q = [_inv(self.q[-1], p) for p in self.q[:-1]]
        # decrypt_scale_and_round (rns.cpp:690-716)
        self.prod_t_gamma_mod_q = [self.t * self.gamma % p for p in self.q]
        self.neg_inv_q_mod_t = (-_inv(self.prod_q, self.t)) % self.t
        self.neg_inv_q_mod_gamma = (-_inv(self.prod_q, self.gamma)) % self.gamma
        self.inv_gamma_mod_t = _inv(self.gamma, self.t)

    # ------------------------------------------------------------ helpers
    @staticmethod
    def _rows(x, count):
        x = _obj(x)
        assert x.ndim == 3 and x.shape[1] == count, (x.shape, count)
        return [x[:, r, :] for r in range(count)]

    @staticmethod
    def _stack(rows):
        return _u64(np.stack(rows, axis=1))

    # ------------------------------------------------------------ the BEHZ conversions
    def fastbconv_m_tilde(self, x):
        """rns.cpp:1025-1068: q rows -> Bsk rows and the m_tilde row of m_tilde x"""
        temp = [row * MT % p for row, p in zip(self._rows(x, self.k), self.q)]
        return self._stack(self.q_to_Bsk.convert(temp) + self.q_to_m_tilde.convert(temp))

    def r_m_tilde(self, m_tilde_row):
        """-(x q^-1) mod m_tilde (rns.cpp:945-957)"""
        return (-(m_tilde_row * self.inv_prod_q_mod_m_tilde)) % MT

    def sm_mrq(self, x, deciding=False):
        """rns.cpp:925-981: Bsk rows and the m_tilde row -> Bsk rows; r_m_tilde is taken centred, at or above 2^31 it
        stands for r - 2^32"""
        rows = self._rows(x, self.Bsk_size + 1)
        r = self.r_m_tilde(rows[-1])
        centred = np.where(r >= MT // 2, r - MT, r)
        out = [(rows[j] + self.prod_q_mod_Bsk[j] * centred) * self.inv_m_tilde_mod_Bsk[j] % b for j, b in enumerate(self.Bsk)]
        return (self._stack(out), r) if deciding else self._stack(out)

    def lift_r_m_tilde(self, x):
        """r_m_tilde of q-basis columns, as the fused lift (fastbconv_m_tilde then sm_mrq) forms it"""
        temp = [row * MT % p for row, p in zip(self._rows(x, self.k), self.q)]
        return self.r_m_tilde(self.q_to_m_tilde.convert(temp)[0])

    def fast_floor(self, x):
        """rns.cpp:983-1023: q rows and Bsk rows -> Bsk rows"""
        rows = self._rows(x, self.k + self.Bsk_size)
        conv = self.q_to_Bsk.convert(rows[:self.k])
        return self._stack([(rows[self.k + j] - conv[j]) * self.inv_prod_q_mod_Bsk[j] % b for j, b in enumerate(self.Bsk)])

    def _sk_parts(self, rows):
        scaled = self.B_to_q.scaled(rows[:self.B_size])
        conv_sk = self.B_to_m_sk.dot(scaled, 0)
        alpha = (conv_sk - rows[self.B_size]) * self.inv_prod_B_mod_m_sk % self.m_sk
        return scaled, conv_sk, alpha

    def fastbconv_sk(self, x, deciding=False):
        """rns.cpp:853-923: Bsk rows -> q rows; alpha_sk above m_sk / 2 stands for alpha_sk - m_sk"""
        rows = self._rows(x, self.Bsk_size)
        scaled, _, alpha = self._sk_parts(rows)
        centred = np.where(alpha > self.m_sk >> 1, alpha - self.m_sk, alpha)
        out = [(self.B_to_q.dot(scaled, i) - self.prod_B_mod_q[i] * centred) % p for i, p in enumerate(self.q)]
        return (self._stack(out), alpha) if deciding else self._stack(out)

    # ------------------------------------------------------------ level-down
    def divide_and_round_q_last(self, x, deciding=False):
        """rns.cpp:731-775: k rows -> k - 1 rows, round(x / q_last) through the last row plus half"""
        assert self.k >= 2
        rows = self._rows(x, self.k)
        last_p = self.q[-1]
        half = last_p >> 1
        last = (rows[-1] + half) % last_p
        out = [(rows[i] - (last % p - half % p)) * self.inv_q_last_mod_q[i] % p for i, p in enumerate(self.q[:-1])]
        return (self._stack(out), last) if deciding else self._stack(out)

    def divide_and_round_q_last_ntt(self, x, ntts, deciding=False):
        """rns.cpp:777-851: the same on NTT-form rows, NTT(divide_and_round_q_last(INTT(x))) row by row; ntts: one
        oracle_lib.MathNtt per prime of the level"""
        x = np.asarray(x, dtype=np.uint64)
        coeff = np.empty(x.shape, dtype=object)
        for i in range(x.shape[0]):
            for r in range(self.k):
                coeff[i, r] = ntts[r].inverse(x[i, r])
        out, last = self.divide_and_round_q_last(_u64(coeff), deciding=True)
        back = np.empty(out.shape, dtype=object)
        for i in range(out.shape[0]):
            for r in range(self.k - 1):
                back[i, r] = ntts[r].forward(out[i, r])
        return (_u64(back), last) if deciding else _u64(back)

    # ------------------------------------------------------------ decryption
    def _dsr_parts(self, rows):
        scaled = self.q_to_t_gamma.scaled([row * c % p for row, c, p in zip(rows, self.prod_t_gamma_mod_q, self.q)])
        vt = self.q_to_t_gamma.dot(scaled, 0) * self.neg_inv_q_mod_t % self.t
        vg = self.q_to_t_gamma.dot(scaled, 1) * self.neg_inv_q_mod_gamma % self.gamma
        return scaled, vt, vg

    def decrypt_scale_and_round(self, x, deciding=False):
        """rns.cpp:1070-1126: k rows -> one row mod t; v_gamma above gamma / 2 stands for v_gamma - gamma. Returns the
        row [items][n]; deciding: also v_gamma and r, the difference before its multiplication by gamma^-1"""
        _, vt, vg = self._dsr_parts(self._rows(x, self.k))
        centred = np.where(vg > self.gamma >> 1, vg - self.gamma, vg)
        r = (vt - centred) % self.t
        out = _u64(r * self.inv_gamma_mod_t % self.t)
        return (out, vg, r) if deciding else out

    # ------------------------------------------------------------ planters
    def _admit(self, row, bound, what):
        if self.q[row] <= bound:
            raise NotPlantable("%s: row %d (a %d-bit prime) does not admit every target" % (what, row, self.q[row].bit_length()))

    def row_above(self, bound):
        """the first row whose prime exceeds `bound`, which then admits every target below it; NotPlantable if none"""
        for r, p in enumerate(self.q):
            if p > bound:
                return r
        raise NotPlantable("no prime of the level exceeds %d" % bound)

    def plant_r_m_tilde(self, x, row, target, mask=None):
        """x with one word per column solved so that r_m_tilde = target there. row None: x is the operand of sm_mrq, and the
        m_tilde word is set. Otherwise x is a q-basis batch (the fused lift) and the word of `row` is solved:
        t_row (q^_row mod 2^32) = A (mod 2^32) has a solution below 2^32 because q^_row is odd, then x_row = t_row (m_tilde
        q^_row^-1)^-1 mod q_row; q_row must exceed 2^32. target: an integer or [items][n]; mask: the columns to plant"""
        x = np.array(x, dtype=np.uint64)
        target = np.broadcast_to(np.asarray(target, dtype=object), (x.shape[0], x.shape[2]))
        mask = np.ones(target.shape, dtype=bool) if mask is None else mask
        want = (-(target * self.prod_q)) % MT  # the m_tilde word: r = -(word prod_q^-1)
        if row is None:
            assert x.shape[1] == self.Bsk_size + 1
            x[:, -1, :][mask] = _u64(want)[mask]
            return x
        self._admit(row, MT, "plant_r_m_tilde")
        assert x.shape[1] == self.k
        p, conv = self.q[row], self.q_to_m_tilde
        temp = [r * MT % pp for r, pp in zip(self._rows(x, self.k), self.q)]
        scaled = conv.scaled(temp)
        rest = sum(s * m for i, (s, m) in enumerate(zip(scaled, conv.matrix[0])) if i != row)
        t_row = (want - rest) * _inv(conv.matrix[0][row], MT) % MT
        word = t_row * _inv(MT * conv.inv_punct[row], p) % p
        x[:, row, :][mask] = _u64(word)[mask]
        return x

    def alpha_sk_targets(self):
        m = self.m_sk
        return (0, 1, 2, self.B_size, (m - 1) // 2, (m + 1) // 2, m - self.B_size, m - 1)

    def plant_alpha_sk(self, x, target, mask=None):
        """x (Bsk rows) with the m_sk word set to conv_sk - target prod_B mod m_sk: alpha_sk = target, always solvable"""
        x = np.array(x, dtype=np.uint64)
        assert x.shape[1] == self.Bsk_size
        target = np.broadcast_to(np.asarray(target, dtype=object), (x.shape[0], x.shape[2]))
        mask = np.ones(target.shape, dtype=bool) if mask is None else mask
        _, conv_sk, _ = self._sk_parts(self._rows(x, self.Bsk_size))
        word = (conv_sk - target * self.prod_B) % self.m_sk
        x[:, -1, :][mask] = _u64(word)[mask]
        return x

    def last_words(self):
        p = self.q[-1]
        half = p >> 1
        words = [0, 1, half - 1, half, half + 1, p - half - 1, p - half, p - 2, p - 1]  # (p odd: the sixth and seventh repeat)
        return sorted(set(words))

    def plant_last(self, n, rng):
        """[count][k][n]: per row above the last, every ordered pair (boundary word of the row, last_words() word of the
        last row) in the slots of linear_layer_ref.boundary_pairs; random words below the primes after them"""
        count = max(2, -(-7 * len(self.last_words()) // n))
        x = np.empty((count, self.k, n), dtype=np.uint64)
        last = None
        for r in range(self.k - 1):
            mods = [self.q[r]]
            a, b = R.boundary_pairs(mods, n, (), R.boundary_words, lambda _p: self.last_words(), rng,
                                    fill_b=lambda _p: self.q[-1], count=count)
            x[:, r, :] = a[:, 0, :]
            if last is None:  # (boundary_pairs shifts the pairs by 3 per row index; every row here is its row 0)
                last = b[:, 0, :]
        x[:, -1, :] = last
        return x

    def vg_targets(self):
        g = self.gamma
        return (0, 1, (g - 1) // 2, (g + 1) // 2, g - 1)

    def plant_vg(self, x, row, target, mask=None):
        """x (q rows) with the word of `row` solved so that v_gamma = target: the scaled word y_row = (A - rest) (q^_row mod
        gamma)^-1 mod gamma lies below gamma, so q_row must exceed gamma; then x_row = y_row (t gamma q^_row^-1)^-1 mod q_row"""
        x = np.array(x, dtype=np.uint64)
        assert x.shape[1] == self.k
        self._admit(row, self.gamma, "plant_vg")
        target = np.broadcast_to(np.asarray(target, dtype=object), (x.shape[0], x.shape[2]))
        mask = np.ones(target.shape, dtype=bool) if mask is None else mask
        p, g, conv = self.q[row], self.gamma, self.q_to_t_gamma
        scaled, _, _ = self._dsr_parts(self._rows(x, self.k))
        rest = sum(s * m for i, (s, m) in enumerate(zip(scaled, conv.matrix[1])) if i != row)
        want = target * _inv(self.neg_inv_q_mod_gamma, g) % g
        y = (want - rest) * _inv(conv.matrix[1][row], g) % g
        word = y * _inv(self.prod_t_gamma_mod_q[row] * conv.inv_punct[row], p) % p
        x[:, row, :][mask] = _u64(word)[mask]
        return x

    def r_zero_columns(self, n):
        """[2][k][n]: the zero item, and the item whose every column is the integer 1 -- non-zero, and r = 0 exactly where
        2 t < prod q: its scaled words sum to t gamma - b prod_q + a prod_q with b = floor(t gamma / prod q) at most gamma / 2
        and 0 <= a < k, which v_t sees as b - a mod t and v_gamma, centred, as the same integer. Where 2 t >= prod q the
        integer 1 decrypts to a non-zero value (as does every other non-zero residue when t >= prod q): NotPlantable"""
        if 2 * self.t >= self.prod_q:
            raise NotPlantable("no small non-zero column decrypts to 0: 2 t >= prod q")
        x = np.zeros((2, self.k, n), dtype=np.uint64)
        x[1] = 1
        return x


# ---------------------------------------------------------------- layout of the plants
def spread(n, n_targets, items=None, pairs=False):
    """(index[items][n], items): which target a column carries, -1 where none. As linear_layer_ref.boundary_rows: columns 0,
    1, n - 2, n - 1 of item m carry targets m, m + 1, m + 2, m + 3; the interior columns, counted j = 0, 1, .. through the
    batch, carry target j / 4 in the even lane (j = 0 mod 4) and j / 4 + n_targets / 2 in the odd lane (j = 1 mod 4); all
    indices mod n_targets. `items` defaults to the fewest that put every target into both lanes and at every corner.
    pairs: the layout covers the columns below n / 2, and column c + n / 2 carries the target after that of column c, so
    that both members of (c, c + n / 2) are planted"""
    width = n // 2 if pairs else n
    assert width >= 8 and width % 4 == 0
    if items is None:
        items = max(R.lead_for(width, n_targets, corners=True), 2)
    idx = np.full((items, width), -1, dtype=np.int64)
    m = np.arange(items)
    for ci, col in enumerate(R.CORNERS):
        idx[:, col] = (m + ci) % n_targets
    inner = idx[:, 2:width - 2].reshape(-1)
    j = np.arange(inner.size)
    even, odd = j % 4 == 0, j % 4 == 1
    inner[even] = (j[even] // 4) % n_targets
    inner[odd] = (j[odd] // 4 + n_targets // 2) % n_targets
    idx[:, 2:width - 2] = inner.reshape(items, width - 4)
    if pairs:
        idx = np.concatenate([idx, np.where(idx >= 0, (idx + 1) % n_targets, -1)], axis=1)
    return idx, items


def targets_at(index, targets):
    """(target[items][n] as integers, mask) of a spread() index"""
    t = np.array([int(v) for v in targets] + [0], dtype=object)
    return t[index], index >= 0


def both_lanes(index, n_targets):
    """every target sits in an even and in an odd column"""
    even, odd = set(index[:, 0::2].ravel().tolist()), set(index[:, 1::2].ravel().tolist())
    want = set(range(n_targets))
    return want <= even and want <= odd
