"""The key switch whose digit rows are stored without the forward transform's last layer, word for word
against the CPU oracle.

ks_products launches the digit transforms with kNttSplitLast (each half-row workgroup transforms one parity class of the
gathered row as a ring of N/2) and the inner product's pair form (ks_mac_pair_kernel) applies the last layer, where the
launches select an integer instance of that form, the batch has at least 16 items and the level's primes lie in
bounds::fwd_split_admits; everything else runs the whole-row launches. Ring 2^14 (the smallest single-pass ring), two
ciphertext primes and one special prime:
  p55    55 + 55 | 55 bits: no load treatment (the conditional subtraction is dropped under fwd_lazy_admits), taken;
  mixed  40 + 55 | 58 bits: Barrett-63 on load (a source prime reaches twice a destination prime), taken. (The conditional
         subtraction survives in ks_digits only where a prime is outside fwd_lazy_admits, which at this ring is where
         fwd_split_admits refuses as well -- a 58-bit prime at 2^16 is the one place the pipeline reaches that instance:
         tests/test_gpu_ks_instances.py goes there (its pair rings), and the kernel-level test below runs it at every ring.)
  p59    59 + 59 | 61 bits: outside the bound -- the query says 0 and the whole-row launches give the same words.
Batches of 16 (two full groups of eight), 17 (and a remainder of one) and 1 (ks_mac_kernel: never split). Item i of a batch
holds pattern i mod 5: random, every word p - 1, zero, p - 1 on even and 0 on odd indices, the reverse. BFV relinearize on
all three sets, CKKS relinearize on p55, one rotation (BFV, p55). No tolerance: every compared word is equal or the test fails.

The kernel-level test runs one split launch through sealhip_debug_ntt_split_last, finishes the last layer on the host with
the ORACLE's root powers (X[2j] = E[j] + w O[j], X[2j+1] = E[j] - w O[j], w = root_powers[N/2 + j]) and compares the canonical
residues with ref_ntt_forward of the whole row: the six (treatment, exact) instances at each of the rings 2^14, 2^15 and 2^16.
A launch that asks for the approximate schedule on a prime outside fwd_lazy_admits gets the exact one, so at 2^16, where that
bound is 57 bits, the approximate Barrett cell takes the 55-bit prime and the exact one the 58-bit prime (what the pipeline
runs there). The pipeline runs of the larger rings are in tests/test_gpu_ks_instances.py."""
import ctypes as C

import numpy as np
import pytest

import hoist_ref as H
import oracle_lib as O
from support import BaseSession, S, rows  # noqa: F401 (S: the device fixture)
from test_ks_instances_host import LAZY_BITS

pytestmark = pytest.mark.gpu

BFV, CKKS = 1, 2
LOGN = 14
SETS = {"p55": [55, 55, 55], "mixed": [40, 55, 58], "p59": [59, 59, 61]}
ADMITTED = {"p55": True, "mixed": True, "p59": False}
BATCHES = (16, 17, 1)


class Session(BaseSession):
    def __init__(self, S, scheme, name, logn=LOGN):
        super().__init__(S, scheme, logn, SETS[name], 1, 0, 65537 if scheme == BFV else 0, 18 + sum(name.encode()) + scheme)
        self.name = name
        self.key_host = rows(self.rng, self.mods, self.n, (self.nd, 2))
        self.key_dev = S.KSwitchKeys(self.ctx, self.key_host)

    def ciphertexts(self, k, count, size):
        """item i holds pattern i mod 5"""
        ct = rows(self.rng, self.mods[:k], self.n, (count, size))
        for i in range(count):
            if i % 5 == 0:
                continue
            hi = np.empty((size, k, self.n), dtype=np.uint64)
            for r, p in enumerate(self.mods[:k]):
                hi[:, r, :] = p - 1
            if i % 5 == 2:
                hi[:] = 0
            elif i % 5 == 3:
                hi[..., 1::2] = 0
            elif i % 5 == 4:
                hi[..., 0::2] = 0
            ct[i] = hi
        return ct

    def expect_split(self, k, count):
        taken = self.ctx.debug_ks_split_last(k, count)
        assert taken == (ADMITTED[self.name] and count >= 16), (self.name, count, taken)

    def relinearize(self, count):
        L, k = O.lib(), self.k_first
        self.expect_split(k, count)
        ct = self.ciphertexts(k, count, 3)
        d = self.ctx.upload(ct)
        self.ev.relinearize_inplace(d, 3, k, count, [self.key_dev])
        got = d.download(ct.shape)
        d.free()
        keys = (C.c_void_p * 1)(self.key_host.ctypes.data)
        for c in range(count):
            want = ct[c].copy()
            assert L.ref_relinearize(C.byref(self.ref.c), k, O.ptr(want), 3, keys) == 0
            assert np.array_equal(got[c, :2], want[:2]), (self.name, "relinearize", count, "item", c)

    def rotate(self, count):
        L, k = O.lib(), self.k_first
        self.expect_split(k, count)
        elt = H.elt_from_step(self.n, 1)
        ct = self.ciphertexts(k, count, 2)
        d = self.ctx.upload(ct)
        self.ev.apply_galois_inplace(d, k, count, elt, self.key_dev)
        got = d.download(ct.shape)
        d.free()
        for c in range(count):
            want = ct[c].copy()
            assert L.ref_apply_galois_inplace(C.byref(self.ref.c), k, O.ptr(want), elt, O.ptr(self.key_host)) == 0
            assert np.array_equal(got[c], want), (self.name, "rotate", count, "item", c)


@pytest.fixture(scope="module")
def sessions(S):
    made = {}

    def get(scheme, name, logn=LOGN):
        if (scheme, name, logn) not in made:
            made[scheme, name, logn] = Session(S, scheme, name, logn)
        return made[scheme, name, logn]

    return get


@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("count", BATCHES)
def test_bfv_relinearize_equals_the_oracle(sessions, name, count):
    sessions(BFV, name).relinearize(count)


@pytest.mark.parametrize("count", BATCHES)
def test_ckks_relinearize_equals_the_oracle(sessions, count):
    sessions(CKKS, "p55").relinearize(count)


def test_rotation_equals_the_oracle(sessions):
    sessions(BFV, "p55").rotate(17)


def test_split_launch_is_refused_outside_the_bound(sessions):
    """a 59-bit row is outside bounds::fwd_split_admits: the entry refuses, it does not transform the row whole"""
    se = sessions(BFV, "p59")
    src, dst = se.ctx.upload(np.zeros(se.n, dtype=np.uint64)), se.ctx.alloc(se.n)
    with pytest.raises(Exception):
        se.ctx.debug_ntt_split_last(0, src, dst, 0, False)
    src.free()
    dst.free()


SPLIT_CELLS = [("p55", 0, 0, False), ("p55", 2, 0, True), ("mixed", 2, 1, False), ("mixed", 1, 1, True), ("p55", 1, 2, False),
               ("mixed", 2, 2, True)]


def split_cell(logn, name, prime_index, treatment):
    """the prime of a cell: at 2^16 the two Barrett cells trade primes (the 58-bit one has no approximate schedule there)"""
    if logn == 16 and name == "mixed" and treatment == 1:
        return 3 - prime_index
    return prime_index


@pytest.mark.parametrize("logn", [14, 15, 16])
@pytest.mark.parametrize("name,prime_index,treatment,exact", SPLIT_CELLS)
def test_split_launch_finished_on_the_host_is_the_whole_transform(sessions, name, prime_index, treatment, exact, logn):
    se = sessions(BFV, name, logn)
    prime_index = split_cell(logn, name, prime_index, treatment)
    n, p = se.n, se.mods[prime_index]
    assert exact or int(p).bit_length() <= LAZY_BITS[logn]  # (else the launch would run the exact instance under this name)
    rng = np.random.default_rng(1800 + prime_index)
    # treatment 1 (Barrett-63): words of another, larger key prime -- anything below 2^63; else canonical residues
    # treatment 2 (one conditional subtraction): words of a key prime below 2p
    x = rng.integers(0, (1 << 62) if treatment == 1 else (2 * p if treatment == 2 else p), size=n, dtype=np.uint64)
    x[:4] = [p - 1, 0, p - 1, p - 1]
    if treatment == 2:
        x[4:8] = [p, 2 * p - 1, p, 2 * p - 1]
    src, dst = se.ctx.upload(x), se.ctx.alloc(n)
    se.ctx.debug_ntt_split_last(prime_index, src, dst, treatment, exact)
    got = dst.download((n,))
    src.free()
    dst.free()
    tables = O.Tables(logn, p)
    w = [int(v) for v in tables.arr("root_powers")]
    e, o = [int(v) for v in got[: n // 2]], [int(v) for v in got[n // 2:]]
    bound = (2 + 4 * (logn - 1)) * p  # bounds::fwd_split_output_mult
    assert max(e) < bound and max(o) < bound
    full = np.empty(n, dtype=np.uint64)
    for j in range(n // 2):
        t = w[n // 2 + j] * o[j] % p
        full[2 * j] = (e[j] + t) % p
        full[2 * j + 1] = (e[j] - t) % p
    want = (x % np.uint64(p)).astype(np.uint64)
    O.lib().ref_ntt_forward(O.ptr(want), C.byref(tables.t), 0)
    assert np.array_equal(full, want % np.uint64(p)), (logn, name, prime_index, treatment, exact)
