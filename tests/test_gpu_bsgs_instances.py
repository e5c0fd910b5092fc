"""hoist_giant_mac_kernel<1..16> (hoist.hip) at the accumulator's worst case, word for word against the
CPU restatement of tests/hoist_bsgs_ref.py.

launch_hoist_giant_mac picks a template instance from the level's digit count nd = ceil(k / nsp). As the extremes section of
tests/test_gpu_ks_instances.py: seventeen 61-bit primes (the widest the context admits), N = 2^10 (four workgroups per row),
nsp = 1, so level k runs instance ND = k; every ciphertext, key and plaintext word is p - 1; and 16 distinct non-identity
giants go in ONE launch, each with its acc_j -- the most terms that meet in the kernel's running sums before it writes:
per giant one inner product of ND products (below ND * 2^122) reduced at once, and its gathered acc_j[0] word. Babies
[g, 1], five ciphertexts (lanes of 4 + 1); the first and the last are compared. No tolerance is involved."""
import numpy as np
import pytest

import hoist_bsgs_ref as HB
import hoist_ref as H
import oracle_lib as O
from support import top

pytestmark = pytest.mark.gpu

LOGN, N = 10, 1 << 10
BITS = [61] * 17
COUNT, ITEMS = 5, (0, 4)
LEVELS = {"1_4": range(1, 5), "5_8": range(5, 9), "9_12": range(9, 13), "13_16": range(13, 17)}


def giants(n):
    """16 distinct elements other than 1: a rotation by one step, conjugation, then odd elements"""
    out = [H.elt_from_step(n, 1), 2 * n - 1]
    g = 3
    while len(out) < 16:
        if g not in out:
            out.append(g)
        g += 2
    return out


@pytest.fixture(scope="module")
def session():
    import sealhip as S

    assert S.num_devices() >= 1
    mods = O.coeff_modulus_create(N, BITS)
    ctx = S.Context(S.SCHEME_CKKS, LOGN, mods, 1, 0)
    ref = O.RefContext(2, LOGN, mods, nsp=1)
    key = top(mods, N, (16, 2))
    # every row of the key is constant, so sigma_{g^-1} of it (H.hoisted_key) is the key itself
    assert np.array_equal(H.hoisted_key(ref, key, 3), key)
    return S, mods, ctx, ref, S.Evaluator(ctx), key, S.KSwitchKeys(ctx, key)


@pytest.mark.parametrize("levels", list(LEVELS))
def test_sixteen_giants_in_one_launch_at_every_instance(session, levels):
    S, mods, ctx, ref, ev, key, dkey = session
    giant = giants(N)
    baby = [giant[2], 1]
    plains = top(mods, N, (len(giant), len(baby)))
    dp = ctx.upload(plains)
    for k in LEVELS[levels]:
        ct = top(mods[:k], N, (COUNT, 2))
        d = ctx.upload(ct)
        out = ctx.alloc(COUNT * 2 * k * N)
        ctx.profile_enable(True)
        ev.apply_galois_bsgs_plain(d, k, COUNT, baby, [dkey, None], giant, [dkey] * 16, dp, out)
        prof = ctx.profile_fetch()
        ctx.profile_enable(False)
        assert prof["hoist_giant_mac"]["launches"] == 1, (k, prof)
        got = out.download((COUNT, 2, k, N))
        for c in ITEMS:
            want = HB.bsgs_one(ref, k, ct[c], baby, [key, None], giant, [key] * 16, plains, [key, None], [key] * 16)
            assert np.array_equal(got[c], want), ("level", k, "item", c)
        d.free()
        out.free()
