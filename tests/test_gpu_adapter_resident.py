"""Resident ciphertexts behind the C++ adapter and the pooled device memory under them, on the device.

tests/host_adapter_resident_check.cpp runs the cfg1 golden chain on DeviceCiphertext, compares every resident method and
destination-taking variant with its host overload word for word (BFV and CKKS, two levels, nsp 1 and 2), checks that a warm
chain makes no allocator call, the deferred transparency exception, and the wire format. The pool's C ABI is checked from
Python: same-lane reuse, cross-lane ordering, bad releases, a miss or a release during a capture, trim, destruction and
the size classes."""
import json
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
from support import S, compile_cpp, run_exe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIG = json.load(open(os.path.join(HERE, "golden", "survey_digests.json")))
MODS = [68719230977, 68719403009, 137438822401]  # cfg1: N = 4096, {36, 36, 37}


def ctx_of(S):
    return S.Context(S.SCHEME_BFV, 12, MODS, 1, 786433)


def test_cpp_resident_adapter(S, tmp_path):
    exe = compile_cpp(tmp_path, "host_adapter_resident_check.cpp", link_sealhip=True)
    cfg3 = [r for r in DIG["end_to_end"] if r["cfg"] == 3][0]
    mods3 = O.coeff_modulus_create(1 << 15, cfg3["bits"])
    stdout = run_exe(exe, "0", *mods3, timeout=600)
    # Encryptor / Decryptor resident overloads equal the host ones and round-trip; DevicePlaintext operations equal the host
    # plaintext forms; the cfg3 encrypt -> ... -> decrypt chain makes no allocator call on its second pass
    for tag in ("cfg1", "cfg3"):
        for what in ("client", "device plaintext", "warm chain"):
            assert "%s %s ok" % (what, tag) in stdout, stdout
    want = [r for r in DIG["end_to_end"] if r["cfg"] == 1][0]["digests"]["modswitch"]
    assert "resident modswitch digest " + want in stdout, stdout
    for line in ("resident equals host ok", "wire ok"):
        assert line in stdout, stdout
    assert "warm pool ok" in stdout and "transparency ok" in stdout, stdout
    # the automorphism of the resident path (equal to the host one inside the check) against the oracle's apply_galois on
    # the same words: the check's BFV operand at k = 2 (splitmix64 from seed 13), the survey's cfg1 key
    import ctypes as C

    import synth

    row = [r for r in DIG["end_to_end"] if r["cfg"] == 1][0]
    inp = synth.end_to_end_inputs(row)
    n, k, mask = 4096, 2, (1 << 64) - 1
    s, vals = 13, []
    for _ in range(2 * k * n):
        s = (s + 0x9E3779B97F4A7C15) & mask
        z = ((s ^ (s >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        vals.append(z ^ (z >> 31))
    x = np.array(vals, dtype=np.uint64).reshape(2, k, n)
    x %= np.array(MODS[:k], dtype=np.uint64)[None, :, None]
    ref = O.RefContext(1, 12, MODS, nsp=1, t=786433)
    L = O.lib()
    elt = L.ref_galois_elt_from_step(n, 1, None)
    assert L.ref_apply_galois_inplace(C.byref(ref.c), k, O.ptr(x), elt, O.ptr(inp["rk"])) == 0
    assert "apply_galois 1 digest %016x" % O.fnv(x) in stdout, stdout


def test_same_lane_reuse_is_a_hit(S):
    ctx = ctx_of(S)
    a = ctx.pool_alloc(1000)
    st0 = ctx.pool_stats()
    assert st0["misses"] == 1 and st0["device_mallocs"] == 1
    assert st0["bytes_in_use"] >= 8000 and st0["bytes_in_use"] < 8000 * 1.25 + 256
    ptr = a.ptr
    a.free()
    st1 = ctx.pool_stats()
    assert st1["bytes_in_use"] == 0 and st1["bytes_cached"] == st0["bytes_in_use"]
    b = ctx.pool_alloc(990)  # same size class
    st2 = ctx.pool_stats()
    assert b.ptr == ptr and st2["hits"] == 1 and st2["device_mallocs"] == 1 and st2["cross_lane_hits"] == 0
    b.upload(np.arange(990, dtype=np.uint64))
    assert np.array_equal(b.download(), np.arange(990, dtype=np.uint64))
    b.free()


def test_cross_lane_reuse_is_ordered(S):
    """thread A enqueues a long write into a block and releases it without waiting; thread B takes the block (a cross-lane
    hit, its stream waits on the release event) and writes it: after a synchronise, B's words are in the block"""
    ctx = ctx_of(S)
    words = 1 << 24  # 128 MiB
    src_a = ctx.upload(np.full(words, 0xAAAA, dtype=np.uint64))
    src_b = ctx.upload(np.full(words, 0xBBBB, dtype=np.uint64))
    ctx.synchronize()
    released, b_ready, b_done = threading.Event(), threading.Event(), threading.Event()
    box, errors = {}, []

    def thread_a():
        try:
            b_ready.wait()  # B holds its own lane before A's exists (an exited thread's lane is handed to the next one)
            blk = ctx.pool_alloc(words)
            box["ptr"] = blk.ptr
            for _ in range(16):  # ~2 GiB of copies queued on A's lane
                ctx.memcpy_d2d(blk, src_a, words)
            blk.free()  # stream-ordered: returns at once
        except Exception as e:  # pragma: no cover - reported below
            errors.append(e)
        finally:
            released.set()
            b_done.wait()

    def thread_b():
        try:
            ctx.memcpy_d2d(src_b, src_b, 0)  # takes this thread's lane
            b_ready.set()
            released.wait()
            blk = ctx.pool_alloc(words)
            box["ptr_b"] = blk.ptr
            ctx.memcpy_d2d(blk, src_b, words)
            box["blk"] = blk
        except Exception as e:  # pragma: no cover
            errors.append(e)
        finally:
            b_ready.set()
            b_done.set()

    ta, tb = threading.Thread(target=thread_a), threading.Thread(target=thread_b)
    ta.start()
    tb.start()
    ta.join()
    tb.join()
    assert not errors, errors
    ctx.synchronize()
    assert box["ptr_b"] == box["ptr"]
    st = ctx.pool_stats()
    assert st["cross_lane_hits"] == 1 and st["device_mallocs"] == 1
    got = box["blk"].download()
    assert (got == 0xBBBB).all()
    box["blk"].free()


def test_bad_release(S):
    import ctypes as C

    ctx = ctx_of(S)
    L = S.lib()
    other = ctx.alloc(16)  # sealhip_malloc, not the pool
    assert L.sealhip_pool_release(ctx.handle, other.ptr) == S.E_INVALIDARG
    blk = ctx.pool_alloc(16)
    ptr = blk.ptr
    blk.free()
    assert L.sealhip_pool_release(ctx.handle, ptr) == S.E_INVALIDARG  # twice
    assert "already released" in L.sealhip_last_error_string().decode()
    st = ctx.pool_stats()
    assert st["device_frees"] == 0 and st["bytes_cached"] > 0  # nothing was freed
    p = C.c_void_p()
    assert L.sealhip_pool_alloc(ctx.handle, 16 * 8, C.byref(p)) == S.S_OK and p.value == ptr
    assert L.sealhip_pool_release(ctx.handle, p.value) == S.S_OK


def test_miss_during_capture(S):
    import ctypes as C

    ctx = ctx_of(S)
    L = S.lib()
    warm = ctx.pool_alloc(64)
    warm.free()
    ctx.synchronize()
    assert L.sealhip_graph_capture_begin(ctx.handle) == S.S_OK
    p = C.c_void_p()
    hit = L.sealhip_pool_alloc(ctx.handle, 64 * 8, C.byref(p))  # cached on this lane: allowed
    assert hit == S.S_OK
    held = p.value
    hr = L.sealhip_pool_alloc(ctx.handle, 1 << 20, C.byref(p))  # a miss
    assert hr == S.COR_E_INVALIDOPERATION
    msg = L.sealhip_last_error_string().decode()
    assert "graph capture" in msg and "discarded" in msg, msg
    g = C.c_void_p()
    assert L.sealhip_graph_capture_end(ctx.handle, C.byref(g)) != S.S_OK  # nothing left to end
    # a release during a capture is refused too (a replay of the graph would still use the block)
    assert L.sealhip_graph_capture_begin(ctx.handle) == S.S_OK
    assert L.sealhip_pool_release(ctx.handle, held) == S.COR_E_INVALIDOPERATION
    assert "discarded" in L.sealhip_last_error_string().decode()
    assert L.sealhip_graph_capture_end(ctx.handle, C.byref(g)) != S.S_OK
    assert L.sealhip_pool_release(ctx.handle, held) == S.S_OK  # after the capture: fine
    # the lane works normally afterwards
    b = ctx.pool_alloc(1 << 17)
    b.upload(np.arange(1 << 17, dtype=np.uint64))
    assert np.array_equal(b.download(), np.arange(1 << 17, dtype=np.uint64))


def test_trim_and_destroy(S):
    ctx = ctx_of(S)
    blocks = [ctx.pool_alloc(w) for w in (10, 1000, 100000, 100000)]
    for b in blocks[:3]:
        b.free()
    st = ctx.pool_stats()
    assert st["bytes_cached"] > 0 and st["device_mallocs"] == 4
    ctx.pool_trim()
    st = ctx.pool_stats()
    assert st["bytes_cached"] == 0 and st["device_frees"] == 3 and st["bytes_in_use"] > 0
    # destroying the context with a block still held (and one cached) frees both
    c = ctx_of(S)
    held = c.pool_alloc(4096)
    c.pool_alloc(8).free()
    held.ptr = None  # the context owns it now
    assert S.lib().sealhip_context_destroy(c.handle) == S.S_OK
    c.handle = None


@pytest.mark.parametrize("nbytes,cls", [(1, 256), (256, 256), (257, 512), (513, 768), (1025, 1280), (1281, 1536),
                                        (1792, 1792), (1793, 2048), (2049, 2560), (100000, 114688), (1 << 20, 1 << 20),
                                        ((1 << 20) + 1, 1310720)])
def test_size_classes(S, nbytes, cls):
    """the rounding rule of the header: a multiple of 256 bytes, then the next m * 2^e with m in 4..7"""
    import ctypes as C

    ctx = ctx_of(S)
    L = S.lib()
    p = C.c_void_p()
    assert L.sealhip_pool_alloc(ctx.handle, nbytes, C.byref(p)) == S.S_OK
    assert ctx.pool_stats()["bytes_in_use"] == cls
    assert cls < 1.25 * ((nbytes + 255) // 256 * 256) or cls == (nbytes + 255) // 256 * 256
    assert L.sealhip_pool_release(ctx.handle, p.value) == S.S_OK
