"""The scoped pool temporaries of the polynomial drivers (gemini-seal_amd/csrc/pool_scratch.hpp) without a
GPU: the release on a return and on an exception thrown between takes, over a stub pool that records takes and releases
(tests/pool_scratch_check.cpp). The release through the context's pool is checked on the GPU (tests/test_gpu_poly_eval.py)."""
from support import compile_cpp, run_exe


def test_pool_scratch_program_under_sanitizers(tmp_path):
    """pool_scratch.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "pool_scratch_check.cpp", sanitize=True)
    assert "pool_scratch_check: OK" in run_exe(exe, timeout=120)
