"""The scoped pool temporaries of the polynomial drivers (gemini-seal_amd/csrc/pool_scratch.hpp) without a
GPU: the release on a return and on an exception thrown between takes, over a stub pool that records takes and releases
(tests/pool_scratch_check.cpp). The release through the context's pool is checked on the GPU (tests/test_gpu_poly_eval.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pool_scratch_program_under_sanitizers(tmp_path):
    """pool_scratch.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = str(tmp_path / "pool_scratch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gemini-seal_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "pool_scratch_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "pool_scratch_check: OK" in out.stdout, out.stdout + out.stderr
