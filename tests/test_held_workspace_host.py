"""The workspace blocks the DFT and bootstrap tables hold (gemini-seal_amd/csrc/held_workspace.hpp) without
a GPU: reuse, growth, the refusal during a graph capture, separate lanes and the release, over a stub pool that records takes
and releases (tests/held_workspace_check.cpp). The held blocks of the context's pool are checked on the GPU
(tests/test_gpu_homdft.py, tests/test_gpu_bootstrap.py, tests/test_gpu_bootstrap_batch.py)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_held_workspace_program_under_sanitizers(tmp_path):
    """held_workspace.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = str(tmp_path / "held_workspace_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gemini-seal_amd", "csrc"), "-o", exe,
                           os.path.join(HERE, "held_workspace_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "held_workspace_check: OK" in out.stdout, out.stdout + out.stderr
