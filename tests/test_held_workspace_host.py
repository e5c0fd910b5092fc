"""The workspace blocks the DFT and bootstrap tables hold (gemini-seal_amd/csrc/held_workspace.hpp) without
a GPU: reuse, growth, the refusal during a graph capture, separate lanes and the release, over a stub pool that records takes
and releases (tests/held_workspace_check.cpp). The held blocks of the context's pool are checked on the GPU
(tests/test_gpu_homdft.py, tests/test_gpu_bootstrap.py, tests/test_gpu_bootstrap_batch.py)."""
from support import compile_cpp, run_exe


def test_held_workspace_program_under_sanitizers(tmp_path):
    """held_workspace.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "held_workspace_check.cpp", sanitize=True)
    assert "held_workspace_check: OK" in run_exe(exe, timeout=120)
