"""csrc/dotacc.hpp on the host: the carry-free dot product of the exact-k BEHZ instances (four multiplier instructions per
term, both factors split at bit 31) is plain 64-bit arithmetic, so the header the kernels include runs here against
unsigned __int128 (tests/dotacc_check.cpp): every accumulator below 2^64 at every term count 1..17 on operands all
2^61 - 1 / all 0 / alternating / random, the assembled sum exact, the packed constant round-trips."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_dotacc31_against_int128(tmp_path, flags):
    exe = str(tmp_path / "dotacc_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "gemini-seal_amd", "csrc"), "-o", exe, os.path.join(HERE, "dotacc_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dotacc_check: OK" in out.stdout, out.stdout + out.stderr
