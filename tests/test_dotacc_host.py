"""csrc/dotacc.hpp on the host: the carry-free dot product of the exact-k BEHZ instances (four multiplier instructions per
term, both factors split at bit 31) is plain 64-bit arithmetic, so the header the kernels include runs here against
unsigned __int128 (tests/dotacc_check.cpp): every accumulator below 2^64 at every term count 1..17 on operands all
2^61 - 1 / all 0 / alternating / random, the assembled sum exact, the packed constant round-trips."""
import pytest

from support import CSRC, compile_cpp, run_exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_dotacc31_against_int128(tmp_path, sanitize):
    """both flavours with warnings as errors; the plain one sees csrc/ too"""
    extra = ("-Wall", "-Werror") + (() if sanitize else ("-I", CSRC))
    exe = compile_cpp(tmp_path, "dotacc_check.cpp", sanitize=sanitize, extra=extra)
    assert "dotacc_check: OK" in run_exe(exe, timeout=300)
