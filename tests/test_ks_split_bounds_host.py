"""The bound under which the key switch stores its digit rows without the forward transform's last layer (ntt_bounds.hpp
section 2c: fwd_split_admits), without a GPU: tests/ks_split_bounds_check.cpp checks the predicate against its recurrence on
both sides of the edge at rings 2^14..2^16, and executes the log n - 1 layers, the inner product's pair butterfly and its
128-bit sums on 64-bit words at the largest admitted prime with every true value shadowed in 128 bits."""
from support import compile_cpp, run_exe


def test_split_bound_and_execution(tmp_path):
    exe = compile_cpp(tmp_path, "ks_split_bounds_check.cpp")
    assert "ks_split_bounds_check: OK" in run_exe(exe, timeout=120)


def test_split_bound_program_under_sanitizers(tmp_path):
    """the same stand-alone program under AddressSanitizer and UBSan (host code only)"""
    exe = compile_cpp(tmp_path, "ks_split_bounds_check.cpp", sanitize=True)
    assert "ks_split_bounds_check: OK" in run_exe(exe, timeout=300)
