"""Which instance of the single-pass NTT kernels a launch runs (gemini-seal_amd/csrc/ntt_select.hpp: select_fwd_half,
select_inv_half and the two instance tables) without a GPU: tests/ntt_select_check.cpp evaluates the rule over rings
2^14..2^16 x the environment switches x live primes on both sides of every predicate's boundary x the launch flags, gather
forms and load treatments. tests/test_host.py pins the predicates (tests/golden/ntt_instance_classes.json); this pins how the
launchers combine them."""
import json
import os

import pytest

from support import CSRC, ROOT, compile_cpp, run_exe

FIXTURE = os.path.join(ROOT, "tests", "golden", "ntt_select_table.json")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return compile_cpp(tmp_path_factory.mktemp("ntt_select"), "ntt_select_check.cpp", extra=("-I", CSRC))


def test_rule_is_closed_over_the_instance_tables_and_meets_its_anchors(exe):
    """Closure: every valid choice names an instance that exists at its ring size; all 24 forward instances are chosen at 2^15
    and 2^16, 23 at 2^14 (no mod-down store there), all 15 inverse ones at the ring sizes they serve; the rule refuses exactly
    the launches the launcher refused before the rule moved (kNttTopDone and kNttReduceOut misuse, the mod-down store without
    its FP64 instance). Anchors: the choices derived by hand from the launchers' ladders, asserted literally."""
    assert "ntt_select_check: OK" in run_exe(exe, timeout=120)


def test_select_table_fixture_is_what_the_rule_gives(exe):
    """tests/golden/ntt_select_table.json is what `ntt_select_check --table` prints: the choice for every input of the domain,
    with repeated rows of choices, and repeated maps from live sets to rows, written once each.
    The fixture was recorded from the launchers' ladders as they stood before the rule moved into the header (their conditions
    cut verbatim into two functions of the same signature); the header's functions reproduce it. A change to the rule, a
    slower-but-exact instance included, fails here."""
    stdout = run_exe(exe, "--table", timeout=120)
    with open(FIXTURE) as f:
        committed = f.read()
    assert stdout == committed
    table = json.loads(committed)
    assert sorted(table["live_sets"]) == ["14", "15", "16"]
    assert len(table["forward"]["cells"]) == len(table["inverse"]["cells"]) == 18  # rings 2^14..2^16 x six switch settings
    assert all(len(ids.split()) == len(table["forward"]["sources"]) for ids in table["forward"]["cells"].values())
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_select_program_under_sanitizers(tmp_path):
    """ntt_select.hpp compiled for the host with AddressSanitizer and UBSan into a program of its own"""
    exe = compile_cpp(tmp_path, "ntt_select_check.cpp", sanitize=True)
    assert "ntt_select_check: OK" in run_exe(exe, timeout=300)
