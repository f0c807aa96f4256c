"""CPU: the kernel-choice switches of the library (fi_set_option / flashinfer._lib.set_option).  Each starts as the
environment gave it when the library was loaded, a set value wins, and None returns it to the environment's value.
No kernel is launched here."""
import os
import subprocess
import sys

import pytest

from flashinfer import _lib
from oracle.plan_ref import decode_plan_ref
from plan_calls import run_plan


@pytest.fixture
def num_cus(fi_lib):
    """Sets FI_NUM_CUS for the test and returns it to the environment's value afterwards."""
    try:
        yield lambda value: _lib.set_option("FI_NUM_CUS", value)
    finally:
        _lib.set_option("FI_NUM_CUS", None)


def test_unknown_name_is_refused_and_named(fi_lib):
    assert fi_lib.fi_set_option(b"FI_NO_SUCH_SWITCH", b"1") != 0
    assert b"FI_NO_SUCH_SWITCH" in fi_lib.fi_last_error()
    with pytest.raises(RuntimeError, match="FI_NO_SUCH_SWITCH"):
        _lib.set_option("FI_NO_SUCH_SWITCH", None)


@pytest.mark.parametrize("value", [b"", b"abc", b"1.5", b"7x", b" ", b"99999999999999999999"])
def test_value_that_is_no_integer_is_refused(fi_lib, num_cus, value):
    num_cus(7)
    assert fi_lib.fi_set_option(b"FI_NUM_CUS", value) != 0
    assert b"not an integer" in fi_lib.fi_last_error()
    assert fi_lib.fi_num_compute_units() == 7  # a refused value changes nothing


def test_num_cus_set_restore_and_ignored_values(fi_lib, num_cus):
    before = fi_lib.fi_num_compute_units()
    num_cus(7)
    assert fi_lib.fi_num_compute_units() == 7
    num_cus(None)
    assert fi_lib.fi_num_compute_units() == before
    for ignored in (0, -3):  # a value <= 0 is no CU count: the device's (or the 256 without one) stands
        num_cus(ignored)
        assert fi_lib.fi_num_compute_units() == before


def test_set_value_wins_over_the_environment_and_none_returns_to_it():
    """One child with FI_NUM_CUS=11 in its environment; it binds the two calls itself, so it starts in no time."""
    code = ("import ctypes, sys\n"
            "l = ctypes.CDLL(sys.argv[1])\n"
            "l.fi_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]\n"
            "seen = [l.fi_num_compute_units()]\n"
            "assert l.fi_set_option(b'FI_NUM_CUS', b'5') == 0; seen.append(l.fi_num_compute_units())\n"
            "assert l.fi_set_option(b'FI_NUM_CUS', None) == 0; seen.append(l.fi_num_compute_units())\n"
            "print(seen)\n")
    r = subprocess.run([sys.executable, "-c", code, _lib._LIB_PATH], env=dict(os.environ, FI_NUM_CUS="11"),
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "[11, 5, 11]"


def test_decode_planner_sizes_its_grid_for_the_set_cu_count(fi_lib, num_cus):
    """max_grid_hint = 0: the planner's grid is 4 waves per CU (16-bit cache, one head tile, one kv head).  Requests of
    64 pages are cut while two chunks each still fit the grid: up to 8 requests on the 16 waves of 4 CUs, up to 16 on
    the 32 waves of 8 CUs.  9 requests are the fewest that split at 8 CUs and not at 4."""
    def plan(batch, n):
        num_cus(n)
        indptr = [64 * i for i in range(batch + 1)]
        got = run_plan(fi_lib, indptr, 1, 1, 16, max_grid=0)
        exp = decode_plan_ref(indptr, 1, 1, 16, max_grid=4 * n)
        for key in ("split_kv", "kv_chunk_size", "padded_batch_size", "num_work", "request_indices",
                    "kv_tile_indices", "o_indptr"):
            assert got[key] == exp[key], (batch, n, key)
        return got

    assert not plan(9, 4)["split_kv"] and plan(9, 8)["split_kv"]
    assert plan(8, 4)["split_kv"] and plan(8, 8)["split_kv"]


def test_second_read_after_set_and_none_sees_the_environment(fi_lib):
    """What the variant fixtures of the GPU suites rely on: set, None, and every later read is the environment's."""
    before = fi_lib.fi_num_compute_units()
    for name, value in (("FI_NUM_CUS", 3), ("FI_DECODE_MFMA16", 0), ("FI_GEMM_BIG_MIN_TILES", 0)):
        _lib.set_option(name, value)
        _lib.set_option(name, None)
    assert fi_lib.fi_num_compute_units() == before
    assert fi_lib.fi_num_compute_units() == before
    indptr = [64 * i for i in range(10)]
    first = run_plan(fi_lib, indptr, 1, 1, 16, max_grid=0)
    _lib.set_option("FI_NUM_CUS", 4)
    _lib.set_option("FI_NUM_CUS", None)
    again = run_plan(fi_lib, indptr, 1, 1, 16, max_grid=0)
    assert {k: v for k, v in again.items() if k != "info"} == {k: v for k, v in first.items() if k != "info"}
