"""CPU: plan_info slot FI_DP_UNIFORM_CHUNKS of the batch-decode planner (through the C ABI, host-only mode).

The slot is n in {2, 4} when the plan is split, is no graph plan, has no planned window and EVERY request is cut into
exactly n chunks; else 0.  run() uses it to merge the chunks inside the decode launch.  Slots 0-15 and the work list
stay what the Python restatement of the planner (oracle/plan_ref.py) gives.  All plans are made for the MI355X grid of
a 16-bit cache: 256 CUs x 4 waves = 1024, page 16 (chunks of 128 tokens unless stated)."""
import pytest

import plan_calls
from attn_inputs import indptr_of
from flashinfer import _lib
from oracle.plan_ref import decode_plan_ref

MAX_GRID = 1024
PAGE = 16


def run_plan(fi_lib, pages, hq, hkv, cuda_graph=False, window_left=-1):
    got = plan_calls.run_plan(fi_lib, indptr_of(pages).tolist(), hq, hkv, PAGE, MAX_GRID, cuda_graph,
                              window_left=window_left)
    return got["info"], got


def check_against_oracle(got, pages, hq, hkv, cuda_graph=False, window_left=-1):
    exp = decode_plan_ref(indptr_of(pages).tolist(), hq, hkv, PAGE, MAX_GRID, cuda_graph, window_left=window_left)
    for key in ("split_kv", "kv_chunk_size", "padded_batch_size", "num_work", "request_indices", "kv_tile_indices",
                "o_indptr"):
        assert got[key] == exp[key], key
    return exp


CASES = [
    # (pages per request, hq, hkv, expected slot, chunks per request)
    ([16, 16, 16], 8, 2, 2, [2, 2, 2]),
    ([9, 12, 16], 8, 2, 2, [2, 2, 2]),          # ragged tails: 2 chunks each all the same
    ([512] * 64, 32, 8, 2, [2] * 64),           # C2: two chunks of 4096 tokens
    ([32, 32], 8, 2, 4, [4, 4]),
    ([32], 4, 1, 4, [4]),
    ([256] * 32, 32, 8, 4, [4] * 32),           # batch 32 x kv 4096: chunks of 1024 tokens
    ([24, 24, 24], 8, 2, 0, [3, 3, 3]),         # uniform, but 3 chunks do not fill a workgroup evenly
    ([16, 32], 8, 2, 0, [2, 4]),
    ([0, 16], 8, 2, 0, [1, 2]),                 # an empty request still takes one chunk
    ([128] * 16, 32, 8, 0, [8] * 16),           # batch 16 x kv 2048: 8 chunks of 256 tokens
    ([512] * 128, 32, 8, 0, [1] * 128),         # whole requests fill the grid: no split
]


@pytest.mark.parametrize("pages,hq,hkv,slot,chunks", CASES)
def test_uniform_chunks_slot(fi_lib, pages, hq, hkv, slot, chunks):
    info, got = run_plan(fi_lib, pages, hq, hkv)
    check_against_oracle(got, pages, hq, hkv)
    per_request = [b - a for a, b in zip(got["o_indptr"], got["o_indptr"][1:])]
    assert per_request == chunks            # the case is what its comment says
    assert len(info) == 17 and _lib.FI_DP_UNIFORM_CHUNKS == 16
    assert info[_lib.FI_DP_UNIFORM_CHUNKS] == slot
    if slot:
        assert got["split_kv"] and info[_lib.FI_DP_ENABLE_CUDA_GRAPH] == 0 and info[_lib.FI_DP_WINDOW_LEFT] == -1


def test_c2_plan_is_unchanged_and_uniform(fi_lib):
    info, got = run_plan(fi_lib, [512] * 64, 32, 8)
    assert got["split_kv"] and got["kv_chunk_size"] == 4096 and got["num_work"] == 128
    assert info[_lib.FI_DP_UNIFORM_CHUNKS] == 2
    # the partial-state region is still reserved: the two-launch path needs it
    assert info[_lib.FI_DP_S_OFFSET] - info[_lib.FI_DP_V_OFFSET] >= 32 * 128 * 128 * 4


@pytest.mark.parametrize("pages,hq,hkv", [([16, 16, 16], 8, 2), ([32, 32], 8, 2), ([512] * 64, 32, 8)])
def test_graph_plans_never_report_uniform_chunks(fi_lib, pages, hq, hkv):
    info, got = run_plan(fi_lib, pages, hq, hkv, cuda_graph=True)
    check_against_oracle(got, pages, hq, hkv, cuda_graph=True)
    assert got["split_kv"] and info[_lib.FI_DP_UNIFORM_CHUNKS] == 0


@pytest.mark.parametrize("window_left", [0, 100, 255, 100000])
def test_window_plans_never_report_uniform_chunks(fi_lib, window_left):
    pages = [16, 16, 16]
    info, got = run_plan(fi_lib, pages, 8, 2, window_left=window_left)
    check_against_oracle(got, pages, 8, 2, window_left=window_left)
    assert info[_lib.FI_DP_WINDOW_LEFT] == window_left and info[_lib.FI_DP_UNIFORM_CHUNKS] == 0


def test_slots_0_to_15_do_not_depend_on_the_new_slot(fi_lib):
    """The same page counts planned as a graph plan and as a plain one differ only where they always did; within one
    mode the first sixteen slots of a uniform plan are those of the work list the oracle gives (checked above) and the
    workspace offsets follow from it."""
    info, got = run_plan(fi_lib, [16, 16, 16], 8, 2)
    padded = got["padded_batch_size"]
    assert info[_lib.FI_DP_PADDED_BATCH_SIZE] == padded == 6
    assert info[_lib.FI_DP_NUM_WORK] == 6 and info[_lib.FI_DP_BATCH_SIZE] == 3
    assert info[_lib.FI_DP_V_OFFSET] == 0 and info[_lib.FI_DP_S_OFFSET] == 8 * padded * 128 * 4  # tmp_v, then tmp_s
    assert info[_lib.FI_DP_REQUEST_INDICES_OFFSET] == 0 and info[_lib.FI_DP_KV_TILE_INDICES_OFFSET] >= 4 * padded
    assert info[_lib.FI_DP_O_INDPTR_OFFSET] >= info[_lib.FI_DP_KV_TILE_INDICES_OFFSET] + 4 * padded
    assert info[15] == 0x4649444543
