"""CPU: the planner and C ABI for prefill with head_dim_qk 192 / head_dim_vo 128 (host-only plans, int_ws = NULL, as
tests/test_plan.py).  No kernel is launched here."""
import ctypes as C
import json
import os

import pytest

from flashinfer import _lib
from plan_calls import prefill_qkvo_plan as plan

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "prefill_plans_equal_dims.json")
ENTRY_ALIGN = 256  # slack for the workspace allocator's alignment of the two partial-state regions


def entries(qo_lens, kv_lens, chunk):
    return sum(q * -(-max(k, 1) // chunk) for q, k in zip(qo_lens, kv_lens))


def test_new_symbols_are_exported(fi_lib):
    for s in ("fi_batch_prefill_qkvo_run", "fi_single_prefill_qkvo_run"):
        assert s in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, s)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("shape", [([1024] * 16, [1024] * 16, 128, 128), ([377, 177, 1], [544, 977, 0], 32, 8),
                                   ([8192], [8192], 16, 16), ([3928], [7563], 128, 128)])
def test_plan_192_128_succeeds_and_is_tagged(fi_lib, shape, graph):
    qo_lens, kv_lens, hq, hkv = shape
    rc, info, lists = plan(fi_lib, qo_lens, kv_lens, hq, hkv, 192, 128, graph=graph, float_bytes=1 << 34)
    assert rc == 0, fi_lib.fi_last_error()
    assert info[_lib.FI_PP_MAGIC] == _lib.FI_PREFILL_QKVO_PLAN_MAGIC != _lib.FI_PREFILL_PLAN_MAGIC
    assert info[_lib.FI_PP_CTA_TILE_Q] == 128  # q tile
    # every (request, q tile) appears, once per kv chunk
    g = hq // hkv
    items = {(r, t) for r, t in zip(lists["req"], lists["tile"]) if r >= 0}
    assert items == {(b, t) for b, q in enumerate(qo_lens) for t in range(-(-q * g // 128))}


def test_forced_split_workspace_is_sized_by_head_dim_vo(fi_lib):
    """A forced split fits in entries x Hq x (128 + 1) x 4 bytes (plus allocator alignment) and is refused below the
    entries x Hq x (128 + 1) x 4 bytes the partial states need."""
    qo_lens, kv_lens, hq, hkv, chunk = [100, 37], [1000, 3000], 16, 4, 256
    need = entries(qo_lens, kv_lens, chunk) * hq * (128 + 1) * 4
    rc, info, _ = plan(fi_lib, qo_lens, kv_lens, hq, hkv, 192, 128, float_bytes=need + ENTRY_ALIGN,
                       fixed_split=chunk)
    assert rc == 0, fi_lib.fi_last_error()
    assert info[_lib.FI_PP_SPLIT_KV] == 1 and info[_lib.FI_PP_KV_CHUNK_SIZE] == chunk
    rc, _, _ = plan(fi_lib, qo_lens, kv_lens, hq, hkv, 192, 128, float_bytes=need - 4, fixed_split=chunk)
    assert rc != 0 and b"float workspace too small" in fi_lib.fi_last_error()
    # the bound is head_dim_vo's: 128 / 128 needs the same bytes (refused just below), 256 / 256 more
    rc, _, _ = plan(fi_lib, qo_lens, kv_lens, hq, hkv, 128, 128, float_bytes=need - 4, fixed_split=chunk)
    assert rc != 0
    rc, _, _ = plan(fi_lib, qo_lens, kv_lens, hq, hkv, 256, 256, float_bytes=need + ENTRY_ALIGN, fixed_split=chunk)
    assert rc != 0


@pytest.mark.parametrize("pair", [(192, 64), (128, 192), (256, 128), (192, 192), (576, 512), (64, 128)])
def test_unsupported_pairs_are_refused(fi_lib, pair):
    rc, _, _ = plan(fi_lib, [10], [20], 4, 4, *pair)
    assert rc != 0
    assert b"unsupported" in fi_lib.fi_last_error()


def _params(**kw):
    base = dict(q=16, k=16, v=16, o=16, q_stride_n=4 * 192, q_stride_h=192, k_stride_n=4 * 192, k_stride_h=192,
                v_stride_n=4 * 128, v_stride_h=128, qo_len=10, kv_len=20, num_qo_heads=4, num_kv_heads=4,
                head_dim_qk=192, head_dim_vo=128, q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16,
                o_dtype=_lib.FI_DTYPE_BF16, mask_mode=1, sm_scale=0.07)
    base.update(kw)
    return _lib.fi_prefill_qkvo_params_t(**base)


@pytest.mark.parametrize("kw,msg", [
    (dict(q_dtype=2, kv_dtype=2), b"fp8"),
    (dict(kv_dtype=0), b"dtype"),
    (dict(pos_encoding_mode=1), b"pos_encoding_mode"),
    (dict(pos_encoding_mode=2), b"pos_encoding_mode"),
    (dict(mask_mode=2), b"mask_mode"),
    (dict(mask_mode=3), b"mask_mode"),
    (dict(logits_soft_cap=30.0), b"logits_soft_cap"),
    (dict(head_dim_vo=64), b"unsupported"),
    (dict(head_dim_qk=128), b"unsupported"),
    (dict(num_qo_heads=6), b"multiple"),
    (dict(v_stride_n=4 * 128 + 4), b"aligned"),
])
def test_single_run_refusals_report_errors(fi_lib, kw, msg):
    """Refused before any launch (the pointers are never dereferenced)."""
    p = _params(**kw)
    rc = fi_lib.fi_single_prefill_qkvo_run(C.byref(p), None, 0, None)
    assert rc != 0
    assert msg in fi_lib.fi_last_error()


def test_runs_refuse_foreign_plans(fi_lib):
    """fi_batch_prefill_qkvo_run takes only a 192 / 128 plan (its partial states are head_dim_vo wide); the paged run
    refuses a 192 / 128 plan."""
    _, info_eq, _ = plan(fi_lib, [10], [20], 4, 4, 128, 128)
    _, info_qkvo, _ = plan(fi_lib, [10], [20], 4, 4, 192, 128)
    p = _params(batch_size=1, qo_indptr=16, kv_indptr=16)
    arr = (C.c_int64 * 16)(*info_eq)
    rc = fi_lib.fi_batch_prefill_qkvo_run(None, 0, 16, 0, arr, 16, C.byref(p), None)
    assert rc != 0 and b"not made for head_dim_qk 192" in fi_lib.fi_last_error()
    bp = _lib.fi_batch_prefill_params_t()
    arr = (C.c_int64 * 16)(*info_qkvo)
    rc = fi_lib.fi_batch_prefill_paged_run(None, 0, 16, 0, arr, 16, C.byref(bp), None)
    assert rc != 0 and b"fi_batch_prefill_qkvo_run" in fi_lib.fi_last_error()


EQUAL_SHAPES = [
    # (qo_lens, kv_lens, hq, hkv, d, causal, graph, fixed_split, page_size)
    ([1024] * 4, [1024] * 4, 32, 8, 128, True, False, -1, 1),
    ([377, 177, 1, 0], [544, 977, 2000, 5], 32, 32, 128, False, False, -1, 16),
    ([16], [8192], 8, 1, 64, True, False, -1, 1),
    ([300, 40], [2000, 100], 16, 4, 256, True, True, -1, 16),
    ([100, 37], [1000, 3000], 16, 4, 128, False, False, 256, 1),
    ([3928], [7563], 128, 128, 128, True, False, -1, 1),
]


def _equal_plans(fi_lib):
    out = []
    for qo_lens, kv_lens, hq, hkv, d, causal, graph, split, ps in EQUAL_SHAPES:
        rc, info, lists = plan(fi_lib, qo_lens, kv_lens, hq, hkv, d, d, causal=causal, graph=graph,
                               fixed_split=split, page_size=ps)
        assert rc == 0, fi_lib.fi_last_error()
        out.append(dict(info=info, **lists))
    return out


def test_equal_head_dim_plans_are_unchanged(fi_lib):
    """Plans for equal head dims match the ones the library produced before the 192 / 128 form existed
    (tests/golden/prefill_plans_equal_dims.json, 256 compute units)."""
    if fi_lib.fi_num_compute_units() != 256:
        pytest.skip("the golden plans were cut for 256 compute units")
    golden = json.load(open(GOLDEN))
    assert _equal_plans(fi_lib) == golden
