"""The device-side prefill planner (fi_batch_prefill_plan_device) against the planner oracle and the host planner, and
flashinfer.prefill.trtllm_batch_context_with_kv_cache against the attention oracle and the host-planned wrapper."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from attn_inputs import indptr_of, make_paged, page_table, poison_, ptol, scatter_to_pages
from flashinfer import _lib
from oracle import attention_ref as R
from oracle.plan_ref import prefill_plan_ref
from plan_calls import run_prefill_plan
from sink_ref import batch_prefill_sink_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HQ, HKV, D = 32, 8, 128
GUARD = 256  # bytes of 0xAB in front of and behind the int workspace


def _rand(n, lo, hi, seed):
    return torch.randint(lo, hi + 1, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


# name -> qo lens, kv lens, page size, blocks per block-table row, max_items_hint; optionally the row stride of the
# block table, window_left, rows of q beyond the last request's
PLAN_CASES = {
    "a_split": dict(qo=[5, 1, 40, 17], kv=[54, 4000, 700, 33], ps=16, mb=250, hint=64),
    "a_items_from_the_device": dict(qo=[5, 1, 40, 17], kv=[54, 4000, 700, 33], ps=16, mb=256, hint=0, extra_rows=9),
    "b_host_known_unsplit": dict(qo=[200, 100], kv=[300, 1000], ps=16, mb=64, hint=2),
    "c_split_branch_nothing_fits": dict(qo=[1] * 6, kv=[500] * 6, ps=16, mb=32, hint=4),
    "d_empty_search_range": dict(qo=[3, 10, 1], kv=[100, 128, 7], ps=16, mb=8, hint=64),
    "d_below_the_search_range": dict(qo=[3, 10, 1], kv=[50, 64, 7], ps=16, mb=4, hint=64),
    "e1_page_size_1": dict(qo=[4, 1, 30], kv=[1, 129, 2000], ps=1, mb=2048, hint=64),
    "e2_full_block_table_rows": dict(qo=[7, 1, 2, 130], kv=[512, 64, 100, 448], ps=64, mb=8, hint=16, stride=11),
    "f_more_requests_than_threads": dict(qo=_rand(300, 0, 3, 1), kv=_rand(300, 1, 3000, 2), ps=16, mb=188, hint=512),
    "f_many_requests_nothing_fits": dict(qo=_rand(300, 0, 3, 1), kv=_rand(300, 1, 3000, 2), ps=16, mb=188, hint=64),
    "g_one_long_request": dict(qo=[16], kv=[131072], ps=16, mb=8192, hint=256),
    "h_edge_lengths": dict(qo=[10, 3, 0, 200, 5], kv=[4, 0, 50, 150, 3000], ps=16, mb=190, hint=64),
    "h_items_from_the_device": dict(qo=[10, 3, 0, 200, 5], kv=[4, 0, 50, 150, 3000], ps=16, mb=190, hint=0),
    "h_sliding_window": dict(qo=[10, 3, 0, 200, 5], kv=[4, 0, 50, 150, 3000], ps=16, mb=190, hint=64, window=100),
    "h_window_items_from_the_device": dict(qo=[10, 3, 0, 200, 5], kv=[4, 0, 50, 150, 3000], ps=16, mb=190, hint=0,
                                           window=100),
}
# the edges of a scan round of 256: qo_indptr has batch + 1 entries, so 255 requests fill one round of its max-scan
# and 256 spill one entry into the next; the sum scans run over batch entries.  Once with a hint under which the
# bisection chooses, once with one below the q tiles x 1 chunk that the requests with rows make anyway.
for _b in (255, 256, 257, 513):
    for _name, _hint in (("split", 512), ("nothing_fits", 64)):
        PLAN_CASES[f"i_round_edge_{_b}_{_name}"] = dict(qo=_rand(_b, 0, 3, _b), kv=_rand(_b, 1, 600, _b + 1), ps=16,
                                                        mb=38, hint=_hint)


def _device_plan(fi_lib, cum_q, seq_lens, ps, mb, hint, rows, stride=None, window=-1, hq=HQ):
    """Run the planner's two launches on raw device values; plan_info, the csr offsets, the int workspace as bytes with
    its two guards, the block table and the float bytes asked for."""
    B = len(seq_lens)
    g = torch.Generator().manual_seed(B * 7 + ps)
    table = torch.randint(0, 1000, (B, stride or mb), generator=g, dtype=torch.int32)
    table_dev = table.to(DEV)[:, :mb]
    lens_dev = torch.tensor(seq_lens, dtype=torch.int32, device=DEV)
    cum_dev = torch.tensor(cum_q, dtype=torch.int32, device=DEV)
    p = _lib.fi_batch_prefill_plan_device_params_t(
        block_tables=table_dev.data_ptr(), seq_lens=lens_dev.data_ptr(), cum_seq_lens_q=cum_dev.data_ptr(),
        block_tables_stride=table_dev.stride(0), batch_size=B, max_blocks=mb, page_size=ps, total_num_rows=rows,
        num_qo_heads=hq, num_kv_heads=HKV, head_dim=D, q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16,
        window_left=window, max_items_hint=hint)
    ib, fb = C.c_size_t(), C.c_size_t()
    assert fi_lib.fi_batch_prefill_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)) == 0
    # not zeroed: whatever is compared below was written by the planner
    int_ws = torch.full((ib.value + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    float_ws = torch.empty(max(fb.value, 16), dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes = int_ws.data_ptr() + GUARD, ib.value
    p.float_ws, p.float_ws_bytes = float_ws.data_ptr(), fb.value
    info, csr = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)(), (C.c_int64 * 4)()
    rc = fi_lib.fi_batch_prefill_plan_device(C.byref(p), info, csr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fi_lib.fi_last_error()
    torch.cuda.synchronize()
    return list(info), list(csr), int_ws.cpu().numpy(), table[:, :mb], fb.value


def _check_plan(fi_lib, info, csr, raw, table, fbytes, qo_indptr, kv_lens, ps, mb, hint, rows, window=-1,
                against_host=False):
    """Everything the planner wrote, against the oracle's graph-mode plan for the (clamped) qo_indptr and kv_lens.
    Returns the byte ranges of the int workspace that were compared."""
    B, group = len(kv_lens), HQ // HKV
    ws = raw[GUARD: len(raw) - GUARD]
    touched = []

    def i32(off, count):
        touched.append((off, off + 4 * count))
        return ws[off: off + 4 * count].view(np.int32).tolist()

    max_items = hint if hint > 0 else max(fi_lib.fi_num_compute_units() * 2 // HKV, 1)
    ref = prefill_plan_ref(qo_indptr, kv_lens, HQ, HKV, causal=True, enable_cuda_graph=True, total_num_rows=rows,
                           num_cus=max_items * HKV // 2, window_left=window)
    n = ref["num_work"]
    t0 = -(-rows * group // 128)
    split = t0 <= max_items
    capacity = max(max_items, t0 + B - 1) if split else t0 + B - 1

    # host-computed plan_info entries
    assert info[_lib.FI_PP_MAGIC] == _lib.FI_PREFILL_PLAN_MAGIC and info[_lib.FI_PP_ENABLE_CUDA_GRAPH] == 1
    assert info[_lib.FI_PP_SPLIT_KV] == int(split) and (fbytes > 0) == split
    assert info[_lib.FI_PP_PADDED_BATCH_SIZE] == capacity >= n
    assert info[_lib.FI_PP_TOTAL_NUM_ROWS] == rows and info[_lib.FI_PP_BATCH_SIZE] == B
    assert info[_lib.FI_PP_KV_CHUNK_SIZE] == 0 and info[_lib.FI_PP_NUM_WORK] == 0 and info[_lib.FI_PP_CTA_TILE_Q] == 128
    if split:
        entries = max_items * (-(-128 // group) + 1)
        assert ref["merge_indptr"][-1] <= entries
        assert info[_lib.FI_PP_S_OFFSET] == 0 and info[_lib.FI_PP_V_OFFSET] == (4 * HQ * entries + 15) // 16 * 16
        assert fbytes == info[_lib.FI_PP_V_OFFSET] + 4 * HQ * entries * D
        assert capacity == ref["padded_batch_size"]

    # the chunk slot, merge_indptr and the work list
    chunk, num_work = i32(info[_lib.FI_PP_KV_CHUNK_SIZE_PTR_OFFSET], 2)
    assert chunk == ref["kv_chunk_size"] and num_work == n
    merge = i32(info[_lib.FI_PP_MERGE_INDPTR_OFFSET], rows + 1)
    used = qo_indptr[-1]
    assert merge[: used + 1] == ref["merge_indptr"] and merge[used + 1:] == [ref["merge_indptr"][-1]] * (rows - used)
    req = i32(info[_lib.FI_PP_REQUEST_INDICES_OFFSET], capacity)
    tile = i32(info[_lib.FI_PP_QO_TILE_INDICES_OFFSET], capacity)
    kvt = i32(info[_lib.FI_PP_KV_TILE_INDICES_OFFSET], capacity)
    items = list(zip(req, tile, kvt))
    assert sorted(items[:n]) == sorted(zip(ref["request_indices"], ref["qo_tile_indices"], ref["kv_tile_indices"]))
    assert items[n:] == [(-1, 0, 0)] * (capacity - n)
    # request order; per request the q tiles from the last one down, per q tile the chunks upwards
    assert items[:n] == sorted(items[:n], key=lambda it: (it[0], -it[1], it[2]))

    if against_host:
        host = run_prefill_plan(fi_lib, qo_indptr, kv_lens, HQ, HKV, causal=True, cuda_graph=True, page_size=ps,
                                window_left=window)
        assert chunk == host["kv_chunk_size"] and n == host["num_work"]
        assert merge[: used + 1] == host["merge_indptr"]
        assert sorted(items[:n]) == sorted(zip(host["request_indices"], host["qo_tile_indices"],
                                               host["kv_tile_indices"]))
        assert set(host["padding"]) <= {-1}
        if split and rows == used:
            assert capacity == host["padded_batch_size"]

    # the clamped query offsets and the CSR page table
    assert i32(csr[3], B + 1) == qo_indptr
    indptr, _, last, _ = page_table(kv_lens, ps)
    pages = (indptr[1:] - indptr[:-1]).tolist()
    assert i32(csr[0], B + 1) == indptr.tolist()
    assert i32(csr[2], B) == last.tolist()
    assert i32(csr[1], int(indptr[-1])) == torch.cat([table[b, :pages[b]] for b in range(B)]).tolist()
    touched.append((csr[3], csr[0]))  # behind qo_indptr: the item and entry scans the two kernels hand each other
    assert csr[0] - csr[3] == 3 * ((4 * (B + 1) + 15) // 16 * 16)
    return touched


@pytest.mark.parametrize("case", PLAN_CASES)
def test_device_plan_equals_the_graph_mode_rule(fi_lib, case):
    c = PLAN_CASES[case]
    qo_indptr = indptr_of(c["qo"]).tolist()
    rows = qo_indptr[-1] + c.get("extra_rows", 0)
    window = c.get("window", -1)
    out = _device_plan(fi_lib, qo_indptr, c["kv"], c["ps"], c["mb"], c["hint"], rows, c.get("stride"), window)
    _check_plan(fi_lib, *out, qo_indptr, c["kv"], c["ps"], c["mb"], c["hint"], rows, window,
                against_host=c["hint"] == 0)


def test_the_branches_the_cases_are_named_for(fi_lib):
    """(b) is unsplit with no float workspace, (c) a split plan of capacity 6 with one chunk per request, (g) cuts one
    request into 256 chunks."""
    def plan(case):
        c = PLAN_CASES[case]
        qo_indptr = indptr_of(c["qo"]).tolist()
        info, _, raw, _, fb = _device_plan(fi_lib, qo_indptr, c["kv"], c["ps"], c["mb"], c["hint"], qo_indptr[-1])
        off = GUARD + info[_lib.FI_PP_KV_CHUNK_SIZE_PTR_OFFSET]
        return info, fb, raw[off: off + 8].view(np.int32).tolist()

    info, fb, slot = plan("b_host_known_unsplit")
    assert info[_lib.FI_PP_SPLIT_KV] == 0 and fb == 0 and slot == [1024, 7 + 4]
    info, fb, slot = plan("c_split_branch_nothing_fits")
    assert info[_lib.FI_PP_SPLIT_KV] == 1 and info[_lib.FI_PP_PADDED_BATCH_SIZE] == 6 and slot == [512, 6]
    info, fb, slot = plan("g_one_long_request")
    assert info[_lib.FI_PP_SPLIT_KV] == 1 and slot == [512, 256]


def test_garbage_on_the_device_is_clamped_and_every_store_stays_in_its_region(fi_lib):
    """cum_seq_lens_q that decreases and runs past total_num_rows, a length past the block-table row and a negative
    one: the plan is the plan of the clamped values, and no byte outside the regions the plan declares changed."""
    ps, mb, hint, rows = 16, 8, 64, 50
    cum_q, seq_lens = [0, 30, 20, 500, 45], [100, 99999, -5, 64]
    qo_indptr, kv_lens = [0, 30, 30, 50, 50], [100, mb * ps, 0, 64]
    info, csr, raw, table, fb = _device_plan(fi_lib, cum_q, seq_lens, ps, mb, hint, rows)
    touched = _check_plan(fi_lib, info, csr, raw, table, fb, qo_indptr, kv_lens, ps, mb, hint, rows)
    untouched = np.ones(len(raw), dtype=bool)
    for lo, hi in touched:
        untouched[GUARD + lo: GUARD + hi] = False
    # the two guards, the padding between regions, and the indices past the pages the requests hold
    assert untouched[:GUARD].all() and untouched[-GUARD:].all()
    assert untouched.sum() >= 2 * GUARD + 4 * (len(kv_lens) * mb - sum(-(-l // ps) for l in kv_lens))
    assert (raw[untouched] == 0xAB).all()


# ---- numerics: the whole call ----

@functools.lru_cache(maxsize=None)
def _workspace(zeroed=False):
    """One buffer for every call (not zeroed: the call must not need it) and one for the host-planned wrapper."""
    return (torch.zeros if zeroed else torch.empty)(160 << 20, dtype=torch.uint8, device=DEV)


def _table_of(indptr, indices, max_blocks, fill, stride=None):
    """Dense block table of a CSR page table; entries past a request's pages hold `fill`."""
    B = len(indptr) - 1
    table = torch.full((B, stride or max_blocks), fill, dtype=torch.int32)
    for b in range(B):
        row = indices[int(indptr[b]): int(indptr[b + 1])]
        table[b, : len(row)] = row
    return table


@functools.lru_cache(maxsize=None)
def _problem(qo, kv, ps, dtype, hq=HQ, hkv=HKV, d=D, kv_dtype=None, window=-1, extra_rows=0, seed=7):
    """An HND cache, a dense block table whose entries past a request's pages point at a valid page of 0xFF bytes (NaN
    in f16, bf16 and e4m3fn: read even under a probability of zero, it turns the result into NaN), the CSR table of the
    same pages for the oracle, and the
    oracle's output, computed once per problem and left unchanged."""
    kv_dtype = kv_dtype or dtype
    B, max_blocks = len(kv), -(-max(kv) // ps) + 2
    cache, indptr, indices, last = make_paged(B, list(kv), ps, hkv, d, kv_dtype, "HND", seed=seed)
    poison = min(set(range(cache.shape[0])) - set(indices.tolist()))
    poison_(cache[poison])
    rows = sum(qo)
    q = torch.randn(rows + extra_rows, hq, d, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    qo_indptr = indptr_of(qo)
    o_ref, _ = R.batch_prefill_ref(q[:rows].float(), qo_indptr, cache.float(), "HND", indptr, indices, last,
                                   causal=True, window_left=window)
    return dict(q=q.to(DEV), cache=cache.to(DEV), cache_cpu=cache, indptr=indptr, indices=indices, last=last,
                qo_indptr=qo_indptr, o_ref=o_ref.float(), rows=rows, window=window, ps=ps, max_blocks=max_blocks,
                table=_table_of(indptr, indices, max_blocks, poison).to(DEV), heads=(hq, hkv, d),
                lens=torch.tensor(kv, dtype=torch.int32, device=DEV), cum=qo_indptr.to(DEV))


def _call(pr, **kw):
    from flashinfer.prefill import trtllm_batch_context_with_kv_cache

    d = pr["heads"][2]
    args = dict(query=pr["q"], kv_cache=pr["cache"], workspace_buffer=_workspace(), block_tables=pr["table"],
                seq_lens=pr["lens"], max_q_len=int(pr["rows"]), max_kv_len=pr["max_blocks"] * pr["ps"],
                bmm1_scale=1.0 / math.sqrt(d), bmm2_scale=1.0, batch_size=len(pr["lens"]), cum_seq_lens_q=pr["cum"],
                cum_seq_lens_kv=None, window_left=pr["window"])
    args.update(kw)
    return trtllm_batch_context_with_kv_cache(**args)


def _is_split(fi_lib, pr):
    hq, hkv, _ = pr["heads"]
    return -(-pr["q"].shape[0] * (hq // hkv) // 128) <= max(fi_lib.fi_num_compute_units() * 2 // hkv, 1)


def _host_planned(pr, dtype, sinks=None):
    """BatchPrefillWithPagedKVCacheWrapper in graph mode, planned on the host for the same batch."""
    import flashinfer

    hq, hkv, d = pr["heads"]
    B = len(pr["last"])
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(
        _workspace(zeroed=True), "HND", use_cuda_graph=True,
        qo_indptr_buf=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indptr_buf=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buf=torch.zeros(len(pr["indices"]), dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buf=torch.zeros(B, dtype=torch.int32, device=DEV))
    w.plan(pr["qo_indptr"], pr["indptr"], pr["indices"], pr["last"], hq, hkv, d, pr["ps"], causal=True,
           window_left=pr["window"], q_data_type=dtype, kv_data_type=pr["cache"].dtype)
    return w.run(pr["q"][: pr["rows"]], pr["cache"], sinks=sinks)


QO_A, KV_A = (5, 1, 40, 17), (54, 4000, 700, 33)
# 2121 rows x 4 heads a kv head = 67 q tiles, more than the 64 items of 256 CUs: the host-known unsplit branch
QO_U = (240,) * 8 + (200, 1)
KV_U = (240, 300, 256, 240, 500, 241, 240, 1000, 200, 77)
# decode-like and prefill-like requests in one step
QO_M, KV_M = (1, 1, 1, 300, 1, 17, 64, 1), (8192, 33, 2000, 300, 700, 4321, 1000, 16)


@pytest.mark.parametrize("ps", [1, 16, 64])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_split_branch_matches_the_oracle_and_equals_the_host_planned_wrapper(fi_lib, dtype, ps):
    pr = _problem(QO_A, KV_A, ps, dtype)
    assert _is_split(fi_lib, pr)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(dtype))
    # The same chunk size, so the same (request, q tile, chunk) items writing the same partial-state entries, merged
    # per row in chunk order: the order of the work list decides when an item runs, never what it computes.
    assert torch.equal(out, _host_planned(pr, dtype))


@pytest.mark.parametrize("dtype,ps", [(torch.float16, 16), (torch.bfloat16, 64)], ids=["f16-16", "bf16-64"])
def test_unsplit_branch_matches_the_oracle_and_the_host_planned_wrapper(fi_lib, dtype, ps):
    pr = _problem(QO_U, KV_U, ps, dtype)
    assert not _is_split(fi_lib, pr)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(dtype))
    # the host's graph plan goes through f32 partial states and the merge, this one writes the output directly
    torch.testing.assert_close(out.float(), _host_planned(pr, dtype).float(), **ptol(dtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_mixed_decode_and_prefill_requests(fi_lib, dtype):
    pr = _problem(QO_M, KV_M, 16, dtype, seed=21)
    assert _is_split(fi_lib, pr)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(dtype))
    assert torch.equal(out, _host_planned(pr, dtype))


@pytest.mark.parametrize("hq,hkv,d", [(40, 8, 128), (32, 8, 64), (16, 4, 256)], ids=["heads40-8", "d64", "d256"])
def test_other_head_shapes(hq, hkv, d):
    """40 / 8 heads: five heads a query row, so a row's heads straddle two 128-row q tiles."""
    dtype = torch.float16
    pr = _problem((5, 1, 77, 17), (54, 2000, 700, 33), 16, dtype, hq, hkv, d, seed=31)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(dtype))


def test_fp8_cache_under_a_bf16_query():
    # the oracle sees the same quantised cache, so the 16-bit bar applies
    pr = _problem(QO_A, KV_A, 16, torch.bfloat16, kv_dtype=torch.float8_e4m3fn, seed=41)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(torch.bfloat16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_sliding_window(dtype):
    pr = _problem(QO_A, KV_A, 16, dtype, window=100, seed=51)
    out = _call(pr)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **ptol(dtype))
    assert not torch.equal(out, _call(pr, window_left=-1)), "the window must change the result"


@pytest.mark.parametrize("branch", ["split", "unsplit"])
def test_sinks(fi_lib, branch):
    dtype = torch.float16
    pr = _problem(QO_A, KV_A, 16, dtype) if branch == "split" else _problem(QO_U, KV_U, 16, dtype)
    assert _is_split(fi_lib, pr) == (branch == "split")
    sinks = torch.randn(HQ, generator=torch.Generator().manual_seed(9))
    o_ref, _ = batch_prefill_sink_ref(pr["q"][: pr["rows"]].float().cpu(), pr["qo_indptr"], pr["cache_cpu"].float(),
                                      "HND", pr["indptr"], pr["indices"], pr["last"], sinks, causal=True)
    for given in (sinks.to(DEV), [sinks.to(DEV)]):
        out = _call(pr, sinks=given)
        torch.cuda.synchronize()
        torch.testing.assert_close(out.float().cpu(), o_ref.float(), **ptol(dtype))


@pytest.mark.parametrize("branch", ["split", "unsplit"])
def test_bmm2_scale_out_in_place_and_rows_no_request_owns(fi_lib, branch):
    """Rows of `out` from cum_seq_lens_q[batch] on are left as they were, with a bmm2_scale too."""
    dtype = torch.float16
    qo, kv = (QO_A, KV_A) if branch == "split" else (QO_U, KV_U)
    pr = _problem(qo, kv, 16, dtype, extra_rows=5)
    assert _is_split(fi_lib, pr) == (branch == "split")
    rows = pr["rows"]
    given = torch.full_like(pr["q"], 7.0)
    one = _call(pr, out=given)
    assert one is given
    torch.cuda.synchronize()
    torch.testing.assert_close(one[:rows].float().cpu(), pr["o_ref"], **ptol(dtype))
    assert (one[rows:] == 7.0).all()
    half = _call(pr, bmm2_scale=0.5, out=torch.full_like(pr["q"], 7.0))
    # one rounding of o / 2 either way: exact in f16 unless o is subnormal
    torch.testing.assert_close(half[:rows].float(), one[:rows].float() * 0.5, rtol=0, atol=2.0 ** -24)
    assert (half[rows:] == 7.0).all()


def test_kv_tuple_and_strided_query():
    dtype = torch.float16
    pr = _problem(QO_A, KV_A, 16, dtype)
    want = _call(pr)
    k, v = pr["cache"][:, 0].contiguous(), pr["cache"][:, 1].contiguous()
    assert torch.equal(_call(pr, kv_cache=(k, v)), want)
    wide = torch.zeros(pr["q"].shape[0], HQ + 8, D, dtype=dtype, device=DEV)
    wide[:, :HQ] = pr["q"]
    q = wide[:, :HQ]
    assert q.stride(0) == (HQ + 8) * D and not q.is_contiguous()
    assert torch.equal(_call(pr, query=q), want)


def test_fp8_query_against_the_fp8_oracle():
    """An e4m3 query and cache with no per-head scales, at the bar tests/test_prefill_gpu.py holds the paged fp8 case
    to (rtol = atol = 5e-2 against the oracle's restatement of the reference's fp8 arithmetic)."""
    hq, hkv, d, ps = 32, 8, 128, 16
    kv_lens, qo_lens = [512, 300, 2000], [256, 300, 1]
    g = torch.Generator().manual_seed(3)
    k8 = torch.randn(sum(kv_lens), hkv, d, generator=g).to(torch.float8_e4m3fn)
    v8 = torch.randn(sum(kv_lens), hkv, d, generator=g).to(torch.float8_e4m3fn)
    q8 = torch.randn(sum(qo_lens), hq, d, generator=g).to(torch.float8_e4m3fn)
    indptr, indices, last, total = page_table(kv_lens, ps, g)
    cache = scatter_to_pages(k8.float(), v8.float(), kv_lens, indptr, indices, ps, total, "HND").to(torch.float8_e4m3fn)
    qo_indptr = indptr_of(qo_lens)
    pr = dict(q=q8.to(DEV), cache=cache.to(DEV), table=_table_of(indptr, indices, 128, 0).to(DEV), ps=ps,
              max_blocks=128, lens=torch.tensor(kv_lens, dtype=torch.int32, device=DEV), cum=qo_indptr.to(DEV),
              rows=sum(qo_lens), window=-1, heads=(hq, hkv, d))
    out = _call(pr, out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    torch.cuda.synchronize()
    one_q, one_kv = torch.ones(hq), torch.ones(hkv)
    off = 0
    for b in range(len(kv_lens)):
        rows = slice(int(qo_indptr[b]), int(qo_indptr[b + 1]))
        o_ref, _ = R.fp8_attention_ref(q8[rows], k8[off: off + kv_lens[b]], v8[off: off + kv_lens[b]], one_q, one_kv,
                                       one_kv, causal=True)
        torch.testing.assert_close(out[rows].float().cpu(), o_ref.float(), rtol=5e-2, atol=5e-2)
        off += kv_lens[b]
    half = _call(pr, out=torch.empty_like(out), bmm2_scale=0.5)
    torch.testing.assert_close(half.float(), out.float() * 0.5, rtol=0, atol=2.0 ** -24)  # halving is exact


# ---- graph: the whole call captured, replayed on other lengths ----

def _replay_case(fi_lib, first, second, dtype, ps=16):
    """Capture the call on the batch `first` = (qo lens, kv lens), overwrite seq_lens, cum_seq_lens_q and block_tables
    in place with those of `second` (the same batch size and rows of q), replay, compare with the oracle."""
    (qo1, kv1), (qo2, kv2) = first, second
    assert len(qo1) == len(qo2) and sum(qo1) == sum(qo2)
    pr2 = _problem(tuple(qo2), tuple(kv2), ps, dtype, seed=61)
    max_blocks = pr2["max_blocks"]
    assert max(kv1) <= max_blocks * ps
    B, pages = len(qo1), pr2["cache"].shape[0]
    # any valid pages will do for the captured lengths
    pr = dict(pr2, table=torch.arange(B * max_blocks, dtype=torch.int32, device=DEV).remainder(pages)
              .reshape(B, max_blocks), lens=torch.tensor(kv1, dtype=torch.int32, device=DEV),
              cum=indptr_of(qo1).to(DEV))
    out = torch.zeros_like(pr["q"])
    _call(pr, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(pr, out=out)
    pr["lens"].copy_(pr2["lens"])
    pr["cum"].copy_(pr2["cum"])
    pr["table"].copy_(pr2["table"])
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr2["o_ref"], **ptol(dtype))
    return pr2


def test_captured_split_call_replans_with_another_chunk_size(fi_lib):
    # 128-token chunks at capture; at replay two long requests whose 128-token chunks would be too many items
    first, second = ([16, 16, 16, 15], [100] * 4), (list(QO_A), [54, 12000, 5000, 33])
    max_items = fi_lib.fi_num_compute_units() * 2 // HKV
    plans = [prefill_plan_ref(indptr_of(qo).tolist(), kv, HQ, HKV, causal=True, enable_cuda_graph=True,
                              num_cus=max_items * HKV // 2) for qo, kv in (first, second)]
    assert plans[0]["kv_chunk_size"] != plans[1]["kv_chunk_size"] and plans[0]["num_work"] != plans[1]["num_work"]
    pr = _replay_case(fi_lib, first, second, torch.float16)
    assert _is_split(fi_lib, pr)


def test_captured_unsplit_call_replans(fi_lib):
    first = ([212] * 9 + [213], [300] * 10)
    pr = _replay_case(fi_lib, first, (list(QO_U), list(KV_U)), torch.bfloat16)
    assert not _is_split(fi_lib, pr)
