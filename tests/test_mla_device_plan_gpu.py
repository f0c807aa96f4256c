"""The device-side MLA planner (fi_batch_mla_plan_device) against the host planner, and
flashinfer.decode.trtllm_batch_decode_with_kv_cache_mla against the attention oracle and the host-planned wrapper."""
import ctypes as C
import functools
import math

import pytest
import torch

from attn_inputs import indptr_of, poison_, tol
from flashinfer import _lib
from mla_plan_free_inputs import CKV, KPE, host_plan, make_case, oracle_out, plan_params, read_plan, workspace_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SM = 1.0 / math.sqrt(128 + 64)
WS_BYTES = 64 << 20


def _mixed_lens(n, hi, seed):
    return torch.randint(1, hi, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _cus():
    return _lib.lib().fi_num_compute_units()


# name -> dict(lens, ps, H, q_len, float_bytes, max_blocks, stride); lens may be a callable, evaluated on the GPU machine
PLAN_CASES = {
    "a_bisection": dict(lens=[54, 4000, 1, 700, 33]),
    # one 16-row tile per request: batch x tiles just reaches max_items, so nothing is split
    "b_unsplit_at_max_items": dict(lens=lambda: _mixed_lens(_cus(), 3000, 2)),
    "b_split_one_below_max_items": dict(lens=lambda: _mixed_lens(_cus() - 1, 3000, 3)),
    "c_empty_search_range": dict(lens=[5, 100, 111, 255]),
    "d_page_size_1": dict(lens=[1, 128, 129, 4096], ps=1),
    "e_200_mixed": dict(lens=_mixed_lens(200, 3000, 1)),
    "f_more_requests_than_threads": dict(lens=_mixed_lens(300, 200, 4)),
    "g_one_long_request": dict(lens=[131072]),
    "h_empty_requests": dict(lens=[54, 0, 700, 0]),
    # 2 x 16 tiles, 8 chunks each by the search: 4096 partial states, 2044 fit 4 MiB, so the chunk doubles twice
    "i_doubling": dict(lens=[32768, 32768], H=128, q_len=2, ps=64, float_bytes=4 << 20),
    "j_length_beyond_the_row": dict(lens=[6 * 16 + 1000, 40, 1 << 30], max_blocks=6),
    "k_negative_length": dict(lens=[-5, 300, -(1 << 31), 2000]),
    "l_row_stride_wider_than_max_blocks": dict(lens=[54, 4000, 1, 700, 33], stride=300),
    "m_tile_spans_query_positions": dict(lens=[8736, 1, 33], H=8, q_len=3, ps=64),
    "n_no_float_workspace": dict(lens=[54, 4000, 1, 700, 33], float_bytes=0),
    # the edges of the scan's round of 256 requests; split or not by the device's compute units, the host plan follows
    "o_round_edge_256": dict(lens=_mixed_lens(256, 601, 256)),
    "o_round_edge_257": dict(lens=_mixed_lens(257, 601, 257)),
    "o_round_edge_513": dict(lens=_mixed_lens(513, 601, 513)),
}


def _device_plan(fi_lib, lens, ps, H, q_len, float_bytes, max_blocks, stride):
    """Run the planner's two launches; (plan_info, the int workspace as a uint8 array)."""
    B = len(lens)
    table = torch.zeros(B, stride, dtype=torch.int32, device=DEV)[:, :max_blocks]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    p = plan_params(B, max_blocks, ps, H, q_len, stride=stride, block_tables=table.data_ptr(),
                    seq_lens=lens_dev.data_ptr())
    ib, fb = workspace_sizes(fi_lib, p)
    assert fb == 0
    # not zeroed: whatever is compared below was written by the planner
    int_ws = torch.full((ib,), 0xAB, dtype=torch.uint8, device=DEV)
    float_ws = torch.empty(max(float_bytes, 16), dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes, p.float_ws, p.float_ws_bytes = int_ws.data_ptr(), ib, float_ws.data_ptr(), float_bytes
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()
    rc = fi_lib.fi_batch_mla_plan_device(C.byref(p), info, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fi_lib.fi_last_error()
    torch.cuda.synchronize()
    return list(info), int_ws.cpu().numpy()


@pytest.mark.parametrize("case", PLAN_CASES)
def test_device_plan_equals_the_host_plan(fi_lib, case):
    c = dict(ps=16, H=16, q_len=1, float_bytes=WS_BYTES, max_blocks=None, stride=None)
    c.update(PLAN_CASES[case])
    lens = c["lens"]() if callable(c["lens"]) else c["lens"]
    ps, H, q_len, B = c["ps"], c["H"], c["q_len"], len(lens)
    max_blocks = c["max_blocks"] or max(-(-max(lens) // ps), 1)
    stride = c["stride"] or max_blocks
    info, raw = _device_plan(fi_lib, lens, ps, H, q_len, c["float_bytes"], max_blocks, stride)
    rows = B * q_len * H
    header, indptr, items = read_plan(raw.tobytes(), rows)

    clamped = [min(max(l, 0), max_blocks * ps) for l in lens]
    host_info, (host_header, host_indptr, host_items) = host_plan(fi_lib, clamped, q_len, H, ps, c["float_bytes"])
    print(case, "num_work", host_header[1], "split", host_header[3], "chunk", host_info[_lib.FI_MLA_KV_CHUNK_SIZE],
          "entries", host_indptr[-1])

    # the int workspace: header slots, merge indptr, items
    assert header == host_header
    assert indptr == host_indptr
    assert len(items) == len(host_items) == host_info[_lib.FI_MLA_NUM_WORK]
    for w, (it, want) in enumerate(zip(items, host_items)):
        b = want["qo_start"] // q_len
        assert it == dict(want, page_base=b * stride), (w, it, want)
    if host_header[3]:
        assert any(it["chunk"] > 0 for it in items)

    # host-known plan_info entries, and values under which fi_batch_mla_run's checks hold for the others
    max_items = fi_lib.fi_num_compute_units()
    tiles = -(-q_len * H // 16)
    capacity = max(max_items, B * tiles)
    L = _lib
    assert len(items) <= capacity
    assert info[L.FI_MLA_MAGIC] == L.FI_MLA_PLAN_MAGIC and info[L.FI_MLA_ENABLE_CUDA_GRAPH] == 1
    assert info[L.FI_MLA_GRID] == max_items == host_info[L.FI_MLA_GRID]
    for slot in (L.FI_MLA_TOTAL_ROWS, L.FI_MLA_NUM_HEADS, L.FI_MLA_BATCH_SIZE, L.FI_MLA_PAGE_SIZE, L.FI_MLA_DTYPE,
                 L.FI_MLA_V_OFFSET, L.FI_MLA_MERGE_INDPTR_OFFSET, L.FI_MLA_ITEMS_OFFSET):
        assert info[slot] == host_info[slot], slot
    assert info[L.FI_MLA_INT_BYTES_USED] == len(raw) == header[2] + 32 * capacity + 4 * (2 * (B + 1) + 1)
    assert [info[s] for s in (L.FI_MLA_NUM_WORK, L.FI_MLA_KV_CHUNK_SIZE, L.FI_MLA_SPLIT_KV, L.FI_MLA_NUM_ENTRIES)] \
        == [0, 0, 0, 0]
    # items past the plan's count are left alone, as by the host planner
    assert (raw[header[2] + 32 * len(items): header[2] + 32 * capacity] == 0xAB).all()


def test_the_doubling_case_doubles():
    """What PLAN_CASES['i_doubling'] is there for: the search alone would cut 4096-token chunks."""
    fi_lib = _lib.lib()
    big, _ = host_plan(fi_lib, [32768, 32768], 2, 128, 64, WS_BYTES)
    small, _ = host_plan(fi_lib, [32768, 32768], 2, 128, 64, 4 << 20)
    assert small[_lib.FI_MLA_KV_CHUNK_SIZE] == 4 * big[_lib.FI_MLA_KV_CHUNK_SIZE]


# ---- numerics: the whole call ----

# (kv lens, q_len_per_request, heads, page size)
ATTENTION_CASES = {
    "one_short_request_page_1": ([17], 1, 16, 1),
    "empty_request_64_heads": ([0, 1, 17], 1, 64, 16),
    "q_len_2_page_64": ([514, 2743, 1], 2, 16, 64),
    "q_len_4_128_heads_page_1": ([17, 514, 0], 4, 128, 1),
    "tile_spans_query_positions": ([8736, 1, 33], 3, 8, 64),
    "split_128_heads": ([2743, 8736, 17], 2, 128, 16),
    "rows_without_a_key": ([1, 2, 600], 4, 16, 16),
    "300_requests": (_mixed_lens(300, 201, 5), 1, 16, 16),
}


@functools.lru_cache(maxsize=None)
def _problem(case, dtype):
    """The inputs of a case on the GPU and its oracle output, built once and left unchanged."""
    lens, q_len, H, ps = ATTENTION_CASES[case]
    c = make_case(lens, q_len, H, ps, dtype, seed=sorted(ATTENTION_CASES).index(case))
    assert c["cache"].isnan().any(), "every case has unowned slots: a spare page at least"
    o_ref = oracle_out(c, SM)
    return dict(c, o_ref=o_ref, q=c["q"].to(DEV), cache=c["cache"].to(DEV), table=c["table"].to(DEV),
                lens=c["lens"].to(DEV))


def _call(pr, **kw):
    from flashinfer.decode import trtllm_batch_decode_with_kv_cache_mla

    if "workspace_buffer" not in kw:  # not zeroed: 0xFF bytes, NaN wherever a float is read before it is written
        kw["workspace_buffer"] = poison_(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV))
    args = dict(query=pr["q"], kv_cache=pr["cache"].unsqueeze(1), qk_nope_head_dim=128, kv_lora_rank=CKV, qk_rope_head_dim=KPE, block_tables=pr["table"],
                seq_lens=pr["lens"], max_seq_len=pr["max_blocks"] * pr["ps"], bmm1_scale=SM, bmm2_scale=1.0)
    args.update(kw)
    return trtllm_batch_decode_with_kv_cache_mla(**args)


def _host_planned(pr):
    """BatchMLAPagedAttentionWrapper in graph mode, planned on the host for the same lengths, causal."""
    from flashinfer.mla import BatchMLAPagedAttentionWrapper

    B, q_len, H = len(pr["kv_lens"]), pr["q_len"], pr["H"]
    bufs = [torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros(B + 1, dtype=torch.int32, device=DEV),
            torch.zeros(max(len(pr["indices"]), 1), dtype=torch.int32, device=DEV),
            torch.zeros(B, dtype=torch.int32, device=DEV)]
    w = BatchMLAPagedAttentionWrapper(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV), True, *bufs)
    w.plan(indptr_of([q_len] * B).to(DEV), pr["indptr"].to(DEV), pr["indices"].to(DEV), pr["lens"], H, CKV, KPE,
           pr["ps"], True, SM, pr["dtype"], pr["dtype"])
    q = pr["q"].view(B * q_len, H, CKV + KPE)
    return w.run(q[..., :CKV], q[..., CKV:], pr["cache"][..., :CKV], pr["cache"][..., CKV:]).view(B, q_len, H, CKV)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ATTENTION_CASES)
def test_output_matches_the_oracle_and_the_host_planned_wrapper(case, dtype):
    pr = _problem(case, dtype)
    out = _call(pr)
    torch.cuda.synchronize()
    assert out.shape == (len(pr["kv_lens"]), pr["q_len"], pr["H"], CKV) and out.dtype == dtype
    assert torch.isfinite(out).all(), "memory that no request owns was read"
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **tol(dtype))
    # rows that see no key: every row of an empty request, row i of a request with kv_len - q_len + i < 0
    for b, kl in enumerate(pr["kv_lens"]):
        for i in range(pr["q_len"]):
            if kl - pr["q_len"] + i < 0:
                assert torch.count_nonzero(out[b, i]) == 0, (b, i)
    # the same work list through the same kernel: the same arithmetic
    assert torch.equal(out, _host_planned(pr))


def test_scales_are_honoured():
    pr = _problem("q_len_2_page_64", torch.float16)
    one = _call(pr)
    assert torch.equal(_call(pr, bmm2_scale=0.5), one * 0.5)
    half = _call(pr, bmm1_scale=SM * 0.5)
    assert not torch.equal(half, one)
    o_ref = oracle_out(dict(pr, q=pr["q"].cpu(), cache=pr["cache"].cpu()), SM * 0.5)
    torch.testing.assert_close(half.float().cpu(), o_ref, **tol(torch.float16))


def test_a_given_out_is_written_in_place_in_both_shapes():
    pr = _problem("q_len_2_page_64", torch.float16)
    want = _call(pr)
    given = torch.full_like(want, 7.0)
    assert _call(pr, out=given) is given and torch.equal(given, want)
    pr = _problem("empty_request_64_heads", torch.float16)  # q_len_per_request = 1
    want = _call(pr)
    B, H = len(pr["kv_lens"]), pr["H"]
    for shape in ((B, H, CKV), (B, 1, H, CKV)):
        given = torch.full(shape, 7.0, dtype=torch.float16, device=DEV)
        assert _call(pr, out=given) is given and torch.equal(given, want.view(shape))


def test_cache_without_the_head_axis_and_views_of_wider_tensors():
    pr = _problem("q_len_2_page_64", torch.bfloat16)
    want = _call(pr)
    assert torch.equal(_call(pr, kv_cache=pr["cache"]), want)
    wide_q = torch.zeros(*pr["q"].shape[:-1], 640, dtype=torch.bfloat16, device=DEV)
    wide_q[..., :576] = pr["q"]
    wide_kv = poison_(torch.empty(*pr["cache"].shape[:-1], 640, dtype=torch.bfloat16, device=DEV))
    wide_kv[..., :576] = pr["cache"]
    assert torch.equal(_call(pr, query=wide_q[..., :576], kv_cache=wide_kv[..., :576]), want)


def test_length_beyond_the_row_is_clamped_to_the_row():
    dtype, ps, max_blocks = torch.float16, 16, 6
    c = make_case([max_blocks * ps, 40], 2, 16, ps, dtype, seed=21, max_blocks=max_blocks)
    pr = dict(c, q=c["q"].to(DEV), cache=c["cache"].to(DEV), table=c["table"].to(DEV), lens=c["lens"].to(DEV))
    at_capacity = _call(pr)
    beyond = _call(pr, seq_lens=torch.tensor([max_blocks * ps + 1000, 40], dtype=torch.int32, device=DEV))
    assert torch.equal(beyond, at_capacity)
    torch.testing.assert_close(at_capacity.float().cpu(), oracle_out(c, SM), **tol(dtype))


def test_captured_call_replans_from_what_it_finds_at_replay(fi_lib):
    """Captured with four 100-token requests (one chunk each); replayed after seq_lens, block_tables, the query and the
    cache were overwritten in place with a case that is split."""
    dtype, ps, B, q_len, H = torch.bfloat16, 64, 4, 2, 16
    first, second = [100] * B, [12000, 17, 5000, 64]
    plans = [host_plan(fi_lib, lens, q_len, H, ps, WS_BYTES)[1] for lens in (first, second)]
    assert plans[0][0][3] == 0 and plans[1][0][3] == 1 and plans[0][0][1] != plans[1][0][1]

    c = make_case(second, q_len, H, ps, dtype, seed=22)
    max_blocks, num_pages = c["max_blocks"], c["cache"].shape[0]
    # any valid pages and any finite values will do for the captured lengths
    pr = dict(q=torch.ones_like(c["q"], device=DEV), cache=torch.ones_like(c["cache"], device=DEV),
              table=torch.arange(B * max_blocks, dtype=torch.int32, device=DEV).remainder(num_pages)
              .reshape(B, max_blocks), lens=torch.tensor(first, dtype=torch.int32, device=DEV), ps=ps,
              max_blocks=max_blocks)
    ws = poison_(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV))
    out = torch.zeros(B, q_len, H, CKV, dtype=dtype, device=DEV)
    _call(pr, workspace_buffer=ws, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(pr, workspace_buffer=ws, out=out)
    pr["lens"].copy_(c["lens"])
    pr["table"].copy_(c["table"])
    pr["q"].copy_(c["q"])
    pr["cache"].copy_(c["cache"])
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    torch.testing.assert_close(out.float().cpu(), oracle_out(c, SM), **tol(dtype))
