"""The device-side decode planner (fi_batch_decode_plan_device) against the host planner and the planner oracle, and
flashinfer.decode.trtllm_batch_decode_with_kv_cache against the attention oracle and the host-planned wrapper."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from attn_inputs import indptr_of, make_paged, page_table, poison_, tol
from flashinfer import _lib
from oracle import attention_ref as R
from oracle.plan_ref import decode_plan_ref
from plan_calls import run_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HQ, HKV, D = 32, 8, 128
LENS_A = [54, 4000, 1, 700, 33]


def _mixed_lens(n, hi, seed):
    return torch.randint(1, hi, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


# name -> (lens, page size, blocks per block-table row, max_grid_hint, row stride of the block table)
PLAN_CASES = {
    "a_split": (LENS_A, 16, 250, 128, None),  # 5 x 8 waves < 128: bisection over [8, 250] pages
    "a_default_grid": (LENS_A, 16, 256, 0, 300),  # the grid sized from the device; rows wider than max_blocks
    "b_unsplit": (LENS_A, 16, 250, 40, None),  # 5 x 8 waves fill a grid of 40
    "c_empty_search_range": ([5, 100, 111, 64], 16, 8, 256, None),  # at most 7 pages < the 8-page lower bound
    "d_page_size_1": ([1, 128, 129, 4096], 1, 4096, 256, None),
    "e_page_multiples_full_row": ([512, 256, 16, 160], 16, 32, 64, None),  # request 0 fills its 32-block row
    "f_more_requests_than_threads": (_mixed_lens(300, 3000, 1), 16, 188, 4096, None),
    "g_one_long_request": ([131072], 16, 8192, 1024, None),
    # beyond the issue's cases: empty requests (one chunk each on the host too) whose entries still fit the list
    "h_empty_requests_that_fit": ([54, 0, 700, 0], 16, 48, 128, None),
}
# the edges of the scan's round of 256 requests: one full round, one request into the second, one into the third;
# 1..600 tokens in 38 blocks a row, once under a grid that splits (batch x 8 < 8192) and once under one that does not
for _b in (256, 257, 513):
    PLAN_CASES[f"i_round_edge_{_b}_split"] = (_mixed_lens(_b, 601, _b), 16, 38, 8192, None)
    PLAN_CASES[f"i_round_edge_{_b}_unsplit"] = (_mixed_lens(_b, 601, _b), 16, 38, 64, None)


def _device_plan(fi_lib, lens, ps, max_blocks, hint, stride):
    """Run the planner's two launches; (plan_info, csr offsets, the int workspace as bytes, the block table)."""
    B = len(lens)
    g = torch.Generator().manual_seed(B * 7 + ps)
    table = torch.randint(0, 1000, (B, stride or max_blocks), generator=g, dtype=torch.int32)
    table_dev = table.to(DEV)[:, :max_blocks]
    lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
    p = _lib.fi_batch_decode_plan_device_params_t(
        block_tables=table_dev.data_ptr(), seq_lens=lens_dev.data_ptr(), block_tables_stride=table_dev.stride(0),
        batch_size=B, max_blocks=max_blocks, page_size=ps, num_qo_heads=HQ, num_kv_heads=HKV, head_dim=D,
        q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16, max_grid_hint=hint)
    ib, fb = C.c_size_t(), C.c_size_t()
    assert fi_lib.fi_batch_decode_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)) == 0
    # not zeroed: whatever is compared below was written by the planner
    int_ws = torch.full((ib.value,), 0xAB, dtype=torch.uint8, device=DEV)
    float_ws = torch.empty(max(fb.value, 16), dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes, p.float_ws, p.float_ws_bytes = int_ws.data_ptr(), ib.value, float_ws.data_ptr(), fb.value
    info, csr = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)(), (C.c_int64 * 3)()
    rc = fi_lib.fi_batch_decode_plan_device(C.byref(p), info, csr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fi_lib.fi_last_error()
    torch.cuda.synchronize()
    return list(info), list(csr), int_ws.cpu().numpy(), table[:, :max_blocks]


@pytest.mark.parametrize("case", PLAN_CASES)
def test_device_plan_equals_the_host_plan(fi_lib, case):
    lens, ps, max_blocks, hint, stride = PLAN_CASES[case]
    B = len(lens)
    info, csr, raw, table = _device_plan(fi_lib, lens, ps, max_blocks, hint, stride)

    def i32(off, count):
        return raw[off: off + 4 * count].view(np.int32).tolist()

    indptr, _, last, _ = page_table(lens, ps)
    host = run_plan(fi_lib, indptr.tolist(), HQ, HKV, ps, hint, cuda_graph=True)
    max_grid = hint if hint > 0 else fi_lib.fi_num_compute_units() * 4  # 16-bit cache, one head tile
    ref = decode_plan_ref(indptr.tolist(), HQ, HKV, ps, max_grid, enable_cuda_graph=True)
    n = host["num_work"]
    assert n == ref["num_work"] and host["split_kv"] == ref["split_kv"]

    # host-computed plan_info entries
    assert info[_lib.FI_DP_MAGIC] == _lib.FI_DECODE_PLAN_MAGIC and info[_lib.FI_DP_ENABLE_CUDA_GRAPH] == 1
    assert bool(info[_lib.FI_DP_SPLIT_KV]) == host["split_kv"]
    assert info[_lib.FI_DP_WINDOW_LEFT] == -1 and info[_lib.FI_DP_UNIFORM_CHUNKS] == 0
    assert info[_lib.FI_DP_BATCH_SIZE] == B and info[_lib.FI_DP_INT_BYTES_USED] == len(raw)
    padded = info[_lib.FI_DP_PADDED_BATCH_SIZE]
    assert padded >= n and padded == (max(max_grid // HKV, B) if host["split_kv"] else B)

    # the work list
    chunk, num_work = i32(info[_lib.FI_DP_KV_CHUNK_SIZE_PTR_OFFSET], 2)
    assert chunk == host["chunk_ptr"] == host["kv_chunk_size"] == ref["kv_chunk_size"]
    assert num_work == n
    req = i32(info[_lib.FI_DP_REQUEST_INDICES_OFFSET], padded)
    tile = i32(info[_lib.FI_DP_KV_TILE_INDICES_OFFSET], padded)
    assert req[:n] == host["request_indices"] == ref["request_indices"]
    assert tile[:n] == host["kv_tile_indices"] == ref["kv_tile_indices"]
    assert not any(req[n:]) and not any(tile[n:])  # as the host planner leaves the padding
    assert i32(info[_lib.FI_DP_O_INDPTR_OFFSET], B + 1) == host["o_indptr"] == ref["o_indptr"]
    if host["split_kv"]:
        off = info[_lib.FI_DP_BLOCK_VALID_MASK_OFFSET]
        mask = raw[off: off + padded].tolist()
        m = min(padded, host["padded_batch_size"])
        assert mask[:m] == host["mask"][:m]
        assert not any(mask[m:]) and not any(host["mask"][m:])

    # the CSR page table
    pages = (indptr[1:] - indptr[:-1]).tolist()
    assert i32(csr[0], B + 1) == indptr.tolist()
    assert i32(csr[2], B) == last.tolist()
    assert i32(csr[1], int(indptr[-1])) == torch.cat([table[b, :pages[b]] for b in range(B)]).tolist()


def test_empty_requests_cannot_outgrow_the_list(fi_lib):
    """One 4000-token request among four empty ones, a list of 16 entries.  The host rule cuts 16 chunks and appends the
    four one-chunk empty requests: 20 entries, and its list grows.  The device list cannot grow, so its search settles on
    the smallest chunk whose entries, empty requests included, fit."""
    lens, ps, hint = [0, 0, 4000, 0, 0], 16, 128
    info, _, raw, _ = _device_plan(fi_lib, lens, ps, 250, hint, None)
    padded = info[_lib.FI_DP_PADDED_BATCH_SIZE]
    assert padded == hint // HKV and info[_lib.FI_DP_SPLIT_KV] == 1
    host = run_plan(fi_lib, page_table(lens, ps)[0].tolist(), HQ, HKV, ps, hint, cuda_graph=True)
    assert host["num_work"] == 20 > padded
    pages_per_chunk = min(c for c in range(128 // ps, 251) if -(-250 // c) + 4 <= padded)
    chunks = [1, 1, -(-250 // pages_per_chunk), 1, 1]
    n = sum(chunks)

    def i32(off, count):
        return raw[off: off + 4 * count].view(np.int32).tolist()

    assert i32(info[_lib.FI_DP_KV_CHUNK_SIZE_PTR_OFFSET], 2) == [pages_per_chunk * ps, n]
    assert i32(info[_lib.FI_DP_O_INDPTR_OFFSET], len(lens) + 1) == indptr_of(chunks).tolist()
    pad = [0] * (padded - n)
    assert i32(info[_lib.FI_DP_REQUEST_INDICES_OFFSET], padded) == [b for b, c in enumerate(chunks) for _ in range(c)] + pad
    assert i32(info[_lib.FI_DP_KV_TILE_INDICES_OFFSET], padded) == [t for c in chunks for t in range(c)] + pad
    off = info[_lib.FI_DP_BLOCK_VALID_MASK_OFFSET]
    assert raw[off: off + padded].tolist() == [1] * n + [0] * (padded - n)


# ---- numerics: the whole call ----

def _table_of(indptr, indices, max_blocks, fill):
    """Dense block table of a CSR page table; entries past a request's pages hold `fill`."""
    B = len(indptr) - 1
    table = torch.full((B, max_blocks), fill, dtype=torch.int32)
    for b in range(B):
        row = indices[int(indptr[b]): int(indptr[b + 1])]
        table[b, : len(row)] = row
    return table


@functools.lru_cache(maxsize=None)
def _problem(dtype):
    """Lens (a), Hq/Hkv/D = 32/8/128, page 16, an HND cache; block-table entries past a request's pages point at a
    valid page of 0xFF bytes (NaN in f16 and bf16), which turns the result into NaN if it is read, even under a
    probability of zero.  The oracle output is shared."""
    ps, max_blocks = 16, 256
    cache, indptr, indices, last = make_paged(len(LENS_A), LENS_A, ps, HKV, D, dtype, "HND", seed=7)
    poison = min(set(range(cache.shape[0])) - set(indices.tolist()))
    poison_(cache[poison])
    q = torch.randn(len(LENS_A), HQ, D, generator=torch.Generator().manual_seed(8)).to(dtype)
    o_ref, _ = R.batch_decode_ref(q.float(), cache.float(), "HND", indptr, indices, last)
    return dict(q=q.to(DEV), cache=cache.to(DEV), indptr=indptr, indices=indices, last=last, o_ref=o_ref.float(),
                table=_table_of(indptr, indices, max_blocks, poison).to(DEV),
                lens=torch.tensor(LENS_A, dtype=torch.int32, device=DEV), ps=ps, max_blocks=max_blocks)


def _call(pr, kv_cache=None, **kw):
    from flashinfer.decode import trtllm_batch_decode_with_kv_cache

    args = dict(query=pr["q"], kv_cache=pr["cache"] if kv_cache is None else kv_cache,
                workspace_buffer=torch.empty(32 << 20, dtype=torch.uint8, device=DEV), block_tables=pr["table"],
                seq_lens=pr["lens"], max_seq_len=pr["max_blocks"] * pr["ps"], bmm1_scale=1.0 / math.sqrt(D),
                bmm2_scale=1.0)
    args.update(kw)
    return trtllm_batch_decode_with_kv_cache(**args)


def _host_planned(pr, dtype, window_left=-1, sinks=None):
    """BatchDecodeWithPagedKVCacheWrapper in graph mode, planned on the host for the same lengths."""
    import flashinfer

    B = len(pr["last"])
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(
        torch.zeros(32 << 20, dtype=torch.uint8, device=DEV), "HND", use_cuda_graph=True,
        paged_kv_indptr_buffer=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buffer=torch.zeros(len(pr["indices"]), dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buffer=torch.zeros(B, dtype=torch.int32, device=DEV))
    w.plan(pr["indptr"], pr["indices"], pr["last"], HQ, HKV, D, pr["ps"], q_data_type=dtype, kv_data_type=dtype,
           window_left=window_left)
    return w.run(pr["q"], pr["cache"], sinks=sinks)


@pytest.mark.parametrize("form", ["tensor", "tuple"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_output_matches_the_oracle_and_the_host_planned_wrapper(dtype, form):
    pr = _problem(dtype)
    kv = pr["cache"] if form == "tensor" else (pr["cache"][:, 0].contiguous(), pr["cache"][:, 1].contiguous())
    out = _call(pr, kv_cache=kv)
    torch.cuda.synchronize()
    torch.testing.assert_close(out.float().cpu(), pr["o_ref"], **tol(dtype))
    # the same work list through the same kernels: the same arithmetic
    assert torch.equal(out, _host_planned(pr, dtype))


def test_bmm2_scale_multiplies_the_output_and_out_is_written_in_place():
    pr = _problem(torch.float16)
    one = _call(pr)
    given = torch.zeros_like(pr["q"])
    half = _call(pr, bmm2_scale=0.5, out=given)
    assert half is given
    assert torch.equal(half, one * 0.5)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_window_and_sinks_agree_with_the_host_planned_wrapper(dtype):
    pr = _problem(dtype)
    sinks = torch.randn(HQ, generator=torch.Generator().manual_seed(9)).to(DEV)
    plain = _call(pr)
    for kw in (dict(window_left=256), dict(sinks=sinks), dict(sinks=[sinks])):
        out = _call(pr, **kw)
        want = _host_planned(pr, dtype, window_left=kw.get("window_left", -1), sinks=sinks if "sinks" in kw else None)
        torch.testing.assert_close(out.float(), want.float(), **tol(dtype))
        assert not torch.equal(out, plain), "the argument must change the result for this to mean anything"


def test_empty_request_gives_a_zero_row_and_leaves_the_others_alone():
    dtype, ps, lens = torch.float16, 16, [54, 0, 700]
    cache, indptr, indices, last = make_paged(3, lens, ps, HKV, D, dtype, "HND", seed=11)
    q = torch.randn(3, HQ, D, generator=torch.Generator().manual_seed(12)).to(dtype)
    pr = dict(q=q.to(DEV), cache=cache.to(DEV), table=_table_of(indptr, indices, 48, 0).to(DEV),
              lens=torch.tensor(lens, dtype=torch.int32, device=DEV), ps=ps, max_blocks=48)
    out = _call(pr, out=torch.full_like(pr["q"], 7.0)).cpu()
    assert torch.count_nonzero(out[1]) == 0
    keep = [0, 2]  # the empty request owns no page: the other two form a page table of their own
    o_ref, _ = R.batch_decode_ref(q[keep].float(), cache.float(), "HND", indptr_of([4, 44]), indices, last[keep])
    torch.testing.assert_close(out[keep].float(), o_ref.float(), **tol(dtype))


def test_length_beyond_the_row_is_clamped_to_the_row():
    dtype, ps, max_blocks = torch.float16, 16, 6
    lens = [max_blocks * ps, 40]
    cache, indptr, indices, last = make_paged(2, lens, ps, HKV, D, dtype, "HND", seed=13)
    q = torch.randn(2, HQ, D, generator=torch.Generator().manual_seed(14)).to(dtype)
    pr = dict(q=q.to(DEV), cache=cache.to(DEV), table=_table_of(indptr, indices, max_blocks, 0).to(DEV),
              lens=torch.tensor(lens, dtype=torch.int32, device=DEV), ps=ps, max_blocks=max_blocks)
    at_capacity = _call(pr)
    beyond = _call(pr, seq_lens=torch.tensor([lens[0] + 1000, 40], dtype=torch.int32, device=DEV))
    assert torch.equal(beyond, at_capacity)
    o_ref, _ = R.batch_decode_ref(q.float(), cache.float(), "HND", indptr, indices, last)
    torch.testing.assert_close(at_capacity.float().cpu(), o_ref.float(), **tol(dtype))


def test_captured_call_replans_from_the_lengths_it_finds_at_replay(fi_lib):
    """Captured with four 100-token requests (4 work items, 128-token chunks); replayed after seq_lens and
    block_tables were overwritten in place with lengths that need more and longer chunks."""
    dtype, ps, B = torch.float16, 16, 4
    first, second = [100] * B, [12000, 17, 5000, 64]
    max_grid = fi_lib.fi_num_compute_units() * 4
    plans = [decode_plan_ref(indptr_of(-(-l // ps) for l in lens).tolist(), HQ, HKV, ps, max_grid, True)
             for lens in (first, second)]
    assert plans[0]["kv_chunk_size"] != plans[1]["kv_chunk_size"] and plans[0]["num_work"] != plans[1]["num_work"]

    max_blocks = -(-max(second) // ps)
    cache, indptr, indices, last = make_paged(B, second, ps, HKV, D, dtype, "HND", seed=15)
    q = torch.randn(B, HQ, D, generator=torch.Generator().manual_seed(16)).to(dtype)
    table = _table_of(indptr, indices, max_blocks, 0)
    # any valid pages will do for the captured lengths
    pr = dict(q=q.to(DEV), cache=cache.to(DEV), table=torch.arange(B * max_blocks, dtype=torch.int32, device=DEV)
              .remainder(cache.shape[0]).reshape(B, max_blocks), ps=ps, max_blocks=max_blocks,
              lens=torch.tensor(first, dtype=torch.int32, device=DEV))
    ws = torch.empty(32 << 20, dtype=torch.uint8, device=DEV)
    out = torch.zeros_like(pr["q"])
    _call(pr, workspace_buffer=ws, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(pr, workspace_buffer=ws, out=out)
    pr["lens"].copy_(torch.tensor(second, dtype=torch.int32))
    pr["table"].copy_(table)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    o_ref, _ = R.batch_decode_ref(q.float(), cache.float(), "HND", indptr, indices, last)
    torch.testing.assert_close(out.float().cpu(), o_ref.float(), **tol(dtype))
