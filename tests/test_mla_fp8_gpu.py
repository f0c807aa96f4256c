"""MLA with an fp8 KV cache on the GPU: the e4m3 cache (and query) against the 16-bit kernel on the upcast tensors, bit for
bit, and against the fp64 oracle; memory no request owns; float and tensor scales, captured; the fp8 append; and
flashinfer.rope.mla_rope_quantize_fp8 against its fp64 restatement."""
import functools
import math

import numpy as np
import pytest
import torch

from attn_inputs import append_problem, indptr_of, poison_, tol
from mla_fp8_ref import FP8, fp8_order, make_fp8_case, rope_quantize_ref
from mla_plan_free_inputs import CKV, KPE, oracle_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SM = 1.0 / math.sqrt(128 + 64)
WS_BYTES = 64 << 20
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
LOG2E = np.float32(1.44269504088896340736)

# (kv lens, q_len_per_request, heads, page size): the lengths around the 64-token tile, every page size class, one and
# two row tiles (8 heads x 3 tokens: 24 packed rows, the second tile half empty), 128 heads once, a split request
STAGING_CASES = {
    "tile_edges_page_1": ([1, 63, 64, 65, 129], 1, 16, 1),
    "tile_edges_page_16": ([1, 63, 64, 65, 129], 1, 16, 16),
    "tile_edges_page_64": ([1, 63, 64, 65, 129], 1, 16, 64),
    "two_row_tiles": ([65, 129, 1], 3, 8, 16),
    "128_heads": ([129], 1, 128, 16),
    "split_and_merge": ([700, 5], 1, 16, 16),
}


@functools.lru_cache(maxsize=None)
def _problem(case, dtype, fp8_query=False):
    """The inputs of a case on the GPU and its oracle output (on the dequantised tensors), built once, left unchanged."""
    lens, q_len, H, ps = STAGING_CASES[case]
    c = make_fp8_case(lens, q_len, H, ps, dtype, seed=sorted(STAGING_CASES).index(case), fp8_query=fp8_query)
    assert c["cache"].isnan().any(), "every case has unowned slots: a spare page at least"
    o_ref = oracle_out(dict(c, q=c["q"].float(), cache=torch.nan_to_num(c["cache"].float())), SM)
    on_gpu = {k: c[k].to(DEV) for k in ("q", "cache", "cache8", "table", "lens")}
    return dict(c, o_ref=o_ref, **on_gpu, q8=None if c["q8"] is None else c["q8"].to(DEV))


def _wrapper(pr, q, cache, sm_scale=SM):
    """BatchMLAPagedAttentionWrapper, host-planned for the case, run on views of the 576-wide q and cache: (o, lse)."""
    from flashinfer.mla import BatchMLAPagedAttentionWrapper

    B, q_len, H = len(pr["kv_lens"]), pr["q_len"], pr["H"]
    w = BatchMLAPagedAttentionWrapper(poison_(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)))
    w.plan(indptr_of([q_len] * B).to(DEV), pr["indptr"].to(DEV), pr["indices"].to(DEV), pr["lens"], H, CKV, KPE,
           pr["ps"], True, sm_scale, q.dtype, cache.dtype)
    q = q.view(B * q_len, H, CKV + KPE)
    return w.run(q[..., :CKV], q[..., CKV:], cache[..., :CKV], cache[..., CKV:], return_lse=True)


def _plan_free(pr, q, cache, **kw):
    from flashinfer.decode import trtllm_batch_decode_with_kv_cache_mla

    if "workspace_buffer" not in kw:
        kw["workspace_buffer"] = poison_(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV))
    args = dict(query=q, kv_cache=cache.unsqueeze(1), qk_nope_head_dim=128, kv_lora_rank=CKV, qk_rope_head_dim=KPE,
                block_tables=pr["table"], seq_lens=pr["lens"], max_seq_len=pr["max_blocks"] * pr["ps"], bmm1_scale=SM)
    args.update(kw)
    return trtllm_batch_decode_with_kv_cache_mla(**args)


def _meets_the_oracle(pr, o, dtype, scale=1.0, o_ref=None):
    o_ref = pr["o_ref"] if o_ref is None else o_ref
    assert torch.isfinite(o).all(), "memory that no request owns was read"
    print("max abs error", (o.float().cpu().view(o_ref.shape) - o_ref * scale).abs().max().item())
    torch.testing.assert_close(o.float().cpu().view(o_ref.shape), o_ref * scale, **tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", STAGING_CASES)
def test_fp8_cache_is_the_16_bit_kernel_on_the_upcast_cache(case, dtype):
    """The wrapper with a 16-bit q.  The upcast is exact and the loop is shared, so o and lse are the bits the 16-bit
    kernel gives for cache.to(dtype) under the same plan.  Unowned slots are NaN (0x7F / the upcast NaN) in both."""
    pr = _problem(case, dtype)
    o8, lse8 = _wrapper(pr, pr["q"], pr["cache8"])
    o16, lse16 = _wrapper(pr, pr["q"], pr["cache"])
    torch.cuda.synchronize()
    assert o8.dtype == dtype
    assert torch.equal(o8, o16) and torch.equal(lse8, lse16)
    _meets_the_oracle(pr, o8, dtype)
    # unchanged by what the unowned slots hold
    clean = torch.where(pr["cache8"].view(torch.uint8) == 0x7F, 0, pr["cache8"].view(torch.uint8)).view(E4M3)
    o_clean, lse_clean = _wrapper(pr, pr["q"], clean)
    assert torch.equal(o8, o_clean) and torch.equal(lse8, lse_clean)


@pytest.mark.parametrize("case", STAGING_CASES)
def test_fp8_query_and_cache_are_the_bf16_kernel_on_the_upcast_tensors(case):
    """The plan-free entry with an e4m3 query and cache (block-table entries past a request's pages point at a page of
    NaN bytes).  The output is bfloat16."""
    pr = _problem(case, torch.bfloat16, True)
    o8 = _plan_free(pr, pr["q8"], pr["cache8"])
    o16 = _plan_free(pr, pr["q"], pr["cache"])
    torch.cuda.synchronize()
    assert o8.dtype == torch.bfloat16 and o8.shape == (*pr["q8"].shape[:-1], CKV)
    assert torch.equal(o8, o16)
    _meets_the_oracle(pr, o8, torch.bfloat16)


def test_separate_caches_that_are_views_of_wider_tensors():
    pr = _problem("tile_edges_page_16", torch.float16)
    want, want_lse = _wrapper(pr, pr["q"], pr["cache8"])
    pages, ps = pr["cache8"].shape[:2]
    wide_ckv = poison_(torch.empty(pages, ps, 640, dtype=torch.uint8, device=DEV)).view(E4M3)
    wide_kpe = poison_(torch.empty(pages, ps, 128, dtype=torch.uint8, device=DEV)).view(E4M3)
    wide_ckv[..., 64:576] = pr["cache8"][..., :CKV]  # starts at byte 64 of each row
    wide_kpe[..., 16:80] = pr["cache8"][..., CKV:]
    wide_q = torch.zeros(*pr["q"].shape[:-1], 640, dtype=torch.float16, device=DEV)
    wide_q[..., :576] = pr["q"]
    from flashinfer.mla import BatchMLAPagedAttentionWrapper

    B, H = len(pr["kv_lens"]), pr["H"]
    w = BatchMLAPagedAttentionWrapper(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV))
    w.plan(indptr_of([1] * B).to(DEV), pr["indptr"].to(DEV), pr["indices"].to(DEV), pr["lens"], H, CKV, KPE, pr["ps"],
           True, SM, torch.float16, E4M3)
    q = wide_q.view(B, H, 640)
    o, lse = w.run(q[..., :CKV], q[..., CKV:576], wide_ckv[..., 64:576], wide_kpe[..., 16:80], return_lse=True)
    assert torch.equal(o, want) and torch.equal(lse, want_lse)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_a_nan_code_that_a_request_owns_is_a_nan(dtype):
    """Both NaN codes upcast to a non-finite value, never to a number: one owned byte each, two output columns."""
    pr = _problem("tile_edges_page_16", dtype)
    cache = pr["cache8"].clone()
    page = int(pr["indices"][int(pr["indptr"][1])])  # request 1's first page, token 0
    cache.view(torch.uint8)[page, 0, 3] = 0x7F
    cache.view(torch.uint8)[page, 0, 300] = 0xFF
    o, _ = _wrapper(pr, pr["q"], cache)
    assert o[1, :, [3, 300]].isnan().all()
    assert o[0].isfinite().all() and o[2:].isfinite().all()


# ---- scales ----

def test_float_scales_against_the_oracle():
    """bmm1_scale is the whole logit scale (k_scale folded in), bmm2_scale multiplies the output."""
    pr = _problem("two_row_tiles", torch.bfloat16, True)
    out = _plan_free(pr, pr["q8"], pr["cache8"], bmm1_scale=SM * 0.5, bmm2_scale=0.37)
    c = dict(pr, q=pr["q"].float().cpu(), cache=torch.nan_to_num(pr["cache"].float().cpu()))
    _meets_the_oracle(pr, out, torch.bfloat16, o_ref=oracle_out(c, SM * 0.5) * 0.37)
    assert not torch.equal(out, _plan_free(pr, pr["q8"], pr["cache8"]))


def _scale_tensors(bmm1, bmm2):
    """What the float path computes on the host: float32(bmm1) x float32(log2 e), and float32(bmm2)."""
    return (torch.tensor([np.float32(bmm1) * LOG2E], dtype=torch.float32, device=DEV),
            torch.tensor([bmm2], dtype=torch.float32, device=DEV))


def test_tensor_scales_are_the_equal_floats_and_take_precedence():
    pr = _problem("two_row_tiles", torch.bfloat16, True)
    want = _plan_free(pr, pr["q8"], pr["cache8"], bmm1_scale=SM * 0.5, bmm2_scale=0.37)
    t1, t2 = _scale_tensors(SM * 0.5, 0.37)
    got = _plan_free(pr, pr["q8"], pr["cache8"], bmm1_scale=123.0, bmm2_scale=-4.0, bmm1_scale_log2_tensor=t1,
                     bmm2_scale_tensor=t2)
    assert torch.equal(got, want)


def test_captured_call_follows_scale_tensors_and_lengths_changed_in_place():
    pr = _problem("split_and_merge", torch.bfloat16, True)
    lens = torch.tensor([100, 5], dtype=torch.int32, device=DEV)
    t1, t2 = _scale_tensors(SM, 1.0)
    ws = poison_(torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV))
    out = torch.zeros(*pr["q8"].shape[:-1], CKV, dtype=torch.bfloat16, device=DEV)
    kw = dict(workspace_buffer=ws, out=out, seq_lens=lens, bmm1_scale_log2_tensor=t1, bmm2_scale_tensor=t2)
    _plan_free(pr, pr["q8"], pr["cache8"], **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _plan_free(pr, pr["q8"], pr["cache8"], **kw)
    lens.copy_(pr["lens"])  # 100 -> 700 tokens: the replay splits and merges
    n1, n2 = _scale_tensors(SM * 0.5, 0.37)
    t1.copy_(n1)
    t2.copy_(n2)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _plan_free(pr, pr["q8"], pr["cache8"], bmm1_scale=SM * 0.5, bmm2_scale=0.37))
    c = dict(pr, q=pr["q"].float().cpu(), cache=torch.nan_to_num(pr["cache"].float().cpu()))
    _meets_the_oracle(pr, out, torch.bfloat16, o_ref=oracle_out(c, SM * 0.5) * 0.37)


# ---- append ----

@pytest.mark.parametrize("fp8_dtype", [E4M3, E5M2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("ps", [1, 16])
@pytest.mark.parametrize("lens,hist", [([1], [0]), ([20, 17], [5, 0])], ids=["nnz_1", "nnz_37"])
def test_fp8_append_writes_the_given_bytes_at_the_oracle_s_slots_and_nothing_else(lens, hist, ps, fp8_dtype):
    import flashinfer

    a = append_problem(lens, hist, ps, spare_pages=2, seed=3)
    nnz = sum(lens)
    g = torch.Generator().manual_seed(nnz + ps)
    rows = torch.randint(0, 256, (nnz, CKV + KPE), generator=g, dtype=torch.uint8).to(DEV)  # any byte, NaN codes too
    cache = torch.full((a["total_pages"], ps, CKV + KPE), 0x5A, dtype=torch.uint8, device=DEV)
    want = cache.clone()
    want.view(-1, CKV + KPE)[a["slot"]] = rows
    flashinfer.append_paged_mla_kv_cache(rows[:, :CKV].view(fp8_dtype), rows[:, CKV:].view(fp8_dtype), a["batch_indices"],
                                         a["positions"], cache[..., :CKV].view(fp8_dtype),
                                         cache[..., CKV:].view(fp8_dtype), a["kv_indices"], a["kv_indptr"], a["last"])
    torch.cuda.synchronize()
    assert torch.equal(cache, want)


# ---- mla_rope_quantize_fp8 ----

MAX_POS = 512


@functools.lru_cache(maxsize=None)
def _cos_sin_cache():
    inv_freq = 1.0 / (1e4 ** (torch.arange(0, KPE, 2, dtype=torch.float64) / KPE))
    ang = torch.arange(MAX_POS, dtype=torch.float64)[:, None] * inv_freq[None]
    return torch.cat([ang.cos(), ang.sin()], dim=1).float()


@functools.lru_cache(maxsize=None)
def _rope_inputs(nnz, H):
    """576-wide q [nnz, H, 576] and k [nnz, 576] in float32 (2 x randn, with +-300 and +-30000 sprinkled in: they
    saturate e4m3 at every scale used, and e5m2 at scale 8), and positions out of order."""
    g = torch.Generator().manual_seed(nnz * 1000 + H)
    q, k = torch.randn(nnz, H, CKV + KPE, generator=g) * 2, torch.randn(nnz, CKV + KPE, generator=g) * 2
    big = torch.tensor([300.0, -300.0, 30000.0, -30000.0])
    for t in (q, k):
        flat = t.view(-1)
        at = torch.randint(0, flat.numel(), (max(8, flat.numel() // 500),), generator=g)
        flat[at] = big[torch.arange(len(at)) % 4]
    k[0, 5], k[0, 6], k[0, CKV + 7], q[0, 0, 9], q[0, 0, CKV + 11] = 300.0, 30000.0, -300.0, -30000.0, 30000.0
    pos = torch.randint(0, MAX_POS, (nnz,), generator=g)
    return q, k, pos


# (input dtype, fp8 type, quant_scale_q, quant_scale_kv, positions' dtype)
ROPE_VARIANTS = {
    "f16_e4m3": (torch.float16, E4M3, 1.0, 0.37, torch.int64),
    "bf16_e5m2": (torch.bfloat16, E5M2, 0.37, 8.0, torch.int64),
    "bf16_e4m3": (torch.bfloat16, E4M3, 8.0, 1.0, torch.int32),
    "f16_e5m2": (torch.float16, E5M2, 8.0, 0.37, torch.int64),
}


@pytest.mark.parametrize("is_neox", [True, False], ids=["neox", "interleaved"])
@pytest.mark.parametrize("variant", ROPE_VARIANTS)
@pytest.mark.parametrize("H", [1, 16, 128])
@pytest.mark.parametrize("nnz", [1, 19, 257])
def test_mla_rope_quantize_fp8(nnz, H, variant, is_neox):
    from flashinfer.rope import mla_rope_quantize_fp8

    dtype, fp8_dtype, scale_q, scale_kv, pos_dtype = ROPE_VARIANTS[variant]
    q32, k32, pos = _rope_inputs(nnz, H)
    q_in, k_in = q32.to(dtype).to(DEV), k32.to(dtype).to(DEV)
    q_out = poison_(torch.empty(nnz, H, CKV + KPE, dtype=torch.uint8, device=DEV)).view(fp8_dtype)
    k_out = poison_(torch.empty(nnz, CKV + KPE, dtype=torch.uint8, device=DEV)).view(fp8_dtype)
    got = mla_rope_quantize_fp8(
        q_in[..., CKV:], k_in[..., CKV:], q_in[..., :CKV], k_in[..., :CKV], _cos_sin_cache().to(DEV),
        pos.to(pos_dtype).to(DEV), is_neox=is_neox, quant_scale_q=scale_q, quant_scale_kv=scale_kv,
        q_rope_out=q_out[..., CKV:], k_rope_out=k_out[..., CKV:], q_nope_out=q_out[..., :CKV],
        k_nope_out=k_out[..., :CKV])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == q_out[..., CKV:].data_ptr() and got[3].data_ptr() == k_out.data_ptr()
    fmax = FP8[fp8_dtype]["max"]
    assert q_out.float().isfinite().all() and k_out.float().isfinite().all(), "a value beyond the largest was not clamped"
    # nope: scale in f32, clamp, round to nearest even -- exactly
    for out, x, s in ((q_out, q_in, scale_q), (k_out, k_in, scale_kv)):
        want = (x[..., :CKV].float() * s).clamp(-fmax, fmax).to(fp8_dtype)
        assert torch.equal(out[..., :CKV].view(torch.uint8), want.view(torch.uint8))
    if fp8_dtype == E4M3 or scale_kv == 8.0:
        assert k_out[..., :CKV].float().abs().max() == fmax  # the sprinkled values saturate
    # rope: the fp64 restatement, up to rare one-code differences where f32 and fp64 round apart
    ref = rope_quantize_ref(q_in[..., CKV:].cpu(), k_in[..., CKV:].cpu(), q_in[..., :1].cpu(), k_in[..., :1].cpu(),
                            _cos_sin_cache(), pos, is_neox, fp8_dtype, scale_q, scale_kv)
    got_order = np.concatenate([fp8_order(t[..., CKV:].float().double().cpu().numpy().ravel(), fp8_dtype)
                                for t in (q_out, k_out)])
    ref_order = np.concatenate([fp8_order(ref[0].ravel(), fp8_dtype), fp8_order(ref[1].ravel(), fp8_dtype)])
    apart = got_order != ref_order
    print("rope elements", apart.size, "differ", int(apart.sum()))
    assert apart.sum() <= 1e-4 * apart.size
    assert (np.abs(got_order - ref_order)[apart] == 1).all()


def test_outputs_are_allocated_in_the_inferred_dtype():
    from flashinfer.rope import mla_rope_quantize_fp8

    q32, k32, pos = _rope_inputs(19, 16)
    q_in, k_in = q32.bfloat16().to(DEV), k32.bfloat16().to(DEV)
    args = (q_in[..., CKV:], k_in[..., CKV:], q_in[..., :CKV], k_in[..., :CKV], _cos_sin_cache().to(DEV), pos.to(DEV))
    outs = mla_rope_quantize_fp8(*args)
    assert [o.dtype for o in outs] == [E4M3] * 4 and [o.shape for o in outs] == [a.shape for a in args[:4]]
    given = torch.empty(19, CKV, dtype=E5M2, device=DEV)
    outs5 = mla_rope_quantize_fp8(*args, k_nope_out=given)
    assert [o.dtype for o in outs5] == [E5M2] * 4 and outs5[3] is given
    again = mla_rope_quantize_fp8(*args, quantize_dtype=E4M3)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, again))


# ---- end to end ----

def test_rope_quantize_then_append_then_decode():
    """The serving path: quantise q and k with their scales, append the fp8 rows, decode with the scales folded into
    bmm1_scale / bmm2_scale; against the fp64 oracle on the dequantised query and cache."""
    import flashinfer
    from flashinfer.rope import mla_rope_quantize_fp8

    lens, H, ps, scale_q, scale_kv = [70, 9], 16, 16, 2.0, 4.0
    B, nnz = len(lens), sum(lens)
    g = torch.Generator().manual_seed(11)
    q_in = (torch.randn(nnz, H, CKV + KPE, generator=g) * 0.5).bfloat16().to(DEV)
    k_in = (torch.randn(nnz, CKV + KPE, generator=g) * 0.5).bfloat16().to(DEV)
    a = append_problem(lens, [0, 0], ps, spare_pages=1, seed=4)
    q8 = torch.empty(nnz, H, CKV + KPE, dtype=E4M3, device=DEV)
    cache8 = torch.zeros(a["total_pages"], ps, CKV + KPE, dtype=torch.uint8, device=DEV).view(E4M3)
    _, k_rope8, _, k_nope8 = mla_rope_quantize_fp8(
        q_in[..., CKV:], k_in[..., CKV:], q_in[..., :CKV], k_in[..., :CKV], _cos_sin_cache().to(DEV), a["positions"],
        quant_scale_q=scale_q, quant_scale_kv=scale_kv, q_rope_out=q8[..., CKV:], q_nope_out=q8[..., :CKV])
    flashinfer.append_paged_mla_kv_cache(k_nope8, k_rope8, a["batch_indices"], a["positions"], cache8[..., :CKV],
                                         cache8[..., CKV:], a["kv_indices"], a["kv_indptr"], a["last"])
    last_rows = (indptr_of(lens)[1:] - 1).long().to(DEV)
    query = q8[last_rows].view(B, 1, H, CKV + KPE).contiguous()
    pages = [-(-l // ps) for l in lens]
    indptr = a["kv_indptr"].cpu()
    table = torch.zeros(B, max(pages), dtype=torch.int32)
    for b in range(B):
        table[b, : pages[b]] = a["kv_indices"].cpu()[int(indptr[b]): int(indptr[b + 1])]
    pr = dict(table=table.to(DEV), lens=torch.tensor(lens, dtype=torch.int32, device=DEV), max_blocks=max(pages), ps=ps)
    out = _plan_free(pr, query, cache8, bmm1_scale=SM / (scale_q * scale_kv), bmm2_scale=1.0 / scale_kv)
    torch.cuda.synchronize()
    c = dict(kv_lens=lens, indptr=indptr, indices=a["kv_indices"].cpu(), q=query.float().cpu() / scale_q,
             cache=cache8.float().cpu() / scale_kv)
    o_ref = oracle_out(c, SM)
    assert out.dtype == torch.bfloat16
    torch.testing.assert_close(out.float().cpu(), o_ref, **tol(torch.bfloat16))
