"""GPU: flashinfer.sparse against the float64 oracle of tests/sparse_ref.py.

BlockSparseAttentionWrapper on the prefill route (full blocks, inner masks, causal, long rows, fp8) and on the decode
route (R = 1), bit for bit against a hand-planned paged wrapper; VariableBlockSparseAttentionWrapper; and the index
kernels of csrc/sparse.hip, called through the C ABI, against their restatements (exact)."""
import functools

import pytest
import torch

import sparse_ref as S
from attn_inputs import DEV, indptr_of, planned_prefill_wrapper, ptol, tol
from oracle import attention_ref as R_

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
WS_BYTES = 32 << 20
LSE_TOL = dict(rtol=1e-3, atol=1e-3)

# (R, C, M, N, Hq, Hkv, D, dtype)
FIRST = (16, 16, 200, 256, 4, 2, 128, F16)        # M % R != 0, GQA
PREFILL_CASES = [
    FIRST,
    (128, 64, 384, 512, 2, 2, 128, BF16),         # full 128-row tiles
    (4, 1, 64, 96, 4, 1, 64, F16),                # C = 1, KV lengths that are no multiple of the 64-row tile
    (64, 4, 192, 256, 1, 1, 256, F16),            # 16 pages per KV tile, two idle waves, head_dim 256
]


def _ws():
    return torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=None)
def _bsr_case(case, seed=0):
    """(q, k, v, indptr, indices) of a case on the CPU: the shared pattern, block row 1 empty and block row 2 full."""
    R, Cc, M, N, hq, hkv, d, dtype = case
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(M, hq, d, generator=g).to(dtype)
    k = torch.randn(N, hkv, d, generator=g).to(dtype)
    v = torch.randn(N, hkv, d, generator=g).to(dtype)
    indptr, indices, _ = S.bsr_pattern(-(-M // R), N // Cc, seed + 1)
    return q, k, v, indptr, indices


@functools.lru_cache(maxsize=None)
def _bsr_oracle(case):
    q, k, v, indptr, indices = _bsr_case(case)
    return S.bsr_attention_gathered(q, k, v, indptr, indices, case[0], case[1])


def _planned(case, indptr, indices, **plan_kw):
    import flashinfer

    R, Cc, M, N, hq, hkv, d, dtype = case
    w = flashinfer.BlockSparseAttentionWrapper(_ws())
    plan_kw.setdefault("q_data_type", dtype)
    plan_kw.setdefault("o_data_type", dtype)
    w.plan(indptr.to(DEV), indices.to(DEV), M, N, R, Cc, hq, hkv, d, **plan_kw)
    return w


def _check(o, lse, o_ref, lse_ref, out_tol):
    err_o = (o.double().cpu() - o_ref).abs().max().item()
    err_lse = (lse.double().cpu() - lse_ref).abs().max().item()
    print(f"max |o - oracle| {err_o:.3e}  max |lse - oracle| {err_lse:.3e}  bars {out_tol} / {LSE_TOL}")
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **out_tol)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), **LSE_TOL)


@pytest.mark.parametrize("case", PREFILL_CASES, ids=lambda c: "R{}_C{}_M{}_N{}_h{}_{}_d{}".format(*c[:7]))
def test_prefill_route_matches_the_oracle(case):
    R = case[0]
    q, k, v, indptr, indices = _bsr_case(case)
    w = _planned(case, indptr, indices)
    assert w._use_tensor_cores
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    assert o.shape == q.shape and o.dtype == case[7] and lse.shape == q.shape[:2]
    _check(o, lse, *_bsr_oracle(case), ptol(case[7]))
    # block row 1 selects nothing: the empty-range result, exactly
    assert torch.all(o[R:2 * R] == 0) and torch.all(lse[R:2 * R] == S.NEG_INF_LSE)
    # without lse, into a caller's buffer
    out = torch.empty_like(o)
    assert w.run(q.to(DEV), k.to(DEV), v.to(DEV), out=out) is out
    assert torch.equal(out, o)


def test_inner_mask_and_its_packed_form():
    """mask (nnz, R, C) with column 0 of every block set (no row fully masked); M = 200 leaves 8 of the last block
    row's 16 rows, so the rows past M must be trimmed.  packed_mask= of the same bits gives the same output."""
    import flashinfer

    R, Cc, M = FIRST[:3]
    q, k, v, indptr, indices = _bsr_case(FIRST)
    nnz = int(indptr[-1])
    mask = torch.rand(nnz, R, Cc, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[:, :, 0] = True
    w = _planned(FIRST, indptr, indices, mask=mask.to(DEV), causal=True)  # causal is ignored with a mask
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    o, lse = w.run(dq, dk, dv, return_lse=True)
    _check(o, lse, *S.bsr_attention_gathered(q, k, v, indptr, indices, R, Cc, block_mask=mask), ptol(F16))

    kv_lens = (indptr[1:] - indptr[:-1]).long() * Cc
    qo_lens = torch.full_like(kv_lens, R)
    qo_lens[-1] = M - (len(kv_lens) - 1) * R
    assert int(qo_lens[-1]) == 8 and int(kv_lens[-1]) > 0
    flat = S.bsr_mask_layout(mask, indptr)
    flat = flat[: flat.numel() - (R - int(qo_lens[-1])) * int(kv_lens[-1])]
    assert flat.numel() == int((qo_lens * kv_lens).sum())
    packed, _ = flashinfer.segment_packbits(flat.to(DEV), indptr_of((qo_lens * kv_lens).tolist()).to(DEV), "little")
    w2 = _planned(FIRST, indptr, indices, packed_mask=packed)
    o2, lse2 = w2.run(dq, dk, dv, return_lse=True)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


def test_causal_against_the_gathered_oracle():
    R, Cc = FIRST[:2]
    q, k, v, indptr, indices = _bsr_case(FIRST)
    w = _planned(FIRST, indptr, indices, causal=True)
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    _check(o, lse, *S.bsr_attention_gathered(q, k, v, indptr, indices, R, Cc, causal=True), ptol(F16))
    assert torch.all(o[R:2 * R] == 0) and torch.all(lse[R:2 * R] == S.NEG_INF_LSE)


@pytest.mark.parametrize("heads", [(8, 2), (2, 2)])
@pytest.mark.parametrize("dtype", [F16, BF16])
def test_decode_route(heads, dtype):
    """R = 1: one block row is one decode request (Quest-style page selection per decode step)."""
    case = (1, 16, 8, 1024, *heads, 128, dtype)
    q, k, v, indptr, indices = _bsr_case(case)
    w = _planned(case, indptr, indices)
    assert not w._use_tensor_cores and w._active is w._decode
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    assert o.shape == q.shape and o.dtype == dtype
    _check(o, lse, *_bsr_oracle(case), tol(dtype))
    assert torch.all(o[1] == 0) and torch.all(lse[1] == S.NEG_INF_LSE)


def test_long_rows():
    """Two block rows of 16 queries over all 128 blocks of an 8192-token KV: the planner is free to split KV."""
    case = (16, 64, 32, 8192, 1, 1, 128, F16)
    g = torch.Generator().manual_seed(4)
    q = torch.randn(32, 1, 128, generator=g).half()
    k, v = torch.randn(8192, 1, 128, generator=g).half(), torch.randn(8192, 1, 128, generator=g).half()
    indptr = torch.tensor([0, 128, 256], dtype=torch.int32)
    indices = torch.cat([torch.randperm(128, generator=g), torch.arange(128)]).to(torch.int32)
    w = _planned(case, indptr, indices)
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    _check(o, lse, *S.bsr_attention_gathered(q, k, v, indptr, indices, 16, 64), ptol(F16))


def test_fp8_e4m3_with_per_head_scales():
    """fp8 q = k = v with per-head scales on the fp8 prefill path; the oracle sees the dequantised inputs.  Output bar
    rtol = atol = 5e-2, the bar of tests/test_prefill_gpu.py for fp8 attention (P is rounded to e4m3)."""
    R, Cc, M, N, hq, hkv, d = 64, 64, 192, 256, 4, 2, 128
    case = (R, Cc, M, N, hq, hkv, d, F16)
    q, k, v, indptr, indices = _bsr_case(case)
    (q8, sq), (k8, sk), (v8, sv) = (R_.per_head_symmetric_quant(x) for x in (q, k, v))
    f8 = torch.float8_e4m3fn
    w = _planned(case, indptr, indices, q_data_type=f8, kv_data_type=f8, o_data_type=F16)
    o, lse = w.run(q8.to(DEV), k8.to(DEV), v8.to(DEV), sq.to(DEV), sk.to(DEV), sv.to(DEV), return_lse=True)
    assert o.dtype == F16
    deq = lambda x8, s: x8.float().double() * s.double()[None, :, None]
    o_ref, lse_ref = S.bsr_attention_gathered(deq(q8, sq), deq(k8, sk), deq(v8, sv), indptr, indices, R, Cc)
    _check(o, lse, o_ref, lse_ref, dict(rtol=5e-2, atol=5e-2))
    assert torch.all(o[R:2 * R] == 0) and torch.all(lse[R:2 * R] == S.NEG_INF_LSE)


def test_same_kernel_as_a_hand_planned_paged_wrapper():
    """A BSR block row is a request with qo_len = R over pages of C rows: the output is bit for bit that of a
    BatchPrefillWithPagedKVCacheWrapper planned on the same table and workspace size."""
    R, Cc, M, N, hq, hkv, d, dtype = FIRST
    q, k, v, indptr, indices = _bsr_case(FIRST)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    o, lse = _planned(FIRST, indptr, indices).run(dq, dk, dv, return_lse=True)
    pages = indptr[1:] - indptr[:-1]
    qo_lens = [R] * (len(pages) - 1) + [M - (len(pages) - 1) * R]
    last = torch.where(pages > 0, Cc, 0).to(torch.int32)  # the suite's table form: 0 for a request without pages
    hand = planned_prefill_wrapper(WS_BYTES, "NHD", indptr_of(qo_lens), indptr, indices, last, hq, hkv, d, Cc,
                                   q_data_type=dtype)
    o_h, lse_h = hand.run(dq, (dk.view(N // Cc, Cc, hkv, d), dv.view(N // Cc, Cc, hkv, d)), return_lse=True)
    assert torch.equal(o, o_h) and torch.equal(lse, lse_h)


# ---- variable blocks ----

def _partition(total, parts, must, g):
    """`parts` positive sizes summing to `total`, the sizes in `must` among them, in a random order."""
    rest, n = total - sum(must), parts - len(must)
    cuts = (torch.randperm(rest - 1, generator=g)[: n - 1] + 1).sort().values.tolist()
    sizes = list(must) + [b - a for a, b in zip([0] + cuts, cuts + [rest])]
    return [sizes[i] for i in torch.randperm(parts, generator=g).tolist()]


@functools.lru_cache(maxsize=None)
def _variable_case():
    """Hkv 2, group 2, D 128, f16; qo_len 300 in 5 block rows, kv_len 520 in 9 block columns, a size 1 and a size over
    64 in each; density 0.5 with block row 1 empty and block row 2 full."""
    g = torch.Generator().manual_seed(11)
    hkv, group, d, qo_len, kv_len, MB, NB = 2, 2, 128, 300, 520, 5, 9
    row_sz = torch.tensor([_partition(qo_len, MB, (1, 70), g) for _ in range(hkv)], dtype=torch.int32)
    col_sz = torch.tensor([_partition(kv_len, NB, (1, 70), g) for _ in range(hkv)], dtype=torch.int32)
    block_map = torch.rand(hkv, MB, NB, generator=g) < 0.5
    block_map[:, 1] = False
    block_map[:, 2] = True
    q = torch.randn(hkv * group, qo_len, d, generator=g).half()
    k, v = torch.randn(hkv, kv_len, d, generator=g).half(), torch.randn(hkv, kv_len, d, generator=g).half()
    return q, k, v, block_map, row_sz, col_sz


@pytest.mark.parametrize("causal", [False, True])
def test_variable_blocks_gqa(causal):
    import flashinfer

    q, k, v, block_map, row_sz, col_sz = _variable_case()
    w = flashinfer.VariableBlockSparseAttentionWrapper(_ws())
    w.plan(block_map.to(DEV), row_sz.to(DEV), col_sz.to(DEV), 4, 2, 128, causal=causal)
    assert w._page_size == 1
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    assert o.shape == q.shape and lse.shape == q.shape[:2] and lse.dtype == torch.float32
    _check(o, lse, *S.variable_block_attention(q, k, v, block_map, row_sz, col_sz, causal=causal), ptol(F16))
    o_only = w.run(q.to(DEV), k.to(DEV), v.to(DEV))
    assert torch.equal(o_only, o)
    out = torch.empty_like(o)
    assert w.run(q.to(DEV), k.to(DEV), v.to(DEV), out=out) is out and torch.equal(out, o)


def test_variable_blocks_multiples_of_16_in_place():
    """Hkv 1, group 1, D 64, bf16, every size a multiple of 16: pages of 16 tokens, q read and out written in place."""
    import flashinfer

    g = torch.Generator().manual_seed(12)
    row_sz = torch.tensor([[16, 48, 32, 64, 32]], dtype=torch.int32)
    col_sz = torch.tensor([[32, 16, 64, 48, 16, 80]], dtype=torch.int32)
    block_map = torch.rand(1, 5, 6, generator=g) < 0.5
    block_map[:, 1] = False
    block_map[:, 2] = True
    q = torch.randn(1, 192, 64, generator=g).bfloat16()
    k, v = torch.randn(1, 256, 64, generator=g).bfloat16(), torch.randn(1, 256, 64, generator=g).bfloat16()
    w = flashinfer.VariableBlockSparseAttentionWrapper(_ws())
    w.plan(block_map.to(DEV), row_sz.to(DEV), col_sz.to(DEV), 1, 1, 64, q_data_type=BF16)
    assert w._page_size == 16
    o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    assert lse.shape == (1, 192)
    _check(o, lse, *S.variable_block_attention(q, k, v, block_map, row_sz, col_sz), ptol(BF16))
    out = torch.full_like(o, float("nan"))
    lse_buf = torch.empty_like(lse)
    got, got_lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), out=out, lse=lse_buf, return_lse=True)
    assert got.data_ptr() == out.data_ptr() and got_lse.data_ptr() == lse_buf.data_ptr()
    assert torch.equal(out, o) and torch.equal(lse_buf, lse)


@pytest.mark.parametrize("case", [FIRST, (1, 16, 8, 1024, 8, 2, 128, F16)], ids=["prefill_route", "decode_route"])
def test_deprecated_forward_sets_the_run_options(case):
    """forward() with its defaults is run() of a default plan, bit for bit; forward(sm_scale=) computes with that scale,
    also right after a run() on the same tensors (the decode wrapper keeps a validated argument block per plan)."""
    R, Cc, dtype = case[0], case[1], case[7]
    q, k, v, indptr, indices = _bsr_case(case)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    w = _planned(case, indptr, indices, sm_scale=0.2)
    o_planned = w.run(dq, dk, dv)
    o_default = w.forward(dq, dk, dv)
    assert torch.equal(o_default, _planned(case, indptr, indices).run(dq, dk, dv))
    assert not torch.equal(o_default, o_planned)
    o_scaled = w.forward(dq, dk, dv, sm_scale=0.05)
    o_ref, _ = S.bsr_attention_gathered(q, k, v, indptr, indices, R, Cc, sm_scale=0.05)
    torch.testing.assert_close(o_scaled.float().cpu(), o_ref.float(), **(ptol(dtype) if R > 1 else tol(dtype)))
    w.end_forward()


def test_variable_blocks_deprecated_forward():
    import flashinfer

    q, k, v, block_map, row_sz, col_sz = _variable_case()
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    w = flashinfer.VariableBlockSparseAttentionWrapper(_ws())
    w.plan(block_map.to(DEV), row_sz.to(DEV), col_sz.to(DEV), 4, 2, 128)
    assert torch.equal(w.forward(dq, dk, dv), w.run(dq, dk, dv))
    o_scaled = w.forward(dq, dk, dv, sm_scale=0.05)
    o_ref, _ = S.variable_block_attention(q, k, v, block_map, row_sz, col_sz, sm_scale=0.05)
    torch.testing.assert_close(o_scaled.float().cpu(), o_ref.float(), **ptol(F16))


# ---- the expansion kernels, through the C ABI ----

def _expand_on_device(block_map, col_sz, granule, capacity=None):
    """(rc of the two calls, row_pages, kv_indices) on the device; kv_indices starts as -1 everywhere."""
    from flashinfer import _lib

    lib = _lib.lib()
    H, MB, NB = block_map.shape
    kv_len = int(col_sz[0].sum())
    mask = block_map.to(DEV).contiguous().view(torch.uint8)
    cs = col_sz.to(DEV).contiguous()
    row_pages = torch.full((H * MB,), -1, dtype=torch.int32, device=DEV)
    stream = _lib.current_stream(torch.device(DEV))
    rc1 = lib.fi_block_mask_row_pages(mask.data_ptr(), cs.data_ptr(), H, MB, NB, granule, kv_len,
                                      row_pages.data_ptr(), stream)
    kv_indptr = torch.zeros(H * MB + 1, dtype=torch.int32, device=DEV)
    kv_indptr[1:] = torch.cumsum(row_pages, 0)
    total = int(kv_indptr[-1])
    capacity = total if capacity is None else capacity
    kv_indices = torch.full((max(capacity, 1),), -1, dtype=torch.int32, device=DEV)
    rc2 = lib.fi_block_mask_to_page_indices(mask.data_ptr(), cs.data_ptr(), kv_indptr.data_ptr(), H, MB, NB, granule,
                                            kv_len, total, capacity, kv_indices.data_ptr(), stream)
    torch.cuda.synchronize()
    return (rc1, rc2), row_pages.cpu(), kv_indptr.cpu(), kv_indices.cpu()[:capacity]


def _expansion_case(H, MB, NB, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = torch.randint(lo, hi + 1, (NB,), generator=g)
    col_sz = torch.stack([sizes[torch.randperm(NB, generator=g)] for _ in range(H)]).to(torch.int32)
    block_map = torch.rand(H, MB, NB, generator=g) < 0.5
    if H > 1:
        block_map[1] = False  # one head with nothing selected
    return block_map, col_sz


@pytest.mark.parametrize("H,MB,NB,lo,hi,scale", [
    (3, 7, 70, 1, 150, 1),     # NB past one wave, blocks past 64 granules, granule 1
    (3, 7, 70, 1, 150, 16),    # the same sizes x 16 at granule 16
    (1, 2, 300, 1, 5, 1),      # NB past the 256 columns a workgroup scans in one pass
])
def test_block_map_expansion_equals_the_restatement(H, MB, NB, lo, hi, scale):
    block_map, col_sz = _expansion_case(H, MB, NB, lo, hi, seed=21)
    col_sz = col_sz * scale
    rcs, row_pages, kv_indptr, kv_indices = _expand_on_device(block_map, col_sz, scale)
    assert rcs == (0, 0)
    ref_pages, ref_indptr, ref_indices = S.expand_block_mask(block_map, col_sz, scale)
    assert torch.equal(row_pages, ref_pages)
    assert torch.equal(kv_indptr, ref_indptr)
    assert torch.equal(kv_indices, ref_indices)
    if scale == 16:  # the page numbers are those of granule 1 on the unscaled sizes
        assert torch.equal(kv_indices, S.expand_block_mask(block_map, col_sz // 16, 1)[2])


def test_block_map_expansion_refuses_a_small_buffer():
    from flashinfer import _lib

    block_map, col_sz = _expansion_case(3, 7, 70, 1, 150, seed=21)
    total = int(S.expand_block_mask(block_map, col_sz, 1)[1][-1])
    rcs, _, _, kv_indices = _expand_on_device(block_map, col_sz, 1, capacity=total - 1)
    assert rcs[0] == 0 and rcs[1] != 0
    assert b"holds" in _lib.lib().fi_last_error()
    assert torch.all(kv_indices == -1), "nothing may be launched"


@pytest.mark.parametrize("block_size,stride_block", [(1, 1), (1, 48), (16, 16 * 24)])
def test_block_sparse_indices_to_vector_sparse_offsets(block_size, stride_block):
    import flashinfer

    g = torch.Generator().manual_seed(31)
    blocks = [3, 1, 4]
    kv_lens = [40, 16, 50] if block_size == 16 else blocks  # not multiples of the block size
    stride_n = 24 if block_size == 16 else 1
    indices = torch.randperm(40, generator=g)[: sum(blocks)].to(torch.int32)
    block_indptr, vector_indptr = indptr_of(blocks), indptr_of(kv_lens)
    out = torch.full((sum(kv_lens) + 5,), -1, dtype=torch.int32, device=DEV)
    got = flashinfer.page.block_sparse_indices_to_vector_sparse_offsets(
        indices.to(DEV), block_indptr.to(DEV), out, vector_indptr.to(DEV),
        torch.tensor(kv_lens, dtype=torch.int32, device=DEV), stride_block, stride_n, block_size)
    torch.cuda.synchronize()
    if block_size == 1:  # the shortcut: nothing is launched, the buffer stays as it was
        assert torch.all(out == -1)
        ref = S.vector_sparse_offsets(indices, block_indptr, vector_indptr, kv_lens, stride_block, stride_n, 1,
                                      sum(kv_lens))
    else:
        assert got is out
        ref = S.vector_sparse_offsets(indices, block_indptr, vector_indptr, kv_lens, stride_block, stride_n,
                                      block_size, out.numel())
    assert torch.equal(got.cpu(), ref)


# ---- errors ----

def test_errors():
    import flashinfer

    R, Cc, M, N, hq, hkv, d, dtype = FIRST
    q, k, v, indptr, indices = _bsr_case(FIRST)
    w = flashinfer.BlockSparseAttentionWrapper(_ws())
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    with pytest.raises(RuntimeError, match="plan"):
        w.run(dq, dk, dv)
    plan = lambda ip, ix, *a, **kw: w.plan(ip.to(DEV), ix.to(DEV), *a, q_data_type=dtype, o_data_type=dtype, **kw)
    with pytest.raises(ValueError, match="divisible"):
        plan(indptr, indices, M, N + 1, R, Cc, hq, hkv, d)
    bad = indices.clone()
    bad[3] = N // Cc
    with pytest.raises(ValueError, match="out of bound"):
        plan(indptr, bad, M, N, R, Cc, hq, hkv, d)
    with pytest.raises(ValueError, match="indptr"):
        plan(indptr[:-1], indices, M, N, R, Cc, hq, hkv, d)
    with pytest.raises(ValueError, match="multiple"):
        plan(indptr, indices, M, N, R, Cc, 3, 2, d)
    with pytest.raises(RuntimeError, match="plan"):  # a refused plan() leaves no plan behind
        w.run(dq, dk, dv)
    plan(indptr, indices, M, N, R, Cc, hq, hkv, d)
    with pytest.raises(ValueError):
        w.run(dq, dk, dv, out=torch.empty(M + 1, hq, d, dtype=dtype, device=DEV))
    with pytest.raises(ValueError):
        w.run(dq, dk, dv, lse=torch.empty(M, hq + 1, dtype=torch.float32, device=DEV), return_lse=True)
    with pytest.raises(ValueError):
        w.run(dq[:-1], dk, dv)

    vw = flashinfer.VariableBlockSparseAttentionWrapper(_ws())
    vq, vk, vv, block_map, row_sz, col_sz = _variable_case()
    with pytest.raises(RuntimeError, match="plan"):
        vw.run(vq.to(DEV), vk.to(DEV), vv.to(DEV))
    uneven = col_sz.clone()
    uneven[1, 0] += 1
    with pytest.raises(ValueError, match="sum"):
        vw.plan(block_map.to(DEV), row_sz.to(DEV), uneven.to(DEV), 4, 2, 128)
    with pytest.raises(ValueError, match="block_mask_map"):
        vw.plan(block_map[:, :, :-1].to(DEV), row_sz.to(DEV), col_sz.to(DEV), 4, 2, 128)
    vw.plan(block_map.to(DEV), row_sz.to(DEV), col_sz.to(DEV), 4, 2, 128)
    with pytest.raises(ValueError, match="out"):
        vw.run(vq.to(DEV), vk.to(DEV), vv.to(DEV), out=torch.empty(4, 299, 128, dtype=F16, device=DEV))
    with pytest.raises(ValueError, match="lse"):
        vw.run(vq.to(DEV), vk.to(DEV), vv.to(DEV), lse=torch.empty(300, 4, dtype=torch.float32, device=DEV),
               return_lse=True)
