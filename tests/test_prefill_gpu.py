"""GPU parity: MFMA prefill kernels (through the C ABI) against the CPU oracle.  Grid modelled on the
reference's tests/attention/test_batch_prefill_kernels.py:228-279, test_single_prefill.py:56-100,
test_fp8_prefill.py:23-191 and test_hopper_fp8_attention.py:64-108."""
import pytest
import torch

from attn_inputs import indptr_of, make_paged, page_table, planned_prefill_wrapper, ptol, scatter_to_pages
from flashinfer import _lib
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def run_batch_prefill(q, qo_lens, cache, layout, indptr, indices, last, hq, hkv, d, ps, **plan_kw):
    qo_indptr = indptr_of(qo_lens)
    w = planned_prefill_wrapper(32 << 20, layout, qo_indptr, indptr, indices, last, hq, hkv, d, ps,
                                q_data_type=q.dtype, kv_data_type=cache.dtype, **plan_kw)
    o, lse = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    return o, lse, qo_indptr


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2), (28, 4)])
@pytest.mark.parametrize("d,ps,layout", [(128, 16, "NHD"), (128, 1, "HND"), (64, 8, "NHD")])
def test_batch_prefill_matches_oracle(dtype, causal, hq, hkv, d, ps, layout):
    kv_lens = [54, 300, 1, 129, 17]
    qo_lens = [37, 300, 1, 17, 0]  # append (qo < kv), full prefill, single row, empty request
    torch.manual_seed(1)
    cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, ps, hkv, d, dtype, layout, seed=21)
    q = torch.randn(sum(qo_lens), hq, d).to(dtype)
    o, lse, qo_indptr = run_batch_prefill(q, qo_lens, cache, layout, indptr, indices, last, hq, hkv, d, ps,
                                          causal=causal)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), layout, indptr, indices, last,
                                         causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("qo_len,kv_len", [(1, 1), (15, 127), (128, 128), (129, 257), (513, 700), (1000, 1000)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
def test_single_prefill_matches_oracle(qo_len, kv_len, causal, layout):
    # ref: tests/attention/test_single_prefill.py (seed 0)
    import flashinfer

    torch.manual_seed(0)
    hq, hkv, d = 8, 2, 128
    q = torch.randn(qo_len, hq, d).half()
    shape = (kv_len, hkv, d) if layout == "NHD" else (hkv, kv_len, d)
    k, v = torch.randn(shape).half(), torch.randn(shape).half()
    o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal,
                                                     kv_layout=layout, return_lse=True)
    kk, vv = (k, v) if layout == "NHD" else (k.transpose(0, 1), v.transpose(0, 1))
    o_ref, lse_ref = R.attention_ref(q.float(), kk.float(), vv.float(), causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("kw", [dict(pos_encoding_mode="ROPE_LLAMA"), dict(pos_encoding_mode="ALIBI"),
                                dict(logits_soft_cap=20.0), dict(window_left=33), dict(sm_scale=0.05)])
def test_single_prefill_variants(kw):
    import flashinfer

    torch.manual_seed(4)
    qo_len, kv_len, hq, hkv, d = 150, 333, 8, 4, 128
    q = torch.randn(qo_len, hq, d).half()
    k, v = torch.randn(kv_len, hkv, d).half(), torch.randn(kv_len, hkv, d).half()
    o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=True,
                                                     return_lse=True, **kw)
    # fused RoPE rounds the rotated q/k to fp16 before QK^T as the reference does (prefill.cuh:465-612); the
    # oracle models that rounding, the kernel's sin / cos may still flip the rounding of single elements
    rope = kw.get("pos_encoding_mode") == "ROPE_LLAMA"
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), causal=True,
                                     rope_round_dtype=torch.float16 if rope else None, **kw)
    t = 2e-3 if rope else 1e-3
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=t, atol=t)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=t, atol=5 * t)


@pytest.mark.parametrize("kv_dtype", [torch.float8_e4m3fn, torch.float8_e5m2])
def test_batch_prefill_fp8_kv_cache(kv_dtype):
    # fp16 queries over an fp8 cache (ref: tests/attention/test_fp8_prefill.py:23-114); the oracle sees the
    # same quantised cache, so the 16-bit tolerance applies.
    hq, hkv, d, ps = 8, 2, 128, 16
    kv_lens, qo_lens = [200, 77], [64, 77]
    cache, indptr, indices, last = make_paged(2, kv_lens, ps, hkv, d, kv_dtype, "NHD", seed=8)
    q = torch.randn(sum(qo_lens), hq, d).half()
    o, lse, qo_indptr = run_batch_prefill(q, qo_lens, cache, "NHD", indptr, indices, last, hq, hkv, d, ps,
                                          causal=True)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last,
                                         causal=True)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("seq_len", [117, 509])
@pytest.mark.parametrize("d", [128, 64, 256])
def test_single_prefill_fp8_qkv(causal, seq_len, d):
    """fp8 q/k/v with per-head scales.  Two bars: (1) against the oracle that restates the reference's
    fp8 arithmetic (P rounded to e4m3, 3-bit significand) -- rtol = atol = 5e-2: the e4m3 rounding of P is
    taken relative to the RUNNING row maximum of the online softmax (in the reference too, with its own
    128-wide tiles, mainloop_mma.cuh:110-129), so it is tile-order dependent at the 2^-4 level and cannot
    be reproduced bit for bit by an untiled oracle; (2) the reference's own bar, MSE < 1.0 against 16-bit
    attention (test_hopper_fp8_attention.py:105-108), tightened here to 1e-3."""
    import flashinfer

    torch.manual_seed(2)
    h = 8
    q, k, v = (torch.randn(seq_len, h, d).half() for _ in range(3))
    q8, sq = R.per_head_symmetric_quant(q)
    k8, sk = R.per_head_symmetric_quant(k)
    v8, sv = R.per_head_symmetric_quant(v)
    o = flashinfer.single_prefill_with_kv_cache(q8.to(DEV), k8.to(DEV), v8.to(DEV), sq.to(DEV), sk.to(DEV),
                                                sv.to(DEV), causal=causal, o_dtype=torch.float16)
    o_ref8, _ = R.fp8_attention_ref(q8, k8, v8, sq, sk, sv, causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref8.float(), rtol=5e-2, atol=5e-2)
    o_16, _ = R.attention_ref(q.float(), k.float(), v.float(), causal=causal)
    assert torch.mean((o.float().cpu() - o_16.float()) ** 2) < 1e-3


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("o_dtype", [torch.float16, torch.bfloat16])
def test_single_prefill_fp8_e5m2_qkv(causal, d, o_dtype):
    """e5m2 q/k/v (the reference's second fp8 attention type, tests/attention/test_hopper_fp8_attention.py:70):
    P is scaled by 57344 and rounded to e5m2 -- a 2-bit significand, so the bar against the oracle that restates
    that arithmetic is 1e-1 (one e5m2 ulp of P is 2^-2 relative, tile-order dependent as in the e4m3 test), plus
    the reference's own bar: MSE < 1.0 against 16-bit attention (tightened to 2e-2)."""
    import flashinfer

    torch.manual_seed(3)
    h, seq_len = 4, 301
    q, k, v = (torch.randn(seq_len, h, d).half() for _ in range(3))
    q8, sq = R.per_head_symmetric_quant(q, torch.float8_e5m2)
    k8, sk = R.per_head_symmetric_quant(k, torch.float8_e5m2)
    v8, sv = R.per_head_symmetric_quant(v, torch.float8_e5m2)
    o = flashinfer.single_prefill_with_kv_cache(q8.to(DEV), k8.to(DEV), v8.to(DEV), sq.to(DEV), sk.to(DEV),
                                                sv.to(DEV), causal=causal, o_dtype=o_dtype)
    assert o.dtype == o_dtype
    o_ref8, _ = R.fp8_attention_ref(q8, k8, v8, sq, sk, sv, causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref8.float(), rtol=1e-1, atol=1e-1)
    o_16, _ = R.attention_ref(q.float(), k.float(), v.float(), causal=causal)
    assert torch.mean((o.float().cpu() - o_16.float()) ** 2) < 2e-2


def test_batch_prefill_fp8_qkv_paged_c3_shape_small():
    """BASELINE config C3 semantics at a reduced size: fp8 e4m3 q and paged kv, causal, GQA 32/8, d128."""
    hq, hkv, d, ps = 32, 8, 128, 16
    kv_lens, qo_lens = [512, 300], [256, 300]
    torch.manual_seed(0)
    kv16 = [torch.randn(l, 2, hkv, d).half() for l in kv_lens]
    q16 = torch.randn(sum(qo_lens), hq, d).half()
    q8, sq = R.per_head_symmetric_quant(q16)
    kcat = torch.cat([x[:, 0] for x in kv16])
    vcat = torch.cat([x[:, 1] for x in kv16])
    k8, sk = R.per_head_symmetric_quant(kcat)
    v8, sv = R.per_head_symmetric_quant(vcat)
    # build the paged cache from the quantised rows (fp8 values are exact in f32)
    indptr, indices, last, total = page_table(kv_lens, ps)
    cache = scatter_to_pages(k8.float(), v8.float(), kv_lens, indptr, indices, ps, total).to(torch.float8_e4m3fn)
    qo_indptr = indptr_of(qo_lens)
    w = planned_prefill_wrapper(32 << 20, "NHD", qo_indptr, indptr, indices, last, hq, hkv, d, ps, causal=True,
                                q_data_type=torch.float8_e4m3fn, kv_data_type=torch.float8_e4m3fn,
                                o_data_type=torch.bfloat16)
    o, lse = w.run(q8.to(DEV), cache.to(DEV), return_lse=True, scale_q=sq.to(DEV), scale_k=sk.to(DEV),
                   scale_v=sv.to(DEV))
    assert o.dtype == torch.bfloat16
    off = 0
    for b in range(2):
        qs = q8[int(qo_indptr[b]):int(qo_indptr[b + 1])]
        o_ref, lse_ref = R.fp8_attention_ref(qs, k8[off:off + kv_lens[b]], v8[off:off + kv_lens[b]], sq, sk, sv,
                                             causal=True)
        got = o[int(qo_indptr[b]):int(qo_indptr[b + 1])].float().cpu()
        torch.testing.assert_close(got, o_ref.float(), rtol=5e-2, atol=5e-2)  # fp8 bar, see test above
        torch.testing.assert_close(lse[int(qo_indptr[b]):int(qo_indptr[b + 1])].cpu(), lse_ref.float(),
                                   rtol=1e-3, atol=2e-3)
        off += kv_lens[b]


def test_prefill_cuda_graph_mode_and_errors():
    import flashinfer

    hq, hkv, d, ps, b = 8, 2, 128, 16, 3
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(
        ws, "NHD", use_cuda_graph=True, qo_indptr_buf=torch.empty(b + 1, dtype=torch.int32, device=DEV),
        paged_kv_indptr_buf=torch.empty(b + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buf=torch.empty(256, dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buf=torch.empty(b, dtype=torch.int32, device=DEV))
    for seed, (kv_lens, qo_lens) in enumerate([([100, 40, 300], [10, 40, 6]), ([5, 500, 64], [5, 16, 35])]):
        cache, indptr, indices, last = make_paged(b, kv_lens, ps, hkv, d, torch.float16, "NHD", seed=seed)
        q = torch.randn(56, hq, d).half()
        qo_indptr = indptr_of(qo_lens)
        w.plan(qo_indptr, indptr, indices, last, hq, hkv, d, ps, causal=True, max_token_per_sequence=64)
        o = w.run(q.to(DEV), cache.to(DEV))
        o_ref, _ = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last, causal=True)
        torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    with pytest.raises(ValueError):
        w.plan(qo_indptr.long(), indptr, indices, last, hq, hkv, d, ps)
    with pytest.raises(ValueError):
        w.plan(qo_indptr, indptr, indices, last, hq, hkv, d, ps, custom_mask=torch.ones(4, dtype=torch.bool))


@pytest.mark.parametrize("f8", [torch.float8_e4m3fn, torch.float8_e5m2])
@pytest.mark.parametrize("d", [128, 64, 256])
def test_fp8_native_kernel_matches_upcast_kernel(f8, d):
    """The fp8-native kernel (MX-scaled MFMA, transposed V image) and the upcast-to-bf16 kernel implement
    the same arithmetic with the same 64-row tiles, so they must agree far tighter than the fp8 bar:
    a sliding window wider than the sequence selects the upcast kernel without changing the result."""
    hq, hkv, ps = 16, 4, 16
    kv_lens, qo_lens = [700, 130], [300, 130]
    torch.manual_seed(3)
    cache16 = [torch.randn(-(-l // ps), 2, ps, hkv, d) for l in kv_lens]
    cache = torch.cat(cache16).to(f8)
    indptr, indices, last, _ = page_table(kv_lens, ps, shuffle=False)
    q8 = torch.randn(sum(qo_lens), hq, d).to(f8)
    qo_indptr = indptr_of(qo_lens)
    sq, sk, sv = torch.rand(hq) + 0.5, torch.rand(hkv) + 0.5, torch.rand(hkv) + 0.5
    outs = []
    for window in (-1, 1 << 30):
        w = planned_prefill_wrapper(32 << 20, "NHD", qo_indptr, indptr, indices, last, hq, hkv, d, ps, causal=True,
                                    window_left=window, q_data_type=f8, kv_data_type=f8, o_data_type=torch.float16)
        outs.append(w.run(q8.to(DEV), cache.to(DEV), return_lse=True, scale_q=sq.to(DEV), scale_k=sk.to(DEV),
                          scale_v=sv.to(DEV)))
    # identical up to e4m3 rounding flips of single probabilities: the native kernel folds the x448 into the
    # exponent (2^(s c - m + log2 448)), the upcast kernel multiplies afterwards, so a probability that sits
    # on a rounding boundary may land on the other side (one 2^-4 relative step of that one term)
    # (second structure of the native kernel: deferred reference exponent, P scaled by 448 / 2^3 .. 448 against
    # the stale maximum -- each probability lands on a slightly different 3-bit grid than with the upcast kernel's
    # x448 against the running maximum; differences at the level of the e4m3 rounding itself, far inside the
    # 5e-2 bar.  The lse comes from the unrounded probabilities and agrees to f32 rounding.)
    # e5m2 (2-bit significand of P): the same statement one octave coarser
    diff = (outs[0][0].float() - outs[1][0].float()).abs()
    if f8 == torch.float8_e4m3fn:
        assert diff.max() < 5e-2 and diff.mean() < 2e-3
    else:
        assert diff.max() < 1e-1 and diff.mean() < 5e-3
    torch.testing.assert_close(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("causal", [False, True])
def test_ragged_kv_prefill_wrapper(layout, causal):
    # ref: BatchPrefillWithRaggedKVCacheWrapper, flashinfer/prefill.py:2255-3007
    import flashinfer

    torch.manual_seed(9)
    hq, hkv, d = 8, 2, 128
    qo_lens, kv_lens = [5, 130, 1, 64], [33, 130, 7, 200]
    q = torch.randn(sum(qo_lens), hq, d).half()
    k = torch.randn(sum(kv_lens), hkv, d).half()
    v = torch.randn(sum(kv_lens), hkv, d).half()
    qo_indptr = indptr_of(qo_lens)
    kv_indptr = indptr_of(kv_lens)
    ws = torch.zeros(16 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, layout)
    w.plan(qo_indptr.to(DEV), kv_indptr.to(DEV), hq, hkv, d, causal=causal)
    kd, vd = (k.to(DEV), v.to(DEV)) if layout == "NHD" else (k.transpose(0, 1).contiguous().to(DEV), v.transpose(0, 1).contiguous().to(DEV))
    o, lse = w.run(q.to(DEV), kd, vd, return_lse=True)
    for b in range(4):
        qs = q[int(qo_indptr[b]):int(qo_indptr[b + 1])].float()
        ks = k[int(kv_indptr[b]):int(kv_indptr[b + 1])].float()
        vs = v[int(kv_indptr[b]):int(kv_indptr[b + 1])].float()
        o_ref, lse_ref = R.attention_ref(qs, ks, vs, causal=causal)
        torch.testing.assert_close(o[int(qo_indptr[b]):int(qo_indptr[b + 1])].float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
        torch.testing.assert_close(lse[int(qo_indptr[b]):int(qo_indptr[b + 1])].cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


# ---- split-KV prefill (ref planner: PrefillSplitQOKVIndptr, scheduler.cuh:495-614) -----------------------
def _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, dtype, causal, seed, layout="NHD", **plan_kw):
    cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, ps, hkv, d, dtype, layout, seed=seed)
    torch.manual_seed(seed + 1)
    q = torch.randn(sum(qo_lens), hq, d).to(dtype)
    qo_indptr = indptr_of(qo_lens)
    w = planned_prefill_wrapper(256 << 20, layout, qo_indptr, indptr, indices, last, hq, hkv, d, ps, causal=causal,
                                q_data_type=dtype, kv_data_type=cache.dtype, **plan_kw)
    o, lse = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    return w, q, cache, qo_indptr, indptr, indices, last, o, lse


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("qo_lens,kv_lens", [([64], [9000]), ([5, 200, 1], [3000, 4097, 130]), ([300], [300])])
def test_batch_prefill_split_kv_matches_oracle_and_unsplit(dtype, causal, qo_lens, kv_lens):
    hq, hkv, d, ps = 8, 2, 128, 16
    w, q, cache, qo_indptr, indptr, indices, last, o, lse = _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, dtype,
                                                                      causal, seed=50)
    # few q tiles x 2 kv heads cannot fill 256 CUs: the planner must have split long kv
    if max(kv_lens) >= 3000:
        assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_PP_KV_CHUNK_SIZE] % 64 == 0
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last,
                                         causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    # disable_split_kv (batch-invariant mode) and a fixed split size give the same answer
    for kw in (dict(disable_split_kv=True), dict(fixed_split_size=512)):
        w2, *_, o2, lse2 = _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, dtype, causal, seed=50, **kw)
        assert w2._plan_info[_lib.FI_PP_SPLIT_KV] == (0 if "disable_split_kv" in kw else int(max(kv_lens) > 512))
        # against the ORACLE at the same bar (two bf16 outputs rounded from nearly equal f32 values may differ by a
        # whole ulp from each other, 2^-8 ... 2^-7 relative, while each is within half an ulp of the oracle)
        torch.testing.assert_close(o2.float().cpu(), o_ref.float(), **ptol(dtype))
        torch.testing.assert_close(lse2, lse, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_batch_prefill_mixed_batch_balance_rule_and_idle_waves(dtype):
    """A mixed batch in the shape of the reference's bench_batch_attention.py hybrids, scaled down: 132 decode-like
    requests (one query token = 7 of a tile's 128 packed rows: three of the four waves have no row and only help
    staging) + 4 long requests of 17 query tokens + one prompt of 300 tokens (wide tiles, interleaved with the narrow
    ones in the work list).  137+ q tiles exceed the resident-workgroup budget, so the reference rule leaves every
    request whole; the balance rule must cut the long ones.  Result against the oracle, and equal to the unsplit plan."""
    hq, hkv, d, ps = 28, 4, 128, 16
    kv_lens = [200 + 3 * i for i in range(132)] + [5000, 4321, 4097, 3500] + [700]
    qo_lens = [1] * 132 + [17] * 4 + [300]
    w, q, cache, qo_indptr, indptr, indices, last, o, lse = _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, dtype, True, seed=77)
    assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_PP_KV_CHUNK_SIZE] < 4097
    assert w._plan_info[_lib.FI_PP_NUM_WORK] > 132 + 4 + 17  # split, extra items
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last, causal=True)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    w2, *_, o2, lse2 = _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, dtype, True, seed=77, disable_split_kv=True)
    assert w2._plan_info[_lib.FI_PP_SPLIT_KV] == 0
    torch.testing.assert_close(o2.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse2, lse, rtol=1e-3, atol=1e-3)


def test_batch_prefill_split_kv_fp8_native_and_rows_without_keys():
    # fp8 attention through the split path against the unsplit run
    hq, hkv, d, ps = 8, 2, 128, 16
    qo_lens, kv_lens = [100], [8192]
    w, q, cache, qo_indptr, indptr, indices, last, o, lse = _plan_run(
        qo_lens, kv_lens, hq, hkv, d, ps, torch.float8_e4m3fn, True, seed=60, o_data_type=torch.bfloat16)
    assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 1
    w2, *_, o2, lse2 = _plan_run(qo_lens, kv_lens, hq, hkv, d, ps, torch.float8_e4m3fn, True, seed=60,
                                 o_data_type=torch.bfloat16, disable_split_kv=True)
    assert w2._plan_info[_lib.FI_PP_SPLIT_KV] == 0
    torch.testing.assert_close(o.float(), o2.float(), rtol=5e-2, atol=5e-2)
    torch.testing.assert_close(lse, lse2, rtol=1e-2, atol=1e-2)
    # causal with qo_len > kv_len: the first rows see no key in any chunk -> o = 0, lse = -5e4 exactly
    qo_lens, kv_lens = [700], [600]
    w, q, cache, qo_indptr, indptr, indices, last, o, lse = _plan_run(qo_lens, kv_lens, 4, 1, 128, 16,
                                                                      torch.float16, True, seed=61,
                                                                      fixed_split_size=128)
    assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 1
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last,
                                         causal=True)
    assert torch.all(o[:100] == 0) and torch.all(lse[:100].cpu() == R.NEG_INF_SENTINEL)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    # the same rows through the unsplit kernel
    w, *_, o, lse = _plan_run(qo_lens, kv_lens, 4, 1, 128, 16, torch.float16, True, seed=61, disable_split_kv=True)
    assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 0
    assert torch.all(o[:100] == 0) and torch.all(lse[:100].cpu() == R.NEG_INF_SENTINEL)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
def test_prefill_head_dim_256(dtype, causal):
    """head_dim 256 (ref: HEAD_DIM dispatch utils.cuh:175-202; e.g. gemma-style heads) -- batch + single."""
    import flashinfer

    hq, hkv, d, ps = 4, 2, 256, 16
    kv_lens, qo_lens = [130, 700, 1], [70, 256, 1]
    torch.manual_seed(77)
    cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, ps, hkv, d, dtype, "NHD", seed=78)
    q = torch.randn(sum(qo_lens), hq, d).to(dtype)
    o, lse, qo_indptr = run_batch_prefill(q, qo_lens, cache, "NHD", indptr, indices, last, hq, hkv, d, ps,
                                          causal=causal)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last,
                                         causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    k, v = torch.randn(300, hkv, d).to(dtype), torch.randn(300, hkv, d).to(dtype)
    qs = torch.randn(200, hq, d).to(dtype)
    os_, lses = flashinfer.single_prefill_with_kv_cache(qs.to(DEV), k.to(DEV), v.to(DEV), causal=causal,
                                                        pos_encoding_mode="ROPE_LLAMA", return_lse=True)
    os_ref, lses_ref = R.attention_ref(qs.float(), k.float(), v.float(), causal=causal, pos_encoding_mode="ROPE_LLAMA",
                                       rope_round_dtype=dtype)
    torch.testing.assert_close(os_.float().cpu(), os_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lses.cpu(), lses_ref.float(), rtol=2e-3, atol=2e-3)


def test_prefill_run_is_graph_capturable_and_replays_after_replan():
    """run() only launches kernels on the current stream: capture it once in a HIP graph, then replay after
    plan() rewrote the work list for other lengths (fixed-shape graph-mode plan; ref: prefill.py:1838-1857)."""
    import flashinfer

    hq, hkv, d, ps, b = 8, 2, 128, 16, 2
    rows = 96
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(
        ws, "NHD", use_cuda_graph=True, qo_indptr_buf=torch.zeros(b + 1, dtype=torch.int32, device=DEV),
        paged_kv_indptr_buf=torch.zeros(b + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buf=torch.zeros(512, dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buf=torch.zeros(b, dtype=torch.int32, device=DEV))
    cases = [([1000, 300], [40, 56]), ([70, 2000], [90, 6])]
    data = []
    for seed, (kv_lens, qo_lens) in enumerate(cases):
        cache, indptr, indices, last = make_paged(b, kv_lens, ps, hkv, d, torch.float16, "NHD", seed=70 + seed,
                                                  extra_pages=200 - sum(-(-l // ps) for l in kv_lens))
        data.append((cache, indptr, indices, last, qo_lens))
    n_pages = data[0][0].shape[0]
    assert all(x[0].shape[0] == n_pages for x in data)
    cache_dev = torch.empty_like(data[0][0], device=DEV)
    q_dev = torch.zeros(rows, hq, d, dtype=torch.float16, device=DEV)
    out = torch.zeros_like(q_dev)

    def plan(i):
        cache, indptr, indices, last, qo_lens = data[i]
        qo_indptr = indptr_of(qo_lens)
        w.plan(qo_indptr, indptr, indices, last, hq, hkv, d, ps, causal=True, max_token_per_sequence=rows // b)
        cache_dev.copy_(cache)
        torch.manual_seed(i)
        q = torch.randn(rows, hq, d).half()
        q_dev.copy_(q)
        return q, qo_indptr

    q, qo_indptr = plan(0)
    w.run(q_dev, cache_dev, out=out)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.run(q_dev, cache_dev, out=out)
    for i in (0, 1, 0):
        q, qo_indptr = plan(i)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cache, indptr, indices, last, qo_lens = data[i]
        n = sum(qo_lens)
        o_ref, _ = R.batch_prefill_ref(q[:n].float(), qo_indptr, cache.float(), "NHD", indptr, indices, last, causal=True)
        torch.testing.assert_close(out[:n].float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("qo_len,kv_len", [(1, 20000), (100, 9000), (130, 131)])
def test_single_prefill_splits_long_kv(causal, qo_len, kv_len):
    """A few query rows on a long context: the single-request entry point splits the kv axis itself
    (scratch from the cached buffer) and merges; window and fp8 variants ride the same path."""
    import flashinfer

    hq, hkv, d = 8, 2, 128
    torch.manual_seed(qo_len)
    q = torch.randn(qo_len, hq, d).half()
    k, v = torch.randn(kv_len, hkv, d).half(), torch.randn(kv_len, hkv, d).half()
    o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_lse=True)
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), causal=causal)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    o = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, window_left=3000)
    o_ref, _ = R.attention_ref(q.float(), k.float(), v.float(), causal=causal, window_left=3000)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)
    mask = torch.rand(qo_len, kv_len) < 0.5
    mask[:, 0] = True
    o = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), custom_mask=mask.to(DEV))
    o_ref, _ = R.attention_ref(q.float(), k.float(), v.float(), custom_mask=mask)
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), rtol=1e-3, atol=1e-3)


def _peaked_fp8_case(f8, d, kv_len, qo_len, tail_lo, tail_hi, peak, seed):
    """q rows close to one +-1 vector u, keys = g_j u / sqrt(d): the logit of key j is ~g_j nats for every query.
    One key (visible to every query under the causal mask) sits at `peak`, the others uniformly in
    [tail_lo, tail_hi]; the values of the tail have mean +1, the peak key's value is -2, so lost tail mass moves
    every output element the same way."""
    g = torch.Generator().manual_seed(seed)
    h = 2
    u = (torch.randint(0, 2, (d,), generator=g) * 2 - 1).float()
    q = u[None, None, :] + 0.05 * torch.randn(qo_len, h, d, generator=g)
    gj = tail_lo + (tail_hi - tail_lo) * torch.rand(kv_len, h, generator=g)
    jstar = int(torch.randint(0, kv_len - qo_len, (1,), generator=g))
    gj[jstar] = peak
    k = gj[:, :, None] * u[None, None, :] / d ** 0.5
    v = torch.randn(kv_len, h, d, generator=g) * 0.5 + 1.0
    v[jstar] = -2.0
    return q.to(f8), k.to(f8), v.to(f8), jstar


@pytest.mark.parametrize("f8", [torch.float8_e4m3fn, torch.float8_e5m2])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_fp8_prefill_peaked_rows(f8, d):
    """Long, peaked rows: one key at +12 nats, 8191 keys at -2..0 nats.  The tail terms are
    e^-12..e^-14 of the row maximum, i.e. at the bottom of the e4m3 range of P (the reference scales P by 448
    against the running maximum, hopper/variants.cuh:72-90: its subnormal step is 4.4e-6 of the maximum; this
    kernel forms P against a deferred reference exponent with 2^3 of headroom, so right after the exponent was set
    its step is up to 8x coarser, prefill_fp8_kernel.h).  What the test pins: (1) the result stays inside the fp8 bar
    against the oracle's restatement of the reference arithmetic, (2) against exact attention on the same fp8
    inputs the error is bounded by the tail mass of the row (2 %), whichever way the tail was rounded, (3) the
    lse, which comes from the unrounded probabilities, is exact to f32."""
    import flashinfer

    kv_len, qo_len = 8192, 64
    q8, k8, v8, _ = _peaked_fp8_case(f8, d, kv_len, qo_len, -2.0, 0.0, 12.0, seed=11)
    one = torch.ones(2)
    o, lse = flashinfer.single_prefill_with_kv_cache(q8.to(DEV), k8.to(DEV), v8.to(DEV), one.to(DEV), one.to(DEV),
                                                     one.to(DEV), causal=True, o_dtype=torch.float16,
                                                     return_lse=True)
    o = o.float().cpu()
    o_ref8, lse_ref = R.fp8_attention_ref(q8, k8, v8, one, one, one, causal=True)
    o_16, _ = R.attention_ref(q8.float(), k8.float(), v8.float(), causal=True)
    err8 = (o - o_ref8.float()).abs().max().item()
    err16 = (o - o_16.float()).abs().max().item()
    ref_err16 = (o_ref8.float() - o_16.float()).abs().max().item()
    print(f"peaked rows {f8} d={d}: |o - fp8 oracle| {err8:.4f}  |o - exact| {err16:.4f}  "
          f"(fp8 oracle vs exact {ref_err16:.4f})")
    bar = 5e-2 if f8 == torch.float8_e4m3fn else 1e-1
    assert err8 < bar
    # exact attention: o = (-2 + eps * ~1) / (1 + eps) with eps = tail mass / peak mass ~ 0.02; all of the tail lost
    # costs 3 eps ~ 0.066 at most (the e5m2 grid of P is one octave coarser at the same exponent range)
    assert err16 < 0.07
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-4, atol=1e-3)


def _bf16_single(q, k, v, **kw):
    import flashinfer

    return flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, return_lse=True, **kw)


@pytest.mark.parametrize("case", ["v_1e-5", "v_1e-6", "logit_spread_20_nats"])
def test_bf16_prefill_f16_pv_mode_small_values_and_wide_logit_spread(case):
    """the default bf16 path runs P.V on the f16 MFMA (P rounded to f16, V converted bf16 -> f16
    while staged).  What could go wrong there and what the kernel does about it:
      * P below 6e-5 would sit in f16's subnormal range -- P is formed 2^9 up (the row sum carries the same factor),
        so a 20-nat logit spread (terms down to e^-20 = 2e-9 of the row maximum) keeps its small terms;
      * |v| < 6.1e-5 lands in f16 subnormals while it is converted (round to nearest even, v_cvt_pk_f16_f32): the
        relative error grows from 2^-11 at 6e-5 to ~3 % at 1e-6 -- unbiased, so the attention AVERAGE stays far
        closer; the test states what is measured, with RELATIVE tolerances, against the exact oracle and against the
        hi + lo mode (`bf16_pv_exact_range=True`), which has no such limit."""
    torch.manual_seed(12)
    h, d, qo_len, kv_len = 4, 128, 96, 700
    q = torch.randn(qo_len, h, d)
    k = torch.randn(kv_len, h, d)
    v = torch.randn(kv_len, h, d)
    if case == "v_1e-5":
        v = v * 1e-5
    elif case == "v_1e-6":
        v = v * 1e-6
    else:
        q = q * 2.6  # logits q.k / sqrt(d) ~ N(0, 2.6^2): the row maximum sits ~ 8 sigma = 20 nats over the typical term
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    o, lse = _bf16_single(q, k, v)
    o_x, lse_x = _bf16_single(q, k, v, bf16_pv_exact_range=True)
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), causal=True)
    scale = o_ref.abs().max().item()
    err = (o.float().cpu() - o_ref.float()).abs().max().item() / scale
    err_x = (o_x.float().cpu() - o_ref.float()).abs().max().item() / scale
    print(f"bf16 f16-P.V mode, {case}: max |o - ref| / max |ref| = {err:.2e}  (hi + lo mode {err_x:.2e})")
    assert torch.isfinite(o.float()).all()
    # bf16 output rounding alone is 2^-9 = 2e-3 relative to the element; relative to the row scale:
    assert err_x < 6e-3
    assert err < (3e-2 if case == "v_1e-6" else 6e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse_x.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


def test_bf16_prefill_values_beyond_f16_range_need_the_exact_range_option():
    """|v| up to 1e5 (bf16 holds it, f16 does not): with `bf16_pv_exact_range=True` (wrapper plan() / single prefill
    keyword; C ABI fi_batch_prefill_params_t.bf16_pv_mode = 1) the kernel keeps V in bf16 and the result meets the
    usual bar; the default f16 P.V mode turns |v| >= 65520 into infinities -- visibly, not a silent clamp (pinned
    here so that a change of that behaviour is a decision, not an accident; documented in INTEGRATION.md)."""
    import flashinfer

    torch.manual_seed(13)
    hq, hkv, d, ps = 8, 2, 128, 16
    kv_lens, qo_lens = [300, 77], [64, 77]
    cache, indptr, indices, last = make_paged(2, kv_lens, ps, hkv, d, torch.bfloat16, "NHD", seed=14)
    cache = cache.float()
    cache[:, 1] *= 3.0e4  # V ~ N(0, 3e4^2): |v| reaches ~1.2e5
    cache = cache.bfloat16()
    q = torch.randn(sum(qo_lens), hq, d).bfloat16()
    o, lse, qo_indptr = run_batch_prefill(q, qo_lens, cache, "NHD", indptr, indices, last, hq, hkv, d, ps, causal=True,
                                          bf16_pv_exact_range=True)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last, causal=True)
    scale = o_ref.abs().max().item()
    assert (o.float().cpu() - o_ref.float()).abs().max().item() / scale < 6e-3
    torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)
    o_def, _, _ = run_batch_prefill(q, qo_lens, cache, "NHD", indptr, indices, last, hq, hkv, d, ps, causal=True)
    assert not torch.isfinite(o_def.float()).all()
