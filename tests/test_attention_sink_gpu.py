"""GPU: attention sinks (per-head softmax sink) in batch decode and batch prefill.

The oracle is tests/sink_ref.py (the attention oracle, then a merge with (0, sink log2 e)), held to the reference's own
statement by tests/test_attention_sink_cpu.py.  Tolerances are the decode bar ``tol(dtype)`` on o and 1e-3 on the
lse: the sink is folded where the kernels normalise a row, so it adds no rounding of its own.  Sinks are distinct per
head (linspace(-4, 6)) so that a head mix-up shows; one head is -inf (sink off) and one +60 (the sink takes nearly
all of the mass: o ~ 0, lse ~ 60 log2 e).

Decode: one case per kernel on one launch; split plans (the FUSE form, a ragged split with the fold in the merge
launch, windowed plans) against the oracle and against the unsplit run; an fp8 cache.  Prefill: paged and ragged,
causal or not, with and without a window, unsplit and split; bf16 runs its default P.V mode, whose row sum carries a
factor 2^9 that the sink term has to carry too.  Then bit-for-bit identity of sinks = -inf with no sinks, a captured
decode run whose sink tensor is rewritten between replays, and the refusals."""
import functools
import math

import pytest
import torch

import sink_ref as S
from attn_inputs import indptr_of, page_table, planned_decode_wrapper, planned_prefill_wrapper, scatter_to_pages, tol
from flashinfer import _lib
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_BYTES = 16 << 20
DTYPES = [torch.float16, torch.bfloat16]


def make_sinks(hq):
    s = torch.linspace(-4.0, 6.0, hq)
    s[1] = float("-inf")
    s[hq - 2] = 60.0
    return s


@functools.lru_cache(maxsize=None)
def decode_case(kv_lens, hq, hkv, d, page, dtype, kv_dtype=None, window_left=-1, seed=0):
    """Seeded inputs and the oracle's answer with sinks, computed once per case and never modified."""
    g = torch.Generator().manual_seed(4000 + seed)
    indptr, indices, last, npages = page_table(kv_lens, page, g, extra_pages=3)
    cache = torch.randn(npages, 2, page, hkv, d, generator=g).to(kv_dtype or dtype)
    q = torch.randn(len(kv_lens), hq, d, generator=g).to(dtype)
    sinks = make_sinks(hq)
    o_ref, lse_ref = S.batch_decode_sink_ref(q.float(), cache.float(), "NHD", indptr, indices, last, sinks,
                                             window_left=window_left)
    return q, cache, indptr, indices, last, sinks, o_ref.float(), lse_ref.float()


def decode_wrapper(c, hq, hkv, d, page, **plan_kw):
    q, cache, indptr, indices, last = c[:5]
    return planned_decode_wrapper(WS_BYTES, "NHD", indptr, indices, last, hq, hkv, d, page, q_data_type=q.dtype,
                                  kv_data_type=cache.dtype, **plan_kw)


def check_decode(c, o, lse, dtype):
    o_ref, lse_ref = c[6], c[7]
    torch.testing.assert_close(o.float().cpu(), o_ref, **tol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref, rtol=1e-3, atol=1e-3)


# ---- decode, one launch: one case per kernel ---------------------------------------------------------------------
ONE_LAUNCH = [(8, 2, 64, 16), (8, 2, 128, 16),  # 16x16x32 matrix-core kernel
              (64, 2, 128, 5),                  # 32x32x16 matrix-core kernel (32 heads per kv head)
              (12, 4, 256, 8),                  # VALU kernel, one 4-head tile per kv head
              (16, 2, 256, 8)]                  # VALU kernel, two head tiles per kv head: a tile past the first finds
                                                # its heads' sinks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hkv,d,page", ONE_LAUNCH)
def test_decode_one_launch(hq, hkv, d, page, dtype):
    c = decode_case((54, 97, 1, 0, 513), hq, hkv, d, page, dtype, seed=1)
    w = decode_wrapper(c, hq, hkv, d, page, disable_split_kv=True)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 0
    o, lse = w.run(c[0].to(DEV), c[1].to(DEV), sinks=c[5].to(DEV), return_lse=True)
    check_decode(c, o, lse, dtype)
    # the empty request: o = 0 and lse = sink log2 e, or FI_NEG_INF for the head whose sink is off
    assert torch.all(o[3] == 0)
    want = torch.where(torch.isinf(c[5]), torch.tensor(R.NEG_INF_SENTINEL), c[5] * S.LOG2E)
    torch.testing.assert_close(lse[3].cpu(), want.float(), rtol=1e-6, atol=1e-5)
    # run_return_lse and use_tensor_cores funnel into the same run()
    o2, lse2 = w.run_return_lse(c[0].to(DEV), c[1].to(DEV), sinks=c[5].to(DEV))
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


# ---- decode, split plans -------------------------------------------------------------------------------------------
def run_split_and_unsplit(kv_lens, dtype, window_left=-1, d=128, seed=2):
    c = decode_case(kv_lens, 8, 2, d, 16, dtype, window_left=window_left, seed=seed)
    q, cache, sinks = c[0].to(DEV), c[1].to(DEV), c[5].to(DEV)
    w = decode_wrapper(c, 8, 2, d, 16, window_left=window_left)
    w._float_workspace_buffer.fill_(0xFF)
    o, lse = w.run(q, cache, sinks=sinks, return_lse=True)
    torch.cuda.synchronize()
    untouched = bool((w._float_workspace_buffer == 0xFF).all())
    check_decode(c, o, lse, dtype)
    w1 = decode_wrapper(c, 8, 2, d, 16, window_left=window_left, disable_split_kv=True)
    assert w1._plan_info[_lib.FI_DP_SPLIT_KV] == 0
    o1, lse1 = w1.run(q, cache, sinks=sinks, return_lse=True)
    check_decode(c, o1, lse1, dtype)
    # a sink folded once per chunk instead of once per row fails here (and above)
    torch.testing.assert_close(o.float(), o1.float(), **tol(dtype))
    torch.testing.assert_close(lse, lse1, rtol=1e-3, atol=1e-3)
    return w, untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_uniform_two_chunks_fold_in_the_fused_launch(dtype):
    w, untouched = run_split_and_unsplit((130, 200, 256), dtype)
    assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 2 and _lib.FI_DP_UNIFORM_CHUNKS == 16
    assert untouched, "the fused launch writes no partial states, with sinks as without"


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_ragged_split_folds_in_the_merge_launch(dtype):
    w, untouched = run_split_and_unsplit((130, 700), dtype)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 0 and not untouched


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_window_64(dtype):
    # the window leaves every request 5 pages, under the planner's smallest chunk: this windowed plan is not split
    w, _ = run_split_and_unsplit((130, 200, 256), dtype, window_left=64)
    assert w._plan_info[_lib.FI_DP_WINDOW_LEFT] == 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_windowed_split_plan(dtype):
    # a window wide enough to be cut into chunks: two launches (a windowed plan has no fused form)
    w, untouched = run_split_and_unsplit((600, 700, 800), dtype, window_left=300, seed=3)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_DP_WINDOW_LEFT] == 300
    assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 0 and not untouched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split", [False, True])
def test_decode_fp8_e4m3_cache(dtype, split):
    # the oracle sees the same (already quantised) cache values, so the 16-bit bars apply
    # (tests/test_decode_gpu.py::test_batch_decode_wide_groups_fp8_cache)
    kv_lens = (130, 200, 256) if split else (54, 97, 1, 0, 513)
    c = decode_case(kv_lens, 8, 2, 128, 16, dtype, kv_dtype=torch.float8_e4m3fn, seed=4)
    w = decode_wrapper(c, 8, 2, 128, 16, disable_split_kv=not split)
    assert bool(w._plan_info[_lib.FI_DP_SPLIT_KV]) == split
    o, lse = w.run(c[0].to(DEV), c[1].to(DEV), sinks=c[5].to(DEV), return_lse=True)
    check_decode(c, o, lse, dtype)


# ---- prefill ---------------------------------------------------------------------------------------------------------
QO_KV = ((1, 37), (17, 17), (64, 300), (5, 0))
PAGE = 16


@functools.lru_cache(maxsize=None)
def prefill_case(d, dtype, causal, window_left, page=PAGE, seed=0):
    """Ragged K / V and the same rows scattered over a shuffled page table, with the oracle's answer."""
    hq, hkv = 8, 2
    g = torch.Generator().manual_seed(5000 + seed)
    qo_lens, kv_lens = [a for a, _ in QO_KV], [b for _, b in QO_KV]
    qo_indptr = indptr_of(qo_lens)
    kv_indptr = indptr_of(kv_lens)
    q = torch.randn(sum(qo_lens), hq, d, generator=g).to(dtype)
    k = torch.randn(sum(kv_lens), hkv, d, generator=g).to(dtype)
    v = torch.randn(sum(kv_lens), hkv, d, generator=g).to(dtype)
    indptr, indices, last, npages = page_table(kv_lens, page, g, extra_pages=3)
    cache = scatter_to_pages(k, v, kv_lens, indptr, indices, page, npages)
    sinks = make_sinks(hq)
    o_ref, lse_ref = S.batch_prefill_sink_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last, sinks,
                                              causal=causal, window_left=window_left)
    return dict(q=q, k=k, v=v, cache=cache, qo_indptr=qo_indptr, kv_indptr=kv_indptr, indptr=indptr, indices=indices,
                last=last, sinks=sinks, o_ref=o_ref.float(), lse_ref=lse_ref.float(), hq=hq, hkv=hkv, d=d)


def check_prefill(c, o, lse, dtype):
    torch.testing.assert_close(o.float().cpu(), c["o_ref"], **tol(dtype))
    torch.testing.assert_close(lse.cpu(), c["lse_ref"], rtol=1e-3, atol=1e-3)


def run_paged_prefill(c, dtype, causal, window_left, sinks, **plan_kw):
    w = planned_prefill_wrapper(WS_BYTES, "NHD", c["qo_indptr"], c["indptr"], c["indices"], c["last"], c["hq"], c["hkv"],
                                c["d"], PAGE, causal=causal, window_left=window_left, q_data_type=dtype,
                                kv_data_type=dtype, **plan_kw)
    o, lse = w.run(c["q"].to(DEV), c["cache"].to(DEV), sinks=sinks, return_lse=True)
    return w, o, lse


def sink_jit_args(dtype, d):
    # the list the reference's test builds (tests/attention/test_attention_sink.py:162-176); entry 12 is CUDA text there
    return ("batch_prefill_attention_sink", dtype, dtype, dtype, torch.int32, d, d, ["sink"], ["float"], ["sm_scale"],
            ["double"], "AttentionSink", "")


def run_ragged_prefill(c, dtype, causal, window_left, **plan_kw):
    """The reference's own call form: a ragged wrapper built with jit_args, run(q, k, v, sink, sm_scale)."""
    import flashinfer

    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(
        torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV), kv_layout="NHD", backend="fa2",
        jit_args=sink_jit_args(dtype, c["d"]), jit_kwargs={"use_sliding_window": window_left >= 0})
    w.plan(c["qo_indptr"], c["kv_indptr"], c["hq"], c["hkv"], c["d"], causal=causal, window_left=window_left,
           q_data_type=dtype, kv_data_type=dtype, **plan_kw)
    args = (c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV), c["sinks"].to(DEV), 1.0 / math.sqrt(c["d"]))
    o, lse = w.run_return_lse(*args)
    assert torch.equal(w.run(*args), o)
    return w, o, lse


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window_left", [-1, 16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_prefill_paged_unsplit_and_split(d, causal, window_left, dtype):
    c = prefill_case(d, dtype, causal, window_left)
    w1, o1, lse1 = run_paged_prefill(c, dtype, causal, window_left, c["sinks"].to(DEV), disable_split_kv=True)
    assert w1._plan_info[_lib.FI_PP_SPLIT_KV] == 0
    check_prefill(c, o1, lse1, dtype)
    # rows of the request without keys: o = 0, lse = sink log2 e (FI_NEG_INF where the sink is off)
    empty = slice(int(c["qo_indptr"][3]), int(c["qo_indptr"][4]))
    want = torch.where(torch.isinf(c["sinks"]), torch.tensor(R.NEG_INF_SENTINEL), c["sinks"] * S.LOG2E).float()
    assert torch.all(o1[empty] == 0)
    torch.testing.assert_close(lse1[empty].cpu(), want.expand(5, -1), rtol=1e-6, atol=1e-5)
    # 64-token chunks: partial states without the sink, folded once by the merge launch
    w2, o2, lse2 = run_paged_prefill(c, dtype, causal, window_left, c["sinks"].to(DEV), fixed_split_size=64)
    assert w2._plan_info[_lib.FI_PP_SPLIT_KV] == 1
    check_prefill(c, o2, lse2, dtype)
    torch.testing.assert_close(o2.float(), o1.float(), **tol(dtype))
    torch.testing.assert_close(lse2, lse1, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window_left", [-1, 16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_prefill_ragged_reference_call_form(d, causal, window_left, dtype):
    c = prefill_case(d, dtype, causal, window_left)
    _, o1, lse1 = run_ragged_prefill(c, dtype, causal, window_left, disable_split_kv=True)
    check_prefill(c, o1, lse1, dtype)
    w2, o2, lse2 = run_ragged_prefill(c, dtype, causal, window_left, fixed_split_size=64)
    assert w2._plan_info[_lib.FI_PP_SPLIT_KV] == 1
    check_prefill(c, o2, lse2, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("causal,window_left", [(True, -1), (True, 16), (False, -1)])
def test_attention_sink_wrapper_page_size_1_shuffled_table(causal, window_left, dtype):
    """BatchAttentionWithAttentionSinkWrapper as the reference's test drives it (tests/attention/
    test_attention_sink.py:242-330): page_size 1, (k, v) as 3-D tensors, a fragmented page table,
    run(q, (k, v), sink, sm_scale)."""
    import flashinfer

    d = 128
    c = prefill_case(d, dtype, causal, window_left)
    g = torch.Generator().manual_seed(77)
    total = int(c["kv_indptr"][-1])
    slots = torch.randperm(2 * total, generator=g)[:total]
    k_pool = torch.zeros(2 * total, c["hkv"], d, dtype=dtype)
    v_pool = torch.zeros(2 * total, c["hkv"], d, dtype=dtype)
    k_pool[slots], v_pool[slots] = c["k"], c["v"]
    w = flashinfer.BatchAttentionWithAttentionSinkWrapper(
        torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV), kv_layout="NHD", backend="fa2", q_data_type=dtype,
        kv_data_type=dtype, head_dim_qk=d, head_dim_vo=d, window_left=window_left)
    last = torch.tensor([1 if n > 0 else 0 for _, n in QO_KV], dtype=torch.int32)
    w.plan(c["qo_indptr"], c["kv_indptr"], slots.to(torch.int32), last, c["hq"], c["hkv"], d, 1, causal=causal,
           window_left=window_left, q_data_type=dtype, kv_data_type=dtype, non_blocking=True)
    o = w.run(c["q"].to(DEV), (k_pool.to(DEV), v_pool.to(DEV)), c["sinks"].to(DEV), 1.0 / math.sqrt(d))
    torch.testing.assert_close(o.float().cpu(), c["o_ref"], **tol(dtype))
    with pytest.raises(ValueError, match="sink, sm_scale"):
        w.run(c["q"].to(DEV), (k_pool.to(DEV), v_pool.to(DEV)))


# ---- identity: sinks = -inf is the run without sinks, bit for bit ------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kv_lens,plan_kw,fused", [
    ((130, 200, 256), {}, True),                                  # FUSE form
    ((130, 700), {}, False),                                      # split, two launches
    ((54, 97, 1, 0, 513), {"disable_split_kv": True}, False),     # unsplit
])
def test_decode_minus_inf_sinks_are_no_sinks(kv_lens, plan_kw, fused, dtype):
    c = decode_case(kv_lens, 8, 2, 128, 16, dtype, seed=2 if len(kv_lens) < 5 else 1)
    q, cache = c[0].to(DEV), c[1].to(DEV)
    w = decode_wrapper(c, 8, 2, 128, 16, **plan_kw)
    w._float_workspace_buffer.fill_(0xFF)
    o0, lse0 = w.run(q, cache, return_lse=True)
    torch.cuda.synchronize()
    if fused:
        assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 2
        assert bool((w._float_workspace_buffer == 0xFF).all()), "sinks=None: the fused plan writes no partial states"
    off = torch.full((8,), float("-inf"), device=DEV)
    o1, lse1 = w.run(q, cache, sinks=off, return_lse=True)
    assert torch.equal(o1, o0) and torch.equal(lse1, lse0)
    o_plain, lse_plain = R.batch_decode_ref(c[0].float(), c[1].float(), "NHD", c[2], c[3], c[4])
    torch.testing.assert_close(o0.float().cpu(), o_plain.float(), **tol(dtype))
    torch.testing.assert_close(lse0.cpu(), lse_plain.float(), rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("plan_kw", [{"disable_split_kv": True}, {"fixed_split_size": 64}])
@pytest.mark.parametrize("d", [64, 128])
def test_prefill_minus_inf_sinks_are_no_sinks(d, plan_kw, dtype):
    c = prefill_case(d, dtype, True, -1)
    _, o0, lse0 = run_paged_prefill(c, dtype, True, -1, None, **plan_kw)
    _, o1, lse1 = run_paged_prefill(c, dtype, True, -1, torch.full((8,), float("-inf"), device=DEV), **plan_kw)
    assert torch.equal(o1, o0) and torch.equal(lse1, lse0)


# ---- graph -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_graph_replay_reads_the_sinks_at_replay(dtype):
    import flashinfer

    kv_lens = (130, 200, 256)
    c = decode_case(kv_lens, 8, 2, 128, 16, dtype, seed=2)
    q, cache, indptr, indices, last, sinks = c[:6]
    w = flashinfer.CUDAGraphBatchDecodeWithPagedKVCacheWrapper(
        torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV),
        torch.empty(64, dtype=torch.int32, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV), "NHD")
    w.plan(indptr, indices, last, 8, 2, 128, 16, q_data_type=dtype, kv_data_type=dtype)
    q_dev, cache_dev, s_dev = q.to(DEV), cache.to(DEV), sinks.to(DEV)
    out = torch.empty_like(q_dev)
    lse = torch.empty(3, 8, dtype=torch.float32, device=DEV)
    w.run(q_dev, cache_dev, out=out, lse=lse, return_lse=True, sinks=s_dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.run(q_dev, cache_dev, out=out, lse=lse, return_lse=True, sinks=s_dev)
    for values in (sinks, torch.linspace(3.0, -2.0, 8)):
        s_dev.copy_(values)  # in place: the captured run reads the tensor at replay
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        o_ref, lse_ref = S.batch_decode_sink_ref(q.float(), cache.float(), "NHD", indptr, indices, last, values)
        torch.testing.assert_close(out.float().cpu(), o_ref.float(), **tol(dtype))
        torch.testing.assert_close(lse.cpu(), lse_ref.float(), rtol=1e-3, atol=1e-3)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    import flashinfer

    c = decode_case((54, 97, 1, 0, 513), 8, 2, 128, 16, torch.float16, seed=1)
    q, cache, good = c[0].to(DEV), c[1].to(DEV), c[5].to(DEV)
    w = decode_wrapper(c, 8, 2, 128, 16)
    pc = prefill_case(128, torch.float16, True, -1)

    def prefill_with(sinks):
        run_paged_prefill(pc, torch.float16, True, -1, sinks)

    for bad in (good.bfloat16(), good[:7].contiguous(), torch.zeros(9, device=DEV), good.cpu(),
                torch.zeros(16, device=DEV)[::2], torch.zeros(8, 1, device=DEV)):
        with pytest.raises(ValueError, match="sinks must be"):
            w.run(q, cache, sinks=bad)
        with pytest.raises(ValueError, match="sinks must be"):
            prefill_with(bad)

    # fp8 queries (the paged prefill wrapper is the one that takes them)
    ws = torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)
    f8 = torch.float8_e4m3fn
    wp = flashinfer.BatchPrefillWithPagedKVCacheWrapper(ws, "NHD")
    wp.plan(pc["qo_indptr"].to(DEV), pc["indptr"].to(DEV), pc["indices"].to(DEV), pc["last"].to(DEV), 8, 2, 128, PAGE,
            causal=True, q_data_type=f8, kv_data_type=f8)
    with pytest.raises(ValueError, match="float16 or bfloat16 queries"):
        wp.run(pc["q"].to(DEV).to(f8), pc["cache"].to(DEV).to(f8), sinks=good)

    # head_dim_qk 192 / head_dim_vo 128: a ragged plan in the AttentionSink call form
    wr = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, "NHD", jit_args=sink_jit_args(torch.float16, 192))
    indptr = torch.tensor([0, 8], dtype=torch.int32)
    wr.plan(indptr, indptr, 8, 2, 192, head_dim_vo=128, causal=True, q_data_type=torch.float16)
    q192 = torch.zeros(8, 8, 192, dtype=torch.float16, device=DEV)
    k192 = torch.zeros(8, 2, 192, dtype=torch.float16, device=DEV)
    v128 = torch.zeros(8, 2, 128, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="192 / head_dim_vo 128"):
        wr.run(q192, k192, v128, good, 0.1)

    # any other jit_args is still refused, and the decode wrapper takes none
    with pytest.raises(ValueError, match="jit_args"):
        flashinfer.BatchPrefillWithPagedKVCacheWrapper(ws, "NHD", jit_args=["x"] * 11 + ["FlashSigmoid", ""])
    with pytest.raises(ValueError, match="jit_args"):
        flashinfer.BatchDecodeWithPagedKVCacheWrapper(ws, "NHD", jit_args=list(sink_jit_args(torch.float16, 128)))

    # MLA has no sink term
    wm = flashinfer.BatchMLAPagedAttentionWrapper(ws)
    with pytest.raises(ValueError, match="attention sinks"):
        wm.run(None, None, None, None, sinks=good)
