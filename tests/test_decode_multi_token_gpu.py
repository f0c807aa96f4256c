"""GPU: batch decode with several query tokens per request, ``run(q, cache, q_len_per_req=T)`` (speculative verify),
on the MULTI form of the 16x16x32 matrix-core kernel (csrc/decode_mfma16_kernel.h).

The reference is the repository's float64 attention oracle run as causal attention with ``qo_len = T`` per request:
token t of a request of L keys sees keys j <= L - T + t (and j >= L - T + t - window_left), sinks join the denominator
(tests/sink_ref.py), a token without a key gives o = 0 and the "no key" lse -5e4.  Tolerances are the decode bars of
tests/attn_inputs.py and the 1e-3 lse bar of the decode suite.

The nine kv lengths cover the 32-token tile edges, lengths below T (rows without a key) and, at batch 9 on 256 CUs,
a split plan with unequal chunk counts (300 -> 3 chunks, 700 -> 6 at 128 tokens)."""
import functools

import pytest
import torch

import flashinfer
from attn_inputs import indptr_of, page_table, planned_decode_wrapper, tol
from flashinfer import _lib
from oracle import attention_ref as R
from sink_ref import fold_sink

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_BYTES = 16 << 20
KV_LENS = (1, 3, 31, 32, 33, 64, 65, 300, 700)
BF16, F16, E4M3 = torch.bfloat16, torch.float16, torch.float8_e4m3fn


@functools.lru_cache(maxsize=None)
def case(T, hq, hkv, d, dtype, page, layout="NHD", kv_dtype=None, kv_lens=KV_LENS, sinks=False, q_gain=1.0,
         v_scale=1.0, **ref_kw):
    """Seeded inputs and the oracle's (o, lse), computed once per distinct case and never modified."""
    g = torch.Generator().manual_seed(7 * T + hq + d + page)
    indptr, indices, last, npages = page_table(kv_lens, page, g, extra_pages=3)
    shape = (npages, 2, page, hkv, d) if layout == "NHD" else (npages, 2, hkv, page, d)
    cache = torch.randn(shape, generator=g).to(kv_dtype or dtype)
    q = (torch.randn(len(kv_lens) * T, hq, d, generator=g) * q_gain).to(dtype)
    o, lse = R.batch_prefill_ref(q.float(), indptr_of([T] * len(kv_lens)), cache.float(), layout, indptr, indices, last,
                                 causal=True, **ref_kw)
    s = None
    if sinks:
        s = torch.randn(hq, generator=g)
        s[1] = float("-inf")
        o, lse = fold_sink(o, lse, s)
    return q, cache, indptr, indices, last, s, (o * v_scale).float(), lse.float()


def check(c, w, dtype, T, **run_kw):
    q, cache, _, _, _, s, o_ref, lse_ref = c
    o, lse = w.run(q.to(DEV), cache.to(DEV), return_lse=True, q_len_per_req=T,
                   sinks=None if s is None else s.to(DEV), **run_kw)
    assert o.shape == q.shape and lse.shape == q.shape[:2]
    torch.testing.assert_close(o.float().cpu(), o_ref, **tol(dtype))
    torch.testing.assert_close(lse.cpu(), lse_ref, rtol=1e-3, atol=1e-3)  # -5e4 exactly on rows without a key
    assert (lse_ref == R.NEG_INF_SENTINEL).any()  # KV_LENS holds requests shorter than T


SHAPES = [(2, 8, 2), (4, 8, 2), (5, 6, 2), (3, 8, 1), (8, 8, 1)]  # 16, 16, 15 (ragged), 24 (two tiles), 64 columns
CASES = [pytest.param(*shape, d, dtype, page, "NHD", {}, {}, id=f"T{shape[0]}-{shape[1]}x{shape[2]}-d{d}-p{page}-{n}")
         for shape in SHAPES for d, dtype, page, n in [(128, BF16, 16, "bf16"), (64, F16, 1, "f16"),
                                                       (128, F16, 1, "f16"), (64, BF16, 16, "bf16")]]
CASES += [
    pytest.param(3, 8, 1, 128, F16, 16, "HND", {}, {}, id="hnd"),
    pytest.param(4, 8, 2, 128, F16, 16, "NHD", dict(kv_dtype=E4M3, sm_scale=0.75 / 128 ** 0.5, v_scale=0.5),
                 dict(k_scale=0.75, v_scale=0.5), id="e4m3-scales"),
    pytest.param(4, 8, 2, 128, BF16, 16, "NHD", dict(window_left=40), {}, id="window40"),
    pytest.param(4, 8, 2, 64, F16, 1, "NHD", dict(window_left=40), {}, id="window40-page1"),
    # a window the planner still splits (700 keys: two chunks), cut from the page of the LAST token's first key: at
    # page 1 that is 3 keys past the first key of token 0
    pytest.param(4, 8, 2, 64, F16, 1, "NHD", dict(window_left=200), dict(split_window=True), id="window200-split"),
    pytest.param(4, 8, 2, 128, BF16, 16, "NHD", dict(logits_soft_cap=30.0, q_gain=3.0), {}, id="softcap30"),
    pytest.param(4, 8, 2, 128, F16, 16, "NHD", dict(sinks=True), {}, id="sinks"),
    pytest.param(4, 8, 2, 128, BF16, 16, "NHD", dict(sinks=True), dict(disable_split_kv=True), id="unsplit-sinks"),
    pytest.param(4, 8, 2, 128, BF16, 16, "NHD", {}, dict(disable_split_kv=True), id="unsplit"),
]


@pytest.mark.parametrize("T,hq,hkv,d,dtype,page,layout,case_kw,kw", CASES)
def test_multi_token_decode_matches_the_oracle(T, hq, hkv, d, dtype, page, layout, case_kw, kw):
    c = case(T, hq, hkv, d, dtype, page, layout, **case_kw)
    plan_kw = {k: case_kw[k] for k in ("window_left", "logits_soft_cap") if k in case_kw}
    run_kw = {k: kw[k] for k in ("k_scale", "v_scale") if k in kw}
    w = planned_decode_wrapper(WS_BYTES, layout, *c[2:5], hq, hkv, d, page, q_data_type=dtype,
                               kv_data_type=c[1].dtype, disable_split_kv=kw.get("disable_split_kv", False), **plan_kw)
    if "window_left" not in case_kw or "split_window" in kw:  # (a window of 40 keys leaves one chunk per request)
        assert bool(w._plan_info[_lib.FI_DP_SPLIT_KV]) != kw.get("disable_split_kv", False)
    check(c, w, dtype, T, **run_kw)


def test_graph_wrapper_replays():
    T, hq, hkv, d = 4, 8, 2, 128
    c = case(T, hq, hkv, d, BF16, 16)
    q, cache, indptr, indices, last, _, o_ref, _ = c
    w = flashinfer.CUDAGraphBatchDecodeWithPagedKVCacheWrapper(
        torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV), torch.empty(len(KV_LENS) + 1, dtype=torch.int32, device=DEV),
        torch.empty(256, dtype=torch.int32, device=DEV), torch.empty(len(KV_LENS), dtype=torch.int32, device=DEV), "NHD")
    w.plan(indptr, indices, last, hq, hkv, d, 16, q_data_type=BF16, kv_data_type=BF16)
    check(c, w, BF16, T)  # eager, which also warms the call up
    qd, cd, out = q.to(DEV), cache.to(DEV), torch.empty(q.shape, dtype=BF16, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w.run(qd, cd, out=out, q_len_per_req=T)
    for _ in range(3):
        out.fill_(float("nan"))
        graph.replay()
        torch.testing.assert_close(out.float().cpu(), o_ref, **tol(BF16))


def test_one_token_is_unchanged_and_refusals():
    q, cache, indptr, indices, last = case(1, 8, 1, 128, F16, 16)[:5]
    qd, cd = q.to(DEV), cache.to(DEV)

    def planned(ws=WS_BYTES, **plan_kw):
        return planned_decode_wrapper(ws, "NHD", indptr, indices, last, 8, 1, 128, 16, q_data_type=F16,
                                      kv_data_type=F16, **plan_kw)

    w = planned()
    base = w.run(qd, cd)
    assert torch.equal(w.run(qd, cd, q_len_per_req=1), base) and torch.equal(w.run(qd, cd, q_len_per_req=None), base)
    q4 = torch.cat([qd] * 4)
    for mode in ("ROPE_LLAMA", "ALIBI"):
        with pytest.raises(NotImplementedError, match="q_len_per_req"):
            planned(pos_encoding_mode=mode).run(q4, cd, q_len_per_req=4)
    with pytest.raises(ValueError, match="BatchPrefillWithPagedKVCacheWrapper"):
        w.run(torch.cat([qd] * 9), cd, q_len_per_req=9)  # 9 x 8 = 72 columns
    with pytest.raises(ValueError, match="q must have shape"):
        w.run(q4, cd, q_len_per_req=3)
    small = planned(ws=128 << 10)  # holds the one-token partial states (16 chunks x 8 heads), not 8 times as many
    assert small._plan_info[_lib.FI_DP_SPLIT_KV] == 1
    small.run(qd, cd)
    with pytest.raises(ValueError, match=r"workspace too small.* \d+ bytes needed"):
        small.run(torch.cat([qd] * 8), cd, q_len_per_req=8)
