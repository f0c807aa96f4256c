"""GPU parity: prefill with head_dim_qk 192 / head_dim_vo 128 (DeepSeek-style MLA prefill, non-absorbed form) against
the CPU oracle.  Grid modelled on the reference's tests/attention/test_deepseek_mla.py:151-275 (single and ragged
batch prefill at 192 / 128)."""
import os
import random

import pytest
import torch

from attn_inputs import indptr_of, ptol
from flashinfer import _lib
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DQK, DVO = 192, 128
SEEDS = range(int(os.environ.get("FI_FUZZ_SEEDS", "24")))
LSE_TOL = dict(rtol=1e-3, atol=1e-3)


def _data(qo_lens, kv_lens, hq, hkv, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(sum(qo_lens), hq, DQK, generator=g).to(dtype)
    k = torch.randn(sum(kv_lens), hkv, DQK, generator=g).to(dtype)
    v = torch.randn(sum(kv_lens), hkv, DVO, generator=g).to(dtype)
    return q, k, v


def _ref(q, k, v, qo_lens, kv_lens, causal, kv_heads=None, **kw):
    """float64 oracle per request; kv_heads: the kv heads (with all their q heads) to check, None = all."""
    hq, hkv = q.shape[1], k.shape[1]
    G = hq // hkv
    if kv_heads is not None:
        qh = [h * G + j for h in kv_heads for j in range(G)]
        q, k, v = q[:, qh], k[:, kv_heads], v[:, kv_heads]
    qi, ki = indptr_of(qo_lens), indptr_of(kv_lens)
    outs, lses = [], []
    for b in range(len(qo_lens)):
        o, s = R.attention_ref(q[qi[b]:qi[b + 1]].float(), k[ki[b]:ki[b + 1]].float(), v[ki[b]:ki[b + 1]].float(),
                               causal=causal, **kw)
        outs.append(o)
        lses.append(s)
    return torch.cat(outs), torch.cat(lses)


def _heads(o, hq, hkv, kv_heads):
    if kv_heads is None:
        return o
    G = hq // hkv
    return o[:, [h * G + j for h in kv_heads for j in range(G)]]


def _ragged(qo_lens, kv_lens, hq, hkv, dtype, causal, q, k, v, layout="NHD", ws_mb=128, **plan_kw):
    import flashinfer

    ws = torch.zeros(ws_mb << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, layout)
    w.plan(indptr_of(qo_lens).to(DEV), indptr_of(kv_lens).to(DEV), hq, hkv, DQK, head_dim_vo=DVO, causal=causal,
           q_data_type=dtype, **plan_kw)
    o, lse = w.run(q, k, v, return_lse=True)
    torch.cuda.synchronize()
    return o, lse, w


def _check(o, lse, o_ref, lse_ref, dtype):
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), **ptol(dtype))
    torch.testing.assert_close(lse.float().cpu(), lse_ref.float(), **LSE_TOL)


# The reference's grid (batch {12, 17} x kv {544, 977} x qo {377, 177} x heads {4, 32, 128} x causal x dtype), trimmed
# so that every value of every axis appears; at 128 heads the float64 oracle checks 3 kv heads.
GRID = [
    (12, 544, 377, 4, True, torch.float16),
    (17, 977, 177, 4, False, torch.bfloat16),
    (12, 977, 177, 32, True, torch.bfloat16),
    (17, 544, 377, 32, False, torch.float16),
    (12, 544, 177, 128, True, torch.float16),
    (17, 977, 377, 128, True, torch.bfloat16),
    (12, 977, 377, 128, False, torch.bfloat16),
]


@pytest.mark.parametrize("batch,kv_len,qo_len,heads,causal,dtype", GRID)
def test_ragged_grid_matches_oracle(batch, kv_len, qo_len, heads, causal, dtype):
    qo_lens, kv_lens = [qo_len] * batch, [kv_len] * batch
    q, k, v = _data(qo_lens, kv_lens, heads, heads, dtype, seed=batch * 1000 + kv_len + heads)
    o, lse, _ = _ragged(qo_lens, kv_lens, heads, heads, dtype, causal, q.to(DEV), k.to(DEV), v.to(DEV))
    assert o.shape == (batch * qo_len, heads, DVO) and o.dtype == dtype
    sub = [0, 61, 127] if heads == 128 else None
    o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, causal, kv_heads=sub)
    _check(_heads(o.cpu(), heads, heads, sub), _heads(lse.cpu(), heads, heads, sub), o_ref, lse_ref, dtype)


@pytest.mark.parametrize("qo_len,kv_len", [(1832, 5532), (3928, 7563)])
@pytest.mark.parametrize("causal", [True, False])
def test_single_prefill_long_matches_oracle(qo_len, kv_len, causal):
    """128 heads; the float64 oracle checks kv heads 0, 77 and 127 (every head runs the same code)."""
    import flashinfer

    dtype = torch.bfloat16
    q, k, v = _data([qo_len], [kv_len], 128, 128, dtype, seed=qo_len + kv_len)
    o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_lse=True)
    torch.cuda.synchronize()
    assert o.shape == (qo_len, 128, DVO)
    sub = [0, 77, 127]
    o_ref, lse_ref = _ref(q, k, v, [qo_len], [kv_len], causal, kv_heads=sub)
    _check(_heads(o.cpu(), 128, 128, sub), _heads(lse.cpu(), 128, 128, sub), o_ref, lse_ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hq,hkv", [(32, 8), (16, 16), (16, 2)])
@pytest.mark.parametrize("causal", [True, False])
def test_gqa_and_sm_scale(dtype, hq, hkv, causal):
    qo_lens, kv_lens = [37, 300, 1, 129], [37, 700, 65, 129]
    q, k, v = _data(qo_lens, kv_lens, hq, hkv, dtype, seed=hq * 10 + hkv)
    o, lse, _ = _ragged(qo_lens, kv_lens, hq, hkv, dtype, causal, q.to(DEV), k.to(DEV), v.to(DEV), sm_scale=0.07)
    o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, causal, sm_scale=0.07)
    _check(o, lse, o_ref, lse_ref, dtype)


def test_bf16_pv_modes():
    """bf16_pv_exact_range=True (hi + lo bf16 P on the bf16 MFMA) meets the same bar as the default f16 P.V."""
    import flashinfer

    dtype = torch.bfloat16
    q, k, v = _data([200], [900], 8, 8, dtype, seed=5)
    o_ref, lse_ref = _ref(q, k, v, [200], [900], True)
    for exact in (False, True):
        o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=True,
                                                         return_lse=True, bf16_pv_exact_range=exact)
        _check(o, lse, o_ref, lse_ref, dtype)


@pytest.mark.parametrize("causal", [True, False])
def test_window_left(causal):
    dtype = torch.float16
    qo_lens, kv_lens = [300, 64], [1000, 500]
    q, k, v = _data(qo_lens, kv_lens, 8, 4, dtype, seed=9)
    o, lse, _ = _ragged(qo_lens, kv_lens, 8, 4, dtype, causal, q.to(DEV), k.to(DEV), v.to(DEV), window_left=200)
    o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, causal, window_left=200)
    _check(o, lse, o_ref, lse_ref, dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_splits_and_empty_requests(dtype):
    """Requests with kv_len 0 give zero rows and lse -inf; a forced split matches the oracle and the unsplit run."""
    qo_lens, kv_lens = [50, 7, 300, 20], [0, 2000, 1500, 0]
    hq, hkv = 8, 8
    q, k, v = _data(qo_lens, kv_lens, hq, hkv, dtype, seed=11)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o0, lse0, w0 = _ragged(qo_lens, kv_lens, hq, hkv, dtype, False, qd, kd, vd, disable_split_kv=True)
    o1, lse1, w1 = _ragged(qo_lens, kv_lens, hq, hkv, dtype, False, qd, kd, vd, fixed_split_size=256)
    assert w0._plan_info[_lib.FI_PP_SPLIT_KV] == 0 and w1._plan_info[_lib.FI_PP_SPLIT_KV] == 1
    o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, False)
    for o, lse in ((o0, lse0), (o1, lse1)):
        _check(o, lse, o_ref, lse_ref, dtype)
    torch.testing.assert_close(o1.float(), o0.float(), **ptol(dtype))
    empty = torch.cat([torch.arange(0, 50), torch.arange(357, 377)])
    assert torch.all(o1[empty] == 0)
    assert torch.all(lse1[empty].cpu() < -1e4)


@pytest.mark.parametrize("layout", ["NHD", "HND"])
def test_strided_views_and_layout(layout):
    """k = cat(k_nope, k_pe) and v = the second half of a fused [nnz, H, 256] kv projection; no copy is made."""
    dtype = torch.bfloat16
    qo_lens, kv_lens = [100, 250], [400, 250]
    hq = hkv = 8
    nnz = sum(kv_lens)
    g = torch.Generator().manual_seed(3)
    q = torch.randn(sum(qo_lens), hq, DQK, generator=g).to(dtype)
    kv_fused = torch.randn(nnz, hkv, 256, generator=g).to(dtype)  # [k_nope | v]
    k_pe = torch.randn(nnz, 1, 64, generator=g).to(dtype).expand(nnz, hkv, 64)
    k = torch.cat([kv_fused[..., :128], k_pe], dim=-1)
    v = kv_fused[..., 128:]
    o_ref, lse_ref = _ref(q, k, v.contiguous(), qo_lens, kv_lens, True)
    fused_d = kv_fused.to(DEV)
    kd = k.to(DEV)
    if layout == "HND":
        fused_d = fused_d.transpose(0, 1).contiguous()
        kd = kd.transpose(0, 1).contiguous()
    vd = fused_d[..., 128:]
    assert not vd.is_contiguous()
    ptr = vd.data_ptr()
    o, lse, _ = _ragged(qo_lens, kv_lens, hq, hkv, dtype, True, q.to(DEV), kd, vd, layout=layout)
    assert vd.data_ptr() == ptr
    _check(o, lse, o_ref, lse_ref, dtype)
    # single prefill over the same views (one request)
    import flashinfer

    n0, m0 = qo_lens[0], kv_lens[0]
    ks = kd[:m0] if layout == "NHD" else kd[:, :m0]
    vs = vd[:m0] if layout == "NHD" else vd[:, :m0]
    os_, lses = flashinfer.single_prefill_with_kv_cache(q[:n0].to(DEV), ks, vs, causal=True, kv_layout=layout,
                                                        return_lse=True)
    _check(os_, lses, o_ref[:n0], lse_ref[:n0], dtype)


@pytest.mark.parametrize("n_prefix", [1, 2])
def test_chunked_prefill_composition(n_prefix):
    """The extend phase: causal attention over the new tokens, non-causal over one or two prefix chunks, merged with
    merge_state / merge_states, equals causal attention over prefix + new tokens."""
    import flashinfer

    dtype = torch.float16
    hq, hkv = 16, 16
    new_lens, prefix_lens = [120, 33], [[500, 260], [700, 130]][:n_prefix]
    g = torch.Generator().manual_seed(21)
    q = torch.randn(sum(new_lens), hq, DQK, generator=g).to(dtype)
    chunks_k = [torch.randn(sum(pl), hkv, DQK, generator=g).to(dtype) for pl in prefix_lens]
    chunks_v = [torch.randn(sum(pl), hkv, DVO, generator=g).to(dtype) for pl in prefix_lens]
    k_new = torch.randn(sum(new_lens), hkv, DQK, generator=g).to(dtype)
    v_new = torch.randn(sum(new_lens), hkv, DVO, generator=g).to(dtype)
    qd = q.to(DEV)
    o_new, s_new, _ = _ragged(new_lens, new_lens, hq, hkv, dtype, True, qd, k_new.to(DEV), v_new.to(DEV))
    states = [(o_new, s_new)]
    for ck, cv, pl in zip(chunks_k, chunks_v, prefix_lens):
        o_c, s_c, _ = _ragged(new_lens, pl, hq, hkv, dtype, False, qd, ck.to(DEV), cv.to(DEV))
        states.append((o_c, s_c))
    if n_prefix == 1:
        o, s = flashinfer.merge_state(states[1][0], states[1][1], states[0][0], states[0][1])
    else:
        o, s = flashinfer.merge_states(torch.stack([x[0] for x in states], 1), torch.stack([x[1] for x in states], 1))
    torch.cuda.synchronize()
    # reference: per request, keys = the prefix chunks then the new tokens, causal (queries are the last rows)
    qi, ni = indptr_of(new_lens), indptr_of(new_lens)
    outs, lses = [], []
    for b in range(len(new_lens)):
        ks, vs = [], []
        for ck, cv, pl in zip(chunks_k, chunks_v, prefix_lens):
            pi = indptr_of(pl)
            ks.append(ck[pi[b]:pi[b + 1]])
            vs.append(cv[pi[b]:pi[b + 1]])
        ks.append(k_new[ni[b]:ni[b + 1]])
        vs.append(v_new[ni[b]:ni[b + 1]])
        o_r, s_r = R.attention_ref(q[qi[b]:qi[b + 1]].float(), torch.cat(ks).float(), torch.cat(vs).float(),
                                   causal=True)
        outs.append(o_r)
        lses.append(s_r)
    _check(o, s, torch.cat(outs), torch.cat(lses), dtype)


def test_graph_replay_after_replan():
    """A use_cuda_graph=True wrapper captured once (one stream, no parallel branches) and replayed after plan()
    changed the lengths and the chunking."""
    import flashinfer

    dtype = torch.bfloat16
    hq, hkv, b, rows, kv_rows = 8, 2, 2, 400, 3000
    ws = torch.zeros(128 << 20, dtype=torch.uint8, device=DEV)
    qo_buf = torch.zeros(b + 1, dtype=torch.int32, device=DEV)
    kv_buf = torch.zeros(b + 1, dtype=torch.int32, device=DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, "NHD", use_cuda_graph=True, qo_indptr_buf=qo_buf,
                                                        kv_indptr_buf=kv_buf)
    # (forced chunk sizes keep the work list within the captured launch's fixed item count)
    cases = [([150, 250], [1000, 2000], None), ([400, 0], [2900, 100], 256), ([1, 399], [64, 2500], 1024)]
    q_dev = torch.zeros(rows, hq, DQK, dtype=dtype, device=DEV)
    k_dev = torch.zeros(kv_rows, hkv, DQK, dtype=dtype, device=DEV)
    v_dev = torch.zeros(kv_rows, hkv, DVO, dtype=dtype, device=DEV)
    out = torch.zeros(rows, hq, DVO, dtype=dtype, device=DEV)
    lse = torch.zeros(rows, hq, dtype=torch.float32, device=DEV)

    def plan(i):
        qo_lens, kv_lens, split = cases[i]
        w.plan(indptr_of(qo_lens).to(DEV), indptr_of(kv_lens).to(DEV), hq, hkv, DQK, head_dim_vo=DVO, causal=True,
               q_data_type=dtype, fixed_split_size=split)
        q, k, v = _data(qo_lens, kv_lens, hq, hkv, dtype, seed=40 + i)
        q_dev.copy_(q.to(DEV))
        k_dev[: k.shape[0]].copy_(k.to(DEV))
        v_dev[: v.shape[0]].copy_(v.to(DEV))
        return q, k, v

    plan(0)
    w.run(q_dev, k_dev, v_dev, out=out, lse=lse, return_lse=True)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.run(q_dev, k_dev, v_dev, out=out, lse=lse, return_lse=True)
    for i in (0, 1, 2, 0):
        q, k, v = plan(i)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        qo_lens, kv_lens, _ = cases[i]
        o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, True)
        _check(out, lse, o_ref, lse_ref, dtype)


def test_refusals():
    import flashinfer

    ws = torch.zeros(16 << 20, dtype=torch.uint8, device=DEV)
    qi, ki = indptr_of([10]).to(DEV), indptr_of([20]).to(DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws)
    with pytest.raises(ValueError, match="fp8"):
        w.plan(qi, ki, 4, 4, DQK, head_dim_vo=DVO, q_data_type=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="pos_encoding_mode"):
        w.plan(qi, ki, 4, 4, DQK, head_dim_vo=DVO, pos_encoding_mode="ROPE_LLAMA", q_data_type=torch.float16)
    with pytest.raises(ValueError, match="pos_encoding_mode"):
        w.plan(qi, ki, 4, 4, DQK, head_dim_vo=DVO, pos_encoding_mode="ALIBI", q_data_type=torch.float16)
    with pytest.raises(ValueError, match="custom masks"):
        w.plan(qi, ki, 4, 4, DQK, head_dim_vo=DVO, custom_mask=torch.ones(200, dtype=torch.bool, device=DEV),
               q_data_type=torch.float16)
    with pytest.raises(ValueError, match="logits_soft_cap"):
        w.plan(qi, ki, 4, 4, DQK, head_dim_vo=DVO, logits_soft_cap=30.0, q_data_type=torch.float16)
    for qk, vo in ((192, 64), (128, 192), (256, 128), (576, 512)):
        with pytest.raises(ValueError, match="unsupported"):
            w.plan(qi, ki, 4, 4, qk, head_dim_vo=vo, q_data_type=torch.float16)
    pw = flashinfer.BatchPrefillWithPagedKVCacheWrapper(ws)
    with pytest.raises(ValueError, match="head_dim_qk == head_dim_vo"):
        pw.plan(qi, indptr_of([2]).to(DEV), torch.arange(2, dtype=torch.int32, device=DEV),
                torch.tensor([4], dtype=torch.int32, device=DEV), 4, 4, DQK, 16, head_dim_vo=DVO,
                q_data_type=torch.float16)
    q = torch.randn(10, 4, DQK, device=DEV).half()
    k = torch.randn(20, 4, DQK, device=DEV).half()
    v = torch.randn(20, 4, DVO, device=DEV).half()
    with pytest.raises(ValueError, match="pos_encoding_mode"):
        flashinfer.single_prefill_with_kv_cache(q, k, v, pos_encoding_mode="ROPE_LLAMA")
    with pytest.raises(ValueError, match="custom masks"):
        flashinfer.single_prefill_with_kv_cache(q, k, v, custom_mask=torch.ones(10, 20, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="fp8"):
        flashinfer.single_prefill_with_kv_cache(q.to(torch.float8_e4m3fn), k.to(torch.float8_e4m3fn),
                                                v.to(torch.float8_e4m3fn), o_dtype=torch.float16)
    with pytest.raises(ValueError, match="unsupported"):
        flashinfer.single_prefill_with_kv_cache(q[..., :128].contiguous(), k[..., :128].contiguous(), v[..., :64])


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sweep(seed):
    rng = random.Random(seed)
    dtype = rng.choice([torch.float16, torch.bfloat16])
    hkv = rng.choice([1, 2, 4, 8])
    hq = hkv * rng.choice([1, 2, 4, 8])
    n = rng.randint(1, 6)
    kv_lens = [rng.choice([0, 1, rng.randint(1, 200), rng.randint(1, 1500)]) for _ in range(n)]
    causal = rng.random() < 0.6
    qo_lens = [rng.randint(1, max(1, kl)) if causal and kl > 0 and rng.random() < 0.8 else rng.randint(1, 300)
               for kl in kv_lens]
    plan_kw = {}
    if rng.random() < 0.3:
        plan_kw["fixed_split_size"] = rng.choice([64, 128, 512])
    if rng.random() < 0.2:
        plan_kw["window_left"] = rng.randint(0, 300)
    if rng.random() < 0.3:
        plan_kw["sm_scale"] = rng.uniform(0.02, 0.2)
    q, k, v = _data(qo_lens, kv_lens, hq, hkv, dtype, seed=1000 + seed)
    o, lse, _ = _ragged(qo_lens, kv_lens, hq, hkv, dtype, causal, q.to(DEV), k.to(DEV), v.to(DEV), ws_mb=256, **plan_kw)
    ref_kw = {k_: v_ for k_, v_ in plan_kw.items() if k_ in ("window_left", "sm_scale")}
    o_ref, lse_ref = _ref(q, k, v, qo_lens, kv_lens, causal, **ref_kw)
    _check(o, lse, o_ref, lse_ref, dtype)
