"""Batch decode with an fp8 (e4m3) query over an e4m3 cache (csrc/decode_fp8_kernel.h): the plan-free call and the
wrapper against two f64 references computed from the same e4m3 values -- the reference's fp8 arithmetic
(fp8_attention_ref, "oracle") and exact attention over the dequantised inputs (attention_ref, "exact").

  1. assert_close(out, oracle, rtol = atol = 5e-2): the bar of the project's fp8 attention.
  2. max|out - exact| <= 2 max|oracle - exact| + 2^-8 max|exact|: the kernel rounds P on the running-maximum grid, the
     oracle on the final-maximum grid -- two draws of the same e4m3 rounding, so the kernel may be as far from exact as
     the oracle is; the last term is the 16-bit output's own rounding.
Block-table entries past a request's pages point at a page of 0xFF bytes (NaN in e4m3): reading one shows."""
import functools

import pytest
import torch

from attn_inputs import DEV, page_table, planned_decode_wrapper, poison_, scatter_to_pages
from flashinfer import _lib
from flashinfer import decode as D
from oracle import attention_ref as R

E4M3 = torch.float8_e4m3fn
LENS = (0, 1, 31, 32, 33, 127, 128, 129, 700)  # the edges of 32- and 128-token tiles, an empty request, several tiles
Q_SCALE, K_SCALE, V_SCALE = 0.5, 2.0, 1.5
GROUPS = [(4, 4), (8, 2), (10, 2), (16, 1)]  # G = 1, 4, 5 (columns past G unused), 16


@functools.lru_cache(maxsize=None)
def _problem(kv_lens, hq, hkv, d, ps, window=-1, peaked=False, seed=3):
    """q, the paged cache (NHD and HND), its CSR and dense page tables, and both references: once per problem."""
    g = torch.Generator().manual_seed(seed)
    B, n = len(kv_lens), sum(kv_lens)
    q = torch.randn(B, hq, d, generator=g).to(E4M3)
    k = torch.randn(n, hkv, d, generator=g).to(E4M3)
    v = torch.randn(n, hkv, d, generator=g).to(E4M3)
    if peaked:
        # logit = (q . k) / sqrt(d) nats with q = 2: rows of -0.0884 r (r in [0, 1]) sit at -2 r, one row of 0.5625 per
        # request at +12.7: its P8 is exactly 448, the tail's 448 e^-13 .. e^-15 straddles e4m3's smallest subnormal
        q = torch.full((B, hq, d), 2.0).to(E4M3)
        k = (-d ** -0.5 * torch.rand(n, hkv, 1, generator=g)).expand(n, hkv, d).contiguous()
        k[torch.tensor([777, kv_lens[0] + kv_lens[1] - 1])] = 0.5625
        k = k.to(E4M3)
    indptr, indices, last, pages = page_table(list(kv_lens), ps, g, extra_pages=1)
    cache = scatter_to_pages(k.float(), v.float(), kv_lens, indptr, indices, ps, pages).to(E4M3)
    poison = (set(range(pages)) - set(indices.tolist())).pop()
    poison_(cache[poison])
    table = torch.full((B, -(-max(kv_lens) // ps) + 2), poison, dtype=torch.int32)
    for b in range(B):
        row = indices[int(indptr[b]): int(indptr[b + 1])]
        table[b, : len(row)] = row
    sm_scale = Q_SCALE * K_SCALE * d ** -0.5
    oracle, exact = torch.zeros(B, hq, d, dtype=torch.float64), torch.zeros(B, hq, d, dtype=torch.float64)
    lse = torch.full((B, hq), R.NEG_INF_SENTINEL, dtype=torch.float64)
    off = 0
    for b, L in enumerate(kv_lens):
        if L:
            kb, vb = k[off: off + L], v[off: off + L]
            oracle[b], lse[b] = (t[0] for t in R.fp8_attention_ref(
                q[b: b + 1], kb, vb, torch.full((hq,), Q_SCALE), torch.full((hkv,), K_SCALE),
                torch.full((hkv,), V_SCALE), window_left=window))
            exact[b] = R.attention_ref(q[b: b + 1].float(), kb.float(), vb.float(), sm_scale=sm_scale,
                                       window_left=window, dtype=torch.float64)[0][0] * V_SCALE
        off += L
    return dict(q=q.to(DEV), nhd=cache.to(DEV), hnd=cache.transpose(2, 3).contiguous().to(DEV), indptr=indptr,
                indices=indices, last=last, table=table.to(DEV), lens=torch.tensor(kv_lens, dtype=torch.int32, device=DEV),
                sm_scale=sm_scale, oracle=oracle, exact=exact, lse=lse, window=window, dims=(hq, hkv, d, ps))


def _check(out, pr, what):
    o = out.cpu().double()
    err = (o - pr["exact"]).abs().max().item()
    oracle_err = (pr["oracle"] - pr["exact"]).abs().max().item()
    print(f"{what}: max|out - exact| = {err:.3e}, max|oracle - exact| = {oracle_err:.3e}, "
          f"ratio {err / max(oracle_err, 1e-300):.2f}")
    torch.testing.assert_close(o, pr["oracle"], rtol=5e-2, atol=5e-2)
    assert err <= 2 * oracle_err + 2.0 ** -8 * pr["exact"].abs().max().item()


def _plan_free(pr, out_dtype=torch.bfloat16, **kw):
    ws = poison_(torch.empty(32 << 20, dtype=torch.uint8, device=DEV))
    ps = pr["dims"][3]
    return D.trtllm_batch_decode_with_kv_cache(pr["q"], pr["hnd"], ws, pr["table"], pr["lens"], pr["table"].shape[1] * ps,
                                               pr["sm_scale"], V_SCALE, window_left=pr["window"], out_dtype=out_dtype, **kw)


def _planned(pr, layout="NHD", **plan_kw):
    hq, hkv, d, ps = pr["dims"]
    return planned_decode_wrapper(32 << 20, layout, pr["indptr"], pr["indices"], pr["last"], hq, hkv, d, ps,
                                  **dict(dict(q_data_type=E4M3, kv_data_type=E4M3, window_left=pr["window"]), **plan_kw))


def _wrapper(pr, layout="NHD", as_tuple=False, out=None):
    w = _planned(pr, layout)
    cache = pr["nhd"] if layout == "NHD" else pr["hnd"]
    o, lse = w.run(pr["q"], (cache[:, 0], cache[:, 1]) if as_tuple else cache, q_scale=Q_SCALE, k_scale=K_SCALE,
                   v_scale=V_SCALE, out=out, return_lse=True)
    torch.testing.assert_close(lse.cpu().double(), pr["lse"], rtol=2e-3, atol=2e-3)
    return w, o


@pytest.mark.gpu
@pytest.mark.parametrize("window", [-1, 40])
@pytest.mark.parametrize("ps,out_dtype", [(16, torch.bfloat16), (1, torch.float16)])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("hq,hkv", GROUPS)
def test_plan_free_call_matches_both_references(hq, hkv, d, ps, out_dtype, window):
    pr = _problem(LENS, hq, hkv, d, ps, window)
    out = _plan_free(pr, out_dtype)
    assert out.dtype == out_dtype and not out[0].any()  # the empty request: a zero row
    _check(out, pr, f"plan-free {hq}/{hkv} d{d} ps{ps} w{window}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout,as_tuple,window", [("NHD", False, -1), ("HND", True, -1), ("NHD", False, 40)])
def test_wrapper_output_and_lse(layout, as_tuple, window):
    """The window of the plan-free cases acts at run only (chunks cut over all pages); here plan() cuts them for it."""
    pr = _problem(LENS, 8, 2, 128, 16, window)
    _, o = _wrapper(pr, layout, as_tuple)
    assert o.dtype == torch.bfloat16
    _check(o, pr, f"wrapper {layout} tuple={as_tuple} w{window}")
    out16 = torch.empty(o.shape, dtype=torch.float16, device=DEV)
    assert _wrapper(pr, layout, as_tuple, out=out16)[1] is out16
    _check(out16, pr, "wrapper, float16 out")


@pytest.mark.gpu
@pytest.mark.parametrize("kv_lens,dims,peaked,split", [
    ((3000, 3000), (32, 8, 128, 16), False, True), ((2048, 2048), (32, 8, 128, 16), True, True),
    (tuple(LENS[i % len(LENS)] for i in range(256)), (16, 8, 64, 16), False, False)],
    ids=["split", "peaked_split", "unsplit_256"])
def test_split_and_unsplit_plans(kv_lens, dims, peaked, split):
    pr = _problem(kv_lens, *dims, peaked=peaked)
    w, o = _wrapper(pr)
    assert bool(w._plan_info[_lib.FI_DP_SPLIT_KV]) == split
    _check(o, pr, f"wrapper {len(kv_lens)} requests, split={split}, peaked={peaked}")
    _check(_plan_free(pr), pr, "the same, plan-free")


@pytest.mark.gpu
def test_captured_call_replans_on_other_lengths():
    """The plan-free call captured on one set of lengths, replayed on another (lengths and block table overwritten in
    place); several replays, all compared with the oracle of what the buffers hold."""
    pr2 = _problem(LENS, 8, 2, 128, 16)
    B, blocks = pr2["table"].shape
    pr = dict(pr2, lens=torch.full((B,), 100, dtype=torch.int32, device=DEV),
              table=pr2["table"][8:9].repeat(B, 1).contiguous())  # captured on 100 tokens of the 700-token request
    out = torch.zeros(B, 8, 128, dtype=torch.bfloat16, device=DEV)
    ws = torch.empty(32 << 20, dtype=torch.uint8, device=DEV)

    def call():
        D.trtllm_batch_decode_with_kv_cache(pr["q"], pr["hnd"], ws, pr["table"], pr["lens"], blocks * 16, pr["sm_scale"],
                                            V_SCALE, out=out)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    pr["lens"].copy_(pr2["lens"])
    pr["table"].copy_(pr2["table"])
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        _check(out, pr2, "graph replay")


def _args(dtype=E4M3, kv_dtype=E4M3, **over):
    args = dict(query=torch.zeros(3, 32, 128).to(dtype), kv_cache=torch.zeros(12, 2, 8, 16, 128).to(kv_dtype),
                workspace_buffer=torch.zeros(1 << 20, dtype=torch.uint8), block_tables=torch.zeros(3, 8, dtype=torch.int32),
                seq_lens=torch.ones(3, dtype=torch.int32), max_seq_len=128, bmm1_scale=1.0, bmm2_scale=1.0,
                out_dtype=torch.bfloat16)
    return dict(args, **over)


@pytest.mark.parametrize("names,over", [
    ("fp8 query.*out_dtype", dict(out_dtype=None)), ("fp8 query", dict(kv_dtype=torch.float16)),
    ("e5m2", dict(dtype=torch.float8_e5m2)), ("e5m2", dict(kv_dtype=torch.float8_e5m2)),
    ("sinks", dict(sinks=torch.zeros(32))), ("q_len_per_req", dict(q_len_per_req=2)),
    ("fp8 output", dict(out_dtype=E4M3))], ids=lambda x: x if isinstance(x, str) else "")
def test_plan_free_refusals_by_name_before_the_library(monkeypatch, names, over):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    with pytest.raises(NotImplementedError, match="trtllm_batch_decode_with_kv_cache: .*" + names):
        D.trtllm_batch_decode_with_kv_cache(**_args(**over))


@pytest.mark.gpu
@pytest.mark.parametrize("names,plan_kw,run_kw", [
    ("pos_encoding_mode", dict(pos_encoding_mode="ROPE_LLAMA"), {}), ("logits_soft_cap", dict(logits_soft_cap=30.0), {}),
    ("fp8 query", dict(kv_data_type=torch.float16), {}), ("e5m2", dict(q_data_type=torch.float8_e5m2), {}),
    ("sinks", {}, dict(sinks=torch.zeros(8))), ("q_len_per_req", {}, dict(q_len_per_req=2))],
    ids=lambda x: x if isinstance(x, str) else "")
def test_wrapper_refusals_by_name(monkeypatch, names, plan_kw, run_kw):
    """Refused at plan() where plan_kw names the cause, else at run() of a wrapper planned for the fp8 pair."""
    pr = _problem(LENS, 8, 2, 128, 16)
    if plan_kw:
        with pytest.raises(NotImplementedError, match=names):
            _planned(pr, **plan_kw)
        return
    w = _planned(pr)
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    with pytest.raises(NotImplementedError, match=names):
        w.run(pr["q"], pr["nhd"], **run_kw)
