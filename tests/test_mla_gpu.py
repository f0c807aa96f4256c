"""GPU: BatchMLAPagedAttentionWrapper and append_paged_mla_kv_cache against the oracle.

The MLA oracle is attention_ref with one KV head, 576 QK dims and 512 VO dims:
    attention_ref(cat(q_nope, q_pe), cat(ckv, kpe)[:, None], ckv[:, None], causal, sm_scale)
(ref: tests/attention/test_deepseek_mla.py:105-150, lse in base 2).
"""
import math

import pytest
import torch

import flashinfer
from attn_inputs import indptr_of, owned_slots, page_table, tol
from oracle.attention_ref import attention_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CKV, KPE = 512, 64


def make_case(kv_lens, qo_lens, H, page_size, dtype, seed=0, nan_fill=False, spare_pages=0):
    """nan_fill: every slot of ckv and kpe that no request owns -- the tail of each last page and the spare_pages
    pages no request references -- holds 0xFF bytes, a NaN in f16 and bf16."""
    g = torch.Generator().manual_seed(seed)
    pages = [-(-l // page_size) for l in kv_lens]
    kv_indptr = indptr_of(pages)
    total_pages = int(kv_indptr[-1])
    num_pages = max(total_pages, 1) + spare_pages
    kv_indices = torch.randperm(num_pages, generator=g)[:total_pages].to(torch.int32)
    qo_indptr = indptr_of(qo_lens)
    nnz = int(qo_indptr[-1])
    ckv = (torch.randn(num_pages, page_size, CKV, generator=g) * 0.5).to(dtype)
    kpe = (torch.randn(num_pages, page_size, KPE, generator=g) * 0.5).to(dtype)
    if nan_fill:
        owned = owned_slots(kv_lens, kv_indptr, kv_indices, page_size, num_pages)
        ckv.view(torch.int16)[~owned] = -1
        kpe.view(torch.int16)[~owned] = -1
    q_nope = torch.randn(nnz, H, CKV, generator=g).to(dtype)
    q_pe = torch.randn(nnz, H, KPE, generator=g).to(dtype)
    return dict(kv_lens=kv_lens, qo_lens=qo_lens, H=H, page_size=page_size, dtype=dtype, qo_indptr=qo_indptr,
                kv_indptr=kv_indptr, kv_indices=kv_indices, kv_len_arr=torch.tensor(kv_lens, dtype=torch.int32),
                q_nope=q_nope.to(DEV), q_pe=q_pe.to(DEV), ckv=ckv.to(DEV), kpe=kpe.to(DEV))


def oracle(c, causal, sm_scale):
    """o [nnz, H, 512] f32, lse [nnz, H] f32 (f64 math on the CPU), returned on the GPU."""
    outs, lses = [], []
    ps = c["page_size"]
    for b, (kl, ql) in enumerate(zip(c["kv_lens"], c["qo_lens"])):
        q0 = int(c["qo_indptr"][b])
        q = torch.cat([c["q_nope"][q0:q0 + ql], c["q_pe"][q0:q0 + ql]], -1).cpu()
        pidx = c["kv_indices"][int(c["kv_indptr"][b]):int(c["kv_indptr"][b + 1])].to(DEV).long()
        ckv = c["ckv"][pidx].reshape(-1, CKV)[:kl]
        kpe = c["kpe"][pidx].reshape(-1, KPE)[:kl]
        ckv, kpe = ckv.cpu(), kpe.cpu()
        k = torch.cat([ckv, kpe], -1)[:, None]
        o, lse = attention_ref(q, k, ckv[:, None], causal, sm_scale)
        outs.append(o.float())
        lses.append(lse.float())
    return torch.cat(outs).to(DEV), torch.cat(lses).to(DEV)


def plan_run(c, causal, sm_scale, ws=None, q_nope=None, q_pe=None, ckv=None, kpe=None):
    ws = ws if ws is not None else torch.empty(128 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, backend="fa2")
    w.plan(c["qo_indptr"].to(DEV), c["kv_indptr"].to(DEV), c["kv_indices"].to(DEV), c["kv_len_arr"].to(DEV),
           c["H"], CKV, KPE, c["page_size"], causal, sm_scale, c["dtype"], c["dtype"])
    o, lse = w.run(c["q_nope"] if q_nope is None else q_nope, c["q_pe"] if q_pe is None else q_pe,
                   c["ckv"] if ckv is None else ckv, c["kpe"] if kpe is None else kpe, return_lse=True)
    torch.cuda.synchronize()
    return w, o, lse


def check(c, o, lse, causal, sm_scale):
    o_ref, lse_ref = oracle(c, causal, sm_scale)
    torch.testing.assert_close(o.float(), o_ref, **tol(c["dtype"]))
    # lse wherever the row sees at least one key
    rows = []
    for kl, ql in zip(c["kv_lens"], c["qo_lens"]):
        for i in range(ql):
            rows.append(kl > 0 and (not causal or kl - ql + i >= 0))
    live = torch.tensor(rows, device=DEV)
    torch.testing.assert_close(lse[live], lse_ref[live], rtol=1e-3, atol=1e-3)


SM = 1.0 / math.sqrt(128 + 64)

GRID = [
    # (kv_lens, qo_len, heads, page_size)
    ([17], 1, 16, 1),
    ([2743], 1, 16, 16),
    ([8736], 1, 128, 64),
    ([0, 1, 17], 1, 64, 16),
    ([514, 2743, 1], 2, 16, 64),
    ([17, 514, 0], 4, 128, 1),
    ([1, 17, 514, 2743, 8736] * 3 + [0, 514], 1, 16, 16),
    ([2743, 8736, 17], 17, 16, 64),
    ([514] * 17, 4, 64, 16),
    ([8736, 1, 2743], 17, 128, 16),
    # head counts that are not multiples of the 16-row tile: one tile holds rows of several query positions
    ([514, 2743, 17], 4, 8, 16),
    ([8736, 1, 33], 17, 8, 64),
    ([300, 1000, 0], 3, 24, 16),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", range(len(GRID)))
def test_mla_grid(case, causal, dtype):
    kv_lens, ql, H, ps = GRID[case]
    qo_lens = [ql] * len(kv_lens)
    if causal:
        # the reference leaves causal with qo_len > kv_len undefined: such requests get kv_len = qo_len instead
        kv_lens = [max(kl, ql) for kl in kv_lens]
    c = make_case(kv_lens, qo_lens, H, ps, dtype, seed=case)
    _, o, lse = plan_run(c, causal, SM)
    check(c, o, lse, causal, SM)


def test_mla_empty_requests():
    c = make_case([0, 300, 0], [1, 1, 2], 16, 16, torch.bfloat16, seed=5)
    _, o, lse = plan_run(c, False, SM)
    assert torch.equal(o[0], torch.zeros_like(o[0])) and torch.equal(o[2:], torch.zeros_like(o[2:]))
    assert torch.all(lse[0] == -5e4) and torch.all(lse[2:] == -5e4)
    check(c, o, lse, False, SM)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("ps", [16, 64, 5, 1])
def test_mla_nan_past_kv_len(ps, causal, dtype):
    """NaN behind every request's last token and in three pages no request references (page 5: a tail on a page that
    is no power of two; page 1: no tails, free pages only): finite, the oracle's result, and bit for bit the result on
    the same cache without the NaN."""
    args = ([17, 2743, 70], [1, 2, 1], 16, ps, dtype)
    c = make_case(*args, seed=6, nan_fill=True, spare_pages=3)
    assert c["ckv"].isnan().sum() >= 3 * ps * CKV and c["kpe"].isnan().sum() >= 3 * ps * KPE
    _, o, lse = plan_run(c, causal, SM)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    check(c, o, lse, causal, SM)
    clean = make_case(*args, seed=6, spare_pages=3)  # the same draws
    assert not clean["ckv"].isnan().any() and torch.equal(clean["q_nope"], c["q_nope"])
    _, o_clean, lse_clean = plan_run(clean, causal, SM)
    assert torch.equal(o.view(torch.int16), o_clean.view(torch.int16)) and torch.equal(lse, lse_clean)


def test_mla_strided_views():
    c = make_case([514, 2743, 17], [1, 4, 2], 64, 16, torch.bfloat16, seed=7)
    q = torch.cat([c["q_nope"], c["q_pe"]], -1)           # one 576-wide tensor
    kv = torch.cat([c["ckv"], c["kpe"]], -1)
    _, o_view, lse_view = plan_run(c, True, SM, q_nope=q[..., :CKV], q_pe=q[..., CKV:], ckv=kv[..., :CKV],
                                   kpe=kv[..., CKV:])
    _, o, lse = plan_run(c, True, SM)
    assert torch.equal(o_view, o) and torch.equal(lse_view, lse)
    check(c, o_view, lse_view, True, SM)


def test_mla_split_and_merge_state():
    c = make_case([32768], [1], 16, 64, torch.bfloat16, seed=8)
    w, o, lse = plan_run(c, False, SM)
    assert w._plan_info[flashinfer._lib.FI_MLA_SPLIT_KV] == 1
    check(c, o, lse, False, SM)
    # merge_state(run(prefix), run(suffix)) == run(whole): pins the base-2 lse convention
    ps, cut = 64, 12800
    pref = dict(c, kv_lens=[cut], kv_len_arr=torch.tensor([cut], dtype=torch.int32),
                kv_indptr=torch.tensor([0, cut // ps], dtype=torch.int32), kv_indices=c["kv_indices"][: cut // ps])
    suf = dict(c, kv_lens=[32768 - cut], kv_len_arr=torch.tensor([32768 - cut], dtype=torch.int32),
               kv_indptr=torch.tensor([0, (32768 - cut) // ps], dtype=torch.int32),
               kv_indices=c["kv_indices"][cut // ps:].contiguous())
    _, o_a, lse_a = plan_run(pref, False, SM)
    _, o_b, lse_b = plan_run(suf, False, SM)
    o_m, lse_m = flashinfer.merge_state(o_a, lse_a, o_b, lse_b)
    torch.testing.assert_close(o_m.float(), o.float(), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(lse_m, lse, rtol=1e-3, atol=1e-3)


def test_mla_graph_replay_after_replan():
    H, ps, dtype, B = 16, 16, torch.bfloat16, 4
    sets = [[100, 3000, 17, 800], [40000, 40000, 40000, 40000], [200000, 1, 1, 2]]
    cases = [make_case(kl, [1] * B, H, ps, dtype, seed=20 + i) for i, kl in enumerate(sets)]
    max_pages = max(int(c["kv_indptr"][-1]) for c in cases)
    ws = torch.empty(128 << 20, dtype=torch.uint8, device=DEV)
    bufs = [torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros(B + 1, dtype=torch.int32, device=DEV),
            torch.zeros(max_pages, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)]
    w = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, True, *bufs)
    # one static cache big enough for every case; each case's pages are copied in before replay
    num_pages = max(c["ckv"].shape[0] for c in cases)
    ckv = torch.zeros(num_pages, ps, CKV, dtype=dtype, device=DEV)
    kpe = torch.zeros(num_pages, ps, KPE, dtype=dtype, device=DEV)
    q_nope = torch.zeros(B, H, CKV, dtype=dtype, device=DEV)
    q_pe = torch.zeros(B, H, KPE, dtype=dtype, device=DEV)
    out = torch.empty(B, H, CKV, dtype=dtype, device=DEV)
    lse = torch.empty(B, H, dtype=torch.float32, device=DEV)

    def load(c):
        n = c["ckv"].shape[0]
        ckv[:n].copy_(c["ckv"])
        kpe[:n].copy_(c["kpe"])
        q_nope.copy_(c["q_nope"])
        q_pe.copy_(c["q_pe"])
        w.plan(c["qo_indptr"].to(DEV), c["kv_indptr"].to(DEV), c["kv_indices"].to(DEV), c["kv_len_arr"].to(DEV),
               H, CKV, KPE, ps, False, SM, dtype, dtype)

    load(cases[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        w.run(q_nope, q_pe, ckv, kpe, out=out, lse=lse, return_lse=True)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.run(q_nope, q_pe, ckv, kpe, out=out, lse=lse, return_lse=True)
    chunks = set()
    for c in cases:
        load(c)
        chunks.add(int(w._plan_info[flashinfer._lib.FI_MLA_KV_CHUNK_SIZE]))
        g.replay()
        torch.cuda.synchronize()
        c = dict(c, ckv=ckv, kpe=kpe)
        check(c, out, lse, False, SM)
    assert len(chunks) > 1, "the re-plans were meant to change the chunking"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_append_paged_mla_kv_cache(dtype):
    torch.manual_seed(9)
    H, ps = 16, 16
    hist = [5, 40, 0]          # tokens already in the cache
    new = [3, 1, 20]           # tokens appended now
    kv_lens = [h + n for h, n in zip(hist, new)]
    kv_indptr, kv_indices, last, total = page_table(kv_lens, ps)
    kv_indptr, kv_indices, last = kv_indptr.to(DEV), kv_indices.to(DEV), last.to(DEV)
    ckv_full = (torch.randn(sum(kv_lens), CKV) * 0.5).to(dtype).to(DEV)   # the whole history, request-major
    kpe_full = (torch.randn(sum(kv_lens), KPE) * 0.5).to(dtype).to(DEV)
    ckv_cache = torch.full((total, ps, CKV), float("nan"), dtype=dtype, device=DEV)
    kpe_cache = torch.full((total, ps, KPE), float("nan"), dtype=dtype, device=DEV)
    starts = indptr_of(kv_lens).tolist()

    def scatter(rows):  # torch index scatter of (request, position) rows
        for b, pos in rows:
            page = int(kv_indices[int(kv_indptr[b]) + pos // ps])
            ckv_cache[page, pos % ps] = ckv_full[starts[b] + pos]
            kpe_cache[page, pos % ps] = kpe_full[starts[b] + pos]

    scatter([(b, p) for b in range(3) for p in range(hist[b])])
    ref_ckv, ref_kpe = ckv_cache.clone(), kpe_cache.clone()
    append_indptr = indptr_of(new, DEV)
    bi, pos = flashinfer.get_batch_indices_positions(append_indptr, flashinfer.get_seq_lens(kv_indptr, last, ps),
                                                     sum(new))
    rows = [(b, hist[b] + i) for b in range(3) for i in range(new[b])]
    idx = torch.tensor([starts[b] + p for b, p in rows], device=DEV)
    flashinfer.append_paged_mla_kv_cache(ckv_full[idx], kpe_full[idx], bi, pos, ckv_cache, kpe_cache, kv_indices,
                                         kv_indptr, last)
    torch.cuda.synchronize()
    for b, p in rows:
        page = int(kv_indices[int(kv_indptr[b]) + p // ps])
        ref_ckv[page, p % ps] = ckv_full[starts[b] + p]
        ref_kpe[page, p % ps] = kpe_full[starts[b] + p]
    assert torch.equal(ckv_cache.view(torch.int16), ref_ckv.view(torch.int16))
    assert torch.equal(kpe_cache.view(torch.int16), ref_kpe.view(torch.int16))
    # decode over the whole history equals the oracle
    c = dict(kv_lens=kv_lens, qo_lens=[1, 1, 1], H=H, page_size=ps, dtype=dtype,
             qo_indptr=torch.arange(4, dtype=torch.int32), kv_indptr=kv_indptr.cpu(), kv_indices=kv_indices.cpu(),
             kv_len_arr=torch.tensor(kv_lens, dtype=torch.int32),
             q_nope=torch.randn(3, H, CKV).to(dtype).to(DEV), q_pe=torch.randn(3, H, KPE).to(dtype).to(DEV),
             ckv=ckv_cache, kpe=kpe_cache)
    _, o, lse = plan_run(c, False, SM)
    check(c, o, lse, False, SM)


def test_mla_graph_replan_must_keep_rows():
    """A captured run() is sized for the first plan's packed rows: a graph re-plan that changes the query count or
    the head count is refused (it would move the work list under the captured merge and the q / o tensors)."""
    B, H, ps = 3, 16, 16
    ws = torch.empty(32 << 20, dtype=torch.uint8, device=DEV)
    bufs = [torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros(B + 1, dtype=torch.int32, device=DEV),
            torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)]
    w = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, True, *bufs)

    def plan(qo_lens, heads=H):
        c = make_case([100, 200, 50], qo_lens, heads, ps, torch.bfloat16)
        w.plan(c["qo_indptr"].to(DEV), c["kv_indptr"].to(DEV), c["kv_indices"].to(DEV), c["kv_len_arr"].to(DEV),
               heads, CKV, KPE, ps, True, SM, torch.bfloat16, torch.bfloat16)

    plan([2, 2, 2])
    plan([1, 4, 1])  # same query count, other split over the requests: allowed
    with pytest.raises(ValueError, match="query count"):
        plan([1, 1, 1])
    with pytest.raises(ValueError, match="query count"):
        plan([4, 4, 4])
    with pytest.raises(ValueError, match="num_heads"):
        plan([2, 2, 2], heads=32)
    plan([3, 2, 1])
