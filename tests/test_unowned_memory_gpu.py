"""GPU: attention must ignore memory that no request owns.

A served cache comes from torch.empty: the slots behind a request's last token, the pages no request references and
the page ids behind a page table's last entry hold arbitrary bits, NaN among them; the float workspace holds the
partial states of an earlier, larger plan.  A kernel that loads one row too many gives it probability 0 -- and
0 * NaN is NaN.  Every case here runs twice, on clean memory and on memory whose unowned parts are 0xFF bytes (a NaN
in f16, bf16, f32, e4m3fn and e5m2), and asserts that the poisoned run

  * is finite,
  * meets the CPU oracle (which slices [:kv_len] and never sees the poison, tests/test_attn_inputs_cpu.py) at the bar
    the entry point's own tests hold it to, and
  * equals the clean run bit for bit -- the net for fp8, where an upcast may turn the NaN code into a number.

No path here is allowed to differ between its two runs: each is a fixed work list merged in a fixed order.
All poison is data in valid memory: surplus page ids always name a valid (poisoned) page."""
import contextlib

import pytest
import torch

import sink_ref
import sparse_ref
from attn_inputs import (DEV, indptr_of, make_paged, owned_slots, planned_decode_wrapper, planned_prefill_wrapper,
                         poison_, poison_unowned, ptol, rope_rt, tol)
from flashinfer import _lib
from oracle import attention_ref as R
from test_decode_gpu import VARIANTS
from test_page_cascade_gpu import _two_level_problem, plan_cascade, three_level_problem

pytestmark = pytest.mark.gpu

F16, BF16, E4M3, E5M2 = torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2
LSE = dict(rtol=1e-3, atol=1e-3)
DECODE_WS = 8 << 20  # the size tests/test_decode_fused_merge_gpu.py plans its 128-token chunks on


@contextlib.contextmanager
def kernel_variant(name):
    """The switches of an entry of test_decode_gpu.VARIANTS, set for the block."""
    try:
        for key, value in VARIANTS[name].items():
            _lib.set_option(key, value)
        yield
    finally:
        for key in VARIANTS[name]:
            _lib.set_option(key, None)


def paged_pair(kv_lens, page, hkv, d, kv_dtype, layout, seed):
    """(clean cache, poisoned cache, indptr, indices, last, a free page): 3 spare pages; every slot no request owns --
    the tail of each last page and the spare pages -- is 0xFF in the second cache."""
    cache, indptr, indices, last = make_paged(len(kv_lens), list(kv_lens), page, hkv, d, kv_dtype, layout, seed=seed,
                                              extra_pages=3)
    owned = owned_slots(kv_lens, indptr, indices, page, cache.shape[0])
    bad = poison_unowned(cache, layout, owned)
    free = sorted(set(range(cache.shape[0])) - set(indices.tolist()))
    assert len(free) == 3 and bool((bad.view(torch.uint8)[free] == 0xFF).all())
    return cache, bad, indptr, indices, last, free[0]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def check_pair(clean, dirty, o_ref, lse_ref, o_tol, lse_tol=LSE):
    """clean, dirty: (o, lse) of the two runs; lse_ref None: no lse bar (the entry point's tests have none)."""
    torch.cuda.synchronize()
    assert torch.isfinite(dirty[0].float()).all() and torch.isfinite(dirty[1]).all()
    torch.testing.assert_close(dirty[0].float().cpu(), o_ref.float(), **o_tol)
    if lse_ref is not None:
        torch.testing.assert_close(dirty[1].cpu(), lse_ref.float(), **lse_tol)
    assert same_bits(clean[0], dirty[0]) and same_bits(clean[1], dirty[1])


def touched(ws):
    return not bool((ws == 0xFF).all())


# ---- batch decode ---------------------------------------------------------------------------------------------------

UNSPLIT, FUSED, TWO_LAUNCH = (1, 15, 17, 33, 130), (130, 200, 256), (130, 700)


def decode_case(plan, hq, hkv, d, page, layout, kv_dtype, seed, kv_lens=None, o_tol=None, lse_tol=LSE, ref_kw=None,
                **plan_kw):
    """One decode problem, planned as `plan` names, run clean (zeroed workspace) and poisoned (0xFF cache slots, 0xFF
    workspace).  plan() leaves the float workspace alone (csrc/decode.hip), so it is poisoned after plan()."""
    kv_lens = kv_lens or dict(unsplit=UNSPLIT, fused=FUSED, two_launch=TWO_LAUNCH)[plan]
    q_dtype = BF16 if kv_dtype == BF16 else F16
    cache, bad, indptr, indices, last, _ = paged_pair(kv_lens, page, hkv, d, kv_dtype, layout, seed)
    q = torch.randn(len(kv_lens), hq, d, generator=torch.Generator().manual_seed(seed + 1)).to(q_dtype)
    # the oracle sees the same (already quantised) cache values, so the 16-bit bar applies to an fp8 cache too
    o_ref, lse_ref = R.batch_decode_ref(q.float(), cache.float(), layout, indptr, indices, last, **(ref_kw or {}))
    if plan == "unsplit":
        plan_kw["disable_split_kv"] = True
    w = planned_decode_wrapper(DECODE_WS, layout, indptr, indices, last, hq, hkv, d, page, q_data_type=q_dtype,
                               kv_data_type=kv_dtype, **plan_kw)
    info = w._plan_info
    if plan == "unsplit":
        assert info[_lib.FI_DP_SPLIT_KV] == 0
    elif plan == "fused":
        assert info[_lib.FI_DP_SPLIT_KV] == 1 and info[_lib.FI_DP_UNIFORM_CHUNKS] == 2
    else:
        assert info[_lib.FI_DP_SPLIT_KV] == 1 and info[_lib.FI_DP_UNIFORM_CHUNKS] == 0
    clean = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    poison_(w._float_workspace_buffer)
    dirty = w.run(q.to(DEV), bad.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, o_tol or tol(q_dtype), lse_tol)
    if plan == "two_launch":
        assert touched(w._float_workspace_buffer), "a split plan on the two-launch path writes its partial states"
    return dirty


# Every kernel form -- 4/4 and 8/2 (the 16x16x32 matrix-core kernel, or the VALU kernel under r1), 32/4 (16x16x32, or
# 32x32x16 under r1) and 64/1 (32x32x16) -- with every kv dtype; the plan, the page size (5: a tail on a page that is
# no power of two), the layout and the head dim rotate through them.
HEADS = [(4, 4), (8, 2), (32, 4), (64, 1)]
DECODE_GRID = []
for _i, (_hq, _hkv) in enumerate(HEADS):
    for _j, _kv_dtype in enumerate([F16, BF16, E4M3, E5M2]):
        _plan = ("unsplit", "fused", "two_launch")[(_i + _j) % 3]
        _page = 16 if _plan == "fused" else (5, 16)[(_i + _j // 2) % 2]
        DECODE_GRID.append((_plan, _hq, _hkv, (128, 64)[(_i + _j) % 2], _page, ("NHD", "HND")[(_i // 2 + _j) % 2],
                            _kv_dtype))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("plan,hq,hkv,d,page,layout,kv_dtype", DECODE_GRID,
                         ids=lambda x: str(x).replace("torch.", "") if not isinstance(x, int) else None)
def test_batch_decode(plan, hq, hkv, d, page, layout, kv_dtype, variant):
    with kernel_variant(variant):
        decode_case(plan, hq, hkv, d, page, layout, kv_dtype, seed=100 + 7 * hq + d + page)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", ["page_1", "d_256", "empty_request", "rope_llama", "window_16", "two_launch_page_5"])
def test_batch_decode_other_forms(case, variant):
    with kernel_variant(variant):
        if case == "page_1":  # no tails, only free pages
            decode_case("unsplit", 8, 2, 128, 1, "HND", F16, seed=201)
        elif case == "d_256":
            decode_case("unsplit", 8, 2, 256, 5, "NHD", BF16, seed=202)
        elif case == "empty_request":  # as tests/test_decode_gpu.py::test_empty_request_edge_case runs one
            o, lse = decode_case("unsplit", 4, 2, 128, 16, "NHD", F16, seed=203, kv_lens=UNSPLIT + (0,))
            assert torch.all(o[-1] == 0) and torch.all(lse[-1] == R.NEG_INF_SENTINEL)
        elif case == "rope_llama":  # bars of tests/test_decode_gpu.py::test_batch_decode_pos_encoding
            decode_case("unsplit", 8, 2, 128, 5, "NHD", F16, seed=204, o_tol=dict(rtol=1e-3, atol=1e-3),
                        lse_tol=dict(rtol=2e-3, atol=2e-3), pos_encoding_mode="ROPE_LLAMA", rope_theta=1e4,
                        rope_scale=1.0, ref_kw=dict(pos_encoding_mode="ROPE_LLAMA", rope_round_dtype=rope_rt(F16, 128)))
        elif case == "window_16":  # bars of tests/test_decode_gpu.py::test_batch_decode_window_and_soft_cap
            decode_case("unsplit", 8, 4, 128, 5, "NHD", BF16, seed=205, lse_tol=dict(rtol=1e-3, atol=2e-3),
                        window_left=16, ref_kw=dict(window_left=16))
        else:
            decode_case("two_launch", 8, 2, 128, 5, "HND", F16, seed=206)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("entry", ["decode", "prefill"])
@pytest.mark.parametrize("kv_dtype", [F16, BF16, E4M3, E5M2], ids=["f16", "bf16", "e4m3", "e5m2"])
def test_the_poison_shows_when_it_is_read(kv_dtype, entry, variant):
    """The checks above mean something only if a slot that IS read shows in the result.  Here one owned slot -- the
    last token of the 130-token request, the slot an off-by-one clamp would swap for its unowned neighbour -- is
    declared unowned and poisoned: that request's output must come out non-finite or differ from the clean run in its
    bits (the second for an fp8 upcast that maps the NaN code to a number), and the other requests must not change."""
    hq, hkv, d, page, layout = 8, 2, 128, 16, "NHD"
    q_dtype = BF16 if kv_dtype == BF16 else F16
    cache, indptr, indices, last = make_paged(len(UNSPLIT), list(UNSPLIT), page, hkv, d, kv_dtype, layout, seed=251)
    owned = owned_slots(UNSPLIT, indptr, indices, page, cache.shape[0])
    victim = len(UNSPLIT) - 1
    owned[int(indices[int(indptr[victim + 1]) - 1]), (UNSPLIT[victim] - 1) % page] = False
    bad = poison_unowned(cache, layout, owned)
    q = torch.randn(len(UNSPLIT), hq, d, generator=torch.Generator().manual_seed(252)).to(q_dtype)
    with kernel_variant(variant):
        if entry == "decode":
            w = planned_decode_wrapper(DECODE_WS, layout, indptr, indices, last, hq, hkv, d, page,
                                       q_data_type=q_dtype, kv_data_type=kv_dtype, disable_split_kv=True)
        else:  # one query row a request: the prefill kernels on the decode problem
            w = planned_prefill_wrapper(32 << 20, layout, indptr_of([1] * len(UNSPLIT)), indptr, indices, last, hq,
                                        hkv, d, page, causal=True, q_data_type=q_dtype, kv_data_type=kv_dtype)
        clean = w.run(q.to(DEV), cache.to(DEV))
        dirty = w.run(q.to(DEV), bad.to(DEV))
    torch.cuda.synchronize()
    assert not torch.isfinite(dirty[victim].float()).all() or not same_bits(clean[victim], dirty[victim])
    assert same_bits(clean[:victim], dirty[:victim]) and torch.isfinite(dirty[:victim].float()).all()


@pytest.mark.parametrize("page", [16, 5])
def test_graph_mode_decode_with_surplus_page_ids(page):
    """CUDAGraphBatchDecodeWithPagedKVCacheWrapper whose indices buffer is longer than the plan needs: the entries
    behind indptr[-1] name a valid page full of NaN."""
    import flashinfer

    hq, hkv, d, kv_lens = 8, 2, 128, (1, 15, 17, 33, 130, 700)
    cache, bad, indptr, indices, last, free = paged_pair(kv_lens, page, hkv, d, F16, "NHD", seed=301)
    q = torch.randn(len(kv_lens), hq, d, generator=torch.Generator().manual_seed(302)).half()
    o_ref, lse_ref = R.batch_decode_ref(q.float(), cache.float(), "NHD", indptr, indices, last)
    ws = torch.zeros(DECODE_WS, dtype=torch.uint8, device=DEV)
    indices_buf = torch.full((len(indices) + 37,), free, dtype=torch.int32, device=DEV)
    w = flashinfer.CUDAGraphBatchDecodeWithPagedKVCacheWrapper(
        ws, torch.zeros(len(kv_lens) + 1, dtype=torch.int32, device=DEV), indices_buf,
        torch.zeros(len(kv_lens), dtype=torch.int32, device=DEV), "NHD")
    w.plan(indptr, indices, last, hq, hkv, d, page, q_data_type=F16, kv_data_type=F16)
    assert torch.all(indices_buf[len(indices):] == free) and torch.equal(indices_buf[: len(indices)].cpu(), indices)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1
    clean = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    poison_(ws)
    dirty = w.run(q.to(DEV), bad.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, tol(F16))
    assert touched(ws)


@pytest.mark.parametrize("page", [16, 5])
def test_sink_decode(page):
    """One decode case with attention sinks (bars of tests/test_attention_sink_gpu.py), split: the sinks fold in the
    merge launch, over partial states that sit in the poisoned workspace."""
    hq, hkv, d = 8, 2, 128
    cache, bad, indptr, indices, last, _ = paged_pair(TWO_LAUNCH, page, hkv, d, BF16, "NHD", seed=311)
    q = torch.randn(len(TWO_LAUNCH), hq, d, generator=torch.Generator().manual_seed(312)).bfloat16()
    sinks = torch.linspace(-4.0, 6.0, hq)
    sinks[1] = float("-inf")
    o_ref, lse_ref = sink_ref.batch_decode_sink_ref(q.float(), cache.float(), "NHD", indptr, indices, last, sinks)
    w = planned_decode_wrapper(DECODE_WS, "NHD", indptr, indices, last, hq, hkv, d, page, q_data_type=BF16,
                               kv_data_type=BF16)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 0
    clean = w.run(q.to(DEV), cache.to(DEV), sinks=sinks.to(DEV), return_lse=True)
    poison_(w._float_workspace_buffer)
    dirty = w.run(q.to(DEV), bad.to(DEV), sinks=sinks.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, tol(BF16))
    assert touched(w._float_workspace_buffer)


# ---- paged prefill --------------------------------------------------------------------------------------------------

QO_KV = [(1, 1), (5, 17), (33, 33), (7, 130), (64, 257)]
QO_LENS, KV_LENS = [a for a, _ in QO_KV], [b for _, b in QO_KV]


def prefill_case(d, page, layout, dtype, causal, seed, hq=8, hkv=2, qo_lens=QO_LENS, kv_lens=KV_LENS, expect_split=None,
                 ws_bytes=32 << 20, **plan_kw):
    """Paged prefill run clean (zeroed workspace) and poisoned (0xFF cache slots and 0xFF workspace; plan() leaves the
    float workspace alone, csrc/prefill.hip, so it is poisoned after plan()).  The workspace is written exactly when
    the plan says it splits."""
    cache, bad, indptr, indices, last, _ = paged_pair(kv_lens, page, hkv, d, dtype, layout, seed)
    q = torch.randn(sum(qo_lens), hq, d, generator=torch.Generator().manual_seed(seed + 1)).to(dtype)
    qo_indptr = indptr_of(qo_lens)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), layout, indptr, indices, last,
                                         causal=causal)
    w = planned_prefill_wrapper(ws_bytes, layout, qo_indptr, indptr, indices, last, hq, hkv, d, page, causal=causal,
                                q_data_type=dtype, kv_data_type=dtype, **plan_kw)
    split = int(w._plan_info[_lib.FI_PP_SPLIT_KV])
    if expect_split is not None:
        assert split == expect_split
    clean = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    poison_(w._float_workspace_buffer)
    dirty = w.run(q.to(DEV), bad.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, ptol(dtype))
    assert touched(w._float_workspace_buffer) == bool(split)
    return dirty


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d,page,layout", [(64, 16, "NHD"), (128, 5, "HND"), (256, 16, "HND"), (128, 16, "NHD"),
                                           (64, 5, "NHD"), (256, 5, "NHD")])
def test_paged_prefill(d, page, layout, causal, dtype):
    prefill_case(d, page, layout, dtype, causal, seed=400 + d + page)


@pytest.mark.parametrize("case", ["page_1", "fixed_split_size_64", "disable_split_kv", "rows_without_keys"])
def test_paged_prefill_other_plans(case):
    if case == "page_1":  # no tails, only free pages
        prefill_case(128, 1, "HND", F16, True, seed=411)
    elif case == "fixed_split_size_64":
        prefill_case(128, 5, "NHD", BF16, True, seed=412, expect_split=1, fixed_split_size=64)
    elif case == "disable_split_kv":
        prefill_case(128, 16, "HND", F16, True, seed=413, expect_split=0, disable_split_kv=True)
    else:
        # causal with qo_len > kv_len (tests/test_prefill_gpu.py): the first 100 rows see no key in any chunk, and
        # some (row, chunk) pairs of the later rows see none either -- their slots are skipped or written empty,
        # never left to whatever the workspace held
        o, lse = prefill_case(128, 16, "NHD", F16, True, seed=414, hq=4, hkv=1, qo_lens=[700], kv_lens=[600],
                              expect_split=1, ws_bytes=256 << 20, fixed_split_size=128)
        assert torch.all(o[:100] == 0) and torch.all(lse[:100] == R.NEG_INF_SENTINEL)


@pytest.mark.parametrize("f8", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_paged_prefill_fp8_native(f8):
    """q, k and v all fp8 at head_dim 128 (the fp8-native kernel), at the fp8 bars of tests/test_prefill_gpu.py: 5e-2
    (e4m3) / 1e-1 (e5m2) against the oracle's restatement of the reference's fp8 arithmetic, lse rtol 1e-3 atol 2e-3."""
    hq, hkv, d, page = 8, 2, 128, 16
    cache, bad, indptr, indices, last, _ = paged_pair(KV_LENS, page, hkv, d, f8, "NHD", seed=421)
    q8 = torch.randn(sum(QO_LENS), hq, d, generator=torch.Generator().manual_seed(422)).to(f8)
    qo_indptr = indptr_of(QO_LENS)
    one_q, one_kv = torch.ones(hq), torch.ones(hkv)
    refs = []
    for b in range(len(KV_LENS)):
        k, v = R.gather_paged_kv(cache.float(), "NHD", indptr, indices, last, b)  # fp8 values are exact in f32
        refs.append(R.fp8_attention_ref(q8[int(qo_indptr[b]): int(qo_indptr[b + 1])], k.to(f8), v.to(f8), one_q,
                                        one_kv, one_kv, causal=True))
    o_ref, lse_ref = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    w = planned_prefill_wrapper(32 << 20, "NHD", qo_indptr, indptr, indices, last, hq, hkv, d, page, causal=True,
                                q_data_type=f8, kv_data_type=f8, o_data_type=F16)
    # 257 keys at most: one pass prices under any split (price_kv_chunk, csrc/prefill.hip), so this is the one-launch
    # form of the fp8-native kernel; its split form runs in tests/test_prefill_gpu.py
    split = int(w._plan_info[_lib.FI_PP_SPLIT_KV])
    assert split == 0
    clean = w.run(q8.to(DEV), cache.to(DEV), return_lse=True)
    poison_(w._float_workspace_buffer)
    dirty = w.run(q8.to(DEV), bad.to(DEV), return_lse=True)
    bar = 5e-2 if f8 == E4M3 else 1e-1
    check_pair(clean, dirty, o_ref, lse_ref, dict(rtol=bar, atol=bar), dict(rtol=1e-3, atol=2e-3))
    assert touched(w._float_workspace_buffer) == bool(split)


def test_paged_prefill_custom_mask_pad_bits():
    """A packed custom mask whose pad bits -- behind each request's last mask bit up to its byte boundary -- are set,
    in a buffer that goes on behind the last request's mask with every bit set: the result of the clean mask, on the
    poisoned cache (bars of tests/test_custom_mask_gpu.py)."""
    import flashinfer

    hq, hkv, d, page = 8, 2, 128, 5
    cache, bad, indptr, indices, last, _ = paged_pair(KV_LENS, page, hkv, d, F16, "NHD", seed=431)
    g = torch.Generator().manual_seed(432)
    q = torch.randn(sum(QO_LENS), hq, d, generator=g).half()
    masks = []
    for ql, kl in QO_KV:
        m = torch.rand(ql, kl, generator=g) < 0.7
        m[:, 0] = True
        masks.append(m.view(-1))
    mask = torch.cat(masks)
    bits = [a * b for a, b in QO_KV]
    assert sum(1 for n in bits if n % 8) >= 3  # requests whose mask ends inside a byte
    qo_indptr = indptr_of(QO_LENS)
    o_ref, lse_ref = R.batch_prefill_ref(q.float(), qo_indptr, cache.float(), "NHD", indptr, indices, last,
                                         custom_mask=mask)
    packed, byte_indptr = flashinfer.segment_packbits(mask.to(DEV), indptr_of(bits).to(DEV), bitorder="little")
    dirty_mask = torch.cat([packed, torch.full((64,), 0xFF, dtype=torch.uint8, device=DEV)])
    for b, n in enumerate(bits):
        if n % 8:  # little bit order: bit i of a byte is mask entry 8 * byte + i
            dirty_mask[int(byte_indptr[b + 1]) - 1] |= (0xFF << (n % 8)) & 0xFF
    assert not torch.equal(dirty_mask[: len(packed)], packed)
    runs = []
    for m, c in ((packed, cache), (dirty_mask, bad)):
        w = planned_prefill_wrapper(32 << 20, "NHD", qo_indptr, indptr, indices, last, hq, hkv, d, page,
                                    packed_custom_mask=m, q_data_type=F16)
        if c is bad:
            poison_(w._float_workspace_buffer)  # after plan(), which leaves it alone
        runs.append(w.run(q.to(DEV), c.to(DEV), return_lse=True))
    check_pair(runs[0], runs[1], o_ref, lse_ref, dict(rtol=1e-3, atol=1e-3))
    # 257 keys at most: the planner leaves every request whole, and the mask kernel writes the output directly
    assert w._plan_info[_lib.FI_PP_SPLIT_KV] == 0 and not touched(w._float_workspace_buffer)


# ---- ragged prefill -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d_qk,d_vo", [(128, 128), (64, 64), (192, 128)], ids=["d128", "d64", "d192_128"])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("plan", ["default", "fixed_split_size_64"])
def test_ragged_prefill_with_padding_rows(plan, layout, d_qk, d_vo):
    """k and v longer than kv_indptr[-1] (graph padding), the surplus rows NaN.  run() takes q of exactly
    qo_indptr[-1] rows, so q is the head of a longer buffer whose surplus rows are NaN.  192/128 is the kernel of
    prefill_qkvo_kernel.h.  fixed_split_size_64: the partial states go through the poisoned workspace."""
    import flashinfer

    hq, hkv, pad, dtype = 8, 2, 40, F16
    g = torch.Generator().manual_seed(500 + d_qk)
    q_buf = torch.randn(sum(QO_LENS) + pad, hq, d_qk, generator=g).to(dtype)
    k_buf = torch.randn(sum(KV_LENS) + pad, hkv, d_qk, generator=g).to(dtype)
    v_buf = torch.randn(sum(KV_LENS) + pad, hkv, d_vo, generator=g).to(dtype)
    q, k, v = q_buf[: sum(QO_LENS)], k_buf[: sum(KV_LENS)], v_buf[: sum(KV_LENS)]
    qo_indptr, kv_indptr = indptr_of(QO_LENS), indptr_of(KV_LENS)
    refs = [R.attention_ref(q[int(qo_indptr[b]): int(qo_indptr[b + 1])].float(),
                            k[int(kv_indptr[b]): int(kv_indptr[b + 1])].float(),
                            v[int(kv_indptr[b]): int(kv_indptr[b + 1])].float(), causal=True) for b in range(len(QO_KV))]
    o_ref, lse_ref = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])

    def on_device(buf, rows, poisoned):
        t = buf.clone()
        if poisoned:
            poison_(t[rows:])
        t = t.to(DEV)
        return t if layout == "NHD" else t.transpose(0, 1).contiguous()

    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, layout)
    kw = dict(fixed_split_size=64) if plan == "fixed_split_size_64" else {}
    w.plan(qo_indptr.to(DEV), kv_indptr.to(DEV), hq, hkv, d_qk, head_dim_vo=d_vo, causal=True, q_data_type=dtype, **kw)
    split = int(w._plan_info[_lib.FI_PP_SPLIT_KV])
    if kw:
        assert split == 1
    runs = []
    for poisoned in (False, True):
        if poisoned:
            poison_(ws)  # plan() leaves the float workspace alone
        qd = q_buf.clone()
        if poisoned:
            poison_(qd[sum(QO_LENS):])
        runs.append(w.run(qd.to(DEV)[: sum(QO_LENS)], on_device(k_buf, sum(KV_LENS), poisoned),
                          on_device(v_buf, sum(KV_LENS), poisoned), return_lse=True))
    check_pair(runs[0], runs[1], o_ref, lse_ref, ptol(dtype))
    assert touched(ws) == bool(split)


# ---- MLA: the workspace (the cache side is tests/test_mla_gpu.py::test_mla_nan_past_kv_len) -----------------------------

@pytest.mark.parametrize("page", [16, 5, 1])
def test_mla_split_plan_on_a_poisoned_workspace(page):
    """257 tokens is the smallest kv_len the MLA planner splits: chunks are cut at 256 tokens and up (kMlaMinChunk,
    csrc/mla.hip), 256 tokens are one chunk.  The clean run has a clean cache and a zeroed workspace; the poisoned run
    the same cache with every unowned slot NaN and a workspace of NaN.  plan() leaves the float workspace alone (it
    reads its size), so the workspace is poisoned after plan()."""
    import flashinfer
    from test_mla_gpu import SM, check, make_case, plan_run

    whole = make_case([256], [1], 16, page, BF16, seed=31)
    assert plan_run(whole, False, SM)[0]._plan_info[_lib.FI_MLA_SPLIT_KV] == 0
    one = make_case([257], [1], 16, page, BF16, seed=33)
    assert plan_run(one, False, SM)[0]._plan_info[_lib.FI_MLA_SPLIT_KV] == 1
    args = ([257, 700, 17], [1, 2, 1], 16, page, BF16)
    cases = [make_case(*args, seed=32, spare_pages=3), make_case(*args, seed=32, nan_fill=True, spare_pages=3)]
    assert not cases[0]["ckv"].isnan().any() and cases[1]["ckv"].isnan().any() and cases[1]["kpe"].isnan().any()
    for causal in (False, True):
        outs = []
        for c, poisoned in zip(cases, (False, True)):
            ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
            w = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, backend="fa2")
            w.plan(c["qo_indptr"].to(DEV), c["kv_indptr"].to(DEV), c["kv_indices"].to(DEV), c["kv_len_arr"].to(DEV),
                   c["H"], 512, 64, c["page_size"], causal, SM, BF16, BF16)
            assert w._plan_info[_lib.FI_MLA_SPLIT_KV] == 1
            if poisoned:
                poison_(ws)
            outs.append(w.run(c["q_nope"], c["q_pe"], c["ckv"], c["kpe"], return_lse=True))
            torch.cuda.synchronize()
            assert touched(ws) or not poisoned
        assert torch.isfinite(outs[1][0].float()).all() and torch.isfinite(outs[1][1]).all()
        check(cases[1], *outs[1], causal, SM)
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])


# ---- sparse ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["small", "long_rows"])
def test_block_sparse_ignores_unreferenced_column_blocks(shape):
    """BlockSparseAttentionWrapper with column blocks no block row references: exactly their K/V rows are NaN, and the
    workspace is NaN after plan() (which leaves it alone).  long_rows: two block rows over 8192 tokens, which the
    planner splits."""
    import flashinfer

    if shape == "small":
        R_, C, M, N, hq, hkv, d = 16, 16, 72, 256, 4, 2, 128  # M % R != 0
        rows = [[0, 5, 3], [], [15, 1, 2, 9, 8, 12], [4, 5], [10]]
    else:
        R_, C, M, N, hq, hkv, d = 16, 64, 32, 8192, 1, 1, 128
        rows = [[b for b in range(128) if b % 16 != 7], [b for b in reversed(range(128)) if b % 16 != 7]]
    g = torch.Generator().manual_seed(600 + M)
    q = torch.randn(M, hq, d, generator=g).half()
    k, v = torch.randn(N, hkv, d, generator=g).half(), torch.randn(N, hkv, d, generator=g).half()
    indptr, indices = indptr_of(len(r) for r in rows), torch.tensor(sum(rows, []), dtype=torch.int32)
    free = sorted(set(range(N // C)) - set(indices.tolist()))
    assert len(free) >= 3
    kb, vb = k.clone(), v.clone()
    for b in free:
        poison_(kb[b * C: (b + 1) * C])
        poison_(vb[b * C: (b + 1) * C])
    o_ref, lse_ref = sparse_ref.bsr_attention_gathered(q, k, v, indptr, indices, R_, C)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BlockSparseAttentionWrapper(ws)
    w.plan(indptr.to(DEV), indices.to(DEV), M, N, R_, C, hq, hkv, d, q_data_type=F16, o_data_type=F16)
    split = int(w._prefill._plan_info[_lib.FI_PP_SPLIT_KV])
    assert w._active is w._prefill and (split == 1 or shape == "small")
    clean = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    poison_(ws)
    dirty = w.run(q.to(DEV), kb.to(DEV), vb.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, ptol(F16))
    assert touched(ws) == bool(split)


def test_block_sparse_decode_route_ignores_unreferenced_column_blocks():
    """R = 1 (one block row is one decode request) over a K/V whose unreferenced column blocks are NaN."""
    import flashinfer

    R_, C, M, N, hq, hkv, d = 1, 16, 4, 1024, 8, 2, 128
    rows = [[3, 60, 1], [], [b for b in range(64) if b % 8 != 5], [17]]
    g = torch.Generator().manual_seed(611)
    q = torch.randn(M, hq, d, generator=g).half()
    k, v = torch.randn(N, hkv, d, generator=g).half(), torch.randn(N, hkv, d, generator=g).half()
    indptr, indices = indptr_of(len(r) for r in rows), torch.tensor(sum(rows, []), dtype=torch.int32)
    kb, vb = k.clone(), v.clone()
    for b in sorted(set(range(N // C)) - set(indices.tolist())):
        poison_(kb[b * C: (b + 1) * C])
        poison_(vb[b * C: (b + 1) * C])
    assert kb.isnan().any()
    o_ref, lse_ref = sparse_ref.bsr_attention_gathered(q, k, v, indptr, indices, R_, C)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.BlockSparseAttentionWrapper(ws)
    w.plan(indptr.to(DEV), indices.to(DEV), M, N, R_, C, hq, hkv, d, q_data_type=F16, o_data_type=F16)
    assert w._active is w._decode
    split = int(w._decode._plan_info[_lib.FI_DP_SPLIT_KV])
    clean = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    poison_(ws)
    dirty = w.run(q.to(DEV), kb.to(DEV), vb.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, tol(F16))
    assert touched(ws) or not split


@pytest.mark.parametrize("shape", ["small", "long_rows"])
def test_variable_block_sparse_ignores_an_all_false_column(shape):
    """VariableBlockSparseAttentionWrapper with a block_mask_map column that is false in every block row of a head:
    exactly that head's K/V rows of the column are NaN; the workspace is NaN after plan().  long_rows: 7168 of 8192
    tokens a block row, which the planner splits."""
    import flashinfer

    if shape == "small":
        hkv, group, d = 2, 2, 128
        row_sz = torch.tensor([[1, 70, 29], [40, 59, 1]], dtype=torch.int32)
        col_sz = torch.tensor([[70, 1, 33, 16, 10], [5, 64, 1, 30, 30]], dtype=torch.int32)
        block_map = torch.tensor([[[1, 0, 1, 0, 1], [0, 0, 0, 0, 0], [1, 0, 1, 1, 1]],
                                  [[1, 1, 1, 0, 0], [1, 1, 0, 0, 1], [0, 1, 1, 0, 1]]], dtype=torch.bool)
        dead = [(0, 1), (1, 3)]  # (kv head, column block) no block row selects
    else:
        hkv, group, d = 1, 1, 128
        row_sz = torch.tensor([[16, 16]], dtype=torch.int32)
        col_sz = torch.tensor([[2048, 1024, 2048, 1024, 1024, 1024]], dtype=torch.int32)
        block_map = torch.ones(1, 2, 6, dtype=torch.bool)
        block_map[0, :, 1] = False
        dead = [(0, 1)]
    qo_len, kv_len = int(row_sz[0].sum()), int(col_sz[0].sum())
    g = torch.Generator().manual_seed(620 + kv_len)
    q = torch.randn(hkv * group, qo_len, d, generator=g).half()
    k, v = torch.randn(hkv, kv_len, d, generator=g).half(), torch.randn(hkv, kv_len, d, generator=g).half()
    kb, vb = k.clone(), v.clone()
    for h, c in dead:
        assert not block_map[h, :, c].any()
        lo = int(col_sz[h, :c].sum())
        poison_(kb[h, lo: lo + int(col_sz[h, c])])
        poison_(vb[h, lo: lo + int(col_sz[h, c])])
    o_ref, lse_ref = sparse_ref.variable_block_attention(q, k, v, block_map, row_sz, col_sz)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.VariableBlockSparseAttentionWrapper(ws)
    w.plan(block_map.to(DEV), row_sz.to(DEV), col_sz.to(DEV), hkv * group, hkv, d)
    split = int(w._prefill._plan_info[_lib.FI_PP_SPLIT_KV])
    assert split == 1 or shape == "small"
    clean = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    poison_(ws)
    dirty = w.run(q.to(DEV), kb.to(DEV), vb.to(DEV), return_lse=True)
    check_pair(clean, dirty, o_ref, lse_ref, ptol(F16))
    assert touched(ws) == bool(split)


# ---- cascade --------------------------------------------------------------------------------------------------------

def test_three_level_cascade_on_a_poisoned_cache_and_workspace():
    """Seed 0 of tests/test_page_cascade_gpu.py's random three-level problem.  A slot is owned when any level's table
    holds a token in it.  The wrapper hands ONE float buffer to all its levels; no level's plan() writes it, so it is
    poisoned after plan()."""
    import flashinfer

    cache, q, plan_args, plan_kw, check = three_level_problem(0)
    (_, kv_indptr, kv_indices, last), ps = plan_args[:4], plan_args[7]
    owned = torch.zeros(cache.shape[0], ps, dtype=torch.bool)
    for ip, ix, lp in zip(kv_indptr, kv_indices, last):
        owned |= owned_slots(R.get_seq_lens(ip, lp, ps).tolist(), ip, ix, ps, cache.shape[0])
    bad = poison_unowned(cache, "NHD", owned)
    assert int((~owned).all(1).sum()) >= 2  # the two spare pages, and every tail
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.MultiLevelCascadeAttentionWrapper(3, ws, "NHD")
    plan_cascade(w, plan_args, plan_kw)
    clean = w.run(q.to(DEV), cache.to(DEV))
    poison_(ws)
    dirty = w.run(q.to(DEV), bad.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(dirty.float()).all()
    check(dirty)
    assert same_bits(clean, dirty)
    # the cache side only: no level of this small problem splits, so the shared buffer is never used (the next test)
    assert not any(p._plan_info[_lib.FI_PP_SPLIT_KV] for p in w._batch_prefill_wrappers) and not touched(ws)


def test_three_level_cascade_whose_shared_levels_split():
    """The workspace side of MultiLevelCascadeAttentionWrapper, which hands ONE float buffer to all its levels: two
    decode-like requests over an 8192-token global level and a 4096-token group level, both of which the planner
    splits (few rows on long keys), and short unique suffixes.  Each level writes its partial states to the same
    buffer and merges them before the next level runs.  Cache and workspace are poisoned as above; bars of
    tests/test_page_cascade_gpu.py."""
    import flashinfer

    hq, hkv, d, ps = 8, 2, 128, 16
    level_lens = [[8192], [4096], [33, 70]]
    g = torch.Generator().manual_seed(711)
    pages = [[-(-n // ps) for n in lens] for lens in level_lens]
    total = sum(sum(p) for p in pages)
    cache = torch.randn(total + 3, 2, ps, hkv, d, generator=g).half()
    perm = torch.randperm(total + 3, generator=g)[:total].to(torch.int32)
    q = torch.randn(2, hq, d, generator=g).half()
    kv_indptr = [indptr_of(p) for p in pages]
    kv_indices = list(perm.split([sum(p) for p in pages]))
    last = [torch.tensor([(n - 1) % ps + 1 for n in lens], dtype=torch.int32) for lens in level_lens]
    qo_indptr = [torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32),
                 torch.tensor([0, 1, 2], dtype=torch.int32)]
    owned = torch.zeros(total + 3, ps, dtype=torch.bool)
    for lens, ip, ix in zip(level_lens, kv_indptr, kv_indices):
        owned |= owned_slots(lens, ip, ix, ps, total + 3)
    bad = poison_unowned(cache, "NHD", owned)
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    w = flashinfer.MultiLevelCascadeAttentionWrapper(3, ws, "NHD")
    plan_cascade(w, (qo_indptr, kv_indptr, kv_indices, last, hq, hkv, d, ps), dict(causal=True, q_data_type=F16))
    splits = [int(p._plan_info[_lib.FI_PP_SPLIT_KV]) for p in w._batch_prefill_wrappers]
    assert splits[0] == 1 and splits[1] == 1
    clean = w.run(q.to(DEV), cache.to(DEV))
    poison_(ws)
    dirty = w.run(q.to(DEV), bad.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(dirty.float()).all() and touched(ws)

    def rows(level, b):
        lo, hi = int(kv_indptr[level][b]), int(kv_indptr[level][b + 1])
        kv = cache[kv_indices[level][lo:hi].long()].float()
        n = level_lens[level][b]
        return kv[:, 0].reshape(-1, hkv, d)[:n], kv[:, 1].reshape(-1, hkv, d)[:n]

    for r in range(2):  # flat attention over [global | group | unique]; one query row, so causal hides nothing
        parts = [rows(0, 0), rows(1, 0), rows(2, r)]
        o_ref, _ = R.attention_ref(q[r:r + 1].float(), torch.cat([p[0] for p in parts]),
                                   torch.cat([p[1] for p in parts]), causal=True)
        torch.testing.assert_close(dirty[r:r + 1].float().cpu(), o_ref.float(), rtol=2e-3, atol=2e-3)
    assert same_bits(clean, dirty)


@pytest.mark.parametrize("wrapper", ["decode", "prefill"])
def test_shared_prefix_wrappers_on_a_poisoned_cache_and_workspace(wrapper):
    """BatchDecode / BatchPrefillWithSharedPrefixPagedKVCacheWrapper (bars of tests/test_page_cascade_gpu.py): the
    unique suffixes sit in a cache whose unowned slots are NaN, the workspace is NaN after the plan (begin_forward of
    the prefill form only records its arguments; the plan happens in the first forward(), on a workspace it leaves
    alone), and so is the cached scratch of the single prefill that attends the shared prefix.  The 3000-token suffix
    makes the batch plan split, the 8192-token prefix makes the single prefill split: both buffers are used."""
    import flashinfer
    from flashinfer.utils import _get_cache_buf

    batch, prefix_len, hq, hkv, d, ps = 5, 8192, 8, 2, 128, 16
    suffix_lens = [9, 16, 31, 2, 3000]
    qo_lens = [1] * batch if wrapper == "decode" else [9, 5, 31, 1, 64]
    cache, sh_idx, un_idx, un_indptr, un_last, _ = _two_level_problem(batch, prefix_len, suffix_lens, hq, hkv, d, ps, 5)
    q = torch.randn(sum(qo_lens), hq, d, generator=torch.Generator().manual_seed(701)).half()
    qo_indptr = indptr_of(qo_lens)
    k_shared = cache[sh_idx.long(), 0].reshape(-1, hkv, d).contiguous()
    v_shared = cache[sh_idx.long(), 1].reshape(-1, hkv, d).contiguous()
    # the shared pages are read as dense rows; in the paged cache only the suffixes are owned
    bad = poison_unowned(cache, "NHD", owned_slots(suffix_lens, un_indptr, un_idx, ps, cache.shape[0]))
    refs = []
    for r in range(batch):
        pages = un_idx[int(un_indptr[r]):int(un_indptr[r + 1])].long()
        ku = cache[pages, 0].reshape(-1, hkv, d)[: suffix_lens[r]]
        vu = cache[pages, 1].reshape(-1, hkv, d)[: suffix_lens[r]]
        refs.append(R.attention_ref(q[int(qo_indptr[r]): int(qo_indptr[r + 1])].float(),
                                    torch.cat([k_shared, ku]).float(), torch.cat([v_shared, vu]).float(),
                                    causal=wrapper == "prefill")[0])
    ref = torch.cat(refs)
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device=DEV)
    if wrapper == "decode":
        w = flashinfer.BatchDecodeWithSharedPrefixPagedKVCacheWrapper(ws, "NHD")
        w.begin_forward(un_indptr.to(DEV), un_idx.to(DEV), un_last.to(DEV), hq, hkv, d, ps, data_type="float16")
        forward = lambda c: w.forward(q.to(DEV), k_shared.to(DEV), v_shared.to(DEV), c.to(DEV))
        split = lambda: int(w._batch_decode_wrapper._plan_info[_lib.FI_DP_SPLIT_KV])
    else:
        w = flashinfer.BatchPrefillWithSharedPrefixPagedKVCacheWrapper(ws, "NHD")
        w.begin_forward(qo_indptr.to(DEV), un_indptr.to(DEV), un_idx.to(DEV), un_last.to(DEV), hq, hkv, d, ps)
        forward = lambda c: w.forward(q.to(DEV), k_shared.to(DEV), v_shared.to(DEV), c.to(DEV), causal=True)
        split = lambda: int(w._batch_prefill_wrapper._plan_info[_lib.FI_PP_SPLIT_KV])
    scratch = _get_cache_buf("single_prefill_with_kv_cache_tmp", 32 * 1024 * 1024, torch.device(DEV))
    scratch.zero_()
    clean = forward(cache)
    poison_(ws)
    poison_(scratch)
    dirty = forward(bad)
    torch.cuda.synchronize()
    assert torch.isfinite(dirty.float()).all()
    torch.testing.assert_close(dirty.float().cpu(), ref.float(), rtol=2e-3, atol=2e-3)
    assert same_bits(clean, dirty)
    assert split() == 1 and touched(ws) and touched(scratch)


# ---- the cached scratch of the single-request entry points -------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
def test_single_prefill_on_stale_scratch(causal):
    """8 query rows over 8192 keys at 8/2 heads: single_prefill_with_kv_cache splits the kv axis through its cached
    scratch, which real use always finds stale.  Proof that it split: the scratch is no longer all 0xFF."""
    import flashinfer
    from flashinfer.utils import _get_cache_buf

    g = torch.Generator().manual_seed(801)
    q = torch.randn(8, 8, 128, generator=g).half()
    k, v = torch.randn(8192, 2, 128, generator=g).half(), torch.randn(8192, 2, 128, generator=g).half()
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), causal=causal)
    scratch = _get_cache_buf("single_prefill_with_kv_cache_tmp", 32 * 1024 * 1024, torch.device(DEV))
    run = lambda: flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal,
                                                          return_lse=True)
    scratch.zero_()
    clean = run()
    poison_(scratch)
    dirty = run()
    check_pair(clean, dirty, o_ref, lse_ref, dict(rtol=1e-3, atol=1e-3))
    assert touched(scratch)


@pytest.mark.parametrize("layout", ["NHD", "HND"])
def test_single_decode_on_stale_scratch(layout):
    """One query over 8192 keys at 8/2 heads through the cached scratch of single_decode_with_kv_cache."""
    import flashinfer
    from flashinfer.utils import _get_cache_buf

    g = torch.Generator().manual_seed(811)
    q = torch.randn(8, 128, generator=g).half()
    shape = (8192, 2, 128) if layout == "NHD" else (2, 8192, 128)
    k, v = torch.randn(shape, generator=g).half(), torch.randn(shape, generator=g).half()
    o_ref, lse_ref = R.single_decode_ref(q.float(), k.float(), v.float(), layout)
    scratch = _get_cache_buf("single_decode_with_kv_cache_tmp", 32 * 1024 * 1024, torch.device(DEV))
    run = lambda: flashinfer.single_decode_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), kv_layout=layout,
                                                         return_lse=True)
    scratch.zero_()
    clean = run()
    poison_(scratch)
    dirty = run()
    check_pair(clean, dirty, o_ref, lse_ref, dict(rtol=1e-3, atol=1e-3))
    assert touched(scratch)
