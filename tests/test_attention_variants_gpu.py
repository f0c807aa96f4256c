"""GPU: the attention kernels at logit scalars away from their defaults and with features combined, every case of
tests/variant_cases.py against the fp64 oracle on the same seeded inputs (o and the lse; the plan-free calls return o
only).  tests/test_attention_variants_cpu.py shows with the oracle alone that each moved scalar and each enabled
feature of a case changes its answer by at least 20x the bar used here, so a kernel that rebuilt 1/sqrt(head_dim),
ignored rope_scale, hard-coded theta or applied ALiBi, cap and mask in another order fails.

Bars (variant_cases.bars): tol(dtype) for decode, ptol(dtype) for prefill, 2e-3 on the lse; with fused RoPE both
doubled / 4e-3 (f16) and 2e-2 (bf16) on the lse, and the oracle rounds the rotated q / k to the 16-bit type where the
kernel that runs does (tests/test_fuzz_gpu.py); v_scale multiplies atol, and 0.37 grants one more rounding of the
output; fp8 q / k / v at 5e-2 and rtol 1e-3 / atol 2e-3 on the lse.

Decode cases run under both kernel choices of tests/test_decode_gpu.py (VARIANTS): the default sends groups of <= 16
heads to the 16x16x32 kernel, r1 (FI_DECODE_MFMA16=0) to the VALU kernel or, for plain logits, to the 32x32x16 one.
Every case prints its worst error in units of its bar before it asserts."""
import pytest
import torch

import variant_cases as V
from attn_inputs import planned_decode_wrapper, planned_prefill_wrapper
from flashinfer import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WS_BYTES = 64 << 20

VARIANTS = {"default": {}, "r1": {"FI_DECODE_MFMA16": 0}}


@pytest.fixture
def kernel_variant(request):
    """Sets the switches of a VARIANTS entry for the test, returns every one of them to the environment's value
    afterwards, and hands the test the entry's name."""
    options = VARIANTS[request.param]
    try:
        for name, value in options.items():
            _lib.set_option(name, value)
        yield request.param
    finally:
        for name in options:
            _lib.set_option(name, None)


both_variants = pytest.mark.parametrize("kernel_variant", list(VARIANTS), indirect=True)


def _dev(inp, *names):
    return [inp[n].to(DEV) for n in names]


def _block_table(inp):
    """Dense [batch, max_blocks] block table of the case's CSR page table; entries past a request's pages name page 0,
    which exists and is never read."""
    indptr, indices = inp["indptr"], inp["indices"]
    pages = (indptr[1:] - indptr[:-1]).tolist()
    table = torch.zeros(len(pages), max(max(pages), 1), dtype=torch.int32)
    for b, n in enumerate(pages):
        table[b, :n] = indices[int(indptr[b]): int(indptr[b]) + n]
    return table.to(DEV)


def _dense_kv(inp):
    """k, v [rows, Hkv, D] of the one-token identity pages a ragged or single-request case is built on."""
    cache = inp["cache"]
    return cache[:, 0, 0].contiguous().to(DEV), cache[:, 1, 0].contiguous().to(DEV)


def _extras(case, inp):
    kw = V.run_kw(case)
    if "sinks" in case.features:
        kw["sinks"] = inp["sinks"].to(DEV)
    return kw


# ---- one runner per entry point: (o, lse or None) ------------------------------------------------------------------
def run_batch_decode(case, inp):
    q, cache = _dev(inp, "q", "cache")
    w = planned_decode_wrapper(WS_BYTES, case.layout, inp["indptr"], inp["indices"], inp["last"], case.hq, case.hkv,
                               case.d, case.page_size, q_data_type=q.dtype, kv_data_type=cache.dtype,
                               **V.plan_kw(case))
    if case.split is False:
        assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 0
    elif "window" not in case.features and max(case.kv_lens) >= 2049:
        assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1, "the 2049-token request is expected to split"
    return w.run(q, cache, return_lse=True, **_extras(case, inp))


def run_single_decode(case, inp):
    import flashinfer

    k, v = _dense_kv(inp)
    o, lse = flashinfer.single_decode_with_kv_cache(inp["q"][0].to(DEV), k, v, return_lse=True, **V.plan_kw(case))
    return o[None], lse[None]


def run_trtllm_decode(case, inp):
    from flashinfer.decode import trtllm_batch_decode_with_kv_cache

    q, cache = _dev(inp, "q", "cache")
    table = _block_table(inp)
    s = case.scalar
    o = trtllm_batch_decode_with_kv_cache(
        query=q, kv_cache=cache, workspace_buffer=torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV),
        block_tables=table, seq_lens=torch.tensor(case.kv_lens, dtype=torch.int32, device=DEV),
        max_seq_len=table.shape[1] * case.page_size, bmm1_scale=s["bmm1_scale"], bmm2_scale=s["bmm2_scale"],
        window_left=V.feature_kw(case).get("window_left", -1))
    return o, None


def _mask_kw(case, inp):
    return dict(custom_mask=inp["mask"].to(DEV)) if "mask" in case.features else {}


def run_paged_prefill(case, inp):
    q, cache = _dev(inp, "q", "cache")
    kw = dict(V.plan_kw(case), **_mask_kw(case, inp))
    run = _extras(case, inp)
    if case.entry == "fp8_prefill":
        kw["o_data_type"] = case.dtype
        run.update(scale_q=inp["sq"].to(DEV), scale_k=inp["sk"].to(DEV), scale_v=inp["sv"].to(DEV))
    w = planned_prefill_wrapper(WS_BYTES, case.layout, inp["qo_indptr"], inp["indptr"], inp["indices"], inp["last"],
                                case.hq, case.hkv, case.d, case.page_size, q_data_type=q.dtype,
                                kv_data_type=cache.dtype, **kw)
    if case.split is not None:
        assert w._plan_info[_lib.FI_PP_SPLIT_KV] == int(case.split)
    o, lse = w.run(q, cache, return_lse=True, **run)
    assert o.dtype == case.dtype
    return o, lse


def run_ragged_prefill(case, inp):
    import flashinfer

    k, v = _dense_kv(inp)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV), "NHD")
    # one-token pages: the page indptr is the kv indptr
    w.plan(inp["qo_indptr"].to(DEV), inp["indptr"].to(DEV), case.hq, case.hkv, case.d, q_data_type=case.dtype,
           **V.plan_kw(case), **_mask_kw(case, inp))
    return w.run(inp["q"].to(DEV), k, v, return_lse=True, **V.run_kw(case))


def run_single_prefill(case, inp):
    import flashinfer

    k, v = _dense_kv(inp)
    kw = V.plan_kw(case)
    if "mask" in case.features:
        kw["custom_mask"] = inp["mask"].reshape(case.qo_lens[0], case.kv_lens[0]).to(DEV)
    return flashinfer.single_prefill_with_kv_cache(inp["q"].to(DEV), k, v, return_lse=True, **kw)


def run_trtllm_context(case, inp):
    from flashinfer.prefill import trtllm_batch_context_with_kv_cache

    q, cache = _dev(inp, "q", "cache")
    table = _block_table(inp)
    s = case.scalar
    o = trtllm_batch_context_with_kv_cache(
        query=q, kv_cache=cache, workspace_buffer=torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV),
        block_tables=table, seq_lens=torch.tensor(case.kv_lens, dtype=torch.int32, device=DEV),
        max_q_len=max(case.qo_lens), max_kv_len=table.shape[1] * case.page_size, bmm1_scale=s["bmm1_scale"],
        bmm2_scale=s["bmm2_scale"], batch_size=len(case.kv_lens), cum_seq_lens_q=inp["qo_indptr"].to(DEV),
        cum_seq_lens_kv=None, window_left=V.feature_kw(case).get("window_left", -1))
    return o, None


RUNNERS = dict(batch_decode=run_batch_decode, single_decode=run_single_decode, trtllm_decode=run_trtllm_decode,
               paged_prefill=run_paged_prefill, fp8_prefill=run_paged_prefill, ragged_prefill=run_ragged_prefill,
               single_prefill=run_single_prefill, trtllm_context=run_trtllm_context)


def worst(got, ref, bar):
    """max |got - ref| / (atol + rtol |ref|): the worst error in units of the bar."""
    return float(((got - ref).abs() / (bar["atol"] + bar["rtol"] * ref.abs())).max()) if ref.numel() else 0.0


def check(case, variant="default"):
    o, lse = RUNNERS[case.entry](case, V.inputs(case))
    torch.cuda.synchronize()
    o_ref, lse_ref = (t.float() for t in V.oracle(case, variant=variant))
    o_bar, lse_bar = V.bars(case)
    o = o.float().cpu()
    line = f"variant-error {case.name} [{variant}] o {worst(o, o_ref, o_bar):.3f}"
    if lse is not None:
        line += f" lse {worst(lse.cpu(), lse_ref, lse_bar):.3f}"
    print(line + " of the bar")
    torch.testing.assert_close(o, o_ref, **o_bar)
    if lse is not None:
        torch.testing.assert_close(lse.cpu(), lse_ref, **lse_bar)
    if case.dead_rows and "sinks" not in case.features:
        dead = lse_ref < -4e4
        assert int(dead.any(dim=1).sum()) == case.dead_rows
        assert float(o[dead.any(dim=1)].abs().max()) == 0.0


def _of(cases, decode):
    return [c for c in cases if c.is_decode == decode]


# ---- A. scalars ----------------------------------------------------------------------------------------------------
@both_variants
@pytest.mark.parametrize("case", _of(V.SCALAR_CASES, True), ids=str)
def test_decode_scalars(case, kernel_variant):
    """sm_scale, rope_theta, rope_scale, q_scale, k_scale and v_scale, each alone and all together, on the batch
    wrapper (group 4 and group 20 at head_dim 128, head_dim 256: the three decode kernels between the two kernel
    choices) and on single_decode_with_kv_cache; k_scale / v_scale over an e4m3 cache; bmm1_scale / bmm2_scale on the
    plan-free call."""
    check(case, kernel_variant)


@pytest.mark.parametrize("case", _of(V.SCALAR_CASES, False), ids=str)
def test_prefill_scalars(case):
    """The same scalars on the paged and ragged wrappers and on single_prefill_with_kv_cache, and the forms whose
    algebra involves the scale: ALiBi alone with sm_scale 0.05 (GEN 1 folds the slope into units of 1/qk_scale), a cap
    with sm_scale, RoPE with theta and scale; k_scale / v_scale over an e4m3 cache; the plan-free call."""
    check(case)


# ---- B. combinations -----------------------------------------------------------------------------------------------
@both_variants
@pytest.mark.parametrize("case", V.DECODE_COMBO_CASES, ids=str)
def test_decode_combinations(case, kernel_variant):
    """RoPE+cap, RoPE+window, ALiBi+cap, ALiBi+window, ALiBi+cap+window and cap+window over groups 1 / 4 / 7 / 16 / 20,
    head_dim 64 / 128 / 256, 16-bit and e4m3 caches, page sizes 1 / 5 / 16; sinks on top of a cap; a request without
    keys."""
    check(case, kernel_variant)


@pytest.mark.parametrize("case", V.PREFILL_COMBO_CASES, ids=str)
def test_prefill_combinations(case):
    """Two or three of ALiBi / cap / mask, and RoPE with cap and / or mask, with and without a window (GEN 15), over
    head_dim 64 / 128 / 256, f16 and bf16 (one case with P as hi + lo halves), 16-bit and e4m3 caches, unsplit and
    split; sinks with a combination (unsplit: the SINK form of GEN 15; split: folded in the merge); fp8 q / k / v with
    a window, a cap, and mask + cap (the upcast kernel)."""
    check(case)
