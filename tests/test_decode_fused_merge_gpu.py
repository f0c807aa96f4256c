"""GPU: batch decode with the split-KV merge folded into the decode launch (decode_mfma16_kernel's FUSE form).

A plan whose requests all have exactly 2 or 4 chunks (plan_info[FI_DP_UNIFORM_CHUNKS]) runs as ONE launch on the
16x16x32 kernel when there is no fused RoPE and no sliding window and a workgroup's kv heads still cover 256 bytes of
a token row: the chunks of a (request, kv head) are waves of one workgroup and meet in LDS.  The fused cases check the
result against the CPU oracle at the decode suite's tolerances and that the float workspace (where the two-launch path
keeps its partial states) is left untouched; the fallback cases check that every other plan / run option still gives
the right answer through the two launches.

Shapes: page 16 on the 256-CU grid, where chunks come out at 128 tokens -- the smallest plans that split at all."""
import functools

import pytest
import torch

from attn_inputs import page_table, planned_decode_wrapper, tol
from flashinfer import _lib
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAGE = 16
WS_BYTES = 8 << 20


@functools.lru_cache(maxsize=None)
def case(kv_lens, hq, hkv, d, dtype, kv_dtype=None, layout="NHD", seed=0, q_gain=1.0, **ref_kw_items):
    """Seeded inputs and the oracle's answer, computed once per distinct case and never modified."""
    g = torch.Generator().manual_seed(1000 + seed)
    indptr, indices, last, npages = page_table(kv_lens, PAGE, g, extra_pages=3)
    shape = (npages, 2, PAGE, hkv, d) if layout == "NHD" else (npages, 2, hkv, PAGE, d)
    cache = torch.randn(shape, generator=g).to(kv_dtype or dtype)
    q = (torch.randn(len(kv_lens), hq, d, generator=g) * q_gain).to(dtype)
    o_ref, lse_ref = R.batch_decode_ref(q.float(), cache.float(), layout, indptr, indices, last, **ref_kw_items)
    return q, cache, indptr, indices, last, o_ref.float(), lse_ref.float()


def plan_wrapper(c, hq, hkv, d, layout="NHD", **plan_kw):
    q, cache, indptr, indices, last = c[:5]
    return planned_decode_wrapper(WS_BYTES, layout, indptr, indices, last, hq, hkv, d, PAGE, q_data_type=q.dtype,
                                  kv_data_type=cache.dtype, **plan_kw)


def run_checked(c, hq, hkv, d, dtype, expect_slot, fused, layout="NHD", lse_tol=1e-3, o_tol=None, **plan_kw):
    """plan, poison the float workspace, run, compare with the oracle.  ``fused``: the workspace must come back
    untouched; otherwise (two launches on a split plan) the partial states must have been written to it."""
    q, cache, _, _, _, o_ref, lse_ref = c
    w = plan_wrapper(c, hq, hkv, d, layout, **plan_kw)
    assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == expect_slot and _lib.FI_DP_UNIFORM_CHUNKS == 16
    w._float_workspace_buffer.fill_(0xFF)
    o, lse = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    torch.cuda.synchronize()
    untouched = bool((w._float_workspace_buffer == 0xFF).all())
    if fused:
        assert untouched, "the fused launch must not write partial states"
    elif w._plan_info[_lib.FI_DP_SPLIT_KV]:
        assert not untouched, "a split plan on the two-launch path writes its partial states"
    torch.testing.assert_close(o.float().cpu(), o_ref, **(o_tol or tol(dtype)))
    torch.testing.assert_close(lse.cpu(), lse_ref, rtol=lse_tol, atol=lse_tol)
    return w, o, lse


# ---- fused ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("d", [128, 64])
def test_two_chunks_odd_batch_ragged_tails(dtype, d):
    # 130 tokens: the second chunk holds 2 tokens (last-tile masking, a tiny partial)
    c = case((130, 200, 256), 8, 2, d, dtype, seed=1)
    run_checked(c, 8, 2, d, dtype, expect_slot=2, fused=True)


@pytest.mark.parametrize("batch,hq,hkv", [(2, 8, 2), (1, 4, 1)])
def test_four_chunks(batch, hq, hkv):
    c = case((512,) * batch, hq, hkv, 128, torch.bfloat16, seed=2)
    run_checked(c, hq, hkv, 128, torch.bfloat16, expect_slot=4, fused=True)


@pytest.mark.parametrize("hq,hkv", [(6, 3), (16, 1), (2, 2)])
def test_kv_heads_not_a_multiple_of_the_heads_per_workgroup(hq, hkv):
    # n = 2: two kv heads per workgroup.  3 kv heads and 1 kv head leave a head block with inactive waves, which
    # still have to reach the barrier; 16 / 1 fills all 16 columns, 2 / 2 uses one.
    c = case((256,) * 3, hq, hkv, 128, torch.float16, seed=3)
    run_checked(c, hq, hkv, 128, torch.float16, expect_slot=2, fused=True)


def test_caller_output_without_lse():
    q, cache, _, _, _, o_ref, _ = c = case((256,) * 3, 8, 2, 128, torch.bfloat16, seed=4)
    w = plan_wrapper(c, 8, 2, 128)
    assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 2
    w._float_workspace_buffer.fill_(0xFF)
    out = torch.full(q.shape, float("nan"), dtype=q.dtype, device=DEV)
    got = w.run(q.to(DEV), cache.to(DEV), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((w._float_workspace_buffer == 0xFF).all())
    torch.testing.assert_close(out.float().cpu(), o_ref, **tol(torch.bfloat16))


def test_soft_cap():
    c = case((256,) * 3, 8, 2, 128, torch.bfloat16, seed=5, q_gain=3.0, logits_soft_cap=30.0)
    run_checked(c, 8, 2, 128, torch.bfloat16, expect_slot=2, fused=True, logits_soft_cap=30.0)


def test_alibi():
    c = case((256,) * 3, 8, 2, 128, torch.float16, seed=6, pos_encoding_mode="ALIBI")
    run_checked(c, 8, 2, 128, torch.float16, expect_slot=2, fused=True, pos_encoding_mode="ALIBI")


def test_alibi_and_soft_cap_together():
    # both logit transforms in one fused launch, q x 3 and a cap of 8 so that the cap bites; the lse at the 2e-3 of
    # tests/test_attention_variants_gpu.py
    kw = dict(pos_encoding_mode="ALIBI", logits_soft_cap=8.0)
    c = case((256,) * 3, 8, 2, 128, torch.float16, seed=13, q_gain=3.0, **kw)
    run_checked(c, 8, 2, 128, torch.float16, expect_slot=2, fused=True, lse_tol=2e-3, **kw)


def test_sm_scale_on_four_chunks():
    # a softmax scale away from 1 / sqrt(head_dim): the chunks' partial states meet in LDS in units of that scale
    c = case((512,) * 2, 8, 2, 128, torch.bfloat16, seed=14, sm_scale=0.05)
    run_checked(c, 8, 2, 128, torch.bfloat16, expect_slot=4, fused=True, lse_tol=2e-3, sm_scale=0.05)


def test_fp8_e4m3_cache():
    # the oracle sees the same (already quantised) cache values, so the 16-bit tolerance applies
    c = case((256,) * 3, 8, 2, 128, torch.float16, kv_dtype=torch.float8_e4m3fn, seed=7)
    run_checked(c, 8, 2, 128, torch.float16, expect_slot=2, fused=True)


def test_hnd_layout():
    c = case((256,) * 3, 8, 2, 128, torch.bfloat16, layout="HND", seed=8)
    run_checked(c, 8, 2, 128, torch.bfloat16, expect_slot=2, fused=True, layout="HND")


def test_fused_equals_unsplit():
    """Merge associativity, at the bars of test_full_size_c2_split_invariance."""
    q, cache = (c := case((130, 200, 256), 8, 2, 128, torch.bfloat16, seed=1))[:2]
    _, o_fused, lse_fused = run_checked(c, 8, 2, 128, torch.bfloat16, expect_slot=2, fused=True)
    w = plan_wrapper(c, 8, 2, 128, disable_split_kv=True)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 0 and w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 0
    o_one, lse_one = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    torch.testing.assert_close(o_fused.float(), o_one.float(), **tol(torch.bfloat16))
    torch.testing.assert_close(lse_fused, lse_one, rtol=1e-4, atol=1e-4)


# ---- fallback: two launches, as before ------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_lens", [(256, 512), (384, 384, 384), (0, 256)])
def test_uneven_or_other_chunk_counts_take_two_launches(kv_lens):
    c = case(kv_lens, 8, 2, 128, torch.float16, seed=9)
    _, o, lse = run_checked(c, 8, 2, 128, torch.float16, expect_slot=0, fused=False)
    if kv_lens[0] == 0:
        assert torch.all(o[0] == 0) and torch.all(lse[0].cpu() == R.NEG_INF_SENTINEL)


def test_fused_rope_takes_two_launches():
    # the plan is uniform (the slot says 2), the run condition is off: the RoPE kernel has no FUSE form
    c = case((256,) * 3, 8, 2, 128, torch.float16, seed=10, pos_encoding_mode="ROPE_LLAMA",
             rope_round_dtype=torch.float16)
    # bars of tests/test_decode_gpu.py::test_batch_decode_pos_encoding
    run_checked(c, 8, 2, 128, torch.float16, expect_slot=2, fused=False, pos_encoding_mode="ROPE_LLAMA",
                rope_theta=1e4, rope_scale=1.0, lse_tol=2e-3, o_tol=dict(rtol=1e-3, atol=1e-3))


@pytest.mark.parametrize("d,kv_dtype", [(128, torch.float8_e4m3fn), (64, torch.float16)])
def test_narrow_rows_take_two_launches(d, kv_dtype):
    # n = 4 leaves one kv head per workgroup: 128 bytes of a token row (fp8 at d 128, 16-bit at d 64), under the 256
    # the dispatcher asks for -- the plan is uniform (the slot says 4), the run condition is off
    c = case((512, 512), 8, 2, d, torch.float16, kv_dtype=kv_dtype, seed=12)
    run_checked(c, 8, 2, d, torch.float16, expect_slot=4, fused=False)


def test_graph_plan_takes_two_launches():
    import flashinfer

    q, cache, indptr, indices, last, o_ref, lse_ref = case((256,) * 3, 8, 2, 128, torch.float16, seed=11)
    ws = torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)
    w = flashinfer.CUDAGraphBatchDecodeWithPagedKVCacheWrapper(
        ws, torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(64, dtype=torch.int32, device=DEV),
        torch.empty(3, dtype=torch.int32, device=DEV), "NHD")
    w.plan(indptr, indices, last, 8, 2, 128, PAGE, q_data_type=torch.float16, kv_data_type=torch.float16)
    assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == 0
    w._float_workspace_buffer.fill_(0xFF)
    o, lse = w.run(q.to(DEV), cache.to(DEV), return_lse=True)
    torch.cuda.synchronize()
    assert not bool((w._float_workspace_buffer == 0xFF).all())
    torch.testing.assert_close(o.float().cpu(), o_ref, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(lse.cpu(), lse_ref, rtol=1e-3, atol=1e-3)
