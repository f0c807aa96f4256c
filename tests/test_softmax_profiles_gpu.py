"""GPU: every attention kernel on inputs whose logits are prescribed (tests/logit_profiles.py), against the fp64 oracle.

The randn grids of the other files leave the row maximum where the first KV tile put it.  Here it moves: up and down by
whole tiles on both sides of the deferred-rescale thresholds, inside every tile, at tile and split-chunk boundaries, on
some rows of a wave only, under a saturated soft cap, and at logit offsets of +-2000 and -30000 nats (-43 281 in the
base-2 units of the lse, next to the "saw no key" sentinel -5e4).  Shapes are the smallest that still cross tiles, chunks
and head packings: kv 333 (five 64-key tiles, the last partial), qo 150, page 16 with a shuffled page table.

Bars: each path keeps the bar its own test file uses for that kernel and type (tol / ptol of attn_inputs.py, the fp8
bars of test_prefill_gpu.py, the MLA file's, V_BAR of test_merge_gpu.py; lse rtol = atol = 1e-3).  The offset profiles
are measured against the f32 evaluation of the oracle, never against the kernel: output atol = max(the file's,
4 x |o_f32oracle - o_f64oracle|max), lse rtol = 0 and atol = max(the file's, 4 x |lse_f32oracle - lse_f64oracle|max) --
the file's rtol at |lse| = 4e4 would hide tens of units; 4 x is the margin of _f32_bar in test_merge_gpu.py for "f32 as
well, summed in another order".  Both are computed per case.  No case is skipped and no element is masked out.

Every test loops its profiles, collects what misses its bar, prints the worst figures of its path and fails at the end
with the whole list.  The docstrings give the worst |got - oracle| measured on the MI355X as "o / lse", and for the
offset profiles as "offset o / lse"; 9.8e-4 and 7.8e-3 in o are half an f16 / bf16 ulp of an output in [2, 4), and
3.9e-3 in an offset lse is one f32 ulp (2^-8) at 43 000.  The offset bars came out at o 2.2e-4 and lse 1.2e-3 for
+-2000 (so the file's 1e-3 holds for o) and o 3.8e-3 and lse 2.0e-2 for -30000.  The soft-cap profile runs wherever the entry point takes a soft cap (not MLA, not 192/128).  Fused
RoPE changes the logits, so a profile would have to be built for the rotated vectors: RoPE is left out here."""
import functools

import pytest
import torch

import logit_profiles as LP
from attn_inputs import indptr_of, page_table, planned_decode_wrapper, planned_prefill_wrapper, ptol, scatter_to_pages, tol
from flashinfer import _lib
from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAGE = 16
LSE_TOL = dict(rtol=1e-3, atol=1e-3)
F16, BF16 = torch.float16, torch.bfloat16
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
ids = lambda x: str(x).replace("torch.", "")  # noqa: E731


class Tally:
    """Compares like torch.testing.assert_close (|got - ref| <= atol + rtol |ref|, nothing non-finite), but goes on to
    the next profile after a miss and keeps the worst figures, apart for the offset profiles."""

    def __init__(self, path):
        self.path, self.fails, self.worst = path, [], {}

    def close(self, what, tag, got, ref, rtol, atol):
        got, ref = got.float().cpu(), ref.float()
        err = (got - ref).abs()
        worst = err.max().item() if err.numel() else 0.0
        self.worst[what] = max(self.worst.get(what, 0.0), worst)
        if got.shape != ref.shape or not torch.isfinite(got).all() or bool((err > atol + rtol * ref.abs()).any()):
            over = (err - (atol + rtol * ref.abs())).max().item() if err.numel() else float("nan")
            atol = atol.max().item() if torch.is_tensor(atol) else atol
            self.fails.append(f"{self.path} {tag}: {what} max err {worst:.3e}, over the bar (rtol {rtol:.2e}, atol "
                              f"{atol:.2e}) by {over:.3e}, finite={bool(torch.isfinite(got).all())}")

    def check(self, tag, o, lse, ref, o_tol, lse_tol=LSE_TOL, o_atol=None):
        """o_atol: a per-element absolute bar, used where it exceeds o_tol's."""
        o_ref, lse_ref, extra = ref
        sfx = ""
        if extra is not None:  # an offset profile: the f32 oracle's own error widens the absolute bars
            sfx = " (offset)"
            o_tol = dict(rtol=o_tol["rtol"], atol=max(o_tol["atol"], extra[0]))
            lse_tol = dict(rtol=0.0, atol=max(lse_tol["atol"], extra[1]))
        if o_atol is not None:
            o_tol = dict(rtol=o_tol["rtol"], atol=o_atol.clamp(min=o_tol["atol"]))
        self.close("o" + sfx, tag, o, o_ref, **o_tol)
        if lse is not None:
            self.close("lse" + sfx, tag, lse, lse_ref, **lse_tol)

    def finish(self):
        print(f"\n[{self.path}] worst: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(self.worst.items())))
        assert not self.fails, f"{len(self.fails)} misses:\n" + "\n".join(self.fails)


def oracle(q, k, v, offset, **kw):
    """(o f32, lse f32, None), or for an offset profile (o, lse, (4 x the f32 oracle's error in o, ... in lse))."""
    o, lse = R.attention_ref(q.float(), k.float(), v.float(), **kw)
    extra = None
    if offset:
        o32, lse32 = R.attention_ref(q.float(), k.float(), v.float(), dtype=torch.float32, **kw)
        extra = (4 * (o32.double() - o).abs().max().item(), 4 * (lse32.double() - lse).abs().max().item())
    return o.float(), lse.float(), extra


@functools.lru_cache(maxsize=96)
def case(name, d, hq, hkv, dtype, causal, kv=LP.KV, qo=LP.QO, dv=None, rows=None, kv_dtype=None, window_left=-1):
    """(q, k, v, run keywords, oracle) of a profile; computed once per distinct case and never modified.  kv_dtype: k
    and v rounded to that fp8 type, which the oracle then sees."""
    q, k, v, kw = LP.inputs(name, d, hq, hkv, dtype, causal, kv, qo, dv, rows)
    if kv_dtype is not None:
        k, v = k.to(kv_dtype), v.to(kv_dtype)
    ref = oracle(q, k, v, LP.is_offset(name), causal=causal, window_left=window_left, **kw)
    return q, k, v, kw, ref


def one_request_pages(kv, seed=5):
    """(indptr, indices, last, num_pages) of one request of kv tokens on shuffled pages with three spare ones."""
    return page_table([kv], PAGE, torch.Generator().manual_seed(seed), extra_pages=3)


def paged(k, v, kv, table):
    indptr, indices, _, num_pages = table
    fp8 = k.dtype in (E4M3, E5M2)
    cache = scatter_to_pages(k.float() if fp8 else k, v.float() if fp8 else v, [kv], indptr, indices, PAGE, num_pages)
    return cache.to(k.dtype)  # fp8 values are exact in f32


# ---- 16-bit prefill (prefill_kernel.h) ------------------------------------------------------------------------------
MODES = {"f16": (F16, {}), "bf16": (BF16, {}), "bf16_exact_range": (BF16, dict(bf16_pv_exact_range=True))}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("mode", MODES)
def test_single_prefill_16bit(mode, d, causal):
    """single_prefill_with_kv_cache, heads 8/2.  Measured: f16 9.8e-4 / 1.5e-5, offset 7.4e-4 / 3.9e-3; bf16 in both
    P.V modes 7.8e-3 / 7.6e-6, offset 2.2e-3 / 3.9e-3."""
    import flashinfer

    dtype, run_kw = MODES[mode]
    t = Tally(f"single prefill {mode} d{d} causal={causal}")
    for name in LP.PROFILES_16:
        q, k, v, kw, ref = case(name, d, 8, 2, dtype, causal)
        o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal,
                                                         return_lse=True, **run_kw, **kw)
        t.check(name, o, lse, ref, ptol(dtype))
    t.finish()


@pytest.mark.parametrize("hq,hkv", [(4, 4), (28, 4)])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_single_prefill_other_head_packings(dtype, hq, hkv):
    """Groups of 1 and 7 query heads per kv head: 64 and 9 query positions per 64-row tile instead of 16.  Measured:
    f16 9.8e-4 / 1.1e-5, offset 7.7e-4 / 3.9e-3; bf16 7.8e-3 / 7.6e-6, offset 2.3e-3 / 3.9e-3."""
    import flashinfer

    t = Tally(f"single prefill {ids(dtype)} heads {hq}/{hkv}")
    for name in LP.PROFILES_16:
        q, k, v, kw, ref = case(name, 128, hq, hkv, dtype, True)
        o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, return_lse=True,
                                                         **kw)
        t.check(name, o, lse, ref, ptol(dtype))
    t.finish()


def run_paged_prefill(t, names, d, hq, hkv, dtype, causal, plan_kw, expect_split, o_tol, kv_dtype=None):
    """Every profile as one request of the paged wrapper; one plan per set of run keywords."""
    table = one_request_pages(LP.KV)
    wrappers = {}
    for name in names:
        q, k, v, kw, ref = case(name, d, hq, hkv, dtype, causal, kv_dtype=kv_dtype)
        key = tuple(sorted(kw.items()))
        if key not in wrappers:
            wrappers[key] = planned_prefill_wrapper(
                32 << 20, "NHD", indptr_of([LP.QO]), *table[:3], hq, hkv, d, PAGE, causal=causal, q_data_type=dtype,
                kv_data_type=kv_dtype or dtype, **plan_kw, **kw)
            assert wrappers[key]._plan_info[_lib.FI_PP_SPLIT_KV] == expect_split
        o, lse = wrappers[key].run(q.to(DEV), paged(k, v, LP.KV, table).to(DEV), return_lse=True)
        t.check(name, o, lse, ref, o_tol)


SPLITS = {"unsplit": (dict(disable_split_kv=True), 0), "split128": (dict(fixed_split_size=128), 1)}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_paged_prefill_16bit(dtype, split, causal):
    """BatchPrefillWithPagedKVCacheWrapper, d 128, heads 8/2, unsplit and in three chunks of 128 keys: the chunk lse
    values then differ by tens of units in the merge (tile_up(7): 14 per chunk; key_ramp: 46; late_spike(40): 58).
    Measured, split and unsplit alike: f16 9.8e-4 / 1.1e-5, offset 8.3e-4 / 3.9e-3; bf16 7.8e-3 / 7.6e-6, offset
    2.2e-3 / 3.9e-3."""
    plan_kw, expect = SPLITS[split]
    t = Tally(f"paged prefill {ids(dtype)} {split} causal={causal}")
    run_paged_prefill(t, LP.PROFILES_16, 128, 8, 2, dtype, causal, plan_kw, expect, ptol(dtype))
    t.finish()


def test_ragged_prefill_16bit():
    """Measured: 9.8e-4 / 7.6e-6, offset 7.4e-4 / 3.9e-3."""
    import flashinfer

    t = Tally("ragged prefill f16")
    wrappers = {}
    for name in LP.PROFILES_16:
        q, k, v, kw, ref = case(name, 128, 8, 2, F16, True)
        key = tuple(sorted(kw.items()))
        if key not in wrappers:
            w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(torch.zeros(16 << 20, dtype=torch.uint8, device=DEV), "NHD")
            w.plan(indptr_of([LP.QO]).to(DEV), indptr_of([LP.KV]).to(DEV), 8, 2, 128, causal=True, **kw)
            wrappers[key] = w
        o, lse = wrappers[key].run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
        t.check(name, o, lse, ref, ptol(F16))
    t.finish()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_custom_mask_on_mixed_rows(dtype):
    """mixed_rows under a random mask with column 0 visible: which key holds a row's maximum is now random too.
    Measured: f16 1.0e-3 / 7.6e-6, bf16 7.0e-3 / 7.6e-6."""
    import flashinfer

    q, k, v, _ = LP.inputs("mixed_rows", 128, 8, 2, dtype)
    mask = torch.rand(LP.QO, LP.KV, generator=torch.Generator().manual_seed(3)) < 0.5
    mask[:, 0] = True
    o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), custom_mask=mask.to(DEV),
                                                     return_lse=True)
    t = Tally(f"custom mask {ids(dtype)}")
    t.check("mixed_rows", o, lse, oracle(q, k, v, False, custom_mask=mask), ptol(dtype))
    t.finish()


def test_window_left_100():
    """A causal window of 101 keys: the first visible tile of a row is not tile 0 and is partly masked.  Measured:
    9.8e-4 / 7.6e-6, offset 7.3e-4 / 3.9e-3."""
    import flashinfer

    t = Tally("window_left=100 f16")
    for name in LP.PROFILES_16:
        q, k, v, kw, ref = case(name, 128, 8, 2, F16, True, window_left=100)
        o, lse = flashinfer.single_prefill_with_kv_cache(q.to(DEV), k.to(DEV), v.to(DEV), causal=True, window_left=100,
                                                         return_lse=True, **kw)
        t.check(name, o, lse, ref, ptol(F16))
    t.finish()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("kv_dtype", [E4M3, E5M2], ids=ids)
def test_fp8_kv_cache_under_16bit_q(kv_dtype, causal):
    """The upcast path: f16 queries over an fp8 cache, at the 16-bit bar; the oracle sees the quantised cache.
    Measured: 9.8e-4 / 1.5e-5, offset 1.7e-3 (e5m2, causal; 1.0e-3 otherwise) / 3.9e-3."""
    t = Tally(f"fp8 kv cache {ids(kv_dtype)} causal={causal}")
    run_paged_prefill(t, LP.PROFILES_16, 128, 8, 2, F16, causal, *SPLITS["unsplit"], ptol(F16), kv_dtype=kv_dtype)
    t.finish()


# ---- fp8 q/k/v (prefill_fp8_kernel.h) -------------------------------------------------------------------------------
FP8_LSE_TOL = dict(rtol=1e-3, atol=2e-3)  # test_batch_prefill_fp8_qkv_paged_c3_shape_small


@functools.lru_cache(maxsize=None)
def fp8_case(name, d, f8, causal):
    q8, k8, v8, sq, sk, sv = LP.fp8_inputs(name, d, f8, causal)
    o, lse = R.fp8_attention_ref(q8, k8, v8, sq, sk, sv, causal=causal)
    return q8, k8, v8, sq, sk, sv, (o.float(), lse.float(), None)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("f8", [E4M3, E5M2], ids=ids)
def test_fp8_native_prefill(f8, d):
    """fp8 q/k/v with per-head scales through single_prefill_with_kv_cache and the paged wrapper, unsplit and split,
    against fp8_attention_ref at the fp8 bars (5e-2 e4m3, 1e-1 e5m2).  Measured: e4m3 7.7e-3 / 3.8e-6, e5m2 2.1e-2 /
    5.7e-6, both on tile_up(2) -- what the fp8 oracle itself is away from exact attention there."""
    import flashinfer

    bar = dict(rtol=LP.FP8_BAR[f8], atol=LP.FP8_BAR[f8])
    t = Tally(f"fp8 native {ids(f8)} d{d}")
    table = one_request_pages(LP.KV)
    wrappers = {}
    for causal in (False, True):
        for split, (plan_kw, expect) in SPLITS.items():
            w = planned_prefill_wrapper(32 << 20, "NHD", indptr_of([LP.QO]), *table[:3], 8, 2, d, PAGE, causal=causal,
                                        q_data_type=f8, kv_data_type=f8, o_data_type=F16, **plan_kw)
            assert w._plan_info[_lib.FI_PP_SPLIT_KV] == expect
            wrappers[split, causal] = w
    for name, causal in LP.PROFILES_FP8:
        q8, k8, v8, sq, sk, sv, ref = fp8_case(name, d, f8, causal)
        scales = [x.to(DEV) for x in (sq, sk, sv)]
        o, lse = flashinfer.single_prefill_with_kv_cache(q8.to(DEV), k8.to(DEV), v8.to(DEV), *scales, causal=causal,
                                                         o_dtype=F16, return_lse=True)
        t.check(f"single {name} causal={causal}", o, lse, ref, bar, FP8_LSE_TOL)
        for split in SPLITS:
            o, lse = wrappers[split, causal].run(q8.to(DEV), paged(k8, v8, LP.KV, table).to(DEV), return_lse=True, scale_q=scales[0],
                           scale_k=scales[1], scale_v=scales[2])
            t.check(f"paged {split} {name} causal={causal}", o, lse, ref, bar, FP8_LSE_TOL)
    t.finish()


# ---- head_dim 192 / 128 (prefill_qkvo_kernel.h) ---------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_prefill_qkvo_192_128(dtype, causal):
    """The ragged wrapper as test_prefill_qkvo_gpu.py sets it up, at the planner's choice and in chunks of 128 keys.
    The structure takes the first 96 of the 192 qk dims; the entry point refuses a soft cap, so cap_saturated is out.
    Measured: f16 9.8e-4 / 1.5e-5, offset 7.6e-4 / 3.9e-3; bf16 7.8e-3 / 1.5e-5, offset 2.1e-3 / 3.9e-3."""
    import flashinfer

    t = Tally(f"qkvo 192/128 {ids(dtype)} causal={causal}")
    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)
    for split in (None, 128):
        w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, "NHD")
        w.plan(indptr_of([LP.QO]).to(DEV), indptr_of([LP.KV]).to(DEV), 8, 2, 192, head_dim_vo=128, causal=causal,
               q_data_type=dtype, fixed_split_size=split)
        assert split is None or w._plan_info[_lib.FI_PP_SPLIT_KV] == 1
        for name in LP.PROFILES_16:
            if name == "cap_saturated":
                continue
            q, k, v, _, ref = case(name, 192, 8, 2, dtype, causal, dv=128)
            o, lse = w.run(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
            t.check(f"{name} split={split}", o, lse, ref, ptol(dtype))
    t.finish()


# ---- decode ---------------------------------------------------------------------------------------------------------
VARIANTS = {"default": {}, "r1": {"FI_DECODE_MFMA16": 0}}
REPS = 4  # requests per decode batch: four query rows over the same keys (mixed_rows: a = 1, -1, 0, 0.01)


@pytest.fixture
def kernel_variant(request):
    """The pattern of test_decode_gpu.py: sets the switches of a VARIANTS entry in this process for the test and
    returns every one of them to the environment's value afterwards."""
    options = VARIANTS[request.param]
    try:
        for name, value in options.items():
            _lib.set_option(name, value)
        yield request.param
    finally:
        for name in options:
            _lib.set_option(name, None)


def run_batch_decode(t, names, kv, d, hq, hkv, dtype, expect_slot, kv_dtype=None):
    """REPS requests that share one profile's pages, one batch per profile; one plan per set of run keywords."""
    table = one_request_pages(kv)
    indptr, indices, last, _ = table
    pages = int(indptr[1])
    b_indptr = torch.arange(REPS + 1, dtype=torch.int32) * pages
    wrappers = {}
    for name in names:
        q, k, v, kw, ref = case(name, d, hq, hkv, dtype, False, kv=kv, qo=1, rows=REPS, kv_dtype=kv_dtype)
        key = tuple(sorted(kw.items()))
        if key not in wrappers:
            w = planned_decode_wrapper(8 << 20, "NHD", b_indptr, indices.repeat(REPS), last.repeat(REPS), hq, hkv, d,
                                       PAGE, q_data_type=dtype, kv_data_type=kv_dtype or dtype, **kw)
            assert w._plan_info[_lib.FI_DP_SPLIT_KV] == 1 and w._plan_info[_lib.FI_DP_KV_CHUNK_SIZE] == LP.CHUNK
            assert w._plan_info[_lib.FI_DP_UNIFORM_CHUNKS] == expect_slot and _lib.FI_DP_UNIFORM_CHUNKS == 16
            wrappers[key] = w
        o, lse = wrappers[key].run(q.to(DEV), paged(k, v, kv, table).to(DEV), return_lse=True)
        t.check(f"kv{kv} {name}", o, lse, ref, tol(dtype))


# kv 333: three chunks, decode launch + merge launch; kv 256 / 512: the plans whose 2 / 4 chunks the 16x16 kernel folds
# in LDS when its run condition holds (FI_DP_UNIFORM_CHUNKS says so; r1 and narrow token rows take two launches)
DECODE_KV = [(LP.KV, 0), (256, 2), (512, 4)]


@pytest.mark.parametrize("kernel_variant", list(VARIANTS), indirect=True)
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("hq,hkv", [(4, 4), (8, 2), (16, 2)])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_batch_decode(kernel_variant, dtype, hq, hkv, d):
    """Groups of 1, 4 and 8 heads at default options (the 16x16 kernel) and with FI_DECODE_MFMA16=0 (VALU kernel for
    groups <= 4, 32x32 kernel above).  Measured, every kernel alike: f16 9.8e-4 / 1.5e-5, offset 7.6e-4 / 7.8e-3;
    bf16 7.8e-3 / 1.5e-5, offset 2.2e-3 / 7.8e-3."""
    t = Tally(f"batch decode {kernel_variant} {ids(dtype)} {hq}/{hkv} d{d}")
    for kv, slot in DECODE_KV:
        run_batch_decode(t, LP.PROFILES_16, kv, d, hq, hkv, dtype, slot)
    t.finish()


@pytest.mark.parametrize("kernel_variant", list(VARIANTS), indirect=True)
def test_batch_decode_group_of_7(kernel_variant):
    """Heads 28/4.  Measured: 9.8e-4 / 1.5e-5, offset 7.7e-4 / 3.9e-3."""
    t = Tally(f"batch decode {kernel_variant} f16 28/4 d128")
    for kv, slot in DECODE_KV:
        run_batch_decode(t, LP.PROFILES_16, kv, 128, 28, 4, F16, slot)
    t.finish()


@pytest.mark.parametrize("kernel_variant", list(VARIANTS), indirect=True)
def test_batch_decode_e4m3_cache(kernel_variant):
    """The oracle sees the quantised cache, so the 16-bit bar applies.  Measured: 9.8e-4 / 1.5e-5, offset 8.8e-4 /
    3.9e-3."""
    t = Tally(f"batch decode {kernel_variant} e4m3 cache")
    for kv, slot in DECODE_KV:
        run_batch_decode(t, LP.PROFILES_16, kv, 128, 8, 2, F16, slot, kv_dtype=E4M3)
    t.finish()


@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_single_decode(dtype):
    """single_decode_with_kv_cache at kv 333, and at kv 8192, which it splits itself (the shape of
    test_single_decode_on_stale_scratch), on tile_up(7), late_spike(8) and offset(-30000).  Measured: f16 9.7e-4 /
    6.1e-5, offset 6.0e-4 / 3.9e-3; bf16 7.8e-3 / 6.1e-5, offset 1.5e-3 / 3.9e-3."""
    import flashinfer

    t = Tally(f"single decode {ids(dtype)}")
    for kv, names in ((LP.KV, LP.PROFILES_16), (8192, ("tile_up(7)", "late_spike(8)", "offset(-30000)"))):
        for name in names:
            q, k, v, kw, ref = case(name, 128, 8, 2, dtype, False, kv=kv, qo=1)
            o, lse = flashinfer.single_decode_with_kv_cache(q[0].to(DEV), k.to(DEV), v.to(DEV), return_lse=True, **kw)
            t.check(f"kv{kv} {name}", o[None], lse[None], ref, tol(dtype))
    t.finish()


# ---- MLA (mla.hip) --------------------------------------------------------------------------------------------------
MLA_NAMES = tuple(n for n in LP.PROFILES_16 if n != "cap_saturated")  # the MLA entry point has no soft cap
MLA_HEADS = 16


@functools.lru_cache(maxsize=8)
def mla_batch(dtype, causal, qo, reps):
    """Every MLA profile `reps` times as requests of qo query rows (the replicas of a profile read the same pages, with
    their own query rows): device tensors for plan() / run() and the oracle per request."""
    n, kv = len(MLA_NAMES), LP.KV
    indptr, indices, _, num_pages = page_table([kv] * n, PAGE, torch.Generator().manual_seed(9), extra_pages=3)
    ckv_cache = torch.zeros(num_pages, PAGE, LP.CKV, dtype=dtype)
    kpe_cache = torch.zeros(num_pages, PAGE, LP.KPE, dtype=dtype)
    tok = torch.arange(kv)
    qs_nope, qs_pe, refs, req_pages = [], [], [], []
    for p, name in enumerate(MLA_NAMES):
        q_nope, q_pe, ckv, kpe = LP.mla_inputs(name, MLA_HEADS, dtype, causal, kv, qo, qo * reps)
        mine = indices[int(indptr[p]):int(indptr[p + 1])]
        slot = mine[tok // PAGE].long()
        ckv_cache[slot, tok % PAGE] = ckv
        kpe_cache[slot, tok % PAGE] = kpe
        kk = torch.cat([ckv, kpe], -1)[:, None]
        for r in range(reps):
            rows = slice(r * qo, (r + 1) * qo)
            q = torch.cat([q_nope[rows], q_pe[rows]], -1)
            ref = oracle(q, kk, ckv[:, None], LP.is_offset(name), causal=causal, sm_scale=LP.MLA_SM)
            p_bar = None
            if dtype == BF16:  # 2^-9 sum_j p_j |v_j| / sum_j p_j: see test_mla
                p_bar = 2.0 ** -9 * R.attention_ref(q.float(), kk.float(), ckv[:, None].float().abs(), causal=causal,
                                                    sm_scale=LP.MLA_SM)[0].float()
            refs.append((ref, p_bar))
            req_pages.append(mine)
        qs_nope.append(q_nope)
        qs_pe.append(q_pe)
    nreq = n * reps
    plan = (indptr_of([qo] * nreq).to(DEV), indptr_of([len(m) for m in req_pages]).to(DEV),
            torch.cat(req_pages).to(DEV), torch.full((nreq,), kv, dtype=torch.int32, device=DEV))
    run = (torch.cat(qs_nope).to(DEV), torch.cat(qs_pe).to(DEV), ckv_cache.to(DEV), kpe_cache.to(DEV))
    return plan, run, refs


@pytest.mark.parametrize("qo", [1, 5])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [F16, BF16], ids=ids)
def test_mla(dtype, causal, qo):
    """BatchMLAPagedAttentionWrapper, 16 heads.  The planner cuts a request of 333 keys into chunks of 256 unless the
    batch fills the grid: every profile once is a split plan (256 + 77 keys, merged by merge.hip), every profile 13
    times (qo 1) or twice (qo 5) an unsplit one.

    bf16: the kernel rounds P to bf16 once before P.V (mla.hip, `sm.p[r][...] = T::from_f32(pv)`), as the reference
    does (mla.cuh:499 and :554, vec_cast<DTypeKV, float> of s_frag ahead of the P.V MMA), while the row sum keeps the
    unrounded P.  Each p_j then carries a relative error of up to 2^-9, and o = sum_j p_j v_j / sum_j p_j moves by up
    to 2^-9 sum_j p_j |v_j| / sum_j p_j.  With randn logits the weights are spread and that stays under the file's
    atol of 2e-3; a moving maximum puts the weight on a few keys, and where those hold large |v| it does not:
    key_ramp(0.25), causal, qo 5, split, missed tol(bf16) by 3.6e-6 on the MI355X (at an element with |o| = 0.134,
    bar 2.66e-3, where sum p |v| / sum p = 1.28; largest error of the case 5.142e-3), and an fp64 restatement of the
    kernel's tile loop with nothing but that rounding and the bf16 rounding of o gives the same two figures on the CPU.  So the absolute bar of a bf16 element is
    max(2e-3, 2^-9 sum_j p_j |v_j| / sum_j p_j), the sum taken from the oracle: where the weights are spread it is the
    file's bar.  f16 rounds P to 11 bits and keeps the file's bar.

    Measured: f16 9.8e-4 / 1.5e-5, offset 9.8e-4 / 3.9e-3; bf16 7.8e-3 / 1.5e-5, offset 2.9e-3 / 3.9e-3."""
    import flashinfer

    t = Tally(f"mla {ids(dtype)} causal={causal} qo{qo}")
    for label, reps, split in (("split", 1, 1), ("unsplit", 13 if qo == 1 else 2, 0)):
        plan, run, refs = mla_batch(dtype, causal, qo, reps)
        w = flashinfer.mla.BatchMLAPagedAttentionWrapper(torch.empty(128 << 20, dtype=torch.uint8, device=DEV), backend="fa2")
        w.plan(*plan, MLA_HEADS, LP.CKV, LP.KPE, PAGE, causal, LP.MLA_SM, dtype, dtype)
        assert w._plan_info[_lib.FI_MLA_SPLIT_KV] == split
        o, lse = w.run(*run, return_lse=True)
        o, lse = o.float().cpu(), lse.cpu()
        for i, (ref, p_bar) in enumerate(refs):
            rows = slice(i * qo, (i + 1) * qo)
            t.check(f"{label} {MLA_NAMES[i // reps]} rep {i % reps}", o[rows], lse[rows], ref, tol(dtype), o_atol=p_bar)
    t.finish()


# ---- the merges, called directly (merge.hip) ------------------------------------------------------------------------
V_BAR = {F16: 1e-3, BF16: 8e-3}  # test_merge_gpu.py
S_ATOL = 1e-4                    # its lse bar; rtol = 0 here, as for every offset case
S_OFFSETS = (4000.0, -4000.0, -43000.0)  # base 2


def merge_states_case(n, d, dtype, offset, seed, rows=6, heads=3):
    """s = offset + randn * 6; in the second half of the rows entry 0 stands 200 units above the others, whose weights
    underflow to 0 next to it."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, n, heads, d, generator=g).to(dtype)
    s = offset + torch.randn(rows, n, heads, generator=g) * 6
    s[rows // 2:, 0] += 200.0
    return v, s


def merge_bars(v, s, dtype, ref_fn):
    """(v_ref, s_ref, v bar, s atol): the f32 evaluation of the oracle sets both, as for the offset profiles."""
    v_ref, s_ref = ref_fn(v.float(), s, torch.float64)
    v32, s32 = ref_fn(v.float(), s, torch.float32)
    v_bar = max(V_BAR.get(dtype, 1e-5), 4 * (v32.double() - v_ref).abs().max().item())
    return v_ref, s_ref, v_bar, max(S_ATOL, 4 * (s32.double() - s_ref).abs().max().item())


@pytest.mark.parametrize("offset", S_OFFSETS)
@pytest.mark.parametrize("dtype,d", [(torch.float32, 128), (torch.float32, 96), (F16, 128), (BF16, 64)], ids=ids)
def test_merge_states_at_large_offsets(dtype, d, offset):
    """merge_states (both merge_n kernels: f32 at d 128 runs merge_n_f32_kernel, the rest the generic one), merge_state
    and fi_variable_length_merge_states.  Measured: v 4.8e-7 (f32), 9.7e-4 (f16), 7.8e-3 (bf16); s equal to the f32
    rounding of the oracle's at every offset."""
    import flashinfer

    t = Tally(f"merge {ids(dtype)} d{d} offset {offset:+.0f}")
    for n in (2, 5, 33, 65):
        v, s = merge_states_case(n, d, dtype, offset, seed=n + d)
        v_ref, s_ref, v_bar, s_atol = merge_bars(v, s, dtype, lambda a, b, dt: R.merge_states_ref(a, b, dtype=dt))
        vm, sm = flashinfer.merge_states(v.to(DEV), s.to(DEV))
        t.close("v", f"merge_states n={n}", vm, v_ref, v_bar, v_bar)
        t.close("s", f"merge_states n={n}", sm, s_ref, 0.0, s_atol)
        # the same entries as one ragged row per (row): fi_variable_length_merge_states
        rows, heads = v.shape[0], v.shape[2]
        ip = indptr_of([n] * rows).to(DEV)
        v_d, s_d = v.float().reshape(rows * n, heads, d).to(DEV), s.reshape(rows * n, heads).to(DEV)  # f32 partials
        vo = torch.full((rows, heads, d), 7.0, dtype=dtype, device=DEV)
        so = torch.full((rows, heads), 7.0, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().fi_variable_length_merge_states(
            v_d.data_ptr(), s_d.data_ptr(), ip.data_ptr(), vo.data_ptr(), so.data_ptr(), rows, heads, d,
            _lib.FI_DTYPE_F32, _lib.fi_dtype(dtype), _lib.current_stream(vo.device)), "vlms")
        torch.cuda.synchronize()
        t.close("v", f"variable_length n={n}", vo, v_ref, v_bar, v_bar)
        t.close("s", f"variable_length n={n}", so, s_ref, 0.0, s_atol)
    v, s = merge_states_case(2, d, dtype, offset, seed=d)
    v_ref, s_ref, v_bar, s_atol = merge_bars(v, s, dtype, lambda a, b, dt: R.merge_state_ref(a[:, 0], b[:, 0], a[:, 1], b[:, 1], dtype=dt))
    vm, sm = flashinfer.merge_state(v[:, 0].to(DEV), s[:, 0].to(DEV), v[:, 1].to(DEV), s[:, 1].to(DEV))
    t.close("v", "merge_state", vm, v_ref, v_bar, v_bar)
    t.close("s", "merge_state", sm, s_ref, 0.0, s_atol)
    t.finish()


@pytest.mark.parametrize("encoding", ["kernel_sentinel", "minus_inf"])
@pytest.mark.parametrize("dtype,d", [(torch.float32, 128), (F16, 128), (BF16, 64)], ids=ids)
def test_live_state_at_minus_43000_next_to_an_empty_one(dtype, d, encoding):
    """A live state 7000 units above the sentinel -5e4 merged with a state that saw no key, in either encoding
    (s = -5e4 or -inf, v = 0): the live state comes back, from merge_state in both orders and from merge_states."""
    import flashinfer

    g = torch.Generator().manual_seed(17)
    rows, heads = 5, 3
    live_v = torch.randn(rows, heads, d, generator=g).to(dtype)
    live_s = -43000.0 + torch.randn(rows, heads, generator=g) * 6
    e_v = torch.zeros_like(live_v)
    e_s = torch.full_like(live_s, R.NEG_INF_SENTINEL if encoding == "kernel_sentinel" else float("-inf"))
    bar = V_BAR.get(dtype, 1e-5)
    t = Tally(f"live at -43000 + empty ({encoding}) {ids(dtype)}")
    lv, ls, ev, es = (x.to(DEV) for x in (live_v, live_s, e_v, e_s))
    for tag, args in (("(live, empty)", (lv, ls, ev, es)), ("(empty, live)", (ev, es, lv, ls))):
        vm, sm = flashinfer.merge_state(*args)
        t.close("v", f"merge_state {tag}", vm, live_v, bar, bar)
        t.close("s", f"merge_state {tag}", sm, live_s, 0.0, S_ATOL)  # the weights are exactly 1 and 0: s comes back as it went in
    for order in ((ev, lv, ev), (lv, ev)):
        ss = [es if x is ev else ls for x in order]
        vm, sm = flashinfer.merge_states(torch.stack(order, 1), torch.stack(ss, 1))
        t.close("v", f"merge_states of {len(order)}", vm, live_v, bar, bar)
        t.close("s", f"merge_states of {len(order)}", sm, live_s, 0.0, S_ATOL)
    t.finish()
