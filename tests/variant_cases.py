"""Case tables for the attention tests on logit scalars away from their defaults and on feature combinations.

Plain data and CPU helpers (no GPU import): tests/test_attention_variants_cpu.py checks with the oracle alone that no
case is vacuous and that the tables cover what they claim; tests/test_attention_variants_gpu.py runs every case on
the kernels.  A case names its entry point, shapes, dtypes, the scalars it moves, the features it switches on and the
plan options; plan_kw / run_kw / oracle_kw turn that into the keywords of plan(), run() and the oracle.

Scalars (away from the defaults 1/sqrt(d), 1e4, 1, 1, 1, 1): sm_scale 0.05, rope_theta 5e5, rope_scale 4,
q_scale 0.5, k_scale 1.5 (product not 1), v_scale 2 (exact in 16 bit) or 0.37; bmm1_scale 0.05 / bmm2_scale 0.5 on
the plan-free calls.  Features: "rope" / "alibi" (pos_encoding_mode), "cap" (logits_soft_cap), "window" (window_left),
"mask" (custom_mask, prefill), "sinks".  Soft-cap cases multiply q by Q_GAIN and use cap CAP so that the cap bites (at
d 128, kv 300, cap 20 and unit-variance q the output moves only 16x the bar; with q x 3 and cap 8 more than 1000x).

Which kernel a case runs (csrc/decode.hip choose_decode, csrc/prefill_inst.hip launch_features):
  decode   group <= 16 at head_dim 64 / 128 -> the 16x16x32 kernel; under r1 (FI_DECODE_MFMA16=0) the VALU kernel, or
           the 32x32x16 kernel for plain logits (groups >= 5, and any group with RoPE or small pages).  Groups above 16
           with ALiBi or a cap, and head_dim 256, run the VALU kernel under both choices.
  prefill  one feature of alibi / cap / mask without RoPE has its own instantiation (GEN 1 / 2 / 4); any two of them,
           and RoPE with any, run the all-features one (GEN 15), which has a SINK twin for unsplit runs.  fp8 q / k / v
           with any feature (a window included) leave the fp8-native kernel for the upcast one.
"""
import dataclasses
import functools
import math
from typing import Optional, Tuple

import torch

from attn_inputs import indptr_of, make_paged, page_table, ptol, scatter_to_pages, tol
from oracle import attention_ref as R

F16, BF16, E4M3 = torch.float16, torch.bfloat16, torch.float8_e4m3fn

SM_SCALE, ROPE_THETA, ROPE_SCALE, Q_SCALE, K_SCALE = 0.05, 5e5, 4.0, 0.5, 1.5
BMM1_SCALE, BMM2_SCALE = 0.05, 0.5
CAP, Q_GAIN = 8.0, 3.0
PLAIN_GAIN = 2.0  # combinations without a cap, and all scalars together: a sharper softmax, so that every item counts
DECODE_WINDOW, PREFILL_WINDOW = 100, 20
LSE_TOL = 2e-3

# every scalar a case may move, with the value that returns it to its default in the oracle
SCALARS = ("sm_scale", "rope_theta", "rope_scale", "q_scale", "k_scale", "v_scale", "bmm1_scale", "bmm2_scale")
TRIVIAL_SCALARS = ("v_scale", "bmm2_scale")  # they multiply the output: exempt from the sensitivity guard
FEATURES = ("rope", "alibi", "cap", "window", "mask", "sinks")
DECODE_ENTRIES = ("batch_decode", "single_decode", "trtllm_decode")
PREFILL_ENTRIES = ("paged_prefill", "ragged_prefill", "single_prefill", "trtllm_context", "fp8_prefill")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    entry: str  # one of DECODE_ENTRIES / PREFILL_ENTRIES
    hq: int
    hkv: int
    d: int
    dtype: torch.dtype  # q and o (fp8_prefill: the output type; q / k / v are e4m3)
    kv_lens: Tuple[int, ...]
    qo_lens: Optional[Tuple[int, ...]] = None  # prefill
    kv_dtype: Optional[torch.dtype] = None  # None: the q dtype
    page_size: int = 16
    layout: str = "NHD"
    causal: bool = False
    features: Tuple[str, ...] = ()
    scalars: Tuple[Tuple[str, float], ...] = ()
    split: Optional[bool] = None  # prefill: False disable_split_kv, True fixed_split_size 128; decode: False disables
    hi_lo: bool = False  # bf16 prefill: bf16_pv_exact_range (P as hi + lo bf16 halves)
    q_gain: float = 1.0
    seed: int = 0
    dead_rows: int = 0  # query rows without a visible key, declared

    @property
    def group(self):
        return self.hq // self.hkv

    @property
    def is_decode(self):
        return self.entry in DECODE_ENTRIES

    @property
    def scalar(self):
        return dict(self.scalars)

    def __str__(self):
        return self.name


# ---- keywords ------------------------------------------------------------------------------------------------------
def feature_kw(case, drop=None):
    """The feature keywords plan() (or the single-request call) and the oracle share."""
    on = [f for f in case.features if f != drop]
    kw = {}
    if "rope" in on:
        kw["pos_encoding_mode"] = "ROPE_LLAMA"
    if "alibi" in on:
        kw["pos_encoding_mode"] = "ALIBI"
    if "cap" in on:
        kw["logits_soft_cap"] = CAP
    if "window" in on:
        kw["window_left"] = DECODE_WINDOW if case.is_decode else PREFILL_WINDOW
    return kw


def plan_kw(case):
    """Keywords of plan() (batch wrappers) or of the call itself (single-request entry points), the mask aside."""
    kw = feature_kw(case)
    s = case.scalar
    kw.update({k: s[k] for k in ("sm_scale", "rope_theta", "rope_scale") if k in s})
    if case.entry in ("single_decode",):
        kw.update({k: s[k] for k in ("q_scale", "k_scale", "v_scale") if k in s})
        return kw
    if case.entry == "single_prefill":
        kw["causal"] = case.causal
        if case.hi_lo:
            kw["bf16_pv_exact_range"] = True
        return kw
    if case.is_decode:
        if case.split is False:
            kw["disable_split_kv"] = True
        return kw
    kw["causal"] = case.causal
    if case.split is False:
        kw["disable_split_kv"] = True
    elif case.split:
        kw["fixed_split_size"] = 128
    if case.hi_lo:
        kw["bf16_pv_exact_range"] = True
    return kw


def run_kw(case):
    """Scalar keywords of the batch wrappers' run()."""
    s = case.scalar
    return {k: s[k] for k in ("q_scale", "k_scale", "v_scale") if k in s}


def decode_kernel(case, variant="default"):
    """The decode kernel a case runs under a VARIANTS entry of tests/test_decode_gpu.py: "valu", "mfma16" or "mfma32"
    (csrc/decode.hip, choose_decode; every case here has a 16-bit q and 31-bit strides).  A restatement: the library
    does not report the kernel it launched, so choose_decode carries a comment that points here and the two change
    together.  A RoPE case whose kernel this names wrongly fails on the GPU, since the oracle's rotation rounding follows
    it and moves the answer by more than the bar (tests/test_decode_gpu.py, the f32-rotation test)."""
    page = 16 if case.entry == "single_decode" else case.page_size
    fp8 = case.kv_dtype is not None and case.kv_dtype != case.dtype
    mfma = case.d in (64, 128)
    plain = "alibi" not in case.features and "cap" not in case.features
    if variant == "default":
        if not (mfma and (plain or case.group <= 16)):
            return "valu"
        return "mfma16" if case.group <= 16 else "mfma32"
    tokens_per_load = 64 // (case.d // (16 if fp8 else 8))
    small_pages = page & (page - 1) != 0 or page < tokens_per_load
    min_group = 1 if "rope" in case.features or small_pages else 3 if fp8 else 5
    return "mfma32" if mfma and plain and case.group >= min_group else "valu"


def rope_round_dtype(case, variant="default"):
    """rope_round_dtype for the oracle: the prefill kernels and the matrix-core decode kernels round the rotated q / k
    to the 16-bit type, the VALU decode kernel rotates in f32 (attn_inputs.rope_rt, per kernel instead of per head_dim:
    a cap or ALiBi moves a RoPE case between kernels)."""
    if "rope" not in case.features:
        return None
    if case.is_decode:
        return None if decode_kernel(case, variant) == "valu" else case.dtype
    return case.dtype


def oracle_kw(case, drop=None, variant="default"):
    """Keywords of the oracle for the case; `drop` names one scalar returned to its default, or one feature switched
    off (the sensitivity guard)."""
    kw = feature_kw(case, drop)
    s = {k: v for k, v in case.scalars if k != drop}
    sm = s.get("sm_scale", s.get("bmm1_scale"))
    qk = s.get("q_scale", 1.0) * s.get("k_scale", 1.0)
    if sm is not None or qk != 1.0:
        kw["sm_scale"] = (1.0 / math.sqrt(case.d) if sm is None else sm) * qk
    kw.update({k: s[k] for k in ("rope_theta", "rope_scale") if k in s})
    if "rope" in case.features and drop != "rope":
        kw["rope_round_dtype"] = rope_round_dtype(case, variant)
    return kw


def out_scale(case):
    s = case.scalar
    return s.get("v_scale", 1.0) * s.get("bmm2_scale", 1.0)


def guard_items(case):
    """What the sensitivity guard switches off one at a time: every moved scalar but the trivial ones, every feature."""
    return [k for k, _ in case.scalars if k not in TRIVIAL_SCALARS] + list(case.features)


# ---- bars ----------------------------------------------------------------------------------------------------------
def bars(case):
    """(o bar, lse bar) as dicts of rtol / atol: the project's own bars.

    decode tol(dtype), prefill ptol(dtype), lse 2e-3.  Fused RoPE: both o terms doubled and the lse at 4e-3 (f16) /
    2e-2 (bf16), as tests/test_fuzz_gpu.py (the rotation is rounded to the 16-bit type; with one or two visible keys the
    lse is a single logit and carries that rounding).  v_scale / bmm2_scale multiply the output, so atol is multiplied
    by them; a scale that is no power of two rounds the 16-bit output a second time, so rtol gains one rounding of the
    output type (2^-11 f16, 2^-8 bf16).  fp8 q / k / v: 5e-2 on o, rtol 1e-3 / atol 2e-3 on the lse
    (tests/test_prefill_gpu.py)."""
    if case.entry == "fp8_prefill":
        return dict(rtol=5e-2, atol=5e-2), dict(rtol=1e-3, atol=2e-3)
    t = dict(tol(case.dtype) if case.is_decode else ptol(case.dtype))
    lse = LSE_TOL
    if "rope" in case.features:
        t = dict(rtol=t["rtol"] * 2, atol=t["atol"] * 2)
        lse = 2e-2 if case.dtype == BF16 else 4e-3
    scale = out_scale(case)
    if scale != 1.0:
        t["atol"] *= scale
        if math.frexp(scale)[0] != 0.5:
            t["rtol"] += 2.0 ** -8 if case.dtype == BF16 else 2.0 ** -11
    return t, dict(rtol=lse, atol=lse)


def bar_of(t, ref):
    """The scalar allowance atol + rtol max|ref| of a bar over a reference tensor (the guard's unit)."""
    return t["atol"] + t["rtol"] * float(ref.abs().max())


# ---- inputs --------------------------------------------------------------------------------------------------------
def make_sinks(hq):
    """One sink logit per head, distinct so that a head mix-up shows, around the size of the logits."""
    return torch.linspace(-2.0, 4.0, hq)


def make_mask(qo_lens, kv_lens, seed):
    """Flat bool mask, request after request: 70 % of the keys at random; every row keeps the last key causal shows it
    (inside any window, so no row dies), and row 0 loses key 0 where causal shows it and it is not that last key."""
    g = torch.Generator().manual_seed(9000 + seed)
    parts = []
    for ql, kl in zip(qo_lens, kv_lens):
        m = torch.rand(ql, kl, generator=g) < 0.7
        if ql and kl:
            assert ql <= kl
            m[torch.arange(ql), kl - ql + torch.arange(ql)] = True
            if kl - ql >= 1:
                m[0, 0] = False
        parts.append(m.reshape(-1))
    return torch.cat(parts)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """Seeded CPU inputs of a case, built once and never modified: q, the paged cache with its page table (one-token
    identity pages for the ragged and single-request entry points), qo_indptr, mask, sinks; fp8_prefill: the quantised
    rows and their per-head scales too."""
    kv_lens = list(case.kv_lens)
    kv_dtype = case.kv_dtype or case.dtype
    dense = case.entry in ("ragged_prefill", "single_prefill", "single_decode")
    page, layout = (1, "NHD") if dense else (case.page_size, case.layout)
    inp = {}
    gq = torch.Generator().manual_seed(100 + case.seed)
    rows = len(kv_lens) if case.is_decode else sum(case.qo_lens)
    if case.entry == "fp8_prefill":
        q16 = (torch.randn(rows, case.hq, case.d, generator=gq) * case.q_gain).half()
        k16 = torch.randn(sum(kv_lens), case.hkv, case.d, generator=gq).half()
        v16 = torch.randn(sum(kv_lens), case.hkv, case.d, generator=gq).half()
        (q, sq), (k8, sk), (v8, sv) = (R.per_head_symmetric_quant(x, E4M3) for x in (q16, k16, v16))
        indptr, indices, last, total = page_table(kv_lens, page, gq, extra_pages=2)
        # scattered in f32 (fp8 values are exact in it)
        cache = scatter_to_pages(k8.float(), v8.float(), kv_lens, indptr, indices, page, total, layout).to(E4M3)
        inp.update(k8=k8, v8=v8, sq=sq, sk=sk, sv=sv)
    else:
        cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, page, case.hkv, case.d, kv_dtype, layout,
                                                  seed=case.seed, shuffle=not dense, extra_pages=0 if dense else 3)
        q = (torch.randn(rows, case.hq, case.d, generator=gq) * case.q_gain).to(case.dtype)
    inp.update(q=q, cache=cache, indptr=indptr, indices=indices, last=last)
    if not case.is_decode:
        inp["qo_indptr"] = indptr_of(case.qo_lens)
    if "mask" in case.features:
        inp["mask"] = make_mask(case.qo_lens, kv_lens, case.seed)
    if "sinks" in case.features:
        inp["sinks"] = make_sinks(case.hq)
    return inp


def visible(case, drop=None):
    """Per request the bool [qo_len, kv_len] visibility of the case (decode: one row that sees the whole window)."""
    kw = feature_kw(case, drop)
    wl = kw.get("window_left", -1)
    inp = inputs(case)
    out, pos = [], 0
    qo_lens = [1] * len(case.kv_lens) if case.is_decode else case.qo_lens
    for ql, kl in zip(qo_lens, case.kv_lens):
        mb = None
        if "mask" in case.features and drop != "mask":
            mb = inp["mask"][pos: pos + ql * kl].reshape(ql, kl)
            pos += ql * kl
        out.append(R.visible_mask(ql, kl, case.causal and not case.is_decode, wl, mb))
    return out


@functools.lru_cache(maxsize=None)
def oracle(case, drop=None, variant="default"):
    """(o, lse) of the fp64 oracle on the case's inputs, the output scale applied; `drop` as in oracle_kw.  Computed
    once per distinct call and never modified."""
    inp = inputs(case)
    kw = oracle_kw(case, drop, variant)
    layout = "NHD" if case.entry in ("ragged_prefill", "single_prefill", "single_decode") else case.layout
    table = (layout, inp["indptr"], inp["indices"], inp["last"])
    if case.entry == "fp8_prefill":
        outs, lses, off, pos = [], [], 0, 0
        kw.pop("sm_scale", None)
        for b, (ql, kl) in enumerate(zip(case.qo_lens, case.kv_lens)):
            rows = slice(int(inp["qo_indptr"][b]), int(inp["qo_indptr"][b + 1]))
            mb = None
            if "mask" in case.features and drop != "mask":
                mb = inp["mask"][pos: pos + ql * kl].reshape(ql, kl)
            pos += ql * kl
            o, lse = R.fp8_attention_ref(inp["q"][rows], inp["k8"][off:off + kl], inp["v8"][off:off + kl], inp["sq"],
                                         inp["sk"], inp["sv"], causal=case.causal, custom_mask=mb, **kw)
            off += kl
            outs.append(o)
            lses.append(lse)
        return torch.cat(outs), torch.cat(lses)
    q, cache = inp["q"].float(), inp["cache"].float()
    if case.is_decode:
        o, lse = R.batch_decode_ref(q, cache, *table, **kw)
    else:
        mask = inp["mask"] if "mask" in case.features and drop != "mask" else None
        o, lse = R.batch_prefill_ref(q, inp["qo_indptr"], cache, *table, causal=case.causal, custom_mask=mask, **kw)
    if "sinks" in case.features and drop != "sinks":
        import sink_ref

        o, lse = sink_ref.fold_sink(o, lse, inp["sinks"])
    return o * out_scale(case), lse


# ---- tables --------------------------------------------------------------------------------------------------------
def _sc(**kw):
    return tuple(kw.items())


ALL_SCALARS = _sc(sm_scale=SM_SCALE, rope_theta=ROPE_THETA, rope_scale=ROPE_SCALE, q_scale=Q_SCALE, k_scale=K_SCALE,
                  v_scale=2.0)
# (suffix, features, scalars, q gain): each scalar alone, then all together
SCALAR_ROWS = (
    ("sm_scale", (), _sc(sm_scale=SM_SCALE), 1.0),
    ("rope_theta", ("rope",), _sc(rope_theta=ROPE_THETA), 1.0),
    ("rope_scale", ("rope",), _sc(rope_scale=ROPE_SCALE), 1.0),
    ("q_scale", (), _sc(q_scale=Q_SCALE), 1.0),
    ("k_scale", (), _sc(k_scale=K_SCALE), 1.0),
    ("v_scale_2", (), _sc(v_scale=2.0), 1.0),
    ("v_scale_0.37", (), _sc(v_scale=0.37), 1.0),
    ("all", ("rope",), ALL_SCALARS, 2 * Q_GAIN),
)
# the keywords single_prefill_with_kv_cache has
SINGLE_PREFILL_ROWS = tuple(r for r in SCALAR_ROWS if not {"q_scale", "k_scale", "v_scale"} & set(dict(r[2]))) + (
    ("all", ("rope",), _sc(sm_scale=SM_SCALE, rope_theta=ROPE_THETA, rope_scale=ROPE_SCALE), 2 * Q_GAIN),)
# prefill: the feature forms whose algebra involves the scale
PREFILL_SCALE_ROWS = (
    ("alibi_sm_scale", ("alibi",), _sc(sm_scale=SM_SCALE), 1.0),  # GEN 1: the slope folded into units of 1/qk_scale
    ("cap_sm_scale", ("cap",), _sc(sm_scale=SM_SCALE), 2 * Q_GAIN),  # GEN 2; the smaller scale needs the larger gain
    ("rope_theta_scale", ("rope",), _sc(rope_theta=ROPE_THETA, rope_scale=ROPE_SCALE), 1.0),
)
DECODE_KV = (1, 54, 700, 2049)  # one request splits
PREFILL_QO, PREFILL_KV = (37, 1, 130, 0), (54, 1, 300, 17)


def _scalar_cases():
    cases = []
    # the three decode kernels: group 4 at d 128 (16x16x32 by default, VALU under r1), group 20 at d 128 (32x32x16 for
    # plain logits and RoPE), d 256 (VALU)
    for tag, hq, hkv, d, dtype, page in (("g4_d128", 8, 2, 128, F16, 16), ("g20_d128", 20, 1, 128, BF16, 5),
                                         ("g4_d256", 8, 2, 256, F16, 16)):
        for i, (name, feats, scal, gain) in enumerate(SCALAR_ROWS):
            cases.append(Case(f"decode_{tag}_{name}", "batch_decode", hq, hkv, d, dtype, DECODE_KV, page_size=page,
                              features=feats, scalars=scal, q_gain=gain, seed=10 + i))
    for i, (name, feats, scal, gain) in enumerate(SCALAR_ROWS):
        cases.append(Case(f"single_decode_{name}", "single_decode", 8, 2, 128, F16, (700,), features=feats,
                          scalars=scal, q_gain=gain, seed=30 + i))
    cases.append(Case("decode_e4m3_k_v_scale", "batch_decode", 8, 2, 128, F16, DECODE_KV, kv_dtype=E4M3,
                      scalars=_sc(k_scale=K_SCALE, v_scale=2.0), seed=40))
    cases.append(Case("decode_e4m3_g20_k_v_scale", "batch_decode", 20, 1, 64, BF16, DECODE_KV, kv_dtype=E4M3,
                      page_size=5, layout="HND", scalars=_sc(k_scale=K_SCALE, v_scale=0.37), seed=41))
    cases.append(Case("trtllm_decode_bmm_scales", "trtllm_decode", 8, 2, 128, F16, DECODE_KV, layout="HND",
                      scalars=_sc(bmm1_scale=BMM1_SCALE, bmm2_scale=BMM2_SCALE), seed=42))
    for i, (name, feats, scal, gain) in enumerate(SCALAR_ROWS + PREFILL_SCALE_ROWS):
        cases.append(Case(f"paged_prefill_{name}", "paged_prefill", 8, 2, 128, BF16 if i % 2 else F16, PREFILL_KV,
                          PREFILL_QO, page_size=(16, 5, 1)[i % 3], layout=("NHD", "HND")[i % 2], causal=i % 3 != 2,
                          features=feats, scalars=scal, q_gain=gain, seed=50 + i))
    # the ragged wrapper: the same rows (every scalar alone, all together, the three scale forms)
    for i, (name, feats, scal, gain) in enumerate(SCALAR_ROWS[:1] + SCALAR_ROWS[-1:] + PREFILL_SCALE_ROWS
                                                  + SCALAR_ROWS[1:-1]):
        cases.append(Case(f"ragged_prefill_{name}", "ragged_prefill", 8, 2, 64 if i % 2 else 128,
                          BF16 if i % 3 == 2 and i >= 5 else F16, PREFILL_KV, PREFILL_QO, causal=i != 7,
                          features=feats, scalars=scal, q_gain=gain, seed=(70 if i < 5 else 170) + i))
    for i, (name, feats, scal, gain) in enumerate(SINGLE_PREFILL_ROWS + PREFILL_SCALE_ROWS[:2]):
        cases.append(Case(f"single_prefill_{name}", "single_prefill", 8, 2, 128, BF16 if i % 2 else F16, (300,),
                          (130,), causal=i % 2 == 0, features=feats, scalars=scal, q_gain=gain, seed=80 + i))
    cases.append(Case("paged_prefill_e4m3_k_v_scale", "paged_prefill", 8, 2, 128, F16, PREFILL_KV, PREFILL_QO,
                      kv_dtype=E4M3, causal=True, scalars=_sc(k_scale=K_SCALE, v_scale=2.0), seed=90))
    cases.append(Case("trtllm_context_bmm_scales", "trtllm_context", 8, 2, 128, BF16, PREFILL_KV, PREFILL_QO,
                      layout="HND", causal=True, scalars=_sc(bmm1_scale=BMM1_SCALE, bmm2_scale=BMM2_SCALE), seed=91))
    return cases


DECODE_COMBOS = (("rope", "cap"), ("rope", "window"), ("alibi", "cap"), ("alibi", "window"),
                 ("alibi", "cap", "window"), ("cap", "window"))
# (hq, hkv): groups 1, 4, 7, 16, 20
DECODE_HEADS = ((2, 2), (8, 2), (14, 2), (16, 1), (20, 1))


def _decode_combo_cases():
    """36 rows: every combination with six of the (group, head_dim, cache, page size, dtype) draws.  Row j takes
    combination j % 6 and group j % 5 (coprime: 30 rows pair every combination with every group), head_dim and page
    size by slower cycles; an e4m3 cache every third row, an unsplit plan every fourth."""
    cases = []
    for j in range(36):
        feats = DECODE_COMBOS[j % 6]
        hq, hkv = DECODE_HEADS[j % 5]
        d = (128, 64, 256)[(j + j // 6) % 3]
        page = (16, 5, 1)[(j + j // 3) % 3]
        dtype = BF16 if (j + j // 2) % 2 else F16
        cases.append(Case(f"decode_{'_'.join(feats)}_g{hq // hkv}_d{d}_{j}", "batch_decode", hq, hkv, d, dtype,
                          DECODE_KV, kv_dtype=E4M3 if j % 3 == 1 else None, page_size=page,
                          layout="HND" if j % 2 else "NHD", features=feats, split=False if j % 4 == 3 else None,
                          q_gain=Q_GAIN if "cap" in feats else PLAIN_GAIN, seed=200 + j))
    # sinks on top of a cap; a request without keys (its row is dead)
    cases.append(Case("decode_sinks_cap_g4_d128", "batch_decode", 8, 2, 128, F16, DECODE_KV,
                      features=("cap", "sinks"), q_gain=Q_GAIN, seed=240))
    cases.append(Case("decode_sinks_cap_window_g20_d64", "batch_decode", 20, 1, 64, BF16, DECODE_KV, page_size=5,
                      features=("cap", "window", "sinks"), q_gain=Q_GAIN, seed=241))
    cases.append(Case("decode_alibi_cap_empty_request_g7_d128", "batch_decode", 14, 2, 128, F16, (54, 0, 700),
                      features=("alibi", "cap"), q_gain=Q_GAIN, seed=242, dead_rows=1))
    return cases


MASK_QO, MASK_KV = (37, 2, 130), (54, 3, 300)
SPLIT_QO, SPLIT_KV = (37, 2, 64), (54, 3, 700)  # fixed_split_size 128 cuts the last request into six chunks
# (features, causal): combinations without a mask come causal and non-causal; a mask replaces the causal mask
PREFILL_COMBOS = tuple((f + w, c) for f, cs in (
    (("alibi", "cap"), (True, False)), (("rope", "cap"), (True, False)), (("alibi", "mask"), (False,)),
    (("cap", "mask"), (False,)), (("alibi", "cap", "mask"), (False,)), (("rope", "mask"), (False,)),
    (("rope", "cap", "mask"), (False,))) for w in ((), ("window",)) for c in cs)


def _prefill_combo_cases():
    """The 18 (combination, window, causal) rows twice over, 36 cases: head_dim, dtype, cache, split and page size
    cycle at different rates.  An e4m3 cache stays at head_dim 64 / 128, as in tests/test_fuzz_gpu.py."""
    cases = []
    for j in range(36):
        feats, causal = PREFILL_COMBOS[j % 18]
        d = (128, 64, 256)[(j + j // 18) % 3]
        split = (j + j // 18) % 2 == 1
        fp8 = d != 256 and j % 4 == 2
        has_mask = "mask" in feats
        qo, kv = (SPLIT_QO, SPLIT_KV) if split else (MASK_QO, MASK_KV) if has_mask else (PREFILL_QO, PREFILL_KV)
        cases.append(Case(f"prefill_{'_'.join(feats)}_{'causal_' if causal else ''}d{d}_{j}", "paged_prefill", 8, 2, d,
                          BF16 if j % 3 == 1 else F16, kv, qo, kv_dtype=E4M3 if fp8 else None,
                          page_size=(16, 5, 1)[(j + j // 5) % 3], layout="HND" if j % 2 else "NHD", causal=causal,
                          features=feats, split=split, q_gain=Q_GAIN if "cap" in feats else PLAIN_GAIN, seed=300 + j))
    cases.append(Case("prefill_alibi_cap_mask_bf16_hi_lo_d128", "paged_prefill", 8, 2, 128, BF16, MASK_KV, MASK_QO,
                      features=("alibi", "cap", "mask"), split=False, hi_lo=True, q_gain=Q_GAIN, seed=340))
    cases.append(Case("ragged_prefill_rope_cap_window_d128", "ragged_prefill", 8, 2, 128, F16, PREFILL_KV, PREFILL_QO,
                      causal=True, features=("rope", "cap", "window"), split=False, q_gain=Q_GAIN, seed=341))
    cases.append(Case("single_prefill_alibi_cap_mask_d64", "single_prefill", 8, 2, 64, BF16, (300,), (130,),
                      features=("alibi", "cap", "mask"), q_gain=Q_GAIN, seed=342))
    # a request without keys: its five rows are dead
    cases.append(Case("prefill_alibi_cap_empty_request_d128", "paged_prefill", 8, 2, 128, F16, (54, 0, 300),
                      (37, 5, 130), causal=True, features=("alibi", "cap"), split=False, q_gain=Q_GAIN, seed=343,
                      dead_rows=5))
    # sinks with a combination: unsplit runs the SINK twin of the all-features kernel, split folds them in the merge
    for j, (feats, dtype, d, split) in enumerate((
            (("cap", "window"), F16, 128, False), (("cap", "window"), BF16, 64, True),
            (("alibi", "cap"), BF16, 128, False), (("alibi", "cap"), F16, 64, True),
            (("rope", "cap"), F16, 64, False), (("rope", "cap"), BF16, 128, True))):
        qo, kv = (SPLIT_QO, SPLIT_KV) if split else (PREFILL_QO, PREFILL_KV)
        cases.append(Case(f"prefill_sinks_{'_'.join(feats)}_d{d}_{'split' if split else 'unsplit'}", "paged_prefill",
                          8, 2, d, dtype, kv, qo, causal=True, features=feats + ("sinks",), split=split,
                          q_gain=Q_GAIN, seed=350 + j))
    # fp8 q / k / v with a feature: the upcast kernel
    for j, (feats, d, split) in enumerate(((("window",), 128, False), (("cap",), 64, True),
                                           (("cap", "mask"), 128, False))):
        qo, kv = (SPLIT_QO, SPLIT_KV) if split else (MASK_QO, MASK_KV)
        cases.append(Case(f"fp8_prefill_{'_'.join(feats)}_d{d}", "fp8_prefill", 8, 2, d, BF16 if j % 2 else F16, kv,
                          qo, kv_dtype=E4M3, page_size=(16, 5, 1)[j], causal="mask" not in feats, features=feats,
                          split=split, q_gain=Q_GAIN if "cap" in feats else PLAIN_GAIN, seed=360 + j))
    return cases


SCALAR_CASES = tuple(_scalar_cases())
DECODE_COMBO_CASES = tuple(_decode_combo_cases())
PREFILL_COMBO_CASES = tuple(_prefill_combo_cases())
ALL_CASES = SCALAR_CASES + DECODE_COMBO_CASES + PREFILL_COMBO_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
