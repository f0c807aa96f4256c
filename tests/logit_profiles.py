"""Attention inputs whose logits are prescribed: the logit of query row i and key j is a[i] * g[j] + offset nats at
sm_scale = 1 / sqrt(d), up to the rounding of the input type and a small per-row noise.  Plain torch on the CPU.

randn inputs give logits of about N(0, 1) nats: the row maximum is found in the first KV tile and hardly moves
afterwards, so the online-softmax rescale of every kernel runs with alpha ~ 1 on every tile but the first.  The
profiles here move the maximum on purpose -- up and down by whole tiles, inside a tile, on one side and the other of
the thresholds of the deferred rescales (2^6 in prefill_kernel.h / prefill_qkvo_kernel.h, 2^3 in prefill_fp8_kernel.h),
at tile and split-chunk boundaries, on some rows of a wave and not on others -- and put the logits at large offsets,
where the maximum subtraction and the base-2 lse work at magnitudes close to the "saw no key" sentinel -5e4.

The oracle always gets the rounded tensors, so the rounding of the inputs is not an error source: it only moves the
logits a little off the prescription (tests/test_logit_profiles_cpu.py bounds that and checks that every profile keeps
the property it is named for)."""
import functools
import math

import torch

LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
TILE = 64     # keys per prefill KV tile
CHUNK = 128   # keys per split-KV chunk in the tests that force a split (fixed_split_size=128; decode plans on page 16)
KV, QO = 333, 150  # five 64-key tiles, the last partial; three 64-row query tiles, the last partial


def _signs(n, gen):
    return (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()


def structured(g, a, heads_q, heads_k, n, sm_scale, gen, offset=0.0, noise=0.05):
    """(q [qo, heads_q, n], k [kv, heads_k, n]) in fp64 with q . k * sm_scale = a[i] g[j] + offset (+ noise).  The
    first half of the n dims carries a[i] g[j] on a +-1 vector u, the second half the offset on a second +-1 vector w,
    so the structured part keeps its resolution next to a large offset: every query holds the same second half and
    every key the same one, whose rounding shifts all logits alike."""
    g, a = g.double(), a.double()
    h = n // 2
    u, w = _signs(h, gen), _signs(n - h, gen)
    s = math.sqrt(1.0 / (sm_scale * h))
    b = math.sqrt(abs(offset) / (sm_scale * (n - h)))
    q = torch.empty(len(a), heads_q, n, dtype=torch.float64)
    k = torch.empty(len(g), heads_k, n, dtype=torch.float64)
    q[:, :, :h] = a[:, None, None] * u * s + noise * torch.randn(len(a), heads_q, h, generator=gen, dtype=torch.float64)
    k[:, :, :h] = g[:, None, None] * u * s
    q[:, :, h:] = b * w
    k[:, :, h:] = math.copysign(b, offset) * w
    return q, k


def build(g, a, d, hq, hkv, dtype, seed, offset=0.0, noise=0.05, dv=None):
    """(q [qo, hq, d], k [kv, hkv, d], v [kv, hkv, dv or d]) of `dtype` (a 16-bit type; quantise afterwards for fp8).
    u is a +-1 vector and s = sqrt(sqrt(d) / (d/2)): q[i, :, :d/2] = a[i] u s + noise * randn, k[j, :, :d/2] = g[j] u s;
    b = sqrt(|offset| sqrt(d) / (d/2)) and w a second +-1 vector: q[:, :, d/2:] = b w, k[:, :, d/2:] = +-b w; v is randn.
    The noise term adds noise * d^-1/4 * N(0, 1) * g[j] to row i's logits: a small change of a[i], per row and head."""
    gen = torch.Generator().manual_seed(seed)
    q, k = structured(g, a, hq, hkv, d, 1.0 / math.sqrt(d), gen, offset, noise)
    v = torch.randn(len(g), hkv, dv or d, generator=gen)
    return q.to(dtype), k.to(dtype), v.to(dtype)


CKV, KPE = 512, 64
MLA_SM = 1.0 / math.sqrt(128 + 64)


def build_mla(g, a, heads, dtype, seed, offset=0.0, noise=0.05):
    """(q_nope [qo, heads, 512], q_pe [qo, heads, 64], ckv [kv, 512], kpe [kv, 64]) for MLA at sm_scale = MLA_SM: the
    structure sits in the 64 rope dims, ckv is randn and q_nope 0.05 * randn (0.08 nats of unstructured logit)."""
    gen = torch.Generator().manual_seed(seed)
    q_pe, kpe = structured(g, a, heads, 1, KPE, MLA_SM, gen, offset, noise)
    ckv = torch.randn(len(g), CKV, generator=gen)
    q_nope = 0.05 * torch.randn(len(a), heads, CKV, generator=gen)
    return q_nope.to(dtype), q_pe.to(dtype), ckv.to(dtype), kpe[:, 0].to(dtype)


# ---- profiles ---------------------------------------------------------------------------------------------------
# g over the kv positions as a function of (kv, vis); vis = the number of keys every query row sees (kv without a
# causal mask, kv - qo + 1 with one), so "the last visible key" is key vis - 1: the last one of row 0.
def _tile_ramp(step):
    return lambda kv, vis: (torch.arange(kv) // TILE).double() * (step * LN2)


def _step_then_flat(step):
    return lambda kv, vis: (torch.arange(kv) >= TILE).double() * (step * LN2)


def _key_ramp(slope):
    return lambda kv, vis: torch.arange(kv).double() * slope


def _spike(at, height):
    """`at`: a key index, or None for the last visible key."""
    def g(kv, vis):
        out = torch.zeros(kv, dtype=torch.float64)
        out[vis - 1 if at is None else at] = height
        return out
    return g


def _alternating(mag):
    return lambda kv, vis: mag * (1.0 - 2.0 * (torch.arange(kv) % 2).double())


def _ones(qo):
    return torch.ones(qo, dtype=torch.float64)


def _mixed(qo):
    return torch.tensor([1.0, -1.0, 0.0, 0.01], dtype=torch.float64).repeat(-(-qo // 4))[:qo]


# name -> (g, a, offset in nats, noise, run keywords)
# The step profiles sit 0.1 log2 units from a threshold: their noise is 0.002 (5 sigma = 0.02 log2 units at 5.9), so
# that with the input rounding (2^-7 relative for bf16: 0.05) every row stays on its side.
_TABLE = {
    **{f"tile_up({s})": (_tile_ramp(s), _ones, 0.0, 0.05, {}) for s in (5, 7, 2, 4)},
    **{f"step_then_flat({s})": (_step_then_flat(s), _ones, 0.0, 0.002, {}) for s in (5.9, 6.1, 2.5, 3.5)},
    **{f"tile_down({s})": (_tile_ramp(-s), _ones, 0.0, 0.05, {}) for s in (4, 7)},
    "key_ramp(0.25)": (_key_ramp(0.25), _ones, 0.0, 0.05, {}),
    "late_spike(8)": (_spike(None, 8.0), _ones, 0.0, 0.05, {}),
    "late_spike(40)": (_spike(None, 40.0), _ones, 0.0, 0.05, {}),
    **{f"spike_at({n})": (_spike(at, 8.0), _ones, 0.0, 0.05, {})
       for n, at in (("63", TILE - 1), ("64", TILE), ("0", 0), ("chunk_end-1", CHUNK - 1), ("chunk_end", CHUNK))},
    "mixed_rows": (_key_ramp(0.25), _mixed, 0.0, 0.05, {}),
    **{f"offset({o:+d})": (_key_ramp(0.05), _ones, float(o), 0.05, {}) for o in (2000, -2000, -30000)},
    "cap_saturated": (_alternating(500.0), _ones, 0.0, 0.05, dict(logits_soft_cap=30.0)),
}

PROFILES_16 = tuple(_TABLE)
# The profiles of the fp8 q/k/v paths, as (name, causal).  A profile is here only if fp8_attention_ref differs from
# exact attention on the same dequantised inputs by at most a quarter of the fp8 bar (the kernel's probabilities land
# on another 3- or 2-bit grid than the untiled oracle's, and the two may differ by about the sum of their own rounding
# errors); tests/test_logit_profiles_cpu.py holds the list to that.  A per-key ramp and the causal tile ramps miss it.
PROFILES_FP8 = (
    ("tile_up(2)", False), ("tile_up(4)", False),
    ("tile_down(4)", False), ("tile_down(4)", True),
    ("step_then_flat(2.5)", False), ("step_then_flat(2.5)", True),
    ("step_then_flat(3.5)", False), ("step_then_flat(3.5)", True),
    ("late_spike(8)", False), ("late_spike(8)", True),
)
FP8_BAR = {torch.float8_e4m3fn: 5e-2, torch.float8_e5m2: 1e-1}  # tests/test_prefill_gpu.py


def spec(name, kv=KV, qo=QO, causal=False, rows=None):
    """(g [kv], a [rows or qo], offset, noise, run keywords) of a profile for requests of qo query rows; rows > qo
    gives the rows of several such requests over the same keys."""
    g, a, offset, noise, kw = _TABLE[name]
    return g(kv, kv - qo + 1 if causal else kv), a(rows or qo), offset, noise, dict(kw)


def is_offset(name):
    return _TABLE[name][2] != 0.0


def seed_of(name, *more):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) + sum(int(m) * 7919 for m in more)


@functools.lru_cache(maxsize=None)
def inputs(name, d, hq, hkv, dtype, causal=False, kv=KV, qo=QO, dv=None, rows=None):
    """(q, k, v, run keywords) of a profile: seeded by the case, computed once and never modified."""
    g, a, offset, noise, kw = spec(name, kv, qo, causal, rows)
    return (*build(g, a, d, hq, hkv, dtype, seed_of(name, d, hq, causal), offset, noise, dv), kw)


@functools.lru_cache(maxsize=None)
def mla_inputs(name, heads, dtype, causal=False, kv=KV, qo=1, rows=None):
    g, a, offset, noise, _ = spec(name, kv, qo, causal, rows)
    return build_mla(g, a, heads, dtype, seed_of(name, heads, causal, qo), offset, noise)


def fp8_inputs(name, d, f8, causal, hq=8, hkv=2):
    """The profile built in fp16, then quantised per head as the fp8 tests do: (q8, k8, v8, sq, sk, sv)."""
    from oracle import attention_ref as R

    q, k, v, _ = inputs(name, d, hq, hkv, torch.float16, causal)
    q8, sq = R.per_head_symmetric_quant(q, f8)
    k8, sk = R.per_head_symmetric_quant(k, f8)
    v8, sv = R.per_head_symmetric_quant(v, f8)
    return q8, k8, v8, sq, sk, sv
