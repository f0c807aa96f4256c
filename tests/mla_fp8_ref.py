"""What the fp8 MLA tests (test_mla_fp8_cpu.py, test_mla_fp8_gpu.py) share: an fp64 restatement of
flashinfer.rope.mla_rope_quantize_fp8 with the fp8 rounding written out in numpy, and paged e4m3 caches whose owned
bytes cover all 254 finite e4m3 codes.

Plain functions, no fixtures."""
import numpy as np
import torch

from mla_plan_free_inputs import CKV, KPE, make_case

FP8 = {torch.float8_e4m3fn: dict(mbits=3, emin=-6, max=448.0, finite=127),    # codes 0x00..0x7E are finite
       torch.float8_e5m2: dict(mbits=2, emin=-14, max=57344.0, finite=124)}   # codes 0x00..0x7B are finite


def fp8_round(x, fp8_dtype):
    """float64 array -> the float64 values of the fp8 type nearest to it: round to nearest even, saturating at the
    largest finite value.  |x| = m 2^e with m in [1, 2) has the quantum 2^(max(e, emin) - mbits); x / quantum is exact
    in fp64 and np.rint rounds halves to even."""
    f = FP8[fp8_dtype]
    a = np.minimum(np.abs(np.asarray(x, dtype=np.float64)), f["max"])
    _, ex = np.frexp(a)  # a = m' 2^ex, m' in [0.5, 1)
    quantum = np.ldexp(1.0, np.maximum(ex - 1, f["emin"]) - f["mbits"])
    return np.copysign(np.minimum(np.rint(a / quantum) * quantum, f["max"]), x)


def fp8_order(values, fp8_dtype):
    """Exact fp8 values (float64) -> their place in the type's order as signed integers: +-(index among the finite
    non-negative codes), so that adjacent codes differ by one (and +0 and -0 are both 0)."""
    f = FP8[fp8_dtype]
    table = torch.arange(f["finite"], dtype=torch.uint8).view(fp8_dtype).double().numpy()
    idx = np.searchsorted(table, np.abs(values))
    assert (table[np.minimum(idx, len(table) - 1)] == np.abs(values)).all(), "not values of the fp8 type"
    return np.where(np.signbit(values), -idx, idx)


def rope_quantize_ref(q_rope, k_rope, q_nope, k_nope, cos_sin_cache, pos_ids, is_neox, fp8_dtype, scale_q, scale_kv):
    """mla_rope_quantize_fp8 in fp64: (q_rope, k_rope, q_nope, k_nope) as float64 arrays of exact fp8 values.  The
    scales are the float32 values the C ABI carries."""
    cs = cos_sin_cache.double().numpy()[pos_ids.long().numpy()]  # [nnz, 64]
    half = cs.shape[1] // 2
    cos, sin = cs[:, :half], cs[:, half:]

    def rotate(x):  # [nnz, (H,) 64]
        x = x.double().numpy()
        c, s = (cos, sin) if x.ndim == 2 else (cos[:, None], sin[:, None])
        y = np.empty_like(x)
        if is_neox:
            a, b = x[..., :half], x[..., half:]
            y[..., :half], y[..., half:] = a * c - b * s, b * c + a * s
        else:
            a, b = x[..., 0::2], x[..., 1::2]
            y[..., 0::2], y[..., 1::2] = a * c - b * s, b * c + a * s
        return y

    sq, sk = float(np.float32(scale_q)), float(np.float32(scale_kv))
    return (fp8_round(rotate(q_rope) * sq, fp8_dtype), fp8_round(rotate(k_rope) * sk, fp8_dtype),
            fp8_round(q_nope.double().numpy() * sq, fp8_dtype), fp8_round(k_nope.double().numpy() * sk, fp8_dtype))


# ---- e4m3 caches that cover every finite code ----
#
# The output bar (attn_inputs.tol) has an absolute part of 1e-3 to 2e-3 that is meant for values of order one, and a
# softmax whose logits are in the hundreds hides every token but one.  So the 254 codes cannot simply be drawn at
# random (their values run from 2^-9 to 448).  Instead every ckv column has a class: one sign and one exponent field
# (2 x 16 classes over 512 columns), and the mantissa is drawn per token.  Within a column nothing cancels, so a
# column of P.V carries the relative error of its terms, which the relative part of the bar covers at any magnitude;
# and q_nope in that column is scaled by 2^-exponent, so every column adds a term of order one to the logits.
# kpe columns hold 0.5 x randn rounded to e4m3.

def _column_classes():
    """(sign bit, exponent field) of each of the 512 ckv columns: the 32 classes in turn."""
    c = torch.arange(CKV)
    return (c % 2).to(torch.uint8), ((c // 2) % 16).to(torch.uint8)


def graded_ckv_bytes(tokens_shape, generator):
    """uint8 [*tokens_shape, 512]: sign and exponent by column class, mantissa random; never a NaN code (mantissa 7 of
    exponent field 15 becomes 6)."""
    sign, expo = _column_classes()
    mant = torch.randint(0, 8, (*tokens_shape, CKV), generator=generator, dtype=torch.uint8)
    mant = torch.where((expo == 15) & (mant == 7), torch.full_like(mant, 6), mant)
    return (sign << 7) | (expo << 3) | mant


def graded_q_nope(shape_prefix, dtype, generator):
    """q_nope [*shape_prefix, 512] of a 16-bit dtype for a graded cache: randn x 2^-(exponent of the column's class),
    so that q x k is of order one in every column."""
    _, expo = _column_classes()
    e = torch.clamp(expo.to(torch.float32), min=1.0) - 7.0  # field f >= 1: values in [2^(f-7), 2^(f-6)); field 0: below 2^-6
    return (torch.randn(*shape_prefix, CKV, generator=generator) * torch.exp2(-e)).to(dtype)


def make_fp8_case(kv_lens, q_len, H, ps, dtype, seed, fp8_query=False, max_blocks=None):
    """mla_plan_free_inputs.make_case with an e4m3 cache: `cache8` [pages, ps, 576] float8_e4m3fn (graded ckv columns,
    natural kpe columns; every byte no request owns is 0x7F, a NaN), `cache` = its exact upcast to `dtype`, `q` in
    `dtype` (graded q_nope) -- or, with fp8_query, `q8` and every cache column 0.5 x randn rounded to e4m3 (a query
    that cannot be graded: 2^-8 x randn is below e4m3's normal range) and `q` the upcast of `q8` to `dtype`.
    A graded cache with a request of 64 tokens or more owns every one of the 254 finite codes."""
    from attn_inputs import owned_slots

    c = make_case(kv_lens, q_len, H, ps, dtype, seed, max_blocks=max_blocks)
    g = torch.Generator().manual_seed(1000 + seed)
    pages = c["cache"].shape[0]
    raw = torch.empty(pages, ps, CKV + KPE, dtype=torch.uint8)
    raw[..., :] = (torch.randn(pages, ps, CKV + KPE, generator=g) * 0.5).to(torch.float8_e4m3fn).view(torch.uint8)
    if not fp8_query:
        raw[..., :CKV] = graded_ckv_bytes((pages, ps), g)
    owned = owned_slots(kv_lens, c["indptr"], c["indices"], ps, pages)
    if not fp8_query and max(kv_lens) >= 64:
        seen = torch.unique(raw[owned])
        assert len(seen) == 254 and 0x7F not in seen and 0xFF not in seen, "the owned bytes must cover the finite codes"
    raw[~owned] = 0x7F
    cache8 = raw.view(torch.float8_e4m3fn)
    B = len(kv_lens)
    if fp8_query:
        q8 = (torch.randn(B, q_len, H, CKV + KPE, generator=g) * 0.5).to(torch.float8_e4m3fn)
        q = q8.to(dtype)
    else:
        q8 = None
        q = torch.cat([graded_q_nope((B, q_len, H), dtype, g),
                       torch.randn(B, q_len, H, KPE, generator=g).to(dtype)], dim=-1)
    return dict(c, cache8=cache8, cache=cache8.to(dtype), q=q, q8=q8)
