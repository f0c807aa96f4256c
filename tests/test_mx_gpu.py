"""GPU: the MXFP4-weight grouped GEMM (csrc/gemm_mxfp4.hip) and the MXFP8 quantiser (csrc/mxfp8_quantize.hip) against
the fp64 oracle of tests/mx_ref.py.

The one-hot tests are the probe of the block-scaled MFMA's operand lane maps: with one operand one-hot every output is
ONE value of the other operand times a power of two, so the 16-bit result is exact and a wrong nibble order, k
permutation, row/column swap, scale-block assignment or group offset of a_scale changes bits.  The random tests hold
the reference test's tolerance (atol = rtol = 1e-2, tests/GEMM/test_groupwise_scaled_gemm_mxfp4.py:351)."""
import functools

import pytest
import torch

import mx_ref as R
from attn_inputs import indptr_of

pytestmark = pytest.mark.gpu

GROUPED = (4, 132, 0, 260)
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
OUT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _run(a, sa, b, sb, ms, out_dtype, fill=0, extra_rows=0, out=None):
    """a fp8 [cum_m, k], sa [cum_m, nkb], b [G, n, k/2], sb [G, n, nkb] on the CPU -> the kernel's result, on the CPU."""
    import flashinfer

    dev = "cuda"
    if extra_rows:
        pad = torch.full((extra_rows, a.shape[1]), 0x38, dtype=torch.uint8).view(a.dtype)
        a = torch.cat([a, pad])
    a_scale = R.group_swizzle_a(sa, ms, fill)
    need_rows = (a.shape[0] + 127 * len(ms)) // 128 * 128
    if need_rows > a_scale.shape[0]:
        a_scale = torch.cat([a_scale, torch.full((need_rows - a_scale.shape[0], a_scale.shape[1]), fill, dtype=torch.uint8)])
    b_scale = R.swizzle_b(sb, fill)
    res = flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise(
        a.to(dev), b.to(dev), a_scale.to(dev), b_scale.to(dev), indptr_of(ms).to(dev), out=out,
        out_dtype=None if out is not None else out_dtype)
    torch.cuda.synchronize()
    return res.cpu()


def _random_fp8_bytes(shape, fp8, g):
    """finite fp8 bit patterns, uniform over the codes"""
    raw = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    if fp8 == torch.float8_e4m3fn:
        raw = torch.where((raw & 0x7F) == 0x7F, raw & 0xF0, raw)  # the two NaN codes
    else:
        raw = torch.where((raw & 0x7C) == 0x7C, raw & 0xBF, raw)  # exponent 31: inf / NaN
    return raw.view(fp8)


# ---- a. lane-map probes, bit-exact ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8,out", [("e4m3", "bf16"), ("e5m2", "bf16"), ("e4m3", "f16")])
@pytest.mark.parametrize("ms,n,k", [((20,), 24, 256), (GROUPED, 136, 384)])
@pytest.mark.parametrize("one_hot", ["a", "b"])
def test_one_hot_is_bit_exact(one_hot, ms, n, k, fp8, out):
    g = torch.Generator().manual_seed(k + n + len(ms))
    fp8_dt, out_dt = FP8[fp8], OUT[out]
    cum_m, G, nkb = sum(ms), len(ms), k // 32
    lo, hi = (124, 131) if out == "f16" else (121, 134)  # f16: nothing overflows or leaves the subnormal range
    sa = torch.randint(lo, hi, (cum_m, nkb), dtype=torch.uint8, generator=g)
    sb = torch.randint(lo, hi, (G, n, nkb), dtype=torch.uint8, generator=g)
    if one_hot == "a":
        a = torch.zeros(cum_m, k, dtype=torch.float32)
        i = torch.arange(cum_m)
        a[i, (37 * i + 5) % k] = 1.0
        a = a.to(fp8_dt)
        b = torch.randint(0, 256, (G, n, k // 2), dtype=torch.uint8, generator=g)
    else:
        a = _random_fp8_bytes((cum_m, k), fp8_dt, g)
        codes = torch.zeros(G, n, k, dtype=torch.uint8)
        j = torch.arange(n)
        codes[:, j, (53 * j + 11) % k] = 2  # e2m1 code of 1.0
        b = codes[..., 0::2] | (codes[..., 1::2] << 4)
    want = R.group_gemm_ref(R.fp8_to_f64(a), sa, b, sb, ms)
    want16 = want.to(out_dt)
    assert torch.equal(want16.double(), want), "the case is not exact in the output dtype"
    got = _run(a, sa, b, sb, ms, out_dt)
    assert got.dtype == out_dt and got.shape == (cum_m, n)
    bad = (got.view(torch.int16) != want16.view(torch.int16)) & ~((got == 0) & (want16 == 0))
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[:4].tolist()}"


# ---- b. random parity at the reference's tolerance ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(ms, n, k, fp8):
    g = torch.Generator().manual_seed(hash((ms, n, k)) % 1000)
    a, sa = R.mx_floor_quantize(torch.randn(sum(ms), k, generator=g), FP8[fp8])
    b, sb = R.mx_floor_quantize(torch.randn(len(ms), n, k, generator=g) / k ** 0.5, "fp4")
    return a, sa, b, sb, R.group_gemm_ref(R.fp8_to_f64(a), sa, b, sb, ms)


@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("fp8", ["e4m3", "e5m2"])
@pytest.mark.parametrize("n,k", [(128, 128), (136, 384), (520, 2944)])
@pytest.mark.parametrize("ms", [(4,), (128,), GROUPED, (300, 8)])
def test_random_parity(ms, n, k, fp8, out):
    a, sa, b, sb, want = _random_case(ms, n, k, fp8)
    got = _run(a, sa, b, sb, ms, OUT[out])
    torch.testing.assert_close(got.double(), want, atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("fp8,out", [("e4m3", "bf16"), ("e5m2", "f16")])
def test_random_parity_many_workgroups(fp8, out):
    ms, n, k = (1000, 24, 2072), 1024, 512
    a, sa, b, sb, want = _random_case(ms, n, k, fp8)
    got = _run(a, sa, b, sb, ms, OUT[out])
    torch.testing.assert_close(got.double(), want, atol=1e-2, rtol=1e-2)


# ---- c. padding does not leak -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["bf16", "f16"])
def test_padding_does_not_leak(out):
    ms, n, k = GROUPED, 136, 384
    a, sa, b, sb, want = _random_case(ms, n, k, "e4m3")
    clean = _run(a, sa, b, sb, ms, OUT[out])
    sentinel = torch.full((sum(ms) + 8, n), 777.0, dtype=OUT[out], device="cuda")
    noisy = _run(a, sa, b, sb, ms, OUT[out], fill=254, extra_rows=8, out=sentinel)
    assert torch.equal(noisy[:sum(ms)].view(torch.int16), clean.view(torch.int16))
    assert bool((noisy[sum(ms):] == 777.0).all())
    torch.testing.assert_close(clean.double(), want, atol=1e-2, rtol=1e-2)


# ---- d. the quantiser, bit-exact ---------------------------------------------------------------------------------------
def _quant_input(m, k, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-20, 21, (m, 1), generator=g).double())
    if dtype == torch.float16:
        mag = mag.clamp(max=2.0 ** 12)  # randn * 2^12 stays finite in f16
    x = (torch.randn(m, k, generator=g).double() * mag).to(dtype)
    nb = k // 32
    # three special blocks in distinct places: all zero; amax exactly 448 * 2^e; amax the next representable value above.
    # (row, block) = (m // 2, nb // 2), (0, 0), (m - 1, nb - 1) differ whenever the input has more than one block; the
    # one-block input (m = 1, k = 32) takes the exact value as f16 and the value above it as bf16.
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    specials = [(0, 0, 1.75 * 2.0 ** 5), (m - 1, k - 32, (1.75 + ulp) * 2.0 ** 5)]  # 448 * 2^-3 = 56
    if m * nb == 1:
        specials = specials[:1] if dtype == torch.float16 else specials[1:]
    else:
        assert len({(m // 2, nb // 2), (0, 0), (m - 1, nb - 1)}) == 3
        x[m // 2, 32 * (nb // 2): 32 * (nb // 2) + 32] = 0
    for row, col, val in specials:
        x[row, col: col + 32] = (torch.rand(32, generator=g) * 20).to(dtype)
        x[row, col + 7] = -val
        assert x[row, col + 7].double().item() == -val
    return x


def _check_quantised(x2d, q, sf_linear, alignment=32):
    want_q, want_sf = R.mxfp8_quantize_ref(x2d, alignment)
    assert torch.equal(sf_linear, want_sf), f"{int((sf_linear != want_sf).sum())} scale bytes differ"
    assert torch.equal(q.view(torch.uint8), want_q.view(torch.uint8)), \
        f"{int((q.view(torch.uint8) != want_q.view(torch.uint8)).sum())} q bytes differ"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("swizzled", [True, False])
@pytest.mark.parametrize("k", [32, 96, 128, 4128])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 300])
def test_quantiser_is_bit_exact(m, k, swizzled, dtype):
    import flashinfer
    from flashinfer import fp8_quantization as Q

    x = _quant_input(m, k, dtype, 1000 * m + k)
    q, sf = flashinfer.mxfp8_quantize(x.cuda(), swizzled)
    assert q.dtype == torch.float8_e4m3fn and q.shape == (m, k) and sf.dtype == torch.uint8 and sf.dim() == 1
    nkb = k // 32
    # every byte of the scale buffer is written: run again into a prefilled buffer
    q2 = torch.empty_like(q)
    sf2 = torch.full_like(sf, 0xAA)
    Q._quantize_into(x.cuda(), q2, sf2, swizzled, 32)
    torch.cuda.synchronize()
    q, sf, sf2 = q.cpu(), sf.cpu(), sf2.cpu()
    assert torch.equal(sf, sf2) and torch.equal(q.view(torch.uint8), q2.cpu().view(torch.uint8))
    if swizzled:
        assert sf.numel() == R.ceil_to(m, 128) * R.ceil_to(nkb, 4)
        _check_quantised(x, q, R.unswizzle(sf, m, nkb))
        assert torch.equal(sf, R.swizzle(R.unswizzle(sf, m, nkb)))  # padding bytes are 0
    else:
        assert sf.numel() == m * nkb
        _check_quantised(x, q, sf.view(m, nkb))


@pytest.mark.parametrize("swizzled", [True, False])
@pytest.mark.parametrize("k,alignment", [(96, 128), (32, 64), (4128, 256)])
def test_quantiser_pads_columns_with_zeros(k, alignment, swizzled):
    import flashinfer

    m = 130
    x = _quant_input(m, k, torch.bfloat16, k)
    q, sf = flashinfer.mxfp8_quantize(x.cuda(), swizzled, alignment)
    q, sf = q.cpu(), sf.cpu()
    k_pad = R.ceil_to(k, alignment)
    nkb = k_pad // 32
    assert q.shape == (m, k_pad) and not q[:, k:].view(torch.uint8).any()
    sf_linear = R.unswizzle(sf, m, nkb) if swizzled else sf.view(m, nkb)
    _check_quantised(x, q, sf_linear, alignment)
    assert not sf_linear[:, k // 32:].any()
    if swizzled:
        assert torch.equal(sf, R.swizzle(sf_linear))


def test_quantiser_3d_and_strided_input():
    import flashinfer

    x = _quant_input(6 * 50, 128, torch.float16, 9).view(6, 50, 128)
    q, sf = flashinfer.mxfp8_quantize(x.cuda(), False)
    assert q.shape == (6, 50, 128)
    _check_quantised(x.view(300, 128), q.cpu().view(300, 128), sf.cpu().view(300, 4))
    wide = torch.zeros(300, 256, dtype=torch.float16)
    wide[:, 64:192] = x.view(300, 128)
    q, sf = flashinfer.mxfp8_quantize(wide.cuda()[:, 64:192], True)  # a view with a row stride of 256
    _check_quantised(x.view(300, 128), q.cpu(), R.unswizzle(sf.cpu(), 300, 4))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_quantiser_grouped_layout(dtype):
    from flashinfer import fp8_quantization as Q

    ms = GROUPED
    for k in (384, 2176):  # 2176: 272 chunks of 8, a partial second pass of the 256-thread row team
        x = _quant_input(sum(ms) + 8, k, dtype, 11)  # 8 rows past m_indptr[G]: quantised, without scales
        q, a_scale = Q.mxfp8_quantize_grouped(x.cuda(), indptr_of(ms).cuda())
        rows = (sum(ms) + 8 + 127 * len(ms)) // 128 * 128
        assert a_scale.shape == (rows, k // 32) and a_scale.dtype == torch.uint8 and q.shape == x.shape
        q, a_scale = q.cpu(), a_scale.cpu()
        want_q, want_sf = R.mxfp8_quantize_ref(x)
        assert torch.equal(q.view(torch.uint8), want_q.view(torch.uint8))
        want_scale = torch.zeros(rows, k // 32, dtype=torch.uint8)
        grouped = R.group_swizzle_a(want_sf[:sum(ms)], ms)
        want_scale[:grouped.shape[0]] = grouped
        assert torch.equal(a_scale, want_scale)  # padding rows and the rows of no group are 0


def test_quantiser_grouped_layout_rows_of_no_group():
    """m_indptr need not start at 0 or end at cum_m: rows below m_indptr[0] and at or past m_indptr[G] belong to no
    group; they are quantised like every other row and have no scale row.  With m_indptr[0] >= 128 (the second input)
    whole scale rows lie in front of the first group: they are padding."""
    from flashinfer import fp8_quantization as Q

    k = 128
    for m, indptr in ((150, [8, 12, 144]), (140, [130, 134])):
        G = len(indptr) - 1
        x = _quant_input(m, k, torch.bfloat16, 13)
        q, a_scale = Q.mxfp8_quantize_grouped(x.cuda(), torch.tensor(indptr, dtype=torch.int32).cuda())
        q, a_scale = q.cpu(), a_scale.cpu()
        want_q, want_sf = R.mxfp8_quantize_ref(x)
        assert torch.equal(q.view(torch.uint8), want_q.view(torch.uint8))
        rows = (m + 127 * G) // 128 * 128
        want_scale = torch.zeros(rows * 4, dtype=torch.uint8)
        for g in range(G):
            first = (indptr[g] + 127 * g) // 128 * 128
            piece = R.swizzle(want_sf[indptr[g]:indptr[g + 1]])
            want_scale[first * 4: first * 4 + piece.numel()] = piece
        assert torch.equal(a_scale, want_scale.view(rows, 4)), indptr


# ---- e. pipeline, f. graph capture --------------------------------------------------------------------------------------
def _pipeline_inputs():
    ms, n, k = GROUPED, 136, 384
    g = torch.Generator().manual_seed(21)
    x = torch.randn(sum(ms), k, generator=g).to(torch.bfloat16)
    b, sb = R.mx_floor_quantize(torch.randn(len(ms), n, k, generator=g) / k ** 0.5, "fp4")
    return ms, x, b, sb


def test_pipeline_quantise_then_gemm():
    import flashinfer
    from flashinfer import fp8_quantization as Q

    ms, x, b, sb = _pipeline_inputs()
    indptr = indptr_of(ms).cuda()
    q, a_scale = Q.mxfp8_quantize_grouped(x.cuda(), indptr)
    out = flashinfer.gemm.group_gemm_mxfp4_nt_groupwise(q, b.cuda(), a_scale, R.swizzle_b(sb).cuda(), indptr)
    torch.cuda.synchronize()
    want_q, want_sf = R.mxfp8_quantize_ref(x)
    assert torch.equal(q.cpu().view(torch.uint8), want_q.view(torch.uint8))
    want = R.group_gemm_ref(R.fp8_to_f64(want_q), want_sf, b, sb, ms)
    torch.testing.assert_close(out.cpu().double(), want, atol=1e-2, rtol=1e-2)


def test_graph_capture_replays_the_eager_result():
    import flashinfer
    from flashinfer import fp8_quantization as Q

    ms, x, b, sb = _pipeline_inputs()
    indptr = indptr_of(ms).cuda()
    xd, bd, sbd = x.cuda(), b.cuda(), R.swizzle_b(sb).cuda()

    def step():
        q, a_scale = Q.mxfp8_quantize_grouped(xd, indptr)
        return flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise(q, bd, a_scale, sbd, indptr)

    eager = step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int16), eager.view(torch.int16))
