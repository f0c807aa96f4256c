"""GPU parity: fp8 groupwise (grouped) GEMM against dequantise-then-matmul, the reference's own check
(tests/GEMM/test_groupwise_scaled_gemm_fp8.py:35-71, 135-192; atol = rtol = 1e-2 in bf16 output).

The library picks the kernel by problem size (256 x 256 tiles from half a tile per CU on, 128 x 256 tiles for groups
of few rows, the 128 x 128 kernel below that).  Every test here runs once per entry of VARIANTS, in this process (the plain
functions are the default run, TestKernelVariants at the end of the file repeats them for the other entries): the
switches are set through _lib.set_option before the test and returned to the environment's values after it.
  default -> the 128 x 128 kernel and the size-based choice
  FI_GEMM_WS_MIN_TILES=0 FI_GEMM_BIG_MIN_TILES=0 -> every shape takes the 256 x 256 kernel (gemm_big.hip)
  FI_GEMM_WS_MIN_TILES=0 FI_GEMM_DMA_TM=256 / 128 -> every shape takes the persistent LDS-DMA kernel with
                                       256 x 128 / 128 x 256 tiles
  ... FI_GEMM_HW_SCALES=0 -> the 256 x 256 kernel without its hardware-scale path (power-of-two scales, which the
                                       reference's quantiser produces, otherwise ride the MFMA's E8M0 block scales)

e5m2 operands and 128-row a_scale blocks (scale_granularity_mnk = (128, 128, 128)) are checked against an fp64 product
of the same fp8 bytes (_fp64_reference; the a_scale row of each row of a is _a_scale_rows), with scales from a formula
that gives neighbouring blocks different values, so that an off-by-one block index cannot pass."""
import math

import pytest
import torch

from attn_inputs import indptr_of
from flashinfer import _lib
from oracle import gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

VARIANTS = {
    "default": {},
    "dma-256x256": {"FI_GEMM_WS_MIN_TILES": 0, "FI_GEMM_BIG_MIN_TILES": 0},
    "dma-256x128": {"FI_GEMM_WS_MIN_TILES": 0, "FI_GEMM_DMA_TM": 256, "FI_GEMM_BIG": 0},
    "dma-128x256": {"FI_GEMM_WS_MIN_TILES": 0, "FI_GEMM_DMA_TM": 128},
    "dma-256x256-fold-only": {"FI_GEMM_WS_MIN_TILES": 0, "FI_GEMM_BIG_MIN_TILES": 0, "FI_GEMM_HW_SCALES": 0},
}


@pytest.fixture(autouse=True)
def kernel_variant(request):
    """Sets the switches of a VARIANTS entry for the test (TestKernelVariants names it; a plain test runs "default")
    and returns every one of them to the environment's value afterwards."""
    options = VARIANTS[getattr(request, "param", "default")]
    try:
        for name, value in options.items():
            _lib.set_option(name, value)
        yield
    finally:
        for name in options:
            _lib.set_option(name, None)


@pytest.mark.parametrize("m", [4, 128, 300, 1024])
@pytest.mark.parametrize("n,k", [(128, 128), (256, 512), (1032, 256)])
@pytest.mark.parametrize("mode", ["MN", "K"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_gemm_fp8_nt_groupwise(m, n, k, mode, out_dtype):
    import flashinfer

    torch.manual_seed(0)
    a = torch.randn(m, k)
    b = torch.randn(n, k) / math.sqrt(k)
    n_pad = -(-n // 128) * 128
    b_pad = torch.zeros(n_pad, k)
    b_pad[:n] = b
    a8, sa = G.quantize_fp8(a, (1, 128), mode)
    b8p, sb = G.quantize_fp8(b_pad, (128, 128), mode)
    b8 = b8p[:n].contiguous()
    out = flashinfer.gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa.to(DEV), sb.to(DEV), scale_major_mode=mode,
                                           out_dtype=out_dtype)
    ref = G.gemm_fp8_nt_groupwise_ref(a8, b8p, sa, sb, mode)[:, :n]
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("mode", ["MN", "K"])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_gemm_fp8_nt_groupwise_large(mode, out_dtype):
    """Enough 256 x 128 tiles (33 x 16 >= 2 x CUs) for the persistent large-problem kernel; random data."""
    import flashinfer

    torch.manual_seed(5)
    m, n, k = 8195, 2048, 640
    a = torch.randn(m, k)
    b = torch.randn(n, k) / math.sqrt(k)
    a8, sa = G.quantize_fp8(a, (1, 128), mode)
    b8, sb = G.quantize_fp8(b, (128, 128), mode)
    out = flashinfer.gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa.to(DEV), sb.to(DEV), scale_major_mode=mode,
                                           out_dtype=out_dtype)
    ref = G.gemm_fp8_nt_groupwise_ref(a8, b8, sa, sb, mode)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("ms", [[4, 128, 0, 260], [512, 512], [128] * 8, [4]])
@pytest.mark.parametrize("n,k", [(256, 256), (512, 1024)])
@pytest.mark.parametrize("mode", ["MN", "K"])
def test_group_gemm_fp8_nt_groupwise(ms, n, k, mode):
    import flashinfer

    torch.manual_seed(0)
    g = len(ms)
    cum = sum(ms)
    a = torch.randn(cum, k)
    b = torch.randn(g, n, k) / math.sqrt(k)
    a8, sa = G.quantize_fp8(a, (1, 128), mode)
    b8, sb = G.quantize_fp8(b, (1, 128, 128), mode)
    m_indptr = indptr_of(ms)
    out = flashinfer.group_gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa.to(DEV), sb.to(DEV), m_indptr.to(DEV),
                                                 scale_major_mode=mode)
    ref = G.group_gemm_fp8_nt_groupwise_ref(a8, b8, sa, sb, m_indptr, mode)
    assert out.dtype == torch.bfloat16
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("scales", ["arbitrary", "one_not_pow2", "subnormal_and_huge"])
@pytest.mark.parametrize("mode", ["MN", "K"])
def test_group_gemm_scales_that_are_not_powers_of_two(scales, mode):
    """The reference takes any f32 scale (csrc/group_gemm_fp8_groupwise_sm100.cu:89-124); its own quantiser happens to
    produce powers of two (flashinfer/testing/utils.py:96-98).  The 256 x 256 kernel feeds power-of-two scales to the
    MFMA's hardware block scales and must fall back to the general fold when a single scale is not one -- checked on
    the device, per call.  (TestKernelVariants sends this case through every large-problem kernel.)"""
    import flashinfer

    torch.manual_seed(5)
    ms, n, k = [260, 4, 512], 512, 512
    g, cum = len(ms), sum(ms)
    a8 = torch.randn(cum, k).to(torch.float8_e4m3fn)
    b8 = (torch.randn(g, n, k) / math.sqrt(k)).to(torch.float8_e4m3fn)
    if scales == "arbitrary":
        sa = torch.rand(k // 128, cum) + 0.5
        sb = torch.rand(g, k // 128, n // 128) + 0.5
    elif scales == "one_not_pow2":
        sa = torch.pow(2.0, torch.randint(-3, 4, (k // 128, cum)).float())
        sb = torch.pow(2.0, torch.randint(-3, 4, (g, k // 128, n // 128)).float())
        sb[2, 3, 1] = 0.75
    else:  # powers of two, but outside what an E8M0 byte of a NORMAL f32 holds, or not positive: no hardware path
        sa = torch.pow(2.0, torch.randint(-3, 4, (k // 128, cum)).float())
        sb = torch.pow(2.0, torch.randint(-3, 4, (g, k // 128, n // 128)).float())
        sa[1, 7] = 2.0 ** -130   # subnormal f32
        sa[2, 300] = -2.0        # negative
    if mode == "K":
        sa, sb = sa.t().contiguous(), sb.transpose(1, 2).contiguous()
    m_indptr = indptr_of(ms)
    out = flashinfer.group_gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa.to(DEV), sb.to(DEV), m_indptr.to(DEV),
                                                 scale_major_mode=mode)
    ref = G.group_gemm_fp8_nt_groupwise_ref(a8, b8, sa, sb, m_indptr, mode)
    torch.testing.assert_close(out.float().cpu(), ref.float(), atol=1e-2, rtol=1e-2)


def test_group_gemm_exact_small_integers():
    """Known-answer: small-integer operands and power-of-two scales are exact in fp8 x fp8 -> f32, so the
    kernel must reproduce the integer result bit for bit (catches operand-layout / k-order mistakes that a
    random-data tolerance could hide)."""
    import flashinfer

    torch.manual_seed(1)
    g, m, n, k = 2, 132, 136, 256
    a = torch.randint(-4, 5, (g * m, k)).float()
    b = torch.randint(-4, 5, (g, n, k)).float()
    a8, b8 = a.to(torch.float8_e4m3fn), b.to(torch.float8_e4m3fn)
    sa = torch.pow(2.0, torch.randint(-2, 3, (k // 128, g * m)).float())
    sb = torch.pow(2.0, torch.randint(-2, 3, (g, k // 128, -(-n // 128))).float())
    m_indptr = torch.tensor([0, m, 2 * m], dtype=torch.int32)
    out = flashinfer.group_gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa.to(DEV), sb.to(DEV), m_indptr.to(DEV),
                                                 out_dtype=torch.float16)
    ref = torch.zeros(g * m, n, dtype=torch.float64)
    for gi in range(g):
        for kb in range(k // 128):
            part = a[gi * m:(gi + 1) * m, kb * 128:(kb + 1) * 128].double() @ b[gi, :, kb * 128:(kb + 1) * 128].double().T
            ref[gi * m:(gi + 1) * m] += part * sa[kb, gi * m:(gi + 1) * m, None].double() * \
                sb[gi, kb].double().repeat_interleave(128)[:n][None]
    assert ref.abs().max() < 60000
    torch.testing.assert_close(out.float().cpu(), ref.float().half().float(), atol=0, rtol=0)


def test_gemm_errors():
    import flashinfer

    a = torch.zeros(8, 128, device=DEV).to(torch.float8_e4m3fn)
    b = torch.zeros(16, 256, device=DEV).to(torch.float8_e4m3fn)
    s = torch.ones(1, 8, device=DEV)
    with pytest.raises(ValueError):
        flashinfer.gemm_fp8_nt_groupwise(a, b, s, s, scale_major_mode="MN")
    with pytest.raises(ValueError):
        flashinfer.gemm_fp8_nt_groupwise(a, a, s, s, scale_major_mode="MN", out_dtype=torch.float32)
    # only 1 or 128 rows of a and 128 x 128 blocks of b per scale: anything else is refused with the granularity in
    # the message, before any kernel is launched (the output keeps what it held)
    b = torch.zeros(16, 128, device=DEV).to(torch.float8_e4m3fn)
    sb = torch.ones(1, 1, device=DEV)
    m_indptr = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    for gran in [(64, 128, 128), (1, 64, 128)]:
        message = r"scale granularity \(%d,%d,%d\)" % gran
        out = torch.full((8, 16), 7.0, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match=message):
            flashinfer.gemm_fp8_nt_groupwise(a, b, s, sb, scale_major_mode="MN", scale_granularity_mnk=gran, out=out)
        with pytest.raises(RuntimeError, match=message):
            flashinfer.group_gemm_fp8_nt_groupwise(a, b[None], s, sb[None], m_indptr, scale_granularity_mnk=gran,
                                                   out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())


E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
FORMAT_PAIRS = [(E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3), (E5M2, E5M2)]
_FMT_ID = {E4M3: "e4m3", E5M2: "e5m2"}.get


def _a_scale_rows(gm, m_indptr):
    """The a_scale row of every row of a (m_indptr = [0, m] for the ungrouped GEMM).  gm == 1: the row itself.
    gm == 128: the group's scale rows start at m_indptr[g] // 128 and block the group's rows from its first one
    (the reference: include/flashinfer/gemm/group_gemm_fp8_groupwise_sm100.cuh:52-69, sf_m_offset)."""
    m_indptr = m_indptr.long()
    rows = torch.arange(int(m_indptr[-1]))
    begin = torch.repeat_interleave(m_indptr[:-1], m_indptr[1:] - m_indptr[:-1])
    return rows if gm == 1 else begin // gm + (rows - begin) // gm


def _formula_scales(ms, n, k, gm):
    """Scales whose neighbouring blocks (along m, n, k and the group) always differ, all powers of two:
    a_scale (k // 128, rows), b_scale (G, k // 128, ceil(n / 128)), both in the "MN" layout."""
    kb = torch.arange(k // 128)
    rows = -(-sum(ms) // gm)
    sa = torch.pow(2.0, ((3 * torch.arange(rows)[None, :] + kb[:, None]) % 5 - 2).float())
    nb = torch.arange(-(-n // 128))
    g = torch.arange(len(ms))
    sb = torch.pow(2.0, ((2 * nb[None, None, :] + kb[None, :, None] + g[:, None, None]) % 3 - 1).float())
    return sa, sb


def _small_integers(shape, fmt):
    """Integers in -3..3 as fp8; both formats hold them exactly."""
    x = torch.randint(-3, 4, shape).float()
    x8 = x.to(fmt)
    assert torch.equal(x8.float(), x)
    return x8


def _fp64_reference(a8, b8, sa, sb, m_indptr, gm):
    """(a . sa) (b[g] . sb[g])^T per group and per 128-wide k block in fp64, from the fp8 bytes the kernel gets.
    a8 (cum_m, k), b8 (G, n, k); sa (k // 128, a-scale rows) and sb (G, k // 128, ceil(n / 128)) in the "MN" layout."""
    cum, k = a8.shape
    n = b8.shape[1]
    a, b = a8.float().double(), b8.float().double()
    a_rows = _a_scale_rows(gm, m_indptr)
    ref = torch.zeros(cum, n, dtype=torch.float64)
    for gi in range(b8.shape[0]):
        lo, hi = int(m_indptr[gi]), int(m_indptr[gi + 1])
        for kb in range(k // 128):
            part = a[lo:hi, kb * 128:(kb + 1) * 128] @ b[gi, :, kb * 128:(kb + 1) * 128].T
            ref[lo:hi] += part * sa[kb, a_rows[lo:hi], None].double() * sb[gi, kb].double().repeat_interleave(128)[:n][None]
    return ref


def _run_gemm(a8, b8, sa, sb, m_indptr, gm, mode, out_dtype, grouped):
    """The kernel's result on the CPU as f32; sa / sb come in the "MN" layout and go out in `mode`'s."""
    import flashinfer

    if mode == "K":
        sa, sb = sa.t(), sb.transpose(1, 2)
    sa, sb = sa.contiguous().to(DEV), sb.contiguous().to(DEV)
    if grouped:
        out = flashinfer.group_gemm_fp8_nt_groupwise(a8.to(DEV), b8.to(DEV), sa, sb, m_indptr.to(DEV),
                                                     scale_granularity_mnk=(gm, 128, 128), scale_major_mode=mode,
                                                     out_dtype=out_dtype)
    else:
        out = flashinfer.gemm_fp8_nt_groupwise(a8.to(DEV), b8[0].to(DEV), sa, sb[0], scale_major_mode=mode,
                                               scale_granularity_mnk=(gm, 128, 128), out_dtype=out_dtype)
    assert out.dtype == out_dtype
    return out.float().cpu()


def _exact_formula_scales(ms, n, k, gm, mode, grouped, fmts=(E4M3, E4M3), last_a_scale=None):
    """Small-integer operands and formula scales: the f16 result must be exact."""
    torch.manual_seed(7)
    a8 = _small_integers((sum(ms), k), fmts[0])
    b8 = _small_integers((len(ms), n, k), fmts[1])
    sa, sb = _formula_scales(ms, n, k, gm)
    if last_a_scale is not None:
        sa[-1, -1] = last_a_scale  # the last element in memory order of either layout
    m_indptr = indptr_of(ms)
    ref = _fp64_reference(a8, b8, sa, sb, m_indptr, gm)
    assert ref.abs().max() < 60000
    out = _run_gemm(a8, b8, sa, sb, m_indptr, gm, mode, torch.float16, grouped)
    torch.testing.assert_close(out, ref.float().half().float(), atol=0, rtol=0)


def _decode_fp8_codes(exp_bits, man_bits, bias):
    """Value of each of the 256 codes of a sign | exponent | mantissa byte in fp64, from the format's definition
    (no infinities or NaNs: the caller masks those codes)."""
    code = torch.arange(256)
    sign = 1.0 - 2.0 * (code >> 7).double()
    e = (code >> man_bits) & ((1 << exp_bits) - 1)
    f = (code & ((1 << man_bits) - 1)).double() / (1 << man_bits)
    normal = torch.pow(2.0, (e - bias).double()) * (1.0 + f)
    subnormal = 2.0 ** (1 - bias) * f
    return sign * torch.where(e == 0, subnormal, normal)


@pytest.mark.parametrize("scale", [1.0, 0.75])
@pytest.mark.parametrize("out_dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("fmt", [E4M3, E5M2], ids=_FMT_ID)
def test_gemm_fp8_format_decode_tables(fmt, side, out_dtype, scale):
    """Every finite code of an fp8 format -- both signs, the subnormals (e5m2 from 2^-16, e4m3 from 2^-9), the largest
    values -- times a 128 x 128 identity in e4m3: the output is the code's value times the scale, bit for bit (scale 1
    can ride the MFMA's hardware scales, 0.75 takes the fold).  An operand decoded in the other format, on either side
    of the MFMA, cannot pass."""
    codes = torch.arange(256, dtype=torch.uint8)
    finite = torch.isfinite(codes.view(fmt).float())
    assert int((~finite).sum()) == (2 if fmt == E4M3 else 8)
    codes = torch.where(finite, codes, torch.zeros_like(codes))
    value = torch.where(finite, _decode_fp8_codes(4, 3, 7) if fmt == E4M3 else _decode_fp8_codes(5, 2, 15),
                        torch.zeros(256, dtype=torch.float64))
    assert torch.equal(codes.view(fmt).float().double(), value)  # torch's table is the format's definition
    x = torch.zeros(256, 128, dtype=torch.uint8)
    x[torch.arange(256), torch.arange(256) % 128] = codes
    x8 = x.view(fmt)
    expected = x8.float().double() * scale  # (256, 128): row r holds code r at column r % 128
    assert torch.equal(expected.float().to(out_dtype).double(), expected)  # exactly representable in the output type
    eye = torch.eye(128).to(E4M3)
    if side == "a":
        a8, b8 = x8, eye[None]
        sa, sb = torch.full((1, 256), scale), torch.ones(1, 1, 1)
    else:
        a8, b8 = eye, x8[None]
        sa, sb = torch.ones(1, 128), torch.full((1, 1, 2), scale)
        expected = expected.t()
    out = _run_gemm(a8, b8, sa, sb, None, 1, "MN", out_dtype, grouped=False)
    torch.testing.assert_close(out, expected.float(), atol=0, rtol=0)


@pytest.mark.parametrize("mode", ["MN", "K"])
@pytest.mark.parametrize("a_fmt,b_fmt", FORMAT_PAIRS, ids=_FMT_ID)
def test_group_gemm_fp8_format_pairs_exact(a_fmt, b_fmt, mode):
    """e4m3 / e5m2 on either side, grouped (an empty group, ragged tiles).  Of the integers -3..3 only +-2 has the same
    byte in both formats (+-1 and +-3 read in the other format are 0.5 / 1.5 or 4 / 2.5), so an operand decoded in the
    wrong format cannot give the exact result."""
    _exact_formula_scales([132, 0, 260, 4], 136, 256, 1, mode, grouped=True, fmts=(a_fmt, b_fmt))


@pytest.mark.parametrize("mode", ["MN", "K"])
@pytest.mark.parametrize("a_fmt,b_fmt", FORMAT_PAIRS[1:], ids=_FMT_ID)
def test_group_gemm_fp8_format_pairs_random(a_fmt, b_fmt, mode):
    """Random normals cast to e5m2 on one side or both (subnormal codes included), against the fp64 product of the same
    bytes: input quantisation is not part of the comparison, so the bar is the file's, whatever the format."""
    torch.manual_seed(11)
    ms, n, k = [260, 4, 512], 512, 512
    g, cum = len(ms), sum(ms)
    a8 = torch.randn(cum, k).to(a_fmt)
    b8 = (torch.randn(g, n, k) / math.sqrt(k)).to(b_fmt)
    sa = torch.pow(2.0, torch.randint(-3, 4, (k // 128, cum)).float())
    sb = torch.pow(2.0, torch.randint(-3, 4, (g, k // 128, n // 128)).float())
    m_indptr = indptr_of(ms)
    ref = _fp64_reference(a8, b8, sa, sb, m_indptr, 1)
    out = _run_gemm(a8, b8, sa, sb, m_indptr, 1, mode, torch.bfloat16, grouped=True)
    torch.testing.assert_close(out, ref.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize("mode", ["MN", "K"])
@pytest.mark.parametrize("m,last_a_scale", [(128, None), (384, None), (300, None), (384, 0.75)])
def test_gemm_fp8_a_scale_blocks_of_128_rows_exact(m, last_a_scale, mode):
    """scale_granularity_mnk = (128, 128, 128): a_scale has ceil(m / 128) rows (m = 300: three, the last block ragged).
    With the LAST a_scale element in memory set to 0.75 the whole call must take the fold: the power-of-two check has
    to scan exactly ceil(m / 128) * k / 128 a scales."""
    _exact_formula_scales([m], 136, 384, 128, mode, grouped=False, last_a_scale=last_a_scale)


@pytest.mark.parametrize("mode", ["MN", "K"])
def test_group_gemm_fp8_a_scale_blocks_of_128_rows_aligned_exact(mode):
    """Every group starts at a multiple of 128: a group's scale rows are the ones of its global rows."""
    ms = [128, 0, 384, 256]
    m_indptr = indptr_of(ms)
    assert torch.equal(_a_scale_rows(128, m_indptr), torch.arange(sum(ms)) // 128)
    _exact_formula_scales(ms, 264, 256, 128, mode, grouped=True)


@pytest.mark.parametrize("mode", ["MN", "K"])
def test_group_gemm_fp8_a_scale_blocks_of_128_rows_unaligned_exact(mode):
    """Groups that start between two multiples of 128: group g's rows are blocked from the GROUP's first row, its scale
    rows start at m_indptr[g] // 128 (see _a_scale_rows) -- not at the global row's block, which is a different scale
    row for some of these rows."""
    ms = [132, 260, 4, 384]
    m_indptr = indptr_of(ms)
    assert int((_a_scale_rows(128, m_indptr) != torch.arange(sum(ms)) // 128).sum()) == 44
    _exact_formula_scales(ms, 264, 256, 128, mode, grouped=True)


@pytest.mark.parametrize("ms,n,k", [([1300, 4, 0, 2300, 520], 400, 256), ([2500], 136, 256), ([128] * 37, 264, 256),
                                    # >= 2 x CUs tiles of 256 x 128: the persistent 256 x 128 kernel (ragged groups,
                                    # an empty group, a partial n tile; odd / even k block counts, one k block)
                                    ([2300, 4, 0, 3100, 1000, 777], 2696, 256), ([8000], 2056, 384),
                                    ([255, 257, 6000, 1], 3584, 128),
                                    # more than 64 groups (two passes of the wave-parallel group search), empty
                                    # groups in between
                                    ([(37 * i) % 301 if i % 5 else 0 for i in range(150)], 264, 128)])
def test_group_gemm_exact_many_tiles_banded_order(ms, n, k):
    _exact_many_tiles(ms, n, k, odd_scale=False)


@pytest.mark.parametrize("ms,n,k", [([8000], 2056, 384), ([255, 257, 6000, 1], 3584, 128)])
def test_group_gemm_mid_size_with_one_scale_that_is_no_power_of_two(ms, n, k):
    """Between one and four 256 x 256 tiles per CU the launcher runs the scale check and the hardware-scale 256 x 256
    variant in front of the kernel it would have chosen anyway; ONE scale of 1.5 must send the whole call to the latter
    (the shapes above with all-power-of-two scales take the former).  Still exact: 1.5 x small integers."""
    _exact_many_tiles(ms, n, k, odd_scale=True)


def _exact_many_tiles(ms, n, k, odd_scale):
    """More m tiles than one band and a ragged last band / last n tile: every (group, m tile, n tile) must
    be visited exactly once by the banded tile order of either kernel.  Small integers -> the result is exact."""
    import flashinfer

    torch.manual_seed(3)
    g = len(ms)
    cum = sum(ms)
    a = torch.randint(-3, 4, (cum, k)).float()
    b = torch.randint(-3, 4, (g, n, k)).float()
    sa = torch.pow(2.0, torch.randint(-1, 2, (k // 128, cum)).float())
    sb = torch.pow(2.0, torch.randint(-1, 2, (g, k // 128, -(-n // 128))).float())
    if odd_scale:
        sa[0, cum // 2] = 1.5
    m_indptr = indptr_of(ms)
    out = flashinfer.group_gemm_fp8_nt_groupwise(a.to(torch.float8_e4m3fn).to(DEV), b.to(torch.float8_e4m3fn).to(DEV),
                                                 sa.to(DEV), sb.to(DEV), m_indptr.to(DEV), out_dtype=torch.float16)
    ref = torch.zeros(cum, n, dtype=torch.float64)
    for gi in range(g):
        lo, hi = int(m_indptr[gi]), int(m_indptr[gi + 1])
        for kb in range(k // 128):
            part = a[lo:hi, kb * 128:(kb + 1) * 128].double() @ b[gi, :, kb * 128:(kb + 1) * 128].double().T
            ref[lo:hi] += part * sa[kb, lo:hi, None].double() * sb[gi, kb].double().repeat_interleave(128)[:n][None]
    assert ref.abs().max() < 60000
    torch.testing.assert_close(out.float().cpu(), ref.float().half().float(), atol=0, rtol=0)


@pytest.mark.parametrize("seed", range(16))
def test_group_gemm_random_shapes_exact(seed):
    """Seeded random (groups, rows per group, n, k, scale layout, output type) with small-integer operands and
    power-of-two scales: the result is exact, whichever kernel / tile shape the size-based dispatch picks."""
    import random

    import flashinfer

    rng = random.Random(1000 + seed)
    torch.manual_seed(1000 + seed)
    g = rng.choice([1, 2, 5, 8, 33, 70])
    big = rng.random() < 0.5
    ms = [rng.choice([0, 1, 7, 64, 128, 129, 255, 256, 300]) * (rng.choice([1, 4, 9]) if big else 1) for _ in range(g)]
    if sum(ms) == 0:
        ms[0] = 5
    n = 8 * rng.randint(1, 380 if big else 40)
    k = 128 * rng.randint(1, 5)
    mode = rng.choice(["MN", "K"])
    out_dtype = rng.choice([torch.float16, torch.bfloat16])
    cum = sum(ms)
    lim = 3 if out_dtype == torch.float16 else 1  # keep every partial sum exactly representable in the output type
    a = torch.randint(-lim, lim + 1, (cum, k)).float()
    b = torch.randint(-1, 2, (g, n, k)).float()
    sa = torch.pow(2.0, torch.randint(-1, 1, (k // 128, cum)).float())
    sb = torch.pow(2.0, torch.randint(-1, 1, (g, k // 128, -(-n // 128))).float())
    m_indptr = indptr_of(ms)
    sa_dev = sa if mode == "MN" else sa.t().contiguous()
    sb_dev = sb if mode == "MN" else sb.permute(0, 2, 1).contiguous()
    out = flashinfer.group_gemm_fp8_nt_groupwise(a.to(torch.float8_e4m3fn).to(DEV), b.to(torch.float8_e4m3fn).to(DEV),
                                                 sa_dev.to(DEV), sb_dev.to(DEV), m_indptr.to(DEV), scale_major_mode=mode,
                                                 out_dtype=out_dtype)
    ref = torch.zeros(cum, n, dtype=torch.float64)
    for gi in range(g):
        lo, hi = int(m_indptr[gi]), int(m_indptr[gi + 1])
        for kb in range(k // 128):
            part = a[lo:hi, kb * 128:(kb + 1) * 128].double() @ b[gi, :, kb * 128:(kb + 1) * 128].double().T
            ref[lo:hi] += part * sa[kb, lo:hi, None].double() * sb[gi, kb].double().repeat_interleave(128)[:n][None]
    torch.testing.assert_close(out.float().cpu(), ref.float().to(out_dtype).float(), atol=0, rtol=0)


def test_group_gemm_graph_replay_follows_the_scale_kind():
    """The choice between the hardware-scale 256 x 256 variant and the fold kernels is made on the DEVICE from the
    scale values of each launch: a captured call replayed after the scale tensor was overwritten in place (powers of
    two -> one scale of 1.5 -> powers of two) must give the exact result every time."""
    import flashinfer

    torch.manual_seed(5)
    m, n, k = 8000, 2056, 384  # 32 x 9 tiles of 256 x 256: between one and four per CU
    a = torch.randint(-3, 4, (m, k)).float()
    b = torch.randint(-3, 4, (1, n, k)).float()
    sa = torch.pow(2.0, torch.randint(-1, 2, (k // 128, m)).float())
    sb = torch.pow(2.0, torch.randint(-1, 2, (1, k // 128, -(-n // 128))).float())
    m_indptr = torch.tensor([0, m], dtype=torch.int32).to(DEV)
    a8, b8 = a.to(torch.float8_e4m3fn).to(DEV), b.to(torch.float8_e4m3fn).to(DEV)
    sa_d, sb_d = sa.to(DEV), sb.to(DEV)
    out = torch.empty(m, n, device=DEV, dtype=torch.float16)

    def reference(sa_h):
        ref = torch.zeros(m, n, dtype=torch.float64)
        for kb in range(k // 128):
            part = a[:, kb * 128:(kb + 1) * 128].double() @ b[0, :, kb * 128:(kb + 1) * 128].double().T
            ref += part * sa_h[kb, :, None].double() * sb[0, kb].double().repeat_interleave(128)[:n][None]
        return ref.float().half().float()

    flashinfer.group_gemm_fp8_nt_groupwise(a8, b8, sa_d, sb_d, m_indptr, out=out)  # warm-up: allocates the flag ring
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flashinfer.group_gemm_fp8_nt_groupwise(a8, b8, sa_d, sb_d, m_indptr, out=out)
    for odd in (False, True, False):
        sa_h = sa.clone()
        if odd:
            sa_h[1, 4321] = 1.5
        sa_d.copy_(sa_h)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(out.float().cpu(), reference(sa_h), atol=0, rtol=0)


# Every test function above once more per non-default entry of VARIANTS; the functions themselves are the default run
# and keep their ids.
TestKernelVariants = pytest.mark.parametrize("kernel_variant", [v for v in VARIANTS if v != "default"], indirect=True)(
    type("TestKernelVariants", (), {name: staticmethod(fn) for name, fn in list(globals().items())
                                    if name.startswith("test_") and callable(fn)}))
