"""GPU: the MXFP4 quantiser and the scale interleave (csrc/mxfp4_quantize.hip) against the fp64 oracle of
tests/fp4_ref.py: scale bytes are compared as bytes, codes after decoding (the sign nibble of a zero is unspecified),
and every byte of a scale buffer must have been written, padding as 0."""
import pytest
import torch

import fp4_ref as F
import mx_ref as R
from attn_inputs import indptr_of
from flashinfer import fp4_quantization as Q  # the module under test: without it nothing here is collected

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# A workgroup takes 256 (row, k block) pairs of the scale tensor as one flat range, so pairs of several rows share a
# workgroup and rows straddle workgroups: 2080 = 65 blocks (one more than 256 threads x 8 elements) and the odd block
# counts 1, 3, 5 never divide 256.  2048 + 128 is the long row for the swizzled layout, whose bytes the reference's
# reshape((-1, k / 32)) takes only when k % 128 == 0.
K_LINEAR = [32, 96, 128, 160, 2080]
K_SWIZZLED = [128, 2048 + 128]


def _check_codes(x2d, packed, sf_linear):
    want_packed, want_sf = F.mxfp4_quantize_ref(x2d)
    assert torch.equal(sf_linear, want_sf), f"{int((sf_linear != want_sf).sum())} scale bytes differ"
    got, want = R.e2m1_to_f64(packed), R.e2m1_to_f64(want_packed)
    assert torch.equal(got, want), f"{int((got != want).sum())} codes differ, first at {(got != want).nonzero()[:4].tolist()}"


def _quantize(x, swizzled):
    """fp4_quantize on the device, and once more into a scale buffer prefilled with 0xAA: every byte must be written."""
    import flashinfer

    xd = x.cuda()
    q, sf = flashinfer.fp4_quantize(xd, None, 32, True, swizzled)
    q2 = torch.full_like(q, 0xAA)
    sf2 = torch.full_like(sf, 0xAA)
    Q._quantize_into(xd.reshape(-1, x.shape[-1]), q2.view(-1, x.shape[-1] // 2), sf2, 1, swizzled)
    torch.cuda.synchronize()
    assert torch.equal(sf, sf2) and torch.equal(q, q2)
    return q.cpu(), sf.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,swizzled", [(k, False) for k in K_LINEAR] + [(k, True) for k in K_SWIZZLED])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 200])
def test_quantiser_is_bit_exact(m, k, swizzled, dtype):
    x = F.block_inputs(m, k, dtype, 1000 * m + k)
    q, sf = _quantize(x, swizzled)
    nkb = k // 32
    assert q.dtype == torch.uint8 and q.shape == (m, k // 2) and sf.dtype == torch.uint8 and sf.shape[1] == nkb
    if swizzled:
        assert sf.numel() == R.ceil_to(m, 128) * R.ceil_to(nkb, 4)
        sf_linear = R.unswizzle(sf, m, nkb)
        assert torch.equal(sf.reshape(-1), R.swizzle(sf_linear))  # padding bytes are 0
    else:
        assert sf.shape == (m, nkb)
        sf_linear = sf
    _check_codes(x, q, sf_linear)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_go_to_even_on_the_device(dtype):
    x = F.tie_block(dtype)
    q, sf = _quantize(x, False)
    assert sf.tolist() == [[127]]
    assert torch.equal(R.e2m1_to_f64(q), F.tie_block_decoded())
    # the same block at other scales and among other blocks: a row of 4 blocks, the tie block times 2^-9, 1, 2^5, 2^11
    scales = [2.0 ** -9, 1.0, 2.0 ** 5, 2.0 ** 11]
    row = torch.cat([x.double() * s for s in scales], dim=1).to(dtype)
    q, sf = _quantize(row, True)
    assert R.unswizzle(sf, 1, 4).tolist() == [[118, 127, 132, 138]]
    assert torch.equal(R.e2m1_to_f64(q), F.tie_block_decoded().repeat(1, 4))
    _check_codes(row, q, R.unswizzle(sf, 1, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_boundary_on_the_device(dtype):
    x, want = F.boundary_rows(dtype)
    q, sf = _quantize(x, False)
    assert torch.equal(sf.view(-1), want)  # amax = 6 * 2^e gets e, the next value of the dtype above it e + 1
    _check_codes(x, q, sf)
    zero = torch.zeros(3, 64, dtype=dtype)
    zero[1, 40] = 3.0
    q, sf = _quantize(zero, False)
    assert sf.tolist() == [[0, 0], [0, 126], [0, 0]]  # an all-zero block: byte 0, zero codes
    assert torch.equal(R.e2m1_to_f64(q), zero.double() * 2)


@pytest.mark.parametrize("swizzled", [True, False])
def test_empty_input(swizzled):
    import flashinfer

    q, sf = flashinfer.fp4_quantize(torch.empty(0, 128, dtype=torch.bfloat16, device="cuda"), None, 32, True, swizzled)
    torch.cuda.synchronize()
    assert q.shape == (0, 64) and q.dtype == torch.uint8 and sf.shape == (0, 4) and sf.dtype == torch.uint8
    out = flashinfer.block_scale_interleave(torch.empty(0, 4, dtype=torch.uint8, device="cuda"))
    assert out.shape == (0,)


def test_3d_strided_and_column_major_input():
    import flashinfer

    x = F.block_inputs(6 * 50, 128, torch.float16, 9)
    q, sf = flashinfer.fp4_quantize(x.view(6, 50, 128).cuda(), None, 32, True, False)
    assert q.shape == (6, 50, 64) and sf.shape == (300, 4)
    _check_codes(x, q.cpu().view(300, 64), sf.cpu())
    wide = torch.zeros(300, 256, dtype=torch.float16)
    wide[:, :128] = x
    view = wide.cuda()[:, :128]  # a view with a row stride of 256
    assert view.stride() == (256, 1)
    q, sf = flashinfer.mxfp4_quantize(view)
    _check_codes(x, q.cpu(), R.unswizzle(sf.cpu(), 300, 4))
    wide[:, 64:192] = x
    q, sf = flashinfer.mxfp4_quantize(wide.cuda()[:, 64:192])
    _check_codes(x, q.cpu(), R.unswizzle(sf.cpu(), 300, 4))
    # column major: stored as [k, m] rows, quantised along m, and both results come back transposed
    base = F.block_inputs(96, 64, torch.bfloat16, 10)
    cm = base.cuda().t()
    assert cm.shape == (64, 96) and cm.stride(-2) == 1
    q, sf = flashinfer.fp4_quantize(cm, None, 32, True, False)
    assert q.shape == (32, 96) and sf.shape == (2, 96)
    _check_codes(base, q.cpu().t().contiguous(), sf.cpu().t().contiguous())


@pytest.mark.parametrize("shape", [(200, 6), (3, 130, 5), (1, 1)])
def test_block_scale_interleave(shape):
    import flashinfer

    g = torch.Generator().manual_seed(sum(shape))
    sf = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    out = flashinfer.block_scale_interleave(sf.cuda())
    torch.cuda.synchronize()
    groups = sf.view(-1, *shape[-2:])
    want = torch.cat([R.swizzle(groups[i]) for i in range(groups.shape[0])])  # padding 0
    assert out.dtype == torch.uint8 and out.shape == want.shape
    assert torch.equal(out.cpu(), want)
    assert flashinfer.nvfp4_block_scale_interleave is flashinfer.block_scale_interleave
    # a non-contiguous input is read as its values
    if len(shape) == 2:
        wide = torch.zeros(shape[0], shape[1] + 3, dtype=torch.uint8)
        wide[:, 1:1 + shape[1]] = sf
        assert torch.equal(flashinfer.block_scale_interleave(wide.cuda()[:, 1:1 + shape[1]]).cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_grouped(dtype):
    import flashinfer

    G, n, k = 3, 136, 256
    x = F.block_inputs(G * n, k, dtype, 11).view(G, n, k)
    b, b_scale = flashinfer.mxfp4_quantize_grouped(x.cuda())
    torch.cuda.synchronize()
    assert b.shape == (G, n, k // 2) and b.dtype == torch.uint8
    assert b_scale.shape == (G, 256, k // 32) and b_scale.dtype == torch.uint8
    want_b, want_sf = F.mxfp4_quantize_ref(x)
    assert torch.equal(b_scale.cpu(), R.swizzle_b(want_sf))  # every group swizzled on its own, padding 0
    assert torch.equal(R.e2m1_to_f64(b.cpu()), R.e2m1_to_f64(want_b))
    # checkpoint route: linear scales through block_scale_interleave give the same bytes
    interleaved = flashinfer.block_scale_interleave(want_sf.cuda())
    assert torch.equal(interleaved.cpu().view(G, 256, k // 32), b_scale.cpu())


def test_quantise_weights_then_gemm():
    import flashinfer

    ms, (G, n, k) = [4, 132, 0, 60], (4, 136, 256)
    g = torch.Generator().manual_seed(21)
    w = (torch.randn(G, n, k, generator=g) / k ** 0.5).to(torch.bfloat16)
    x = torch.randn(sum(ms), k, generator=g).to(torch.bfloat16)
    indptr = indptr_of(ms).cuda()
    b, b_scale = flashinfer.mxfp4_quantize_grouped(w.cuda())
    a, a_scale = flashinfer.fp8_quantization.mxfp8_quantize_grouped(x.cuda(), indptr)
    out = flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise(a, b, a_scale, b_scale, indptr)
    torch.cuda.synchronize()
    want_b, want_sb = F.mxfp4_quantize_ref(w)
    want_a, want_sa = R.mxfp8_quantize_ref(x)
    want = R.group_gemm_ref(R.fp8_to_f64(want_a), want_sa, want_b, want_sb, ms)
    assert out.shape == (sum(ms), n) and out.dtype == torch.bfloat16
    torch.testing.assert_close(out.cpu().double(), want, atol=1e-2, rtol=1e-2)
    assert want.abs().max().item() > 0.5  # the product is not all noise-level numbers


def test_graph_capture_replays_on_new_data():
    import flashinfer

    x0 = F.block_inputs(200, 128, torch.bfloat16, 31)
    x1 = F.block_inputs(200, 128, torch.bfloat16, 32)
    xd = x0.cuda()
    flashinfer.mxfp4_quantize(xd)  # the library is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q, sf = flashinfer.mxfp4_quantize(xd)
    xd.copy_(x1)
    q.fill_(0xAA)
    sf.fill_(0xAA)
    graph.replay()
    torch.cuda.synchronize()
    eager_q, eager_sf = flashinfer.mxfp4_quantize(x1.cuda())
    assert torch.equal(q, eager_q) and torch.equal(sf, eager_sf)
    _check_codes(x1, q.cpu(), R.unswizzle(sf.cpu(), 200, 4))
