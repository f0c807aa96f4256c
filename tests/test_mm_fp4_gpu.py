"""GPU: flashinfer.mm_fp4 (csrc/mm_fp4.hip) against the fp64 oracle of tests/mm_fp4_ref.py, every shape through the
entry point's own choice and through each of its two kernels (FI_MM_FP4_KERNEL unset, 1 = streaming, 2 = tiled).

The one-hot tests are the probe of the block-scaled MFMA's lane maps with BOTH operands fp4: with one operand one-hot
every output is ONE e2m1 value of the other operand times a power of two, so the 16-bit result is exact and a wrong nibble
order, k permutation, row / column swap or scale-block assignment changes bits.  The small-integer tests make every
partial sum exact in f32, so the bits do not depend on the accumulation order or on the k split either."""
import functools

import pytest
import torch

import mm_fp4_ref as M
import mx_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 128), (17, 136, 384), (130, 264, 256), (300, 520, 640), (1000, 1024, 512)]
OUT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.fixture(params=[None, 1, 2], ids=["choose", "streaming", "tiled"])
def kernel(request):
    from flashinfer import _lib

    _lib.set_option("FI_MM_FP4_KERNEL", request.param)
    yield request.param
    _lib.set_option("FI_MM_FP4_KERNEL", None)


def _device_args(a_q, sa, b_q, sb, fill=0):
    """CPU a_q [m, k/2], sa [m, nkb], b_q [n, k/2], sb [n, nkb] -> the four tensors as the reference's test passes them."""
    nkb = sa.shape[1]
    a_sf = R.swizzle(sa, fill).view(-1, nkb).cuda()
    b_sf = R.swizzle(sb, fill).view(-1, nkb).cuda()
    return a_q.cuda(), b_q.cuda().T, a_sf, b_sf.T


def _run(a_q, sa, b_q, sb, out_dtype, alpha=None, fill=0, out=None):
    import flashinfer

    a, b, a_sf, b_sf = _device_args(a_q, sa, b_q, sb, fill)
    alpha_t = None if alpha is None else torch.tensor([alpha], dtype=torch.float32, device="cuda")
    res = flashinfer.mm_fp4(a, b, a_sf, b_sf, alpha_t, out_dtype, out, block_size=32, use_nvfp4=False)
    torch.cuda.synchronize()
    assert res.dtype == out_dtype and res.shape == (a_q.shape[0], b_q.shape[0])
    if out is not None:
        assert res is out
    return res.cpu()


def _assert_same_bits(got, want16):
    """equal bits, +0 and -0 alike (a sum that cancels has no sign the two sides must agree on)"""
    bad = (got.view(torch.int16) != want16.view(torch.int16)) & ~((got == 0) & (want16 == 0))
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[:4].tolist()}: " \
                          f"got {got[bad][:4].tolist()} want {want16[bad][:4].tolist()}"


# ---- 1. lane-map probes, bit-exact ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _one_hot_case(one_hot, m, n, k, narrow):
    g = torch.Generator().manual_seed(m + n + k)
    lo, hi = (124, 131) if narrow else (121, 134)  # f16: nothing overflows or leaves the normal range
    sa = torch.randint(lo, hi, (m, k // 32), dtype=torch.uint8, generator=g)
    sb = torch.randint(lo, hi, (n, k // 32), dtype=torch.uint8, generator=g)
    rows, other = (m, n) if one_hot == "a" else (n, m)
    codes = torch.zeros(rows, k, dtype=torch.uint8)
    i = torch.arange(rows)
    codes[i, (37 * i + 5) % k] = 2  # e2m1 code of 1.0
    hot = M.pack_codes(codes)
    rand = torch.randint(0, 256, (other, k // 2), dtype=torch.uint8, generator=g)
    a_q, b_q = (hot, rand) if one_hot == "a" else (rand, hot)
    return a_q, sa, b_q, sb, M.mm_fp4_ref(a_q, sa, b_q, sb)


@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("one_hot", ["a", "b"])
def test_one_hot_is_bit_exact(one_hot, m, n, k, out, kernel):
    a_q, sa, b_q, sb, want = _one_hot_case(one_hot, m, n, k, out == "f16")
    want16 = want.to(OUT[out])
    assert torch.equal(want16.double(), want), "the case is not exact in the output dtype"
    _assert_same_bits(_run(a_q, sa, b_q, sb, OUT[out]), want16)


# ---- 2. small-integer sums, bit-exact -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sum_case(m, n, k, mixed):
    """Random codes in both operands; scale bytes 127, or in {126, 127, 128} on each side.  Every product is a multiple of
    2^-4 of magnitude at most 36 * 4 = 144, so for 144 k <= 2^20 every partial sum in any order is a multiple of 2^-4 below
    2^20: exact in f32, whatever the accumulation order and the k split."""
    assert 144 * k <= 2 ** 20
    g = torch.Generator().manual_seed(3 * m + 5 * n + 7 * k + int(mixed))
    a_q = torch.randint(0, 256, (m, k // 2), dtype=torch.uint8, generator=g)
    b_q = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, generator=g)
    if mixed:
        sa = torch.randint(126, 129, (m, k // 32), dtype=torch.uint8, generator=g)
        sb = torch.randint(126, 129, (n, k // 32), dtype=torch.uint8, generator=g)
    else:
        sa = torch.full((m, k // 32), 127, dtype=torch.uint8)
        sb = torch.full((n, k // 32), 127, dtype=torch.uint8)
    want = M.mm_fp4_ref(a_q, sa, b_q, sb)
    assert want.abs().max().item() < 2 ** 20 and torch.equal(want * 16, (want * 16).round())
    return a_q, sa, b_q, sb, want


@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("mixed", [False, True], ids=["unit-scales", "mixed-scales"])
def test_small_integer_sums_are_bit_exact(mixed, m, n, k, out, kernel):
    a_q, sa, b_q, sb, want = _sum_case(m, n, k, mixed)
    _assert_same_bits(_run(a_q, sa, b_q, sb, OUT[out]), M.round_once(want, OUT[out]))


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_streaming_kernel_without_the_k_split(m, n, k):
    """The streaming kernel splits k over a workgroup's waves only while 128-row workgroups would leave compute units
    idle; told that there is one compute unit it takes the other form at every shape."""
    from flashinfer import _lib

    a_q, sa, b_q, sb, want = _sum_case(m, n, k, True)
    _lib.set_option("FI_MM_FP4_KERNEL", 1)
    _lib.set_option("FI_NUM_CUS", 1)
    try:
        got = _run(a_q, sa, b_q, sb, torch.bfloat16)
    finally:
        _lib.set_option("FI_NUM_CUS", None)
        _lib.set_option("FI_MM_FP4_KERNEL", None)
    _assert_same_bits(got, M.round_once(want, torch.bfloat16))


# ---- 3. alpha ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_alpha(m, n, k, out, kernel):
    a_q, sa, b_q, sb, want = _sum_case(m, n, k, False)
    dt = OUT[out]
    # a power of two: still exact
    _assert_same_bits(_run(a_q, sa, b_q, sb, dt, alpha=0.25), M.round_once(want * 0.25, dt))
    # 0.3 as f32: one more rounding, within one ulp of the output dtype of the fp64 value
    alpha = torch.tensor(0.3, dtype=torch.float32).double().item()
    got = _run(a_q, sa, b_q, sb, dt, alpha=0.3).double()
    exact = want * alpha
    err = (got - exact).abs()
    bound = M.ulp(exact, dt)
    assert bool((err <= bound).all()), f"worst {float((err / bound).max())} ulp"
    # no alpha is alpha = 1
    assert torch.equal(_run(a_q, sa, b_q, sb, dt, alpha=None).view(torch.int16),
                       _run(a_q, sa, b_q, sb, dt, alpha=1.0).view(torch.int16))


# ---- 4. realistic inputs, quantised on the device -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _realistic_case(m, n, k):
    import flashinfer

    g = torch.Generator().manual_seed(m * n + k)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16).cuda()
    w = torch.randn(n, k, generator=g).to(torch.bfloat16).cuda()
    x_q, x_sf = flashinfer.mxfp4_quantize(x)
    w_q, w_sf = flashinfer.mxfp4_quantize(w)
    sa = R.unswizzle(x_sf.cpu(), m, k // 32)
    sb = R.unswizzle(w_sf.cpu(), n, k // 32)
    want = M.mm_fp4_ref(x_q.cpu(), sa, w_q.cpu(), sb)
    mag = M.abs_product_ref(x_q.cpu(), sa, w_q.cpu(), sb)
    dense = torch.mm(x, w.T).float().cpu()
    return x_q, x_sf, w_q, w_sf, want, mag, dense


@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_realistic_inputs(m, n, k, out, kernel):
    import flashinfer

    x_q, x_sf, w_q, w_sf, want, mag, dense = _realistic_case(m, n, k)
    got = flashinfer.mm_fp4(x_q, w_q.T, x_sf, w_sf.T, None, OUT[out], block_size=32, use_nvfp4=False)
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == OUT[out] and got.shape == (m, n)
    # half an output ulp plus an f32 accumulation bound: derived, not tuned
    r = 2.0 ** -8 if out == "bf16" else 2.0 ** -11
    err = (got.double() - want).abs()
    bound = r * want.abs() + k * 2.0 ** -23 * mag
    assert bool((err <= bound).all()), f"worst {float((err / bound.clamp(min=1e-300)).max())} of the bound"
    cos = torch.nn.functional.cosine_similarity(dense.reshape(-1).double(), got.reshape(-1).double(), dim=0)
    assert cos.item() > 0.97, cos.item()


# ---- 5. padding does not leak ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", ["bf16", "f16"])
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_padding_does_not_leak(m, n, k, out, kernel):
    a_q, sa, b_q, sb, _ = _sum_case(m, n, k, True)
    dt = OUT[out]
    clean = _run(a_q, sa, b_q, sb, dt)
    sentinel = torch.full((m, n), 60000.0, dtype=dt, device="cuda")  # far above any sum of these cases
    mark = sentinel[0, 0].item()
    assert not bool((clean == mark).any())
    noisy = _run(a_q, sa, b_q, sb, dt, fill=0xFE, out=sentinel)
    assert torch.equal(noisy.view(torch.int16), clean.view(torch.int16))
    assert not bool((noisy == mark).any())


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,force", [(17, 136, 384, None), (300, 520, 640, 2)], ids=["17x136x384", "300x520x640-tiled"])
def test_graph_replay_reads_new_inputs(m, n, k, force):
    import flashinfer
    from flashinfer import _lib

    _lib.set_option("FI_MM_FP4_KERNEL", force)
    try:
        a1, sa1, b_q, sb, _ = _sum_case(m, n, k, True)
        a2, sa2, _, _, _ = _sum_case(m, n, k, False)
        a, b, a_sf, b_sf = _device_args(a1, sa1, b_q, sb)
        alpha = torch.tensor([1.0], dtype=torch.float32, device="cuda")
        out = torch.empty(m, n, dtype=torch.bfloat16, device="cuda")
        call = lambda: flashinfer.mm_fp4(a, b, a_sf, b_sf, alpha, torch.bfloat16, out, block_size=32, use_nvfp4=False)  # noqa: E731
        call()  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        # new inputs, in place
        a.copy_(a2.cuda())
        a_sf.copy_(R.swizzle(sa2).view(-1, k // 32).cuda())
        alpha.fill_(0.25)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.cpu().clone()
        eager = call().cpu()
        torch.cuda.synchronize()
        assert torch.equal(replayed.view(torch.int16), eager.view(torch.int16))
        want = M.mm_fp4_ref(a2, sa2, b_q, sb, 0.25)
        _assert_same_bits(replayed, M.round_once(want, torch.bfloat16))
    finally:
        _lib.set_option("FI_MM_FP4_KERNEL", None)
