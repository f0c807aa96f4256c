"""The masked batched fp8 GEMM (flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise, csrc/gemm_masked.hip) against an f64
reference computed here: dequantise a and b with their scales, einsum per expert over the first min(masked_m[e], m)
rows.  The exact cases use integers in [-4, 4] and power-of-two scales (2^-2 .. 2^2), so every product and sum is exact in
f32 and the comparison is at atol = rtol = 0; the random cases hold the bar of tests/test_gemm_gpu.py (1e-2, the
reference's own test).  Everything is compared on the CPU."""
import pytest
import torch

SENTINEL = 12345.0
SMALL = (3, 40, 256, 384)  # two n tiles, three k blocks
MASKS = [(0, 1, 40), (17, 33, 16), (15, 31, 32)]
EXPECTED = [1, 16, 17, 40, 128]  # row tiles of 16, 16, 32, 64, 128


def exact_problem(E, m, n, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (E, m, k), generator=g).float().to(torch.float8_e4m3fn)
    b = torch.randint(-4, 5, (E, n, k), generator=g).float().to(torch.float8_e4m3fn)
    sa = torch.exp2(torch.randint(-2, 3, (E, m, k // 128), generator=g).float())
    sb = torch.exp2(torch.randint(-2, 3, (E, n // 128, k // 128), generator=g).float())
    return a, b, sa, sb


def random_problem(E, m, n, k, seed=1):
    from oracle.gemm_ref import quantize_fp8

    g = torch.Generator().manual_seed(seed)
    a, sa = quantize_fp8(torch.randn(E, m, k, generator=g), (1, 1, 128), "K")
    b, sb = quantize_fp8(torch.randn(E, n, k, generator=g), (1, 128, 128), "K")
    # the quantiser's scales are powers of two: make them anything
    return a, b, sa * (1 + torch.rand(sa.shape, generator=g)), sb * (1 + torch.rand(sb.shape, generator=g))


def expected_out(a, b, sa, sb, masked, dtype):
    """The sentinel everywhere but the live rows, which hold the f64 product rounded to dtype."""
    E, m, _ = a.shape
    ad = a.double() * sa.double().repeat_interleave(128, 2)
    bd = b.double() * sb.double().repeat_interleave(128, 1).repeat_interleave(128, 2)
    out = torch.full((E, m, b.shape[1]), SENTINEL, dtype=dtype)
    for e, r in enumerate(masked):
        r = max(min(r, m), 0)
        out[e, :r] = torch.einsum("ik,jk->ij", ad[e, :r], bd[e]).to(dtype)
    return out


def run(a, b, sa, sb, masked, expected_m, dtype, via=None):
    """The call on poisoned inputs (NaN in the dead rows of a and a_scale) into a sentinel-filled out; returns it on the CPU."""
    import flashinfer.gemm

    a, sa = a.clone().view(torch.uint8), sa.clone()
    for e, r in enumerate(masked):
        a[e, max(r, 0):] = 0x7F
        sa[e, max(r, 0):] = float("nan")
    out = torch.full((a.shape[0], a.shape[1], b.shape[1]), SENTINEL, dtype=dtype, device="cuda")
    mm = torch.tensor(masked, dtype=torch.int32, device="cuda")
    args = (a.view(torch.float8_e4m3fn).cuda(), b.cuda(), sa.cuda(), sb.cuda(), mm, expected_m)
    res = (via or flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise)(*args, out=out)
    assert res is out
    return out.cpu()


def assert_exact(out, want):
    torch.testing.assert_close(out, want, atol=0, rtol=0)
    dead = want == SENTINEL  # a live value equal to the sentinel passes either way
    assert torch.equal(out.view(torch.int16)[dead], want.view(torch.int16)[dead])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("expected_m", EXPECTED)
@pytest.mark.parametrize("shape,masked", [(SMALL, mk) for mk in MASKS] + [
    ((5, 130, 128, 256), (130, 0, 129, 1, 128)),  # more than one 128-row tile, empty experts between live ones
    ((3, 40, 128, 128), (41, 1000, -3)),  # masked_m past m is clamped, a negative one is empty
])
def test_exact_small_integers(shape, masked, expected_m, dtype):
    p = exact_problem(*shape)
    assert_exact(run(*p, masked, expected_m, dtype), expected_out(*p, masked, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("expected_m", EXPECTED)
@pytest.mark.parametrize("masked", MASKS)
def test_random_operands(masked, expected_m, dtype):
    p = random_problem(*SMALL)
    out, want = run(*p, masked, expected_m, dtype), expected_out(*p, masked, dtype)
    torch.testing.assert_close(out.float(), want.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("expected_m", [1, 128])
def test_many_experts_few_rows(expected_m):
    """260 experts (more than a wave scans at once) of 0 .. 8 rows on a grid of 8 workgroups: every workgroup walks
    several tiles."""
    from flashinfer import _lib

    masked = tuple(min(e % 9, 8) for e in range(260))
    p = exact_problem(260, 8, 128, 128)
    _lib.set_option("FI_NUM_CUS", 4)
    try:
        out = run(*p, masked, expected_m, torch.bfloat16)
    finally:
        _lib.set_option("FI_NUM_CUS", None)
    assert_exact(out, expected_out(*p, masked, torch.bfloat16))


@pytest.mark.gpu
def test_expected_m_does_not_change_the_result():
    """Bit-identical under every row-tile height: a row's sum is taken k block by k block whatever the tile is, and
    the 16x16x128 MFMA is the same instruction in every instantiation."""
    p = random_problem(*SMALL)
    outs = [run(*p, MASKS[1], em, torch.bfloat16) for em in EXPECTED]
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


@pytest.mark.gpu
def test_graph_replay_follows_masked_m():
    import flashinfer.gemm

    a, b, sa, sb = exact_problem(*SMALL)
    dev = [t.cuda() for t in (a, b, sa, sb)]
    mm = torch.tensor(MASKS[1], dtype=torch.int32, device="cuda")
    out = torch.full((3, 40, 256), SENTINEL, dtype=torch.bfloat16, device="cuda")
    flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise(*dev, mm, 16, out=out)  # not the first call under capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise(*dev, mm, 16, out=out)
    mm.copy_(torch.tensor(MASKS[2], dtype=torch.int32))
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert_exact(out.cpu(), expected_out(a, b, sa, sb, MASKS[2], torch.bfloat16))


@pytest.mark.gpu
def test_deep_gemm_spelling_gives_the_same_output():
    import flashinfer.deep_gemm

    def via(a, b, sa, sb, mm, expected_m, out):
        assert flashinfer.deep_gemm.m_grouped_fp8_gemm_nt_masked((a, sa), (b, sb), out, mm, expected_m) is None
        return out

    p = random_problem(*SMALL)
    assert torch.equal(run(*p, MASKS[1], 16, torch.bfloat16, via=via).view(torch.int16),
                       run(*p, MASKS[1], 16, torch.bfloat16).view(torch.int16))


E5M2, E4M3 = torch.float8_e5m2, torch.float8_e4m3fn
REFUSALS = {  # name: (changes to the arguments of a valid (2, 8, 128, 256) call, exception)
    "rank": (dict(a=torch.zeros(8, 256).to(E4M3)), ValueError),
    "experts": (dict(b=torch.zeros(3, 128, 256).to(E4M3)), ValueError),
    "k_mismatch": (dict(b=torch.zeros(2, 128, 128).to(E4M3)), ValueError),
    "n_not_128": (dict(b=torch.zeros(2, 64, 256).to(E4M3), b_scale=torch.ones(2, 1, 2)), ValueError),
    "k_not_128": (dict(a=torch.zeros(2, 8, 192).to(E4M3), b=torch.zeros(2, 128, 192).to(E4M3)), ValueError),
    "non_contiguous": (dict(a=torch.zeros(2, 256, 8).to(E4M3).transpose(1, 2)), ValueError),
    "a_scale_shape": (dict(a_scale=torch.ones(2, 2, 8)), ValueError),
    "b_scale_shape": (dict(b_scale=torch.ones(2, 2, 1)), ValueError),
    "operand_dtype": (dict(a=torch.zeros(2, 8, 256, dtype=torch.float16)), ValueError),
    "scale_dtype": (dict(a_scale=torch.ones(2, 8, 2, dtype=torch.float16)), ValueError),
    "out_dtype": (dict(out_dtype=torch.float32), ValueError),
    "masked_m_dtype": (dict(masked_m=torch.ones(2, dtype=torch.int64)), ValueError),
    "masked_m_shape": (dict(masked_m=torch.ones(3, dtype=torch.int32)), ValueError),
    "expected_m": (dict(expected_m=0), ValueError),
    "scale_granularity_mnk": (dict(scale_granularity_mnk=(128, 128, 128)), NotImplementedError),
    "e5m2_a": (dict(a=torch.zeros(2, 8, 256).to(E5M2)), NotImplementedError),
    "e5m2_b": (dict(b=torch.zeros(2, 128, 256).to(E5M2)), NotImplementedError),
    "cpu_tensors": (dict(), RuntimeError),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name, monkeypatch):
    import flashinfer.gemm
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    change, exc = REFUSALS[name]
    kw = dict(a=torch.zeros(2, 8, 256).to(E4M3), b=torch.zeros(2, 128, 256).to(E4M3), a_scale=torch.ones(2, 8, 2),
              b_scale=torch.ones(2, 1, 2), masked_m=torch.ones(2, dtype=torch.int32), expected_m=8)
    kw.update(change)
    with pytest.raises(exc, match="scale_granularity_mnk|float8_e5m2" if exc is NotImplementedError else None):
        flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise(**kw)
