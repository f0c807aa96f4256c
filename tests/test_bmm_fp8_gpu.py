"""flashinfer.bmm_fp8 (csrc/bmm_fp8.hip) against an f64 reference computed here: dequantise with the two scalars, einsum
per batch entry, round to dtype.  The exact cases use integers in [-4, 4] (exact in e4m3 and e5m2) and power-of-two scales,
so every product and sum is exact in f32 at these k and the comparison is at atol = rtol = 0; the random cases hold the
bar of tests/test_gemm_gpu.py and tests/test_masked_gemm_gpu.py (1e-2).  Everything is compared on the CPU."""
import pytest
import torch

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
PAIRS = [(E4M3, E4M3), (E4M3, E5M2), (E5M2, E4M3)]
SENTINEL = 12288.0  # exact in bf16


def exact_problem(b, m, n, k, seed=0):
    """A (b, m, k), B (b, k, n) column-major and the two scales, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (b, m, k), generator=g).float().to(E4M3)
    w = torch.randint(-4, 5, (b, n, k), generator=g).float().to(E4M3)
    sa, sb = (torch.exp2(torch.randint(-2, 3, (1,), generator=g).float()) for _ in range(2))
    return a, w.transpose(-2, -1), sa, sb


def random_problem(b, m, n, k, a_dtype, b_dtype, seed=1):
    def to_float8(x, dtype):  # the reference's per-tensor quantiser (its bmm_fp8 docstring and test)
        finfo = torch.finfo(dtype)
        scale = finfo.max / x.abs().max().clamp(min=1e-12)
        return (x * scale).clamp(min=finfo.min, max=finfo.max).to(dtype), scale.float().reciprocal().reshape(1)

    g = torch.Generator().manual_seed(seed)
    a, sa = to_float8(torch.randn(b, m, k, generator=g), a_dtype)
    w, sb = to_float8(torch.randn(b, n, k, generator=g), b_dtype)
    return a, w.transpose(-2, -1), sa, sb


def expected_out(a, bt, sa, sb, dtype):
    return (sa.double() * sb.double() * torch.einsum("bik,bkj->bij", a.double(), bt.double())).to(dtype)


def run(a, bt, sa, sb, dtype):
    import flashinfer

    return flashinfer.bmm_fp8(a.cuda(), bt.transpose(-2, -1).cuda().transpose(-2, -1), sa.cuda(), sb.cuda(), dtype).cpu()


def waves_along_k(b, m, n, k, cus):
    """The host's choice rule (csrc/bmm_fp8.hip, bmm_waves_along_k)."""
    bm = 16 if m <= 16 else 32 if m <= 32 else 64 if m <= 64 else 128
    return bm <= 32 and -(-k // 128) >= 4 and b * -(-m // bm) * -(-n // 128) < cus


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("m", [1, 16, 17, 40, 65, 130])  # row tiles 16, 16, 32, 64, 128, 2 x 128 with a 2-row tail
@pytest.mark.parametrize("family", [
    (3, 256, 384),  # two n tiles, three k blocks
    (2, 80, 64),    # the reference test's n and k: an n tail, less than one k block
    (1, 8, 208),    # narrowest n, a k tail that is no multiple of 32
])
def test_exact_small_integers(family, m, dtype):
    b, n, k = family
    p = exact_problem(b, m, n, k)
    torch.testing.assert_close(run(*p, dtype), expected_out(*p, dtype), atol=0, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("cus", [2, 4, 256])
@pytest.mark.parametrize("m,k", [(16, 640), (17, 656)])  # BM 16; BM 32 with a k tail: the fourth wave's last block is partial
def test_both_wave_arrangements(m, k, cus):
    """(1, m, 256, k) has 2 wide tiles and 5 resp. 6 k blocks: by the choice rule FI_NUM_CUS = 2 takes waves along n
    (2 tiles are not fewer than 2 units), FI_NUM_CUS = 4 and 256 take waves along k (2 < 4).  Setting the count in every
    run keeps the test independent of the device."""
    from flashinfer import _lib

    assert waves_along_k(1, m, 256, k, cus) == (cus != 2)
    p = exact_problem(1, m, 256, k)
    _lib.set_option("FI_NUM_CUS", cus)
    try:
        out = run(*p, torch.bfloat16)
    finally:
        _lib.set_option("FI_NUM_CUS", None)
    torch.testing.assert_close(out, expected_out(*p, torch.bfloat16), atol=0, rtol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("a_dtype,b_dtype", PAIRS)
@pytest.mark.parametrize("shape", [(3, 40, 256, 384), (2, 48, 80, 64)])
def test_random_operands(shape, a_dtype, b_dtype, dtype):
    p = random_problem(*shape, a_dtype, b_dtype)
    torch.testing.assert_close(run(*p, dtype).float(), expected_out(*p, dtype).float(), atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 17, 80, 208), (1, 17, 40, 656)])  # m, n and k tails; the second splits k on a full chip
def test_neighbouring_memory_is_left_alone(shape):
    """A, B and out are slices of larger buffers: NaN codes (0x7F in both formats) lie right around the operands, a
    sentinel around the output.  No NaN may reach the result and the sentinel must survive."""
    import flashinfer

    b, m, n, k = shape
    a, bt, sa, sb = exact_problem(*shape)
    a_big = torch.full((b + 2, m, k), 0x7F, dtype=torch.uint8, device="cuda")
    w_big = torch.full((b + 2, n, k), 0x7F, dtype=torch.uint8, device="cuda")
    out_big = torch.full((b + 2, m, n), SENTINEL, dtype=torch.bfloat16, device="cuda")
    a_big[1:-1] = a.view(torch.uint8).cuda()
    w_big[1:-1] = bt.transpose(-2, -1).contiguous().view(torch.uint8).cuda()
    out = flashinfer.bmm_fp8(a_big[1:-1].view(E4M3), w_big[1:-1].view(E4M3).transpose(-2, -1), sa.cuda(), sb.cuda(),
                             torch.bfloat16, out=out_big[1:-1])
    assert out.data_ptr() == out_big[1:-1].data_ptr()
    torch.testing.assert_close(out.cpu(), expected_out(a, bt, sa, sb, torch.bfloat16), atol=0, rtol=0)
    assert bool((out_big[[0, -1]] == SENTINEL).all())


@pytest.mark.gpu
def test_graph_replay_follows_the_scales():
    import flashinfer

    a, bt, sa, sb = exact_problem(3, 40, 256, 384)
    dev_a, dev_b = a.cuda(), bt.transpose(-2, -1).cuda().transpose(-2, -1)
    dev_sa, dev_sb = sa.cuda(), sb.cuda()
    out = torch.full((3, 40, 256), SENTINEL, dtype=torch.bfloat16, device="cuda")
    flashinfer.bmm_fp8(dev_a, dev_b, dev_sa, dev_sb, torch.bfloat16, out=out)  # not the first call under capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        flashinfer.bmm_fp8(dev_a, dev_b, dev_sa, dev_sb, torch.bfloat16, out=out)
    new_sa, new_sb = torch.tensor([8.0]), torch.tensor([0.125 / 4])
    dev_sa.copy_(new_sa)
    dev_sb.copy_(new_sb)
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(out.cpu(), expected_out(a, bt, new_sa, new_sb, torch.bfloat16), atol=0, rtol=0)


def _weight(b, n, k, dtype=E4M3):
    return torch.zeros(b, n, k).to(dtype).transpose(-2, -1)


REFUSALS = {  # name: (changes to the arguments of a valid (2, 8, 64, 128) call, exception)
    "both_e5m2": (dict(A=torch.zeros(2, 8, 128).to(E5M2), B=_weight(2, 64, 128, E5M2)), ValueError),
    "b_row_major": (dict(B=torch.zeros(2, 128, 64).to(E4M3)), ValueError),
    "rank": (dict(A=torch.zeros(8, 128).to(E4M3)), ValueError),
    "batch": (dict(B=_weight(3, 64, 128)), ValueError),
    "k_mismatch": (dict(B=_weight(2, 64, 256)), ValueError),
    "k_not_16": (dict(A=torch.zeros(2, 8, 24).to(E4M3), B=_weight(2, 64, 24)), ValueError),
    "n_not_8": (dict(B=_weight(2, 60, 128)), ValueError),
    "dtype_f32": (dict(dtype=torch.float32), ValueError),
    "scale_two_elements": (dict(A_scale=torch.ones(2)), ValueError),
    "scale_f16": (dict(B_scale=torch.ones(1, dtype=torch.float16)), ValueError),
    "out_shape": (dict(out=torch.zeros(2, 8, 32, dtype=torch.bfloat16)), ValueError),
    "out_dtype": (dict(out=torch.zeros(2, 8, 64, dtype=torch.float16)), ValueError),
    "backend": (dict(backend="triton"), ValueError),
    "cpu_tensors": (dict(), RuntimeError),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name, monkeypatch):
    import flashinfer
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    change, exc = REFUSALS[name]
    kw = dict(A=torch.zeros(2, 8, 128).to(E4M3), B=_weight(2, 64, 128), A_scale=torch.ones(1), B_scale=torch.ones(()),
              dtype=torch.bfloat16)
    kw.update(change)
    with pytest.raises(exc, match="GPU" if exc is RuntimeError else None):
        flashinfer.bmm_fp8(**kw)
