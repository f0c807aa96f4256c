"""The contiguous-layout grouped fp8 GEMM (flashinfer.gemm.group_deepgemm_fp8_nt_groupwise, csrc/gemm_contig.hip)
against an f64 reference computed here: dequantise a and b with their scales, matmul per 128-row block with the group
of the block's first row.  The exact cases use integers in [-4, 4] and power-of-two scales (2^-2 .. 2^2), so every
product and sum is exact in f32 and the comparison is at atol = rtol = 0; the random case holds the bar of
tests/test_gemm_gpu.py (1e-2, the reference's own test).  Everything is compared on the CPU."""
import pytest
import torch

SENTINEL = 12345.0
N, K = 256, 384  # two n tiles, three k blocks
# name: (G, [(group of the block, rows that carry it; the rest of the 128 are -1)], m or None for 128 per block)
LAYOUTS = {
    "unsorted_repeated_dead_between": (3, [(2, 128), (0, 128), (2, 128), (-1, 0), (1, 128)], None),
    "tail_padding_1_127_128": (3, [(0, 1), (1, 127), (2, 128)], None),
    "short_last_block": (2, [(1, 128), (0, 128), (1, 128)], 128 * 2 + 40),
    "index_at_and_past_G": (2, [(2, 128), (1, 128), (10 ** 6, 128)], None),
    "all_dead": (2, [(-1, 0), (-7, 128)], None),
}
SORTED = (3, [(0, 128), (0, 128), (1, 128), (2, 128)], None)  # padding-free: m_indptr 0, 256, 384, 512


def indices_of(blocks, m):
    idx = torch.cat([torch.cat([torch.full((rows,), g), torch.full((128 - rows,), -1)]) for g, rows in blocks])
    return idx[:m].to(torch.int32)


def exact_problem(G, m, n, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-4, 5, (m, k), generator=g).float().to(torch.float8_e4m3fn)
    b = torch.randint(-4, 5, (G, n, k), generator=g).float().to(torch.float8_e4m3fn)
    sa = torch.exp2(torch.randint(-2, 3, (m, k // 128), generator=g).float())
    sb = torch.exp2(torch.randint(-2, 3, (G, n // 128, k // 128), generator=g).float())
    return a, b, sa, sb


def random_problem(G, m, n, k, seed=1):
    from oracle.gemm_ref import quantize_fp8

    g = torch.Generator().manual_seed(seed)
    a, sa = quantize_fp8(torch.randn(m, k, generator=g), (1, 128), "K")
    b, sb = quantize_fp8(torch.randn(G, n, k, generator=g), (1, 128, 128), "K")
    # the quantiser's scales are powers of two: make them anything
    return a, b, sa * (1 + torch.rand(sa.shape, generator=g)), sb * (1 + torch.rand(sb.shape, generator=g))


def live_rows(idx, G):
    """Rows that are computed: a non-negative index in a block whose first row names a group."""
    first = idx[torch.arange(idx.numel()) // 128 * 128]
    return (first >= 0) & (first < G) & (idx >= 0), first


def expected_out(a, b, sa, sb, idx, dtype):
    """The sentinel everywhere but the live rows, which hold the f64 product rounded to dtype."""
    live, first = live_rows(idx, b.shape[0])
    ad = a.double() * sa.double().repeat_interleave(128, 1)
    bd = b.double() * sb.double().repeat_interleave(128, 1).repeat_interleave(128, 2)
    out = torch.full((a.shape[0], b.shape[1]), SENTINEL, dtype=dtype)
    for m0 in range(0, a.shape[0], 128):
        rows = torch.nonzero(live[m0:m0 + 128]).flatten() + m0
        if rows.numel():
            out[rows] = (ad[rows] @ bd[first[m0]].T).to(dtype)
    return out


def run(a, b, sa, sb, idx, dtype, via=None):
    """The call on poisoned inputs (NaN in every row of a and a_scale that is not live) into a sentinel-filled out;
    returns it on the CPU."""
    import flashinfer.gemm

    live, _ = live_rows(idx, b.shape[0])
    a, sa = a.clone().view(torch.uint8), sa.clone()
    a[~live] = 0x7F
    sa[~live] = float("nan")
    out = torch.full((a.shape[0], b.shape[1]), SENTINEL, dtype=dtype, device="cuda")
    args = (a.view(torch.float8_e4m3fn).cuda(), b.cuda(), sa.cuda(), sb.cuda(), idx.cuda())
    res = (via or flashinfer.gemm.group_deepgemm_fp8_nt_groupwise)(*args, out=out)
    assert res is out
    return out.cpu()


def assert_exact(out, want):
    torch.testing.assert_close(out, want, atol=0, rtol=0)
    dead = want == SENTINEL  # a live value equal to the sentinel passes either way
    assert torch.equal(out.view(torch.int16)[dead], want.view(torch.int16)[dead])


def problem_of(layout, make, n=N, k=K):
    G, blocks, m = layout
    idx = indices_of(blocks, m)
    return make(G, idx.numel(), n, k), idx


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_exact_small_integers(name, dtype):
    p, idx = problem_of(LAYOUTS[name], exact_problem)
    assert_exact(run(*p, idx, dtype), expected_out(*p, idx, dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_random_operands(dtype):
    p, idx = problem_of(LAYOUTS["unsorted_repeated_dead_between"], random_problem)
    out, want = run(*p, idx, dtype), expected_out(*p, idx, dtype)
    torch.testing.assert_close(out.float(), want.float(), atol=1e-2, rtol=1e-2)


@pytest.mark.gpu
def test_persistent_walk():
    """40 blocks over 9 experts (unsorted, some dead, some tail-padded) at n = 384 -- a full and a half n tile -- on a
    grid of 8 workgroups: every workgroup walks several tiles and stores each behind the next one's first loads."""
    from flashinfer import _lib

    blocks = [(-1, 0) if i % 11 == 5 else ((7 * i) % 9, 128 - (i % 3) * 50) for i in range(40)]
    p, idx = problem_of((9, blocks, None), exact_problem, n=384, k=128)
    _lib.set_option("FI_NUM_CUS", 4)
    try:
        out = run(*p, idx, torch.bfloat16)
    finally:
        _lib.set_option("FI_NUM_CUS", None)
    assert_exact(out, expected_out(*p, idx, torch.bfloat16))


@pytest.mark.gpu
def test_more_blocks_than_the_kernel_lists():
    """2033 blocks, one more than the kernel's list of live blocks holds: it then walks every block and skips the dead
    ones (every fifth, and the last) where they lie."""
    blocks = [(-1, 0) if i % 5 == 4 or i == 2032 else (i % 3, 128 - (i % 2)) for i in range(2033)]
    p, idx = problem_of((3, blocks, None), exact_problem, n=128, k=128)
    assert_exact(run(*p, idx, torch.bfloat16), expected_out(*p, idx, torch.bfloat16))


@pytest.mark.gpu
@pytest.mark.parametrize("make", [exact_problem, random_problem])
def test_equals_the_m_indptr_path_on_a_sorted_layout(make):
    """Bit for bit on the exact operands; within one rounding of the output (bf16: 2^-7 relative) on the random ones."""
    import flashinfer.gemm

    p, idx = problem_of(SORTED, make)
    indptr = torch.tensor([0, 256, 384, 512], dtype=torch.int32, device="cuda")
    other = flashinfer.gemm.group_gemm_fp8_nt_groupwise(*(t.cuda() for t in p), indptr, scale_major_mode="K").cpu()
    out = run(*p, idx, torch.bfloat16)
    if make is exact_problem:
        assert torch.equal(out.view(torch.int16), other.view(torch.int16))
    else:
        torch.testing.assert_close(out.float(), other.float(), atol=2.0 ** -14, rtol=2.0 ** -7)


@pytest.mark.gpu
def test_deep_gemm_spelling_gives_the_same_output():
    import flashinfer.deep_gemm

    def via(a, b, sa, sb, idx, out):
        assert flashinfer.deep_gemm.m_grouped_fp8_gemm_nt_contiguous((a, sa), (b, sb), out, idx) is None
        return out

    p, idx = problem_of(LAYOUTS["tail_padding_1_127_128"], random_problem)
    assert torch.equal(run(*p, idx, torch.bfloat16, via=via).view(torch.int16),
                       run(*p, idx, torch.bfloat16).view(torch.int16))
