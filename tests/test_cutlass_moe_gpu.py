"""GPU: the unquantised MoE layer (flashinfer.fused_moe_16bit.cutlass_fused_moe) on the grouped 16-bit GEMM of csrc/gemm_16bit.hip
against the fp64 oracle of tests/moe_16bit_ref.py: the GEMM bit for bit on integer operands, its SwiGLU epilogue within two
ulp, the sort against moe_permute_mxfp8, the finalize, then the layer -- bit-identical to its four stages called by hand and
at the reference's own bar against the oracle.

Layouts are the smallest at which the kernel can still go wrong: a single row, an empty group beside one that crosses a
128-row tile and ends in a partial tile, and 72 groups (a second pass of the 64-group tile lookup); (n, k) = (192, 320) has a
half-filled n tile and five k steps, more than the ring holds."""
import pytest
import torch

import moe_16bit_ref as R16
import moe_ref as M
from test_fused_moe_gpu import PERMUTE_CASES, _activations

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
LAYOUTS = {
    "one_row": [0, 1],
    "ragged": [0, 5, 5, 133, 300],
    "72_groups": [0] + torch.randint(0, 4, (72,), generator=torch.Generator().manual_seed(72)).cumsum(0).tolist(),
}
TAIL = 3  # rows of d past m_indptr[-1]: prefilled, must stay


def _fm():
    from flashinfer import fused_moe

    return fused_moe


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _gemm_case(layout, n, k, dtype, gather, amax, bmax, live_k=None):
    """Integer operands: (a, b, m_indptr, row_ids or None, rows of d).  live_k: only that many columns of a are non-zero,
    spread over all k steps, which bounds |a . b| by live_k * amax * bmax."""
    indptr = torch.tensor(LAYOUTS[layout], dtype=torch.int32)
    rows, G = int(indptr[-1]) + TAIL, len(indptr) - 1
    a_rows = 37 if gather else rows
    a = _ints((a_rows, k), -amax, amax, 1)
    if live_k is not None:
        a[:, torch.arange(k) % (k // live_k) != 0] = 0
    b = _ints((G, n, k), -bmax, bmax, 2)
    # non-monotone with repeats; the entries of the tail rows are never read
    row_ids = torch.cat([_ints((rows - TAIL,), 0, a_rows - 1, 3), torch.full((TAIL,), -7.0)]).int() if gather else None
    return a.to(dtype), b.to(dtype), indptr, row_ids, rows


def _run_gemm(a, b, indptr, row_ids, rows, **kw):
    out = torch.full((rows, b.shape[1] // (2 if kw.get("swiglu") else 1)), 0.4375, dtype=a.dtype, device=DEV)
    _fm().moe_group_gemm_16bit(a.to(DEV), b.to(DEV), indptr.to(DEV), None if row_ids is None else row_ids.to(DEV), out=out,
                               **{k_: v.to(DEV) if torch.is_tensor(v) else v for k_, v in kw.items()})
    out = out.cpu()
    assert bool((out[rows - TAIL:] == 0.4375).all()), "rows at or past m_indptr[-1] were written"
    return out[:rows - TAIL]


@pytest.mark.parametrize("gather", [False, True], ids=["rows", "gather"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("n,k", [(64, 64), (192, 320)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_group_gemm_is_exact_on_integers(dtype, n, k, layout, gather):
    """Operands in [-4, 4], k <= 512: every partial sum is an integer below 2^24, so the f32 accumulation is exact in any
    order and the result (at most 8192) is rounded once: bit-equal to the rounded fp64 product."""
    a, b, indptr, row_ids, rows = _gemm_case(layout, n, k, dtype, gather, 4, 4)
    got = _run_gemm(a, b, indptr, row_ids, rows)
    want = (R16.group_gemm_ref(a, b, indptr, row_ids) + 0.0).to(dtype)  # + 0.0: no -0 from a row of zero products
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("gated", [False, True], ids=["silu", "alpha_beta_limit"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("I,k", [(64, 64), (192, 320)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_swiglu_epilogue(dtype, I, k, layout, gated):
    """Operands in [-1, 1] with 64 live columns of a: the accumulators are exact integers of magnitude <= 64, so exp(alpha
    |x1|) (alpha <= 1) stays inside f32 and |act| inside f16.  What is left is the f32 evaluation of the sigmoid and of two
    products, far below a 16-bit ulp, and the one rounding: one ulp, a second for a flip at a rounding boundary."""
    a, b, indptr, row_ids, rows = _gemm_case(layout, 2 * I, k, dtype, True, 1, 1, live_k=64)
    G = len(indptr) - 1
    kw = {}
    if gated:
        kw = dict(alpha=torch.linspace(0.5, 1.0, G), beta=torch.linspace(0.0, 1.0, G), limit=torch.linspace(5.0, 9.0, G))
    got = _run_gemm(a, b, indptr, row_ids, rows, swiglu=True, **kw).double()
    want = R16.group_gemm_ref(a, b, indptr, row_ids, swiglu=True, **kw)
    swapped = R16.group_gemm_ref(a, torch.cat(b.chunk(2, dim=1)[::-1], dim=1), indptr, row_ids, swiglu=True, **kw)
    assert not torch.equal(want.to(dtype), swapped.to(dtype)), "the inputs cannot tell the gate from the linear half"
    rounded = want.to(dtype).double()
    err = (got - rounded).abs() / R16.ulp(rounded, dtype)
    print("swiglu max error in ulp:", err.max().item())
    assert bool((err <= 2).all())


@pytest.mark.parametrize("case", sorted(PERMUTE_CASES))
def test_sort_matches_the_permute(case):
    build, offset, G = PERMUTE_CASES[case]
    ids = build()
    x_q, x_sf = _activations(ids.shape[0], 128, seed=1)
    want_indptr, want_map = _fm().moe_permute_mxfp8(ids.to(DEV), x_q, x_sf, offset, G)[:2]
    m_indptr, emap, p2e = _fm().moe_sort(ids.to(DEV), offset, G)
    assert torch.equal(m_indptr, want_indptr) and torch.equal(emap, want_map)
    inverse = M.permute_ref(ids, offset, G)[2]
    assert p2e.cpu()[:len(inverse)].tolist() == list(inverse)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_finalize_16bit(dtype):
    """f32 fma in the order of the slots, one rounding: half an ulp of the result, plus 2^-22 of the sum of |terms| for the
    accumulation.  Token 1 has a slot outside the window (-1), token 3 none inside: zeros."""
    T, top_k, H, rows = 5, 3, 264, 9
    g = torch.Generator().manual_seed(5)
    y = torch.randn(rows, H, generator=g).to(dtype)
    w = torch.rand(T, top_k, generator=g)
    emap = torch.tensor([0, 4, 8, 2, -1, 5, 7, 6, 1, -1, -1, -1, 3, 3, 0], dtype=torch.int32)
    out = torch.full((T, H), 9.0, dtype=dtype, device=DEV)
    assert _fm().moe_finalize_16bit(y.to(DEV), w.to(DEV), emap.to(DEV), out) is out
    want, sum_abs = M.finalize_ref(y.double(), w.double(), emap, top_k)
    err = (out.cpu().double() - want).abs()
    assert bool((err <= 0.5 * R16.ulp(want, dtype) * (1 + 2.0 ** -10) + 2.0 ** -22 * sum_abs).all()), err.max().item()
    assert bool((out.cpu()[3] == 0).all())


# ---- the layer ----------------------------------------------------------------------------------------------------------
LAYER_CASES = {
    # name: (T, E, top_k, H, I, gated, ep_size, ep_rank)
    "reference_case": (1, 2, 2, 128, 128, False, 1, 0),
    "ragged": (67, 8, 2, 256, 192, False, 1, 0),
    "alpha_beta_limit": (67, 8, 2, 256, 192, True, 1, 0),
    "ep_rank_1_of_4": (67, 8, 2, 256, 192, False, 4, 1),
}


def _layer_inputs(case, dtype):
    """randn / 5 inputs and softmax top-k routing, as the reference's test makes them; the weights of the local experts."""
    T, E, top_k, H, I, gated, ep_size, ep_rank = LAYER_CASES[case]
    g = torch.Generator().manual_seed(42)
    x = (torch.randn(T, H, generator=g) / 5).to(dtype)
    scales, ids = torch.topk(torch.softmax(torch.randn(T, E, generator=g), dim=-1), top_k, dim=-1)
    G = E // ep_size
    w31 = (torch.randn(E, 2 * I, H, generator=g) / 5).to(dtype)[ep_rank * G:(ep_rank + 1) * G].contiguous()
    w2 = (torch.randn(E, H, I, generator=g) / 5).to(dtype)[ep_rank * G:(ep_rank + 1) * G].contiguous()
    gates = [t.contiguous() for t in (torch.linspace(0.5, 1.0, G), torch.linspace(0.0, 1.0, G), torch.linspace(1.0, 7.0, G))]
    return x, ids.int(), scales.float(), w31, w2, (gates if gated else [None] * 3), top_k, ep_size, ep_rank


def _to_dev(ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.mark.parametrize("case", sorted(LAYER_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_layer_against_the_oracle(dtype, case):
    """All elements at the reference's bar (test_trtllm_cutlass_fused_moe.py:273): rtol = atol = 1e-2 in f16, and the same
    scaled by the ulp ratio 2^-8 / 2^-11 in bf16.  Measured maxima: DESIGN.md 3.13c."""
    x, ids, scales, w31, w2, gates, top_k, ep_size, ep_rank = _layer_inputs(case, dtype)
    dx, dids, dscales, dw31, dw2 = _to_dev([x, ids, scales, w31, w2])
    dgates = _to_dev(gates)
    out = torch.empty_like(dx)
    from flashinfer.fused_moe_16bit import cutlass_fused_moe

    res = cutlass_fused_moe(dx, dids, dscales, dw31, dw2, dtype, quant_scales=None, swiglu_alpha=dgates[0],
                            swiglu_beta=dgates[1], swiglu_limit=dgates[2], ep_size=ep_size, ep_rank=ep_rank, output=out)
    assert isinstance(res, list) and len(res) == 1 and res[0] is out
    G = w31.shape[0]
    want = R16.moe_16bit_ref(x, ids, scales, w31, w2, ep_rank * G, *gates)
    err = (out.cpu().double() - want).abs()
    print(f"{case} {dtype}: max abs error {err.max().item():.3e}, max |want| {want.abs().max().item():.3e}")
    tol = 1e-2 if dtype == torch.float16 else 8e-2
    torch.testing.assert_close(out.cpu().double(), want, rtol=tol, atol=tol)
    if case == "ragged":  # bit for bit the four stages called by hand
        F = _fm()
        m_indptr, emap, p2e = F.moe_sort(dids, 0, G)
        act = F.moe_group_gemm_16bit(dx, dw31, m_indptr, a_row_ids=p2e, swiglu=True, a_row_ids_div=top_k)
        y = F.moe_group_gemm_16bit(act, dw2, m_indptr)
        by_hand = F.moe_finalize_16bit(y, dscales, emap)
        assert torch.equal(by_hand.view(torch.int16), out.view(torch.int16))
