"""GPU: flashinfer.SegmentGEMMWrapper (csrc/segment_gemm.hip) against the fp64 product, segment by segment.

Shapes (d_in, d_out) and the form each runs (long k: d_out <= 128 and d_in >= 256; else wide n):
  (8, 8)     wide n  less than one 32-element MFMA step on both sides
  (320, 16)  long k  10 k steps, which do not divide evenly over the four waves; half a column pair
  (264, 40)  long k  a k tail (8 of 32) in the ninth step, two column pairs with the second one a quarter full
  (16, 200)  wide n  k below one step, a partial 256-column tile (wave 3 has 8 live columns)
  (72, 40)   wide n  k tail and n tail together
  (136, 8)   wide n  two 128-element chunks of x through LDS, the second one a k tail of 8; one column tile
  (264, 136) wide n  three chunks (both x buffers reused), a k tail in the third, an n tail in wave 2
Segment layouts: one row; empty segments beside one that crosses a 16-row and a 32-row tile, with partial last tiles;
70 segments of 0-3 rows (the record scan crosses a wave, seven probes of the binary search); 300 segments of 0-3 rows
(a second, partial pass of the 256-segment record kernel: row and tile carries, records of two passes in one search)."""
import pytest
import torch

import flashinfer

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
SHAPES = [(8, 8), (320, 16), (264, 40), (16, 200), (72, 40), (136, 8), (264, 136)]
LAYOUTS = {
    "one_row": [1],
    "ragged": [0, 5, 0, 17, 33],
    "70_segments": torch.randint(0, 4, (70,), generator=torch.Generator().manual_seed(70)).tolist(),
    "300_segments": torch.randint(0, 4, (300,), generator=torch.Generator().manual_seed(300)).tolist(),
}
TAIL = 3  # rows of x and out past seg_indptr[-1]
SENTINEL = 0.4375  # no integer, exact in both dtypes


def _ints(shape, seed):
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).float()


def _weight_ids(batch, num_weights):
    """Repeats, not monotone, reaching into the upper entries: 3, nw - 2, 1, nw - 4, 3, ..."""
    i = torch.arange(batch)
    return (3 - i) % 4 + (i % 2) * (num_weights - 4)


def _ref(x, w, lens, ids, column_major):
    want, r = torch.zeros(x.shape[0], w.shape[1] if column_major else w.shape[2], dtype=torch.float64), 0
    for n, i in zip(lens, ids):
        if 0 <= i < w.shape[0]:
            want[r:r + n] = x[r:r + n].double() @ (w[i].double().T if column_major else w[i].double())
        r += n
    return want


def _run(x, w, lens, ids, column_major, given):
    out = torch.full((x.shape[0], w.shape[1] if column_major else w.shape[2]), SENTINEL, dtype=x.dtype, device=DEV)
    if given == "lens_cpu":
        seg = dict(seg_lens=torch.tensor(lens, dtype=torch.int64))
    else:
        seg = dict(seg_indptr=torch.tensor([0] + lens, dtype=torch.int64).cumsum(0).to(DEV))
    wrapper = flashinfer.SegmentGEMMWrapper(torch.empty(1024, dtype=torch.int8, device=DEV))
    got = wrapper.run(x.to(DEV), w.to(DEV), len(lens), column_major, out=out, weight_indices=ids, **seg)
    assert got is out
    return out.cpu()


def _written(lens, ids, num_weights, rows):
    live = torch.zeros(rows, dtype=torch.bool)
    r = 0
    for n, i in zip(lens, ids):
        live[r:r + n] = 0 <= i < num_weights
        r += n
    return live


def _case(lens, d_in, d_out, dtype, column_major, num_weights, maker):
    rows = sum(lens) + TAIL
    x = maker((rows, d_in), 1).to(dtype)
    w = maker((num_weights, d_out, d_in) if column_major else (num_weights, d_in, d_out), 2).to(dtype)
    return x, w


@pytest.mark.parametrize("given", ["lens_cpu", "indptr_device"])
@pytest.mark.parametrize("indexed", [False, True], ids=["own_weight", "weight_indices"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("d_in,d_out", SHAPES)
@pytest.mark.parametrize("column_major", [True, False], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_segment_gemm_is_exact_on_integers(dtype, column_major, d_in, d_out, layout, indexed, given):
    """Operands in [-4, 4], d_in <= 512: every partial sum is an integer below 2^24, so f32 accumulation is exact in any
    order, the four-way k split included, and the result is rounded once: bit-equal to the rounded fp64 product.  The
    rows past the last segment keep what they held."""
    lens = LAYOUTS[layout]
    num_weights = len(lens) + 3 if indexed else len(lens)
    ids = _weight_ids(len(lens), num_weights) if indexed else None
    x, w = _case(lens, d_in, d_out, dtype, column_major, num_weights, _ints)
    got = _run(x, w, lens, ids, column_major, given)
    id_list = ids.tolist() if indexed else list(range(len(lens)))
    want = (_ref(x, w, lens, id_list, column_major) + 0.0).to(dtype)  # + 0.0: no -0 from a row of zero products
    live = _written(lens, id_list, num_weights, x.shape[0])
    assert bool((got[~live] == SENTINEL).all()), "rows of no segment were written"
    assert torch.equal(got[live].view(torch.int16), want[live].view(torch.int16))


@pytest.mark.parametrize("d_in,d_out", [(320, 16), (16, 200)], ids=["long_k", "wide_n"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_segments_with_a_weight_id_out_of_range_are_skipped(dtype, d_in, d_out):
    """Weight ids num_weights and -1: the rows of those segments keep the sentinel, every other row is exact."""
    lens, num_weights = [4, 17, 2, 20, 9], 6
    ids = torch.tensor([5, num_weights, 0, -1, 5])
    x, w = _case(lens, d_in, d_out, dtype, True, num_weights, _ints)
    got = _run(x, w, lens, ids, True, "lens_cpu")
    want = (_ref(x, w, lens, ids.tolist(), True) + 0.0).to(dtype)
    live = _written(lens, ids.tolist(), num_weights, x.shape[0])
    assert int(live.sum()) == 15
    assert bool((got[~live] == SENTINEL).all()), "rows of a skipped segment, or of none, were written"
    assert torch.equal(got[live].view(torch.int16), want[live].view(torch.int16))


@pytest.mark.parametrize("column_major", [True, False], ids=["colmajor", "rowmajor"])
@pytest.mark.parametrize("d_in,d_out", [(2048, 16), (16, 1024)], ids=["long_k", "wide_n"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_segment_gemm_on_reals(dtype, d_in, d_out, column_major):
    """randn operands against the fp64 product `want`.  Per element |got - want| <= u |want| + d_in 2^-23 S: one rounding
    to the output type (u = 2^-11 for f16, 2^-8 for bf16) and f32 accumulation of d_in terms in any order, each step's
    error at most 2^-24 of a partial sum that S = sum_i |x_i| |w_i| bounds.  Every element is compared."""
    lens = LAYOUTS["ragged"]
    num_weights = len(lens) + 3
    ids = _weight_ids(len(lens), num_weights)

    def randn(shape, seed):
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed))

    x, w = _case(lens, d_in, d_out, dtype, column_major, num_weights, randn)
    got = _run(x, w, lens, ids, column_major, "indptr_device")[:-TAIL].double()
    want = _ref(x, w, lens, ids.tolist(), column_major)[:-TAIL]
    S = _ref(x.abs(), w.abs(), lens, ids.tolist(), column_major)[:-TAIL]
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    excess = (got - want).abs() - (u * want.abs() + d_in * 2.0 ** -23 * S)
    print("largest error over its bar:", ((got - want).abs() / (u * want.abs() + d_in * 2.0 ** -23 * S)).max().item())
    assert got.shape == want.shape and bool((excess <= 0).all())
