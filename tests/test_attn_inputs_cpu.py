"""CPU: the shared input builders of tests/attn_inputs.py -- prefix sums, page-table invariants, cache shapes, the
dense scatter, and a pin of the seeded draw order every GPU test's inputs depend on."""
import pytest
import torch

from attn_inputs import indptr_of, make_paged, page_table, scatter_to_pages


def test_indptr_of():
    assert indptr_of([]).tolist() == [0]
    assert indptr_of([0, 3, 0, 0, 5]).tolist() == [0, 0, 3, 3, 3, 8]
    assert indptr_of(torch.tensor([2, 1])).tolist() == [0, 2, 3]
    assert indptr_of([2 ** 30, 2 ** 30 - 1]).tolist() == [0, 2 ** 30, 2 ** 31 - 1]  # no int32 step on the way
    for lens in ([], [4, 1]):
        t = indptr_of(lens)
        assert t.dtype == torch.int32 and t.device.type == "cpu"
        assert indptr_of(lens, "cpu").device.type == "cpu" and indptr_of(lens, "meta").device.type == "meta"


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("page", [1, 5, 16])
def test_page_table_invariants(page, extra):
    kv_lens = (0, 1, page, page + 1)
    indptr, indices, last, num_pages = page_table(kv_lens, page, torch.Generator().manual_seed(1), extra_pages=extra)
    assert indptr.dtype == indices.dtype == last.dtype == torch.int32
    assert indptr.diff().tolist() == [-(-l // page) for l in kv_lens] == [0, 1, 1, 2]
    assert last.tolist() == [0, 1, page, 1] == [(l - 1) % page + 1 if l else 0 for l in kv_lens]
    total = int(indptr[-1])
    assert num_pages == total + extra and len(indices) == total == len(set(indices.tolist()))
    assert 0 <= int(indices.min()) and int(indices.max()) < num_pages
    plain = page_table(kv_lens, page, extra_pages=extra, shuffle=False)
    assert plain[1].tolist() == list(range(total)) and plain[3] == num_pages
    assert torch.equal(plain[0], indptr) and torch.equal(plain[2], last)


def test_page_table_without_generator_draws_once_from_the_global_rng():
    torch.manual_seed(3)
    indices = page_table([40, 7], 16, extra_pages=2)[1]
    after = torch.rand(1)
    torch.manual_seed(3)
    assert torch.equal(indices, torch.randperm(6)[:4].to(torch.int32)) and torch.equal(after, torch.rand(1))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float8_e4m3fn])
def test_make_paged_shapes_and_dtype(dtype):
    kv_lens, page, hkv, d = [5, 16, 17, 0], 8, 3, 16
    for layout, shape in (("NHD", (9, 2, page, hkv, d)), ("HND", (9, 2, hkv, page, d))):
        cache, indptr, indices, last = make_paged(4, kv_lens, page, hkv, d, dtype, layout, seed=2)
        assert cache.shape == shape and cache.dtype == dtype
        assert len(indices) == int(indptr[-1]) == 6 and last.tolist() == [5, 8, 1, 0]
    assert make_paged(4, kv_lens, page, hkv, d, dtype, "NHD", seed=2, extra_pages=0)[0].shape[0] == 6
    assert make_paged(4, kv_lens, page, hkv, d, dtype, "NHD", seed=2, shuffle=False)[2].tolist() == list(range(6))


@pytest.mark.parametrize("layout", ["NHD", "HND"])
def test_scatter_to_pages_round_trip(layout):
    kv_lens, page, h, d = [13, 0, 8, 1], 4, 2, 8
    g = torch.Generator().manual_seed(5)
    k = torch.randn(sum(kv_lens), h, d, generator=g).half()
    v = torch.randn(sum(kv_lens), h, d, generator=g).half()
    indptr, indices, last, num_pages = page_table(kv_lens, page, g, extra_pages=2)
    cache = scatter_to_pages(k, v, kv_lens, indptr, indices, page, num_pages, layout)
    assert cache.dtype == k.dtype
    assert cache.shape == ((num_pages, 2, page, h, d) if layout == "NHD" else (num_pages, 2, h, page, d))
    nhd = cache if layout == "NHD" else cache.transpose(2, 3)
    off = 0
    for b, n in enumerate(kv_lens):
        pages = nhd[indices[int(indptr[b]):int(indptr[b + 1])].long()]  # [pages, 2, page, h, d]
        assert torch.equal(pages[:, 0].reshape(-1, h, d)[:n], k[off:off + n])
        assert torch.equal(pages[:, 1].reshape(-1, h, d)[:n], v[off:off + n])
        assert not pages[-1:, :, (n - 1) % page + 1:].any()  # the tail of the last page stays zero
        off += n
    used = torch.zeros(num_pages, dtype=torch.bool)
    used[indices.long()] = True
    assert not nhd[~used].any()  # spare pages stay zero


def test_make_paged_draw_order_is_pinned():
    """The values the builder gave before it moved here: the page permutation is drawn first, then the cache."""
    cache, indptr, indices, last = make_paged(4, [5, 16, 17, 0], 8, 1, 8, torch.float16, "NHD", seed=11)
    assert indptr.tolist() == [0, 1, 3, 6, 6]
    assert indices.tolist() == [0, 8, 2, 1, 7, 3]
    assert last.tolist() == [5, 8, 1, 0]
    assert cache.shape == (9, 2, 8, 1, 8) and cache.dtype == torch.float16
    assert cache.flatten()[0].item() == 1.0419921875
    hnd = make_paged(4, [5, 16, 17, 0], 8, 1, 8, torch.float16, "HND", seed=11)[0]
    assert hnd.shape == (9, 2, 1, 8, 8)
