"""CPU: the shared input builders of tests/attn_inputs.py -- prefix sums, page-table invariants, cache shapes, the
dense scatter, and a pin of the seeded draw order every GPU test's inputs depend on."""
import pytest
import torch

from attn_inputs import (indptr_of, make_paged, owned_slots, page_table, poison_, poison_unowned,
                         scatter_to_pages)
from oracle import attention_ref as R


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


@pytest.mark.parametrize("page", [1, 5, 16])
def test_owned_slots_marks_exactly_the_tokens(page):
    kv_lens = [0, 1, page, page + 1, 3 * page + 2]
    indptr, indices, last, num_pages = page_table(kv_lens, page, torch.Generator().manual_seed(4), extra_pages=3)
    # surplus entries (graph padding) behind indptr[-1] own nothing, whichever page they name
    padded = torch.cat([indices, indices[:2]])
    owned = owned_slots(kv_lens, indptr, padded, page, num_pages)
    assert owned.shape == (num_pages, page) and owned.dtype == torch.bool
    want = torch.zeros(num_pages * page, dtype=torch.bool)
    for b, n in enumerate(kv_lens):  # token by token, the definition
        for t in range(n):
            slot = int(indices[int(indptr[b]) + t // page]) * page + t % page
            assert not want[slot]  # no slot is held twice
            want[slot] = True
    assert torch.equal(owned.flatten(), want) and int(owned.sum()) == sum(kv_lens)
    used = torch.zeros(num_pages, dtype=torch.bool)
    used[indices.long()] = True
    assert int((~used).sum()) == 3 and not owned[~used].any()  # the spare pages are wholly unowned


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float8_e4m3fn,
                                   torch.float8_e5m2])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
def test_poison_unowned_is_nan_on_the_complement_and_leaves_the_tokens(dtype, layout):
    page, hkv, d = 5, 2, 8
    kv_lens = [0, 1, page, page + 1]
    cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, page, hkv, d, dtype, layout, seed=6)
    owned = owned_slots(kv_lens, indptr, indices, page, cache.shape[0])
    before = cache.clone()
    bad = poison_unowned(cache, layout, owned)
    assert torch.equal(cache.view(torch.uint8), before.view(torch.uint8))  # a copy: the argument is left alone
    assert bad.dtype == dtype and bad.shape == cache.shape
    nhd = lambda c: c if layout == "NHD" else c.transpose(2, 3)  # [pages, 2, page, H, D]
    slots = lambda c: nhd(c).transpose(1, 2)  # [pages, page, 2, H, D]
    assert torch.equal(slots(bad.view(torch.uint8))[owned], slots(cache.view(torch.uint8))[owned])
    assert (slots(bad.view(torch.uint8))[~owned] == 0xFF).all()
    assert slots(bad.float())[~owned].isnan().all() and not slots(bad.float())[owned].isnan().any()
    k, v = poison_unowned((cache[:, 0], cache[:, 1]), layout, owned)  # the tuple form
    assert torch.equal(k.view(torch.uint8), bad[:, 0].view(torch.uint8))
    assert torch.equal(v.view(torch.uint8), bad[:, 1].view(torch.uint8))
    t = torch.zeros(3, 4, dtype=dtype)
    assert poison_(t) is t and t.float().isnan().all()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("page", [5, 16])
def test_the_oracle_never_reads_an_unowned_slot(page, layout, dtype):
    """batch_decode_ref and batch_prefill_ref slice [:kv_len], they do not mask: (o, lse) for the poisoned cache are
    bit-identical to those for the clean one, and finite.  This is what lets the GPU tests hold a kernel that ran on
    the poisoned cache to the oracle of the clean one."""
    hq, hkv, d = 4, 2, 16
    kv_lens = [1, page + 1, 2 * page + 1, 130, page, 0]
    qo_lens = [1, 3, 2 * page + 1, 2, 1, 2]
    cache, indptr, indices, last = make_paged(len(kv_lens), kv_lens, page, hkv, d, dtype, layout, seed=3)
    g = torch.Generator().manual_seed(4)
    owned = owned_slots(kv_lens, indptr, indices, page, cache.shape[0])
    bad = poison_unowned(cache, layout, owned)
    assert bad.float().isnan().any()
    q = torch.randn(len(kv_lens), hq, d, generator=g)
    clean = R.batch_decode_ref(q, cache.float(), layout, indptr, indices, last)
    dirty = R.batch_decode_ref(q, bad.float(), layout, indptr, indices, last)
    for a, b in zip(clean, dirty):
        assert torch.equal(a, b) and torch.isfinite(b).all()
    qp = torch.randn(sum(qo_lens), hq, d, generator=g)
    for causal in (False, True):
        clean = R.batch_prefill_ref(qp, indptr_of(qo_lens), cache.float(), layout, indptr, indices, last, causal=causal)
        dirty = R.batch_prefill_ref(qp, indptr_of(qo_lens), bad.float(), layout, indptr, indices, last, causal=causal)
        for a, b in zip(clean, dirty):
            assert torch.equal(a, b) and not b.isnan().any()


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
