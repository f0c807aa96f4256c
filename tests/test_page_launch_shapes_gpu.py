"""GPU: position expansion, the paged-cache append kernels, packbits and the gated activations at the sizes where
their launches change (csrc/page.hip, csrc/rope.hip, csrc/quantization.hip, csrc/activation.hip).

The position kernels run one workgroup of 256 threads per request, looping i += 256; the append kernels cap the grid
at 256 * 8 workgroups of 256 items; packbits caps it at 65535 workgroups of 256 bytes; act_and_mul caps gridDim.y at
65535 tokens.  Behind every cap stands a stride loop that the other tests never enter.  Each shape below is the
smallest past one cap, with the arithmetic next to it and an assert that recomputes the regime from the launcher's
constants as of this commit.

Copies and scatters are compared bit for bit with a torch index-scatter (or numpy.packbits) into a copy of a cache that
was filled first (NaN for 16-bit types, 0xA5 bytes for fp8 / uint8), which also shows any write outside the target.
"""
import numpy as np
import pytest
import torch

import norm_ref as NR
from attn_inputs import append_problem, indptr_of
from oracle import rope_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

POSITION_THREADS = 256               # rope_positions_kernel / batch_indices_positions_kernel: i += 256 per request
APPEND_GRID_ITEMS = 256 * 8 * 256    # append kernels: 256 * 8 workgroups x 256 items = 524,288 items per pass
PACK_GRID_BYTES = 65535 * 256        # packbits kernels: 65535 workgroups x 256 output bytes per pass
ACT_MAX_GRID_Y = 65535               # act_and_mul_kernel: tokens per pass
FILL_BYTE = 0xA5


def bits(x):
    """integer view of the same bytes (equality on floats would trip over NaN, and fp8 has few torch ops)"""
    x = x.contiguous()
    return x.view(torch.uint8) if x.element_size() == 1 else x.view(torch.int16)


def filled(shape, dtype):
    if dtype in (torch.float16, torch.bfloat16):
        return torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    return torch.full(shape, FILL_BYTE, dtype=torch.uint8, device=DEV).view(dtype)


# ---- C1: position expansion ----------------------------------------------------------------------------------------

LENS = [1, 255, 256, 257, 513, 1000, 0, 3]  # 255 / 256 / 257: either side of one pass; 513, 1000: three and four passes


def _expected_expansion(lens, first_pos):
    """(batch index, position) of every appended token by repeat_interleave / arange."""
    lens_t = torch.tensor(lens)
    bi = torch.repeat_interleave(torch.arange(len(lens)), lens_t)
    starts = indptr_of(lens)[:-1].long()
    pos = torch.arange(int(lens_t.sum())) - starts[bi] + torch.tensor(first_pos)[bi]
    return bi.to(torch.int32), pos.to(torch.int32)


def test_get_batch_indices_positions_beyond_one_pass():
    import flashinfer
    from flashinfer import _lib

    assert max(LENS) > 3 * POSITION_THREADS and {POSITION_THREADS - 1, POSITION_THREADS, POSITION_THREADS + 1} <= set(LENS)
    assert 0 in LENS
    hist = [3, 17, 40, 5, 100, 7, 9, 64]  # tokens each request already holds: nonzero and all different
    nnz = sum(LENS)
    indptr = indptr_of(LENS, DEV)
    seq_lens = torch.tensor([h + n for h, n in zip(hist, LENS)], dtype=torch.int32, device=DEV)
    want_bi, want_pos = _expected_expansion(LENS, hist)
    assert int(want_pos.min()) >= 1
    # through the C entry point into buffers filled with -1 first (the Python wrapper allocates its own)
    bi = torch.full((nnz,), -1, dtype=torch.int32, device=DEV)
    pos = torch.full((nnz,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().fi_get_batch_indices_positions(indptr.data_ptr(), seq_lens.data_ptr(), len(LENS), nnz,
                                                         bi.data_ptr(), pos.data_ptr(), _lib.current_stream(bi.device)),
               "get_batch_indices_positions")
    assert torch.equal(bi.cpu(), want_bi) and torch.equal(pos.cpu(), want_pos)
    bi2, pos2 = flashinfer.get_batch_indices_positions(indptr, seq_lens, nnz)
    assert torch.equal(bi2.cpu(), want_bi) and torch.equal(pos2.cpu(), want_pos)


def test_rope_indptr_form_beyond_one_pass():
    """apply_rope_inplace (indptr, offsets) == apply_rope_pos_ids_inplace on the expanded positions, bit for bit, with
    rope_theta = 1 on one 16-wide head so that the position is the rotation angle itself."""
    import flashinfer
    from flashinfer import _lib

    assert max(LENS) > 3 * POSITION_THREADS
    offsets = [1, 50, 7, 300, 2, 1000, 11, 4]
    nnz = sum(LENS)
    indptr = indptr_of(LENS, DEV)
    offs = torch.tensor(offsets, dtype=torch.int32, device=DEV)
    _, want_pos = _expected_expansion(LENS, offsets)
    assert torch.equal(want_pos.long(), RR.positions_from_indptr(indptr.cpu(), offs.cpu()))
    # the expansion kernel alone, into a buffer filled with -1 first
    pos = torch.full((nnz,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().fi_rope_positions_from_indptr(indptr.data_ptr(), offs.data_ptr(), len(LENS), nnz,
                                                        pos.data_ptr(), _lib.current_stream(pos.device)), "rope positions")
    assert torch.equal(pos.cpu(), want_pos)
    g = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randn(nnz, 1, 16, device=DEV, generator=g).half()
    k = torch.randn(nnz, 1, 16, device=DEV, generator=g).half()
    q1, k1, q2, k2 = q.clone(), k.clone(), q.clone(), k.clone()
    flashinfer.apply_rope_inplace(q1, k1, indptr, offs, rope_theta=1.0)
    flashinfer.apply_rope_pos_ids_inplace(q2, k2, want_pos.to(DEV), rope_theta=1.0)
    assert torch.equal(bits(q1), bits(q2)) and torch.equal(bits(k1), bits(k2))
    changed = (bits(q1) != bits(q)).flatten(1).any(dim=1)
    assert bool(changed.all()), "rows were left unrotated"


# ---- C2: append_paged_kv_cache past the grid cap ---------------------------------------------------------------------

APPEND_LENS = [1, 257, 4000, 12241, 1]
APPEND_HIST = [3, 21, 5, 50, 15]  # nonzero, no multiple of the page size


@pytest.mark.parametrize("as_tuple", [False, True], ids=["5d", "tuple"])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("dtype,hkv", [(torch.float16, 2), (torch.float8_e4m3fn, 4)], ids=["fp16", "fp8"])
def test_append_paged_kv_cache_past_grid_cap(dtype, hkv, layout, as_tuple):
    """One item is one 16-byte chunk: fp16 2 heads * 128 * 2 B / 16 = 32 items per token, fp8 4 heads * 128 B / 16 =
    32 items per token; 16500 tokens * 32 = 528,000 items against 524,288 per pass.  Cache 17 MB."""
    import flashinfer

    d, ps, hq = 128, 16, 2 * hkv
    nnz = sum(APPEND_LENS)
    items = nnz * hkv * (d * dtype.itemsize // 16)
    assert nnz == 16500 and items == 528_000 and APPEND_GRID_ITEMS < items <= 2 * APPEND_GRID_ITEMS
    assert all(h > 0 and h % ps for h in APPEND_HIST)
    pt = append_problem(APPEND_LENS, APPEND_HIST, ps, spare_pages=7, seed=11)
    pages = pt["total_pages"]
    g = torch.Generator(device=DEV).manual_seed(12)
    if dtype == torch.float16:
        packed = torch.randn(nnz, (hq + 2 * hkv) * d, device=DEV, generator=g).to(dtype)
    else:  # any byte is an fp8 number and the kernel only copies
        packed = torch.randint(0, 256, (nnz, (hq + 2 * hkv) * d), device=DEV, generator=g, dtype=torch.uint8).view(dtype)
    k = packed[:, hq * d: (hq + hkv) * d].view(nnz, hkv, d)
    v = packed[:, (hq + hkv) * d:].view(nnz, hkv, d)
    assert not k.is_contiguous() and not v.is_contiguous()
    one = (pages, ps, hkv, d) if layout == "NHD" else (pages, hkv, ps, d)
    if as_tuple:
        cache = (filled(one, dtype), filled(one, dtype))  # two separate allocations
        k_cache, v_cache = cache
    else:
        cache = filled((pages, 2) + one[1:], dtype)
        k_cache, v_cache = cache[:, 0], cache[:, 1]
    # reference: index-scatter into a copy of the filled cache
    page, entry = pt["slot"] // ps, pt["slot"] % ps
    refs = []
    for c, rows in ((k_cache, k), (v_cache, v)):
        ref = bits(c).clone()
        if layout == "NHD":
            ref[page, entry] = bits(rows)
        else:
            ref[page, :, entry] = bits(rows)
        refs.append(ref)
    flashinfer.append_paged_kv_cache(k, v, pt["batch_indices"], pt["positions"], cache, pt["kv_indices"],
                                     pt["kv_indptr"], pt["last"], kv_layout=layout)
    assert torch.equal(bits(k_cache), refs[0]), "k cache differs from the scatter"
    assert torch.equal(bits(v_cache), refs[1]), "v cache differs from the scatter"


# ---- C3: append_paged_mla_kv_cache past the grid cap -----------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_append_paged_mla_kv_cache_past_grid_cap(dtype):
    """72 chunks per token (64 of ckv, 8 of kpe): 7300 tokens * 72 = 525,600 items against 524,288 per pass.  The
    append rows are slices of wider buffers (row stride 584 = 8 * 73 elements)."""
    import flashinfer

    ckv_dim, kpe_dim, ps = 512, 64, 16
    lens, hist = [1, 3000, 4299], [9, 0, 30]
    nnz = sum(lens)
    items = nnz * (ckv_dim + kpe_dim) * 2 // 16
    assert nnz == 7300 and items == 525_600 and APPEND_GRID_ITEMS < items <= 2 * APPEND_GRID_ITEMS
    pt = append_problem(lens, hist, ps, spare_pages=5, seed=21)
    g = torch.Generator(device=DEV).manual_seed(22)
    wide = (torch.randn(nnz, ckv_dim + kpe_dim + 8, device=DEV, generator=g) * 0.5).to(dtype)
    ckv, kpe = wide[:, :ckv_dim], wide[:, ckv_dim: ckv_dim + kpe_dim]
    assert ckv.stride(0) % 8 == 0 and ckv.stride(0) != ckv_dim and kpe.stride(0) != kpe_dim
    ckv_cache = filled((pt["total_pages"], ps, ckv_dim), dtype)
    kpe_cache = filled((pt["total_pages"], ps, kpe_dim), dtype)
    page, entry = pt["slot"] // ps, pt["slot"] % ps
    ref_ckv, ref_kpe = bits(ckv_cache).clone(), bits(kpe_cache).clone()
    ref_ckv[page, entry] = bits(ckv)
    ref_kpe[page, entry] = bits(kpe)
    flashinfer.append_paged_mla_kv_cache(ckv, kpe, pt["batch_indices"], pt["positions"], ckv_cache, kpe_cache,
                                         pt["kv_indices"], pt["kv_indptr"], pt["last"])
    assert torch.equal(bits(ckv_cache), ref_ckv), "ckv cache differs from the scatter"
    assert torch.equal(bits(kpe_cache), ref_kpe), "kpe cache differs from the scatter"


# ---- C4: packbits past 65535 workgroups ------------------------------------------------------------------------------

PACK_N = PACK_GRID_BYTES * 8 + 8 * 300 + 3  # 134,218,083 bools -> 301 output bytes belong to the second pass


@pytest.fixture(scope="module")
def big_bits():
    """(x on the GPU [5 + PACK_N + 13] bool, the same on the host as numpy uint8); made once, never written."""
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randint(0, 2, (5 + PACK_N + 13,), device=DEV, generator=g, dtype=torch.uint8).bool()
    host = x.view(torch.uint8).cpu().numpy()
    yield x, host
    del x
    torch.cuda.empty_cache()


def _packbits_filled(x, little):
    """fi_packbits into an output filled with 0xA5 first (the Python wrapper allocates its own)."""
    from flashinfer import _lib

    xb = x.view(torch.uint8)
    y = torch.full(((xb.numel() + 7) // 8,), FILL_BYTE, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().fi_packbits(xb.data_ptr(), xb.numel(), little, y.data_ptr(), _lib.current_stream(y.device)),
               "packbits")
    return y


@pytest.mark.parametrize("start,bitorder", [(0, "little"), (0, "big"), (3, "little")])
def test_packbits_past_grid_cap(big_bits, start, bitorder):
    """start 0: the buffer is 8-byte aligned, every thread takes the 64-bit load; start 3: no group of 8 is aligned,
    every thread takes the byte-wise branch.  Both need the stride pass."""
    import flashinfer

    x, host = big_bits
    xs, hs = x[start: start + PACK_N], host[start: start + PACK_N]
    assert (xs.data_ptr() % 8 == 0) == (start == 0)
    assert (PACK_N + 7) // 8 > PACK_GRID_BYTES and PACK_N % 8 != 0
    want = torch.from_numpy(np.packbits(hs, bitorder=bitorder))
    got = _packbits_filled(xs, int(bitorder == "little"))
    assert torch.equal(got.cpu(), want)
    assert torch.equal(flashinfer.packbits(xs, bitorder), got)


@pytest.mark.parametrize("bitorder", ["little", "big"])
def test_segment_packbits_past_grid_cap(big_bits, bitorder):
    """segments of 5, PACK_N and 13 bools: 1 + 16,777,261 + 2 output bytes against 16,776,960 per pass; the long
    segment starts at byte 5, so its threads take the byte-wise branch."""
    import flashinfer
    from flashinfer import _lib

    x, host = big_bits
    seg = [5, PACK_N, 13]
    indptr = torch.tensor([0, 5, 5 + PACK_N, 5 + PACK_N + 13], dtype=torch.int32, device=DEV)
    out_lens = [(n + 7) // 8 for n in seg]
    assert sum(out_lens) > PACK_GRID_BYTES
    want = torch.from_numpy(np.concatenate([np.packbits(host[int(indptr[i]): int(indptr[i + 1])], bitorder=bitorder)
                                            for i in range(3)]))
    out_indptr = indptr_of(out_lens, DEV)
    y = torch.full((sum(out_lens),), FILL_BYTE, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().fi_segment_packbits(x.view(torch.uint8).data_ptr(), indptr.data_ptr(), out_indptr.data_ptr(), 3,
                                              y.numel(), int(bitorder == "little"), y.data_ptr(),
                                              _lib.current_stream(y.device)), "segment_packbits")
    assert torch.equal(y.cpu(), want)
    y2, new_indptr = flashinfer.segment_packbits(x, indptr, bitorder)
    assert torch.equal(new_indptr, out_indptr) and torch.equal(y2, y)


# ---- C5: gated activations past 65535 tokens -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("act", ["silu", "gelu", "gelu_tanh"])
def test_act_and_mul_past_grid_y_cap(act, dtype):
    """gridDim.y = min(tokens, 65535): with 65535 + 5 tokens the last 5 rows are each thread's second trip."""
    import flashinfer

    tokens, d = ACT_MAX_GRID_Y + 5, 128
    assert ACT_MAX_GRID_Y < tokens <= 2 * ACT_MAX_GRID_Y
    g = torch.Generator(device=DEV).manual_seed(41)
    x = (torch.randn(tokens, 2 * d, device=DEV, generator=g) * 3.0).to(dtype)
    out = filled((tokens, d), dtype)
    fn = getattr(flashinfer, f"{act}_and_mul")
    assert fn(x, out=out) is out
    want = NR.act_and_mul_ref(x, act)
    NR.assert_close(out[-5:], want[-5:], dtype, f"{act}_and_mul, the rows past {ACT_MAX_GRID_Y}")
    NR.assert_close(out, want, dtype, f"{act}_and_mul")
