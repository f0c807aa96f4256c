"""Inputs, tolerances and wrapper set-up shared by the attention tests: prefix sums, shuffled page tables, paged
caches (random, or scattered from dense rows), the decode and prefill output bars, and "make a wrapper, plan it".

Plain functions, no fixtures.  Every builder draws from the generator it is given (or the global RNG) in a fixed order,
which tests/test_attn_inputs_cpu.py pins: the seeded inputs of the whole suite hang on it."""
import itertools

import torch

DEV = "cuda:0"


def indptr_of(lens, device=None):
    """int32 prefix sums [0, l0, l0 + l1, ...] of a list of lengths (summed as Python ints)."""
    return torch.tensor([0, *itertools.accumulate(int(l) for l in lens)], dtype=torch.int32, device=device)


def page_table(kv_lens, page_size, generator=None, extra_pages=0, shuffle=True):
    """(indptr, indices, last_page_len, num_pages) of requests holding kv_lens tokens: ceil(l / page_size) pages each,
    taken from one randperm over num_pages = total + extra_pages pages (arange without shuffle); last_page_len is 0 for
    an empty request."""
    indptr = indptr_of(-(-l // page_size) for l in kv_lens)
    total = int(indptr[-1])
    last = torch.tensor([(l - 1) % page_size + 1 if l > 0 else 0 for l in kv_lens], dtype=torch.int32)
    perm = torch.randperm(total + extra_pages, generator=generator)[:total] if shuffle else torch.arange(total)
    return indptr, perm.to(torch.int32), last, total + extra_pages


def make_paged(batch, kv_lens, page_size, hkv, d, dtype, layout, seed, shuffle=True, extra_pages=3):
    """A random paged cache: (cache, indptr, indices, last_page_len).  Draws the page permutation, then the cache."""
    g = torch.Generator().manual_seed(seed)
    indptr, indices, last, pages = page_table(kv_lens, page_size, g, extra_pages, shuffle)
    shape = (pages, 2, page_size, hkv, d) if layout == "NHD" else (pages, 2, hkv, page_size, d)
    return torch.randn(shape, generator=g).to(dtype), indptr, indices, last


def scatter_to_pages(k, v, kv_lens, indptr, indices, page_size, num_pages, layout="NHD"):
    """k, v rows [sum(kv_lens), H, D], request after request, written to their slots of a zeroed paged cache of the
    rows' dtype."""
    cache = torch.zeros(num_pages, 2, page_size, *k.shape[1:], dtype=k.dtype)
    off = 0
    for b, n in enumerate(kv_lens):
        t = torch.arange(n)
        pages = indices[int(indptr[b]) + t // page_size].long()
        cache[pages, 0, t % page_size] = k[off:off + n]
        cache[pages, 1, t % page_size] = v[off:off + n]
        off += n
    return cache if layout == "NHD" else cache.transpose(2, 3).contiguous()


def append_problem(lens, hist, ps, spare_pages, seed):
    """Page table (shuffled, with spare pages) and per-token (batch index, position) of appending lens[r] tokens to
    requests that already hold hist[r] tokens.  Everything by tensor ops."""
    lens_t, hist_t = torch.tensor(lens), torch.tensor(hist)
    pages = (lens_t + hist_t + ps - 1) // ps
    kv_indptr = indptr_of(pages)
    total_pages = int(kv_indptr[-1]) + spare_pages
    perm = torch.randperm(total_pages, generator=torch.Generator().manual_seed(seed))
    kv_indices = perm[: int(kv_indptr[-1])].to(torch.int32)
    batch_indices = torch.repeat_interleave(torch.arange(len(lens)), lens_t)
    starts = indptr_of(lens)[:-1].long()
    positions = torch.arange(int(lens_t.sum())) - starts[batch_indices] + hist_t[batch_indices]
    slot_page = kv_indices[(kv_indptr[batch_indices].long() + positions // ps)].long()
    slot = slot_page * ps + positions % ps  # flat (page, entry) slot every token lands in
    last = ((lens_t + hist_t - 1) % ps + 1).to(torch.int32)
    return dict(kv_indptr=kv_indptr.to(DEV), kv_indices=kv_indices.to(DEV), last=last.to(DEV), total_pages=total_pages,
                batch_indices=batch_indices.to(torch.int32).to(DEV), positions=positions.to(torch.int32).to(DEV),
                slot=slot.to(DEV))


def tol(dtype):
    """The decode output bar.  rtol = atol = 1e-3 (the reference's bar) for fp16 outputs.  A bf16 output cannot carry
    1e-3: its own rounding is half an ulp = 2^-9 relative, so that is added on top for bf16."""
    if dtype == torch.bfloat16:
        return dict(rtol=1e-3 + 2.0 ** -8, atol=2e-3)
    return dict(rtol=1e-3, atol=1e-3)


def ptol(dtype):
    """The prefill output bar.  fp16: rtol = atol = 1e-3 (the reference's bar).  bf16: the same bar plus the rounding
    of the bf16 output itself (half an ulp = 2^-9 relative; 2^-8 granted).  The bf16 kernel runs P.V on the f16 MFMA (P
    rounded to f16, 11 mantissa bits, V converted while staged; bf16_pv_mode = 1 selects hi + lo bf16 halves instead);
    with the reference's single bf16 rounding of P (prefill.cuh:962-985; bf16_pv_mode = 3) 83 of the 383 bf16 cases of
    the 900-seed fuzz sweep exceed even rtol 2^-7 / atol 2e-3, all on cancelling rows (|o| << |v|: the error is
    ~2^-9 sum |p v|; worst 4.6e-3 at seed 637, request 1, row 544, head 16 -- tools/bf16_error_scan.py prints the
    census)."""
    if dtype == torch.bfloat16:
        return dict(rtol=1e-3 + 2.0 ** -8, atol=1e-3)
    return dict(rtol=1e-3, atol=1e-3)


def rope_rt(q_dtype, head_dim):
    """rope_round_dtype for the oracle: decode with fused RoPE runs on the matrix-core kernel for head_dim 64 / 128,
    which rounds the rotated q / k to the 16-bit type (as the reference's tensor-core decode = its prefill kernel
    does, prefill.cuh:465-612); other head dims stay on the VALU kernel, which rotates in f32 (decode.cuh:445-466)."""
    return q_dtype if head_dim in (64, 128) else None


def planned_decode_wrapper(ws_bytes, layout, indptr, indices, last, *plan_args, **plan_kw):
    """BatchDecodeWithPagedKVCacheWrapper on a zeroed workspace of ws_bytes (the planner's chunk choice reads the
    size), planned for the page table (moved to the device) with plan_args / plan_kw as plan() takes them."""
    import flashinfer

    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV), layout)
    w.plan(indptr.to(DEV), indices.to(DEV), last.to(DEV), *plan_args, **plan_kw)
    return w


def planned_prefill_wrapper(ws_bytes, layout, qo_indptr, indptr, indices, last, *plan_args, **plan_kw):
    """BatchPrefillWithPagedKVCacheWrapper, set up like planned_decode_wrapper."""
    import flashinfer

    w = flashinfer.BatchPrefillWithPagedKVCacheWrapper(torch.zeros(ws_bytes, dtype=torch.uint8, device=DEV), layout)
    w.plan(qo_indptr.to(DEV), indptr.to(DEV), indices.to(DEV), last.to(DEV), *plan_args, **plan_kw)
    return w


def owned_slots(kv_lens, indptr, indices, page_size, num_pages):
    """bool [num_pages, page_size]: true where some request holds a token (request b's token t sits in entry
    t % page_size of page indices[indptr[b] + t // page_size]).  Entries of indices past indptr[-1] own nothing."""
    owned = torch.zeros(num_pages, page_size, dtype=torch.bool)
    for b, n in enumerate(kv_lens):
        t = torch.arange(int(n))
        owned[indices[int(indptr[b]) + t // page_size].long(), t % page_size] = True
    return owned


def poison_unowned(cache, layout, owned):
    """A copy of a paged cache ([pages, 2, ...] or a (k, v) tuple of [pages, ...]) whose unowned slots hold 0xFF bytes
    in K and in V: a NaN in f16, bf16, f32, e4m3fn and e5m2.  Written through a uint8 view, owned slots untouched."""
    if isinstance(cache, tuple):
        return tuple(poison_unowned(c.unsqueeze(1), layout, owned).squeeze(1) for c in cache)
    out = cache.clone()
    raw = out.view(torch.uint8)  # [pages, kv, page, H, D * itemsize] (NHD) or [pages, kv, H, page, D * itemsize] (HND)
    if layout == "HND":
        raw = raw.transpose(2, 3)
    raw.transpose(1, 2)[~owned] = 0xFF  # [pages, page, kv, H, bytes]
    return out


def poison_(t):
    """Every byte of t becomes 0xFF, in place (workspaces, padding rows); returns t."""
    t.view(torch.uint8).fill_(0xFF)
    return t
