"""Oracle of the block-sparse attention tests: float64 on the CPU, written as loops over block rows.

Two statements of BSR attention (gathered: the KV rows of a block row in the order of ``indices``; dense: the
``[M, N]`` boolean mask), the variable-block form, plain restatements of the index expansions, and the pattern
builder the tests share.  Every logsumexp is base 2; a row that sees no key gives ``o = 0``, ``lse = -5e4``."""
import math

import torch

NEG_INF_LSE = -5.0e4  # FI_NEG_INF, include/fi_mi355.h


def masked_attention(q, k, v, allowed, sm_scale=None):
    """q [qo, Hq, D], k / v [kv, Hkv, D], allowed [qo, kv] bool -> (o [qo, Hq, D], lse [qo, Hq]), float64."""
    q, k, v = q.double(), k.double(), v.double()
    group = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(group, 1), v.repeat_interleave(group, 1)
    scale = 1.0 / math.sqrt(q.shape[-1]) if sm_scale is None else sm_scale
    s = torch.einsum("qhd,khd->qhk", q, k) * scale
    s = s.masked_fill(~allowed[:, None, :], float("-inf"))
    seen = allowed.any(1)
    lse = torch.full(s.shape[:2], NEG_INF_LSE, dtype=torch.float64)
    o = torch.zeros(q.shape[0], q.shape[1], v.shape[-1], dtype=torch.float64)
    if bool(seen.any()):
        lse[seen] = torch.logsumexp(s[seen], -1) * math.log2(math.e)
        o[seen] = torch.einsum("qhk,khd->qhd", torch.softmax(s[seen], -1), v)
    return o, lse


def causal_allowed(qo_len, kv_len):
    """The kernels' causal rule: row i of qo_len sees gathered positions <= kv_len - qo_len + i."""
    return torch.arange(kv_len)[None, :] <= (kv_len - qo_len + torch.arange(qo_len))[:, None]


def bsr_attention_gathered(q, k, v, indptr, indices, R, C, block_mask=None, causal=False, sm_scale=None):
    """Per block row: gather its KV rows in the order of ``indices``; ``block_mask`` (nnz, R, C) or the causal rule."""
    M = q.shape[0]
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.zeros(q.shape[:2], dtype=torch.float64)
    for i in range(len(indptr) - 1):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        r0, r1 = i * R, min((i + 1) * R, M)
        tokens = (indices[lo:hi].long()[:, None] * C + torch.arange(C)[None, :]).reshape(-1)
        if block_mask is not None:
            allowed = torch.cat([block_mask[b] for b in range(lo, hi)] + [torch.zeros(R, 0, dtype=torch.bool)], 1)
            allowed = allowed[: r1 - r0].bool()
        elif causal:
            allowed = causal_allowed(r1 - r0, len(tokens))
        else:
            allowed = torch.ones(r1 - r0, len(tokens), dtype=torch.bool)
        o[r0:r1], lse[r0:r1] = masked_attention(q[r0:r1], k[tokens], v[tokens], allowed, sm_scale)
    return o, lse


def bsr_dense_mask(indptr, indices, M, N, R, C):
    """The [M, N] boolean mask of a BSR pattern with full blocks."""
    mask = torch.zeros(M, N, dtype=torch.bool)
    for i in range(len(indptr) - 1):
        for j in indices[int(indptr[i]):int(indptr[i + 1])].tolist():
            mask[i * R:(i + 1) * R, j * C:(j + 1) * C] = True
    return mask


def bsr_attention_dense(q, k, v, indptr, indices, R, C, sm_scale=None):
    return masked_attention(q, k, v, bsr_dense_mask(indptr, indices, q.shape[0], k.shape[0], R, C), sm_scale)


def variable_block_attention(q, k, v, block_mask_map, block_row_sz, block_col_sz, causal=False, sm_scale=None):
    """q [Hq, qo_len, D], k / v [Hkv, kv_len, D]; block row i of kv head h sees the column blocks block_mask_map[h, i]
    selects, in increasing order -> (o [Hq, qo_len, D], lse [Hq, qo_len])."""
    Hq, Hkv = q.shape[0], k.shape[0]
    group = Hq // Hkv
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.zeros(q.shape[:2], dtype=torch.float64)
    for h in range(Hkv):
        row_start = [0, *torch.cumsum(block_row_sz[h], 0).tolist()]
        col_start = [0, *torch.cumsum(block_col_sz[h], 0).tolist()]
        heads = slice(h * group, (h + 1) * group)
        for i in range(block_mask_map.shape[1]):
            tokens = [t for c in range(block_mask_map.shape[2]) if block_mask_map[h, i, c]
                      for t in range(col_start[c], col_start[c + 1])]
            tokens = torch.tensor(tokens, dtype=torch.long)
            r0, r1 = row_start[i], row_start[i + 1]
            allowed = causal_allowed(r1 - r0, len(tokens)) if causal else torch.ones(r1 - r0, len(tokens),
                                                                                      dtype=torch.bool)
            oi, li = masked_attention(q[heads, r0:r1].transpose(0, 1), k[h, tokens][:, None], v[h, tokens][:, None],
                                      allowed, sm_scale)
            o[heads, r0:r1], lse[heads, r0:r1] = oi.transpose(0, 1), li.transpose(0, 1)
    return o, lse


def expand_block_mask(block_mask_map, block_col_sz, granule):
    """(row_pages [H * MB], kv_indptr [H * MB + 1], kv_indices) of a block map over pages of ``granule`` tokens: head h
    owns tokens [h * kv_len, (h + 1) * kv_len); a selected block emits its pages in order."""
    H, MB, NB = block_mask_map.shape
    kv_len = int(block_col_sz[0].sum())
    row_pages, indices = [], []
    for h in range(H):
        start = [h * kv_len]
        for c in range(NB):
            start.append(start[-1] + int(block_col_sz[h, c]))
        for i in range(MB):
            before = len(indices)
            for c in range(NB):
                if block_mask_map[h, i, c]:
                    indices.extend(range(start[c] // granule, start[c + 1] // granule))
            row_pages.append(len(indices) - before)
    indptr = [0]
    for n in row_pages:
        indptr.append(indptr[-1] + n)
    as_i32 = lambda x: torch.tensor(x, dtype=torch.int32)
    return as_i32(row_pages), as_i32(indptr), as_i32(indices)


def bsr_mask_layout(mask, indptr):
    """(nnz, R, C) block masks -> the flattened layout: per block row, its blocks side by side as one row-major
    [R, blocks * C] matrix."""
    parts = []
    for i in range(len(indptr) - 1):
        blocks = [mask[b] for b in range(int(indptr[i]), int(indptr[i + 1]))]
        if blocks:
            parts.append(torch.cat(blocks, 1).reshape(-1))
    return torch.cat(parts) if parts else mask.reshape(-1)


def vector_sparse_offsets(indices, block_indptr, vector_indptr, kv_lens, stride_block, stride_n, block_size, out_len):
    """Restatement of block_sparse_indices_to_vector_sparse_offsets; entries no request writes stay -1."""
    out = torch.full((out_len,), -1, dtype=torch.int32)
    for b in range(len(block_indptr) - 1):
        for pos in range(int(kv_lens[b])):
            block = int(indices[int(block_indptr[b]) + pos // block_size])
            out[int(vector_indptr[b]) + pos] = block * stride_block + (pos % block_size) * stride_n
    return out


def bsr_pattern(MB, NB, seed):
    """(indptr, indices, block map [MB, NB]): density 0.5, block row 1 empty, block row 2 full, every row's indices
    in a random order."""
    g = torch.Generator().manual_seed(seed)
    block_map = torch.rand(MB, NB, generator=g) < 0.5
    block_map[1] = False
    block_map[2] = True
    rows = []
    for i in range(MB):
        cols = torch.nonzero(block_map[i]).flatten()
        rows.append(cols[torch.randperm(len(cols), generator=g)])
    indptr = torch.tensor([0, *torch.cumsum(torch.tensor([len(r) for r in rows]), 0).tolist()], dtype=torch.int32)
    return indptr, torch.cat(rows).to(torch.int32), block_map
