"""What the two test files of the plan-free MLA call (test_mla_device_plan_cpu.py, test_mla_device_plan_gpu.py) share:
the params of fi_batch_mla_plan_device, the host planner's int workspace read back field by field, and a poisoned
paged 576-wide cache with its dense block table and its oracle output.

Plain functions, no fixtures."""
import ctypes as C

import numpy as np
import torch

from attn_inputs import indptr_of, owned_slots
from flashinfer import _lib

CKV, KPE = 512, 64
ITEM_FIELDS = ("qo_start", "row0", "qo_len", "kv_start", "kv_end", "kv_len", "page_base", "chunk")
HEADER_BYTES = 64  # the int workspace: header, merge indptr [rows + 1], items (csrc/mla_plan.h)


def plan_params(B=3, max_blocks=8, ps=16, H=16, q_len=1, hint=0, stride=None, **over):
    kw = dict(block_tables=None, seq_lens=None, block_tables_stride=stride or max_blocks, int_ws=None, int_ws_bytes=0,
              float_ws=None, float_ws_bytes=0, batch_size=B, max_blocks=max_blocks, page_size=ps, num_heads=H,
              q_len_per_request=q_len, head_dim_ckv=CKV, head_dim_kpe=KPE, q_dtype=_lib.FI_DTYPE_BF16,
              kv_dtype=_lib.FI_DTYPE_BF16, max_items_hint=hint)
    kw.update(over)
    return _lib.fi_batch_mla_plan_device_params_t(**kw)


def workspace_sizes(fi_lib, p):
    ib, fb = C.c_size_t(), C.c_size_t()
    assert fi_lib.fi_batch_mla_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)) == 0, fi_lib.fi_last_error()
    return ib.value, fb.value


def read_plan(raw, rows):
    """(header slots [4], merge indptr [rows + 1], items as dicts) of an MLA int workspace given as a uint8 array."""
    i32 = np.frombuffer(raw, dtype=np.int32)
    header = i32[:4].tolist()
    indptr = i32[HEADER_BYTES // 4: HEADER_BYTES // 4 + rows + 1].tolist()
    off, n = header[2] // 4, header[1]
    items = [dict(zip(ITEM_FIELDS, i32[off + 8 * w: off + 8 * w + 8].tolist())) for w in range(n)]
    return header, indptr, items


def host_plan(fi_lib, kv_lens, q_len, H, ps, float_bytes, int_bytes=8 << 20):
    """fi_batch_mla_plan in host-only mode with enable_cuda_graph = 1 for q_len query tokens in every request."""
    B = len(kv_lens)
    qo_indptr = (C.c_int32 * (B + 1))(*range(0, (B + 1) * q_len, q_len))
    kv_indptr = (C.c_int32 * (B + 1))(*indptr_of(-(-k // ps) for k in kv_lens).tolist())
    kv_len = (C.c_int32 * B)(*kv_lens)
    pinned = (C.c_char * int_bytes)()
    p = _lib.fi_batch_mla_plan_params_t(
        int_ws=None, pinned_int_ws=C.addressof(pinned), int_ws_bytes=int_bytes, float_ws_bytes=float_bytes,
        qo_indptr_h=C.addressof(qo_indptr), kv_indptr_h=C.addressof(kv_indptr), kv_len_arr_h=C.addressof(kv_len),
        batch_size=B, num_heads=H, head_dim_ckv=CKV, head_dim_kpe=KPE, page_size=ps, causal=1,
        q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16, enable_cuda_graph=1, fixed_split_size=0)
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()
    assert fi_lib.fi_batch_mla_plan(C.byref(p), info, None) == 0, fi_lib.fi_last_error()
    return list(info), read_plan(bytes(pinned), B * q_len * H)


def make_case(kv_lens, q_len, H, ps, dtype, seed, max_blocks=None, spare_pages=2):
    """A paged [pages, ps, 576] cache for requests of kv_lens tokens, q [B, q_len, H, 576], and the dense block table.
    Every cache slot no request owns holds 0xFF bytes (a NaN in f16 and bf16); block-table entries past a request's
    pages point at a spare page filled the same way, never out of range.  All on the CPU."""
    g = torch.Generator().manual_seed(seed)
    B = len(kv_lens)
    pages = [-(-l // ps) for l in kv_lens]
    indptr = indptr_of(pages)
    total = int(indptr[-1])
    num_pages = total + spare_pages
    perm = torch.randperm(num_pages, generator=g)
    indices, spare = perm[:total].to(torch.int32), int(perm[total])
    cache = (torch.randn(num_pages, ps, CKV + KPE, generator=g) * 0.5).to(dtype)
    owned = owned_slots(kv_lens, indptr, indices, ps, num_pages)
    cache.view(torch.int16)[~owned] = -1
    q = torch.randn(B, q_len, H, CKV + KPE, generator=g).to(dtype)
    max_blocks = max_blocks or max(max(pages), 1)
    table = torch.full((B, max_blocks), spare, dtype=torch.int32)
    for b in range(B):
        table[b, : pages[b]] = indices[int(indptr[b]): int(indptr[b + 1])]
    return dict(kv_lens=list(kv_lens), q_len=q_len, H=H, ps=ps, dtype=dtype, q=q, cache=cache, table=table,
                indptr=indptr, indices=indices, max_blocks=max_blocks,
                lens=torch.tensor(kv_lens, dtype=torch.int32))


def oracle_out(c, sm_scale):
    """[B, q_len, H, 512] f32 from oracle.attention_ref, one KV head of 576 QK dims and 512 VO dims, causal with the
    query rows aligned to the end of the keys; a row that sees no key is zeros."""
    from oracle.attention_ref import attention_ref

    outs = []
    for b, kl in enumerate(c["kv_lens"]):
        pidx = c["indices"][int(c["indptr"][b]): int(c["indptr"][b + 1])].long()
        kv = c["cache"][pidx].reshape(-1, CKV + KPE)[:kl]
        o, _ = attention_ref(c["q"][b], kv[:, None], kv[:, None, :CKV], True, sm_scale)
        outs.append(o.float())
    return torch.stack(outs)

