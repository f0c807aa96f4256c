"""The host planners called through the C ABI in host-only mode (int_ws = NULL: no kernel is launched), with the work
lists read back from the pinned buffer.  Shared by the CPU planner tests."""
import ctypes as C

import numpy as np

from attn_inputs import indptr_of
from flashinfer import _lib

F16, BF16 = 0, 1  # fi_dtype codes


def run_plan(fi_lib, indptr, hq, hkv, page_size, max_grid, cuda_graph=False, head_dim=128,
             float_bytes=1 << 30, window_left=-1):
    n = len(indptr) - 1
    pinned = (C.c_char * (8 << 20))()
    arr = (C.c_int32 * len(indptr))(*indptr)
    info = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)()
    rc = fi_lib.fi_batch_decode_plan(None, float_bytes, None, pinned, len(pinned), arr, n, hq, hkv,
                                     page_size, int(cuda_graph), head_dim, 1, 1, max_grid, window_left, info, None)
    assert rc == 0, fi_lib.fi_last_error()
    info = list(info)
    raw = np.frombuffer(pinned, dtype=np.uint8)

    def i32(off, count):
        return raw[off: off + 4 * count].view(np.int32).tolist()

    padded, nwork = info[_lib.FI_DP_PADDED_BATCH_SIZE], info[_lib.FI_DP_NUM_WORK]
    out = dict(split_kv=bool(info[_lib.FI_DP_SPLIT_KV]), kv_chunk_size=info[_lib.FI_DP_KV_CHUNK_SIZE],
               padded_batch_size=padded, num_work=nwork,
               request_indices=i32(info[_lib.FI_DP_REQUEST_INDICES_OFFSET], nwork),
               kv_tile_indices=i32(info[_lib.FI_DP_KV_TILE_INDICES_OFFSET], nwork),
               o_indptr=i32(info[_lib.FI_DP_O_INDPTR_OFFSET], n + 1),
               chunk_ptr=i32(info[_lib.FI_DP_KV_CHUNK_SIZE_PTR_OFFSET], 1)[0], info=info)
    if out["split_kv"]:
        mask_off = info[_lib.FI_DP_BLOCK_VALID_MASK_OFFSET]
        out["mask"] = raw[mask_off: mask_off + padded].tolist()
    return out


def run_prefill_plan(fi_lib, qo_indptr, kv_lens, hq, hkv, causal=False, cuda_graph=False, fixed=-1, disable=False,
                     page_size=16, float_bytes=1 << 32, window_left=-1):
    n = len(kv_lens)
    pinned = (C.c_char * (8 << 20))()
    qo = (C.c_int32 * (n + 1))(*qo_indptr)
    kvp = [0]
    for k in kv_lens:
        kvp.append(kvp[-1] + -(-k // page_size))
    kvi = (C.c_int32 * (n + 1))(*kvp)
    kvl = (C.c_int32 * max(n, 1))(*kv_lens)
    info = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)()
    rc = fi_lib.fi_batch_prefill_plan(None, float_bytes, None, pinned, len(pinned), qo, kvi, kvl, qo_indptr[-1], n,
                                      hq, hkv, page_size, int(cuda_graph), 128, 128, int(causal), window_left, fixed,
                                      int(disable), info, None)
    assert rc == 0, fi_lib.fi_last_error()
    info = list(info)
    raw = np.frombuffer(pinned, dtype=np.uint8)

    def i32(off, count):
        return raw[off: off + 4 * count].view(np.int32).tolist()

    nwork = info[_lib.FI_PP_NUM_WORK]
    padded = info[_lib.FI_PP_PADDED_BATCH_SIZE]
    out = dict(split_kv=bool(info[_lib.FI_PP_SPLIT_KV]), kv_chunk_size=info[_lib.FI_PP_KV_CHUNK_SIZE],
               padded_batch_size=padded, num_work=nwork,
               request_indices=i32(info[_lib.FI_PP_REQUEST_INDICES_OFFSET], nwork),
               qo_tile_indices=i32(info[_lib.FI_PP_QO_TILE_INDICES_OFFSET], nwork),
               kv_tile_indices=i32(info[_lib.FI_PP_KV_TILE_INDICES_OFFSET], nwork),
               padding=i32(info[_lib.FI_PP_REQUEST_INDICES_OFFSET], padded)[nwork:])
    out["merge_indptr"] = [0]
    if out["split_kv"]:
        out["merge_indptr"] = i32(info[_lib.FI_PP_MERGE_INDPTR_OFFSET], info[_lib.FI_PP_TOTAL_NUM_ROWS] + 1)
    return out


def prefill_qkvo_plan(fi_lib, qo_lens, kv_lens, hq, hkv, dqk, dvo, causal=True, float_bytes=1 << 30, graph=False,
         fixed_split=-1, disable_split=False, window_left=-1, page_size=1):
    """fi_batch_prefill_plan on the host: (rc, plan_info, request / q tile / kv tile / merge_indptr lists)."""
    n = len(qo_lens)
    qo = indptr_of(qo_lens).numpy()
    kvp = indptr_of(-(-k // page_size) for k in kv_lens).numpy()
    kl = np.array(kv_lens, dtype=np.int32)
    pinned = (C.c_char * (8 << 20))()
    info = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)()
    rc = fi_lib.fi_batch_prefill_plan(None, float_bytes, None, pinned, len(pinned), qo.ctypes.data, kvp.ctypes.data,
                                      kl.ctypes.data, int(qo[-1]), n, hq, hkv, page_size, int(graph), dqk, dvo,
                                      int(causal), window_left, fixed_split, int(disable_split), info, None)
    if rc != 0:
        return rc, None, None
    info = list(info)
    raw = np.frombuffer(pinned, dtype=np.uint8)

    def i32(off, count):
        return raw[off: off + 4 * count].view(np.int32).tolist()

    padded, rows = info[_lib.FI_PP_PADDED_BATCH_SIZE], info[_lib.FI_PP_TOTAL_NUM_ROWS]
    lists = dict(req=i32(info[_lib.FI_PP_REQUEST_INDICES_OFFSET], padded),
                 tile=i32(info[_lib.FI_PP_QO_TILE_INDICES_OFFSET], padded),
                 kvt=i32(info[_lib.FI_PP_KV_TILE_INDICES_OFFSET], padded),
                 merge=i32(info[_lib.FI_PP_MERGE_INDPTR_OFFSET], rows + 1) if info[_lib.FI_PP_SPLIT_KV] else [],
                 chunk=i32(info[_lib.FI_PP_KV_CHUNK_SIZE_PTR_OFFSET], 1))
    return rc, info, lists


def mla_plan(fi_lib, qo_lens, kv_lens, H, page_size=16, ckv=512, kpe=64, q_dt=BF16, kv_dt=BF16, int_bytes=8 << 20,
         float_bytes=128 << 20, graph=0, fixed_split=0):
    B = len(qo_lens)
    qo_indptr = (C.c_int32 * (B + 1))(*indptr_of(qo_lens).tolist())
    pages = [-(-k // page_size) for k in kv_lens]
    kv_indptr = (C.c_int32 * (B + 1))(*indptr_of(pages).tolist())
    kv_len = (C.c_int32 * max(B, 1))(*kv_lens)
    pinned = (C.c_char * int_bytes)()
    p = _lib.fi_batch_mla_plan_params_t(int_ws=None, pinned_int_ws=C.addressof(pinned), int_ws_bytes=int_bytes,
                           float_ws_bytes=float_bytes, qo_indptr_h=C.addressof(qo_indptr),
                           kv_indptr_h=C.addressof(kv_indptr), kv_len_arr_h=C.addressof(kv_len), batch_size=B,
                           num_heads=H, head_dim_ckv=ckv, head_dim_kpe=kpe, page_size=page_size, causal=0,
                           q_dtype=q_dt, kv_dtype=kv_dt, enable_cuda_graph=graph, fixed_split_size=fixed_split)
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()
    rc = fi_lib.fi_batch_mla_plan(C.byref(p), info, None)
    return rc, list(info), pinned
