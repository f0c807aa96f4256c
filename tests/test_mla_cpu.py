"""CPU: the MLA entry points exist in header, library and binding; fi_batch_mla_plan rejects what the kernel does
not cover; its work list covers every (request, row) once and tiles every kv range; the Python API has the
reference's signatures.  Plans run on the host only (int_ws = NULL); no kernel is launched."""
import ctypes as C
import inspect
import os
import random
import re

import numpy as np
import pytest

from attn_inputs import indptr_of
from plan_calls import BF16, F16, mla_plan as plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fi_mi355.h")
MLA_SYMBOLS = ["fi_batch_mla_plan", "fi_batch_mla_run", "fi_append_paged_mla_kv_cache"]
ROWS_PER_ITEM = 16


def test_mla_symbols_everywhere(fi_lib):
    from flashinfer import _lib

    declared = set(re.findall(r"FI_API\s+[\w\s\*]+?\b(fi_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for s in MLA_SYMBOLS:
        assert s in declared and s in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, s), s
    assert fi_lib.fi_abi_version() == 2


def test_plan_rejects_unsupported(fi_lib):
    cases = [
        (dict(ckv=256), b"head_dim_ckv"),
        (dict(kpe=128), b"head_dim_kpe"),
        (dict(q_dt=F16, kv_dt=BF16), b"dtype"),
        (dict(int_bytes=256), b"workspace too small"),
    ]
    for kw, msg in cases:
        rc, _, _ = plan(fi_lib, [1, 1], [100, 2000], 16, **kw)
        assert rc != 0, kw
        assert msg in fi_lib.fi_last_error(), (kw, fi_lib.fi_last_error())
    rc, _, _ = plan(fi_lib, [1, 1], [100, 2000], 16)
    assert rc == 0, fi_lib.fi_last_error()


def decode_plan(info, pinned, qo_lens, H):
    from flashinfer import _lib

    buf = np.frombuffer(pinned, dtype=np.int32)
    total_rows = info[_lib.FI_MLA_TOTAL_ROWS]
    assert total_rows == sum(qo_lens) * H
    o = info[_lib.FI_MLA_MERGE_INDPTR_OFFSET] // 4
    indptr = buf[o:o + total_rows + 1]
    n = info[_lib.FI_MLA_NUM_WORK]
    i = info[_lib.FI_MLA_ITEMS_OFFSET] // 4
    items = buf[i:i + 8 * n].reshape(n, 8)
    return indptr, items


@pytest.mark.parametrize("graph", [0, 1])
def test_plan_invariants_sweep(fi_lib, graph):
    from flashinfer import _lib

    rng = random.Random(1234 + graph)
    for trial in range(60):
        B = rng.choice([1, 2, 3, 7, 17, 64])
        H = rng.choice([16, 64, 128])
        qo_lens = [rng.choice([1, 1, 2, 4, 17]) for _ in range(B)]
        kv_lens = [rng.choice([0, 1, 17, 514, 2743, 8736, 32768]) for _ in range(B)]
        float_bytes = rng.choice([128 << 20, 4 << 20])
        rc, info, pinned = plan(fi_lib, qo_lens, kv_lens, H, page_size=rng.choice([1, 16, 64]),
                                float_bytes=float_bytes, graph=graph)
        assert rc == 0, fi_lib.fi_last_error()
        assert info[_lib.FI_MLA_MAGIC] == 0x46494D4C41
        indptr, items = decode_plan(info, pinned, qo_lens, H)
        chunk = info[_lib.FI_MLA_KV_CHUNK_SIZE]
        assert chunk > 0 and chunk % 64 == 0
        qo_starts = indptr_of(qo_lens).numpy()
        # every (request, packed row, kv token) exactly once
        cover = {}
        for qo_start, row0, qo_len, k0, k1, kv_len, page_base, ch in items.tolist():
            b = int(np.searchsorted(qo_starts, qo_start, side="right") - 1)
            while qo_lens[b] == 0 or qo_starts[b] != qo_start:
                b += 1
            assert qo_len == qo_lens[b] and kv_len == kv_lens[b]
            assert 0 <= k0 <= k1 <= kv_len and (k1 - k0) <= chunk
            assert row0 % ROWS_PER_ITEM == 0 and row0 < qo_len * H
            for r in range(row0, min(row0 + ROWS_PER_ITEM, qo_len * H)):
                cover.setdefault((b, r), []).append((k0, k1, ch))
        n_entries = 0
        for b in range(B):
            for r in range(qo_lens[b] * H):
                spans = sorted(cover.pop((b, r)))
                # the chunks tile [0, kv_len): no gap, no overlap
                assert spans[0][0] == 0 and spans[-1][1] == kv_lens[b]
                for (a0, a1, _), (b0, _, _) in zip(spans, spans[1:]):
                    assert a1 == b0 and a1 > a0
                g = qo_starts[b] * H + r
                n = indptr[g + 1] - indptr[g]
                if len(spans) == 1:
                    assert spans[0][2] == -1 and n == 0
                else:
                    assert sorted(s[2] for s in spans) == list(range(len(spans))) and n == len(spans)
                n_entries += n
        assert not cover
        # partial states stay inside the float workspace
        assert indptr[-1] == n_entries == info[_lib.FI_MLA_NUM_ENTRIES]
        v_off = info[_lib.FI_MLA_V_OFFSET]
        assert n_entries * 4 <= v_off and v_off + n_entries * 512 * 4 <= float_bytes


def test_graph_plan_grid_is_fixed(fi_lib):
    from flashinfer import _lib

    grids, chunks = set(), set()
    for kv in ([100, 3000, 17, 800], [40000, 40000, 40000, 40000], [200000, 1, 1, 2]):
        rc, info, _ = plan(fi_lib, [1] * 4, kv, 16, graph=1)
        assert rc == 0
        grids.add(info[_lib.FI_MLA_GRID])
        chunks.add(info[_lib.FI_MLA_KV_CHUNK_SIZE])
    assert len(grids) == 1 and len(chunks) == 3


def test_python_api_signatures():
    import flashinfer
    from flashinfer.mla import BatchMLAPagedAttentionWrapper

    assert flashinfer.BatchMLAPagedAttentionWrapper is BatchMLAPagedAttentionWrapper
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(BatchMLAPagedAttentionWrapper.__init__) == [
        "self", "float_workspace_buffer", "use_cuda_graph", "qo_indptr", "kv_indptr", "kv_indices", "kv_len_arr",
        "backend"]
    assert names(BatchMLAPagedAttentionWrapper.plan) == [
        "self", "qo_indptr", "kv_indptr", "kv_indices", "kv_len_arr", "num_heads", "head_dim_ckv", "head_dim_kpe",
        "page_size", "causal", "sm_scale", "q_data_type", "kv_data_type", "use_profiler"]
    assert names(BatchMLAPagedAttentionWrapper.run) == [
        "self", "q_nope", "q_pe", "ckv_cache", "kpe_cache", "out", "lse", "return_lse", "profiler_buffer", "kv_len",
        "page_table"]
    assert names(flashinfer.append_paged_mla_kv_cache) == [
        "append_ckv", "append_kpe", "batch_indices", "positions", "ckv_cache", "kpe_cache", "kv_indices",
        "kv_indptr", "kv_last_page_len"]


def test_cutlass_backend_is_refused():
    import torch

    from flashinfer.mla import BatchMLAPagedAttentionWrapper

    with pytest.raises(ValueError, match="cutlass"):
        BatchMLAPagedAttentionWrapper(torch.empty(16, dtype=torch.uint8), backend="cutlass")


def test_run_rejects_rows_other_than_planned(fi_lib):
    """run() refuses q tensors whose packed row count differs from the plan's (the error is raised on the host,
    before any launch, so the placeholder pointers below are never dereferenced)."""
    from flashinfer import _lib

    rc, info, _ = plan(fi_lib, [1, 2], [100, 2000], 16)
    assert rc == 0
    plan_info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)(*info)
    fake = 1 << 20  # 16-byte aligned, non-null
    for rows in (3 * 16 - 16, 3 * 16 + 16):
        p = _lib.fi_batch_mla_params_t(q_nope=fake, q_nope_stride_n=16 * 512, q_nope_stride_h=512, q_pe=fake, q_pe_stride_n=16 * 64,
                           q_pe_stride_h=64, ckv=fake, ckv_stride_page=16 * 512, ckv_stride_n=512, kpe=fake,
                           kpe_stride_page=16 * 64, kpe_stride_n=64, kv_indices=fake, o=fake, lse=None, float_ws=fake,
                           float_ws_bytes=128 << 20, int_ws=fake, int_ws_bytes=8 << 20, num_rows=rows, num_heads=16,
                           page_size=16, dtype=BF16, causal=0, sm_scale=0.1)
        rc = fi_lib.fi_batch_mla_run(plan_info, _lib.FI_MLA_PLAN_INFO_LEN, C.byref(p), None)
        assert rc != 0 and b"packed rows" in fi_lib.fi_last_error()
