"""MLA with an fp8 cache, without a GPU: the signature of flashinfer.rope.mla_rope_quantize_fp8, what the Python entries
accept and refuse before they reach the library, what the C entries refuse before any launch, and the numpy fp8
rounding the GPU tests compare against."""
import contextlib
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from flashinfer import _lib
from flashinfer import decode as D
from flashinfer import rope
from flashinfer.mla import BatchMLAPagedAttentionWrapper
from mla_fp8_ref import fp8_order, fp8_round, make_fp8_case, rope_quantize_ref
from mla_plan_free_inputs import host_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
EMPTY = inspect.Parameter.empty

# ref flashinfer/rope.py:1154-1169: names, order, defaults
REFERENCE_PARAMETERS = [
    ("q_rope", EMPTY), ("k_rope", EMPTY), ("q_nope", EMPTY), ("k_nope", EMPTY), ("cos_sin_cache", EMPTY),
    ("pos_ids", EMPTY), ("is_neox", True), ("quantize_dtype", None), ("quant_scale_q", 1.0), ("quant_scale_kv", 1.0),
    ("q_rope_out", None), ("k_rope_out", None), ("q_nope_out", None), ("k_nope_out", None),
]


def test_signature_is_the_reference_s():
    params = inspect.signature(rope.mla_rope_quantize_fp8).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_PARAMETERS
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_it_lives_in_flashinfer_rope_only():
    import flashinfer

    assert not hasattr(flashinfer, "mla_rope_quantize_fp8")


class _Reached(Exception):
    """Carries the params struct the library would have been given."""


def _capture_library(monkeypatch):
    """No GPU check, and a library whose every entry raises _Reached with its arguments."""
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    class Lib:
        def __getattr__(self, name):
            def entry(*args):
                raise _Reached(name, args)
            return entry

    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "current_stream", lambda device: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def _rope_args(nnz=3, H=2, dtype=torch.float16, **over):
    args = dict(q_rope=torch.zeros(nnz, H, 64, dtype=dtype), k_rope=torch.zeros(nnz, 64, dtype=dtype),
                q_nope=torch.zeros(nnz, H, 512, dtype=dtype), k_nope=torch.zeros(nnz, 512, dtype=dtype),
                cos_sin_cache=torch.zeros(16, 64), pos_ids=torch.zeros(nnz, dtype=torch.int32))
    args.update(over)
    return args


def test_cos_sin_cache_must_be_float32(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="cos_sin_cache should be float32"):
        rope.mla_rope_quantize_fp8(**_rope_args(cos_sin_cache=torch.zeros(16, 64, dtype=torch.float16)))


@pytest.mark.parametrize("given,want", [(None, E4M3), ("k_nope_out", E5M2), ("q_rope_out", E4M3)])
def test_quantize_dtype_is_inferred_from_the_first_output_given(monkeypatch, given, want):
    _capture_library(monkeypatch)
    args = _rope_args()
    if given:
        args[given] = torch.zeros_like(args[given[:-4]], dtype=want)
    with pytest.raises(_Reached) as e:
        rope.mla_rope_quantize_fp8(**args)
    name, (params_ref, _stream) = e.value.args
    assert name == "fi_mla_rope_quantize"
    p = params_ref._obj
    assert p.out_dtype == _lib.fi_dtype(want) and p.dtype == _lib.FI_DTYPE_F16
    assert (p.nnz, p.num_heads, p.rope_dim, p.nope_dim, p.interleave, p.pos_ids_int64) == (3, 2, 64, 512, 0, 0)
    assert (p.q_nope_stride_n, p.q_nope_stride_h, p.k_rope_stride_n) == (1024, 512, 64)


def test_an_explicit_quantize_dtype_and_int64_positions_reach_the_library(monkeypatch):
    _capture_library(monkeypatch)
    with pytest.raises(_Reached) as e:
        rope.mla_rope_quantize_fp8(**_rope_args(pos_ids=torch.zeros(3, dtype=torch.int64), is_neox=False,
                                                quantize_dtype=E5M2, quant_scale_q=0.5, quant_scale_kv=2.0))
    p = e.value.args[1][0]._obj
    assert (p.out_dtype, p.pos_ids_int64, p.interleave) == (_lib.FI_DTYPE_FP8_E5M2, 1, 1)
    assert (p.quant_scale_q, p.quant_scale_kv) == (0.5, 2.0)


def test_bad_rope_quantize_arguments_are_value_errors(monkeypatch):
    _no_library(monkeypatch)
    for over in (dict(quantize_dtype=torch.float16), dict(k_rope=torch.zeros(3, 64, dtype=torch.bfloat16)),
                 dict(k_nope=torch.zeros(4, 512, dtype=torch.float16)), dict(pos_ids=torch.zeros(3)),
                 dict(q_nope_out=torch.zeros(3, 2, 512, dtype=E4M3), k_nope_out=torch.zeros(3, 512, dtype=E5M2)),
                 dict(q_rope=torch.zeros(3, 2, 128, dtype=torch.float16)[..., ::2])):
        with pytest.raises(ValueError):
            rope.mla_rope_quantize_fp8(**_rope_args(**over))


# ---- trtllm_batch_decode_with_kv_cache_mla ----

def _mla_args(B=3, q_len=2, H=16, ps=16, max_blocks=8, pages=12, dtype=E4M3, **over):
    args = dict(query=torch.zeros(B, q_len, H, 576).to(dtype), kv_cache=torch.zeros(pages, 1, ps, 576).to(dtype),
                workspace_buffer=torch.zeros(1 << 20, dtype=torch.uint8), qk_nope_head_dim=128, kv_lora_rank=512,
                qk_rope_head_dim=64, block_tables=torch.zeros(B, max_blocks, dtype=torch.int32),
                seq_lens=torch.ones(B, dtype=torch.int32), max_seq_len=max_blocks * ps)
    args.update(over)
    return args


def test_an_fp8_pair_reaches_the_library(monkeypatch):
    """e4m3 query and cache, with or without both tensor scales, a given bf16 out, views of wider tensors."""
    _no_library(monkeypatch)
    t = torch.ones(1)
    wide_q = torch.zeros(3, 2, 16, 640).to(E4M3)[..., :576]
    wide_kv = torch.zeros(12, 16, 640).to(E4M3)[..., :576]
    for over in (dict(), dict(bmm1_scale=0.1, bmm2_scale=0.5), dict(bmm1_scale_log2_tensor=t, bmm2_scale_tensor=t),
                 dict(out=torch.zeros(3, 2, 16, 512, dtype=torch.bfloat16)), dict(query=wide_q), dict(kv_cache=wide_kv)):
        with pytest.raises(AssertionError, match="the library was reached"):
            D.trtllm_batch_decode_with_kv_cache_mla(**_mla_args(**over))


def test_an_fp8_pair_computes_and_writes_bf16(monkeypatch):
    _capture_library(monkeypatch)
    with pytest.raises(_Reached) as e:
        D.trtllm_batch_decode_with_kv_cache_mla(**_mla_args())
    name, (plan_ref, _sizes, _more) = e.value.args[0], e.value.args[1][:3]
    assert name == "fi_batch_mla_plan_device_workspace"
    # the planner is handed the compute dtype for both fields: its fp8 refusal stays as it is
    assert (plan_ref._obj.q_dtype, plan_ref._obj.kv_dtype) == (_lib.FI_DTYPE_BF16, _lib.FI_DTYPE_BF16)
    _no_library(monkeypatch)
    for bad_out in (torch.zeros(3, 2, 16, 512, dtype=torch.float16), torch.zeros(3, 2, 16, 512).to(E4M3)):
        with pytest.raises(ValueError, match="out"):
            D.trtllm_batch_decode_with_kv_cache_mla(**_mla_args(out=bad_out))


F16_Q, F16_KV = torch.zeros(3, 2, 16, 576, dtype=torch.float16), torch.zeros(12, 16, 576, dtype=torch.float16)
REFUSALS = [
    ("fp8 query", dict(kv_cache=F16_KV)),
    ("fp8 query or kv_cache", dict(query=F16_Q)),
    ("mixed", dict(query=F16_Q.bfloat16())),
    ("e5m2", dict(dtype=E5M2)),
    ("fp8 query or kv_cache", dict(dtype=E5M2)),
    ("e5m2", dict(kv_cache=torch.zeros(12, 16, 576).to(E5M2))),
    ("bmm1_scale_log2_tensor alone", dict(bmm1_scale_log2_tensor=torch.ones(1))),
    ("bmm2_scale_tensor alone", dict(bmm2_scale_tensor=torch.ones(1))),
    ("bmm1_scale_log2_tensor / bmm2_scale_tensor with a 16-bit query",
     dict(dtype=torch.bfloat16, bmm1_scale_log2_tensor=torch.ones(1), bmm2_scale_tensor=torch.ones(1))),
    ("sinks", dict(sinks=[torch.zeros(16)])),
]


@pytest.mark.parametrize("names,over", REFUSALS, ids=[f"{i}_{r[0][:24].replace(' ', '_')}" for i, r in enumerate(REFUSALS)])
def test_what_is_not_offered_is_refused_by_name_before_the_library(monkeypatch, names, over):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=names):
        D.trtllm_batch_decode_with_kv_cache_mla(**_mla_args(**over))


def test_bad_fp8_arguments_are_value_errors(monkeypatch):
    _no_library(monkeypatch)
    for over in (dict(bmm1_scale_log2_tensor=torch.ones(1, dtype=torch.float64), bmm2_scale_tensor=torch.ones(1)),
                 dict(bmm1_scale_log2_tensor=torch.ones(2), bmm2_scale_tensor=torch.ones(1)),
                 dict(query=torch.zeros(3, 2, 16, 584).to(E4M3)[..., :576]),    # stride 584: 8 | 584, 16 does not
                 dict(kv_cache=torch.zeros(12, 16, 584).to(E4M3)[..., :576]),
                 dict(query=torch.zeros(3 * 2 * 16 * 576 + 16).to(E4M3)[8:-8].view(3, 2, 16, 576))):
        with pytest.raises(ValueError):
            D.trtllm_batch_decode_with_kv_cache_mla(**_mla_args(**over))


# ---- BatchMLAPagedAttentionWrapper.plan ----

class _PlanOnly(BatchMLAPagedAttentionWrapper):
    """What plan() touches of a wrapper, on the CPU (the constructor pins host memory, which needs a GPU)."""

    def __init__(self):
        self._use_cuda_graph = False
        self._fixed_batch_size = 0
        self._graph_rows = None
        self.device = torch.device("cpu")
        self._float_workspace_buffer = torch.zeros(1024, dtype=torch.uint8)
        self._int_workspace_buffer = torch.zeros(1024, dtype=torch.uint8)
        self._pin_memory_int_workspace_buffer = torch.zeros(1024, dtype=torch.uint8)


def _wrapper_plan(q_dtype, kv_dtype):
    i32 = dict(dtype=torch.int32)
    _PlanOnly().plan(torch.tensor([0, 1], **i32), torch.tensor([0, 1], **i32), torch.tensor([0], **i32),
                     torch.tensor([5], **i32), 16, 512, 64, 16, True, 0.1, q_dtype, kv_dtype)


@pytest.mark.parametrize("q_dtype", [torch.float16, torch.bfloat16])
def test_wrapper_plan_accepts_an_fp8_cache(monkeypatch, q_dtype):
    """The planner is reached, and is handed the compute dtype for both of its dtype fields."""
    _capture_library(monkeypatch)
    with pytest.raises(_Reached) as e:
        _wrapper_plan(q_dtype, E4M3)
    name, args = e.value.args
    assert name == "fi_batch_mla_plan"
    assert (args[0]._obj.q_dtype, args[0]._obj.kv_dtype) == (_lib.fi_dtype(q_dtype),) * 2


@pytest.mark.parametrize("q_dtype,kv_dtype", [(E4M3, E4M3), (E4M3, torch.bfloat16), (torch.float16, E5M2),
                                               (torch.float16, torch.bfloat16)])
def test_wrapper_plan_refuses_an_fp8_query_and_other_pairs(monkeypatch, q_dtype, kv_dtype):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="q_data_type|kv_data_type"):
        _wrapper_plan(q_dtype, kv_dtype)


# ---- the C entries, before any launch ----

def test_new_symbol_and_fields_are_in_the_header_the_library_and_the_binding(fi_lib):
    with open(os.path.join(ROOT, "include", "fi_mi355.h")) as f:
        header = f.read()
    assert re.search(r"FI_API int fi_mla_rope_quantize\(", header)
    assert "fi_mla_rope_quantize" in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, "fi_mla_rope_quantize")
    fields = [name for name, _ in _lib.fi_batch_mla_params_t._fields_]
    assert fields[-4:] == ["sm_scale", "q_fp8", "kv_fp8", "sm_scale_log2_dev"]  # appended: zero means "as before"


def _error(fi_lib, rc):
    assert rc != 0
    return fi_lib.fi_last_error().decode()


def test_batch_mla_run_refusals(fi_lib):
    H, ps, float_bytes = 16, 16, 1 << 20
    info, _ = host_plan(fi_lib, [40, 7], 1, H, ps, float_bytes)
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)(*info)
    buf = (C.c_char * 256)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    fp8 = _lib.FI_DTYPE_FP8_E4M3

    def error(**over):
        kw = dict(q_nope=base, q_pe=base, ckv=base, kpe=base, kv_indices=base, o=base, float_ws=base, int_ws=base,
                  float_ws_bytes=float_bytes, int_ws_bytes=8 << 20, num_rows=2 * H, num_heads=H, page_size=ps,
                  dtype=_lib.FI_DTYPE_BF16, causal=1, sm_scale=0.1,
                  q_nope_stride_n=H * 576, q_nope_stride_h=576, q_pe_stride_n=H * 576, q_pe_stride_h=576,
                  ckv_stride_page=ps * 576, ckv_stride_n=576, kpe_stride_page=ps * 576, kpe_stride_n=576)
        kw.update(over)
        p = _lib.fi_batch_mla_params_t(**kw)
        return _error(fi_lib, fi_lib.fi_batch_mla_run(info, _lib.FI_MLA_PLAN_INFO_LEN, C.byref(p), None))

    assert "null tensor" in error(ckv=None, kv_fp8=fp8)
    assert "fp8 query with a 16-bit cache" in error(q_fp8=fp8)
    assert "e5m2" in error(kv_fp8=_lib.FI_DTYPE_FP8_E5M2)
    assert "e5m2" in error(q_fp8=_lib.FI_DTYPE_FP8_E5M2, kv_fp8=fp8)
    assert "fp8 cache must be multiples of 16" in error(kv_fp8=fp8, ckv_stride_n=584, ckv_stride_page=ps * 584)
    assert "fp8 query must be multiples of 16" in error(q_fp8=fp8, kv_fp8=fp8, q_pe_stride_h=584)
    assert "multiples of 8" in error(ckv_stride_n=580)  # the 16-bit rule is the one it was
    assert "16-byte aligned" in error(kv_fp8=fp8, kpe=base + 8)
    assert "fp8 cache only" in error(sm_scale_log2_dev=base)


def test_append_paged_mla_kv_cache_refusals(fi_lib):
    buf = (C.c_char * 256)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16

    def error(**over):
        kw = dict(append_ckv=base, append_kpe=base, batch_indices=base, positions=base, ckv_cache=base, kpe_cache=base,
                  kv_indices=base, kv_indptr=base, append_ckv_stride_n=512, append_kpe_stride_n=64,
                  ckv_stride_page=16 * 512, ckv_stride_n=512, kpe_stride_page=16 * 64, kpe_stride_n=64, nnz=1,
                  page_size=16, head_dim_ckv=512, head_dim_kpe=64, dtype=_lib.FI_DTYPE_FP8_E4M3)
        kw.update(over)
        p = _lib.fi_append_paged_mla_kv_params_t(**kw)
        return _error(fi_lib, fi_lib.fi_append_paged_mla_kv_cache(C.byref(p), None))

    assert "null tensor" in error(kpe_cache=None)
    assert "unsupported dtype" in error(dtype=_lib.FI_DTYPE_F32)
    for dtype in (_lib.FI_DTYPE_FP8_E4M3, _lib.FI_DTYPE_FP8_E5M2):
        assert "multiples of 16 elements" in error(dtype=dtype, ckv_stride_n=520)  # 8 | 520: fine at 16 bit only
        assert "16-byte aligned" in error(dtype=dtype, append_kpe=base + 8)
    assert "multiples of 8 elements" in error(dtype=_lib.FI_DTYPE_BF16, ckv_stride_n=516)


def test_mla_rope_quantize_refusals(fi_lib):
    buf = (C.c_char * 256)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16

    def error(**over):
        kw = dict(q_rope=base, k_rope=base, q_nope=base, k_nope=base, q_rope_out=base, k_rope_out=base, q_nope_out=base,
                  k_nope_out=base, cos_sin_cache=base, pos_ids=base, q_rope_stride_n=128, q_rope_stride_h=64,
                  k_rope_stride_n=64, q_nope_stride_n=1024, q_nope_stride_h=512, k_nope_stride_n=512,
                  q_rope_out_stride_n=128, q_rope_out_stride_h=64, k_rope_out_stride_n=64, q_nope_out_stride_n=1024,
                  q_nope_out_stride_h=512, k_nope_out_stride_n=512, nnz=1, num_heads=2, rope_dim=64, nope_dim=512,
                  dtype=_lib.FI_DTYPE_BF16, out_dtype=_lib.FI_DTYPE_FP8_E4M3, quant_scale_q=1.0, quant_scale_kv=1.0)
        kw.update(over)
        p = _lib.fi_mla_rope_quantize_params_t(**kw)
        return _error(fi_lib, fi_lib.fi_mla_rope_quantize(C.byref(p), None))

    assert fi_lib.fi_mla_rope_quantize(None, None) != 0
    assert "null tensor" in error(k_nope_out=None)
    assert "null tensor" in error(cos_sin_cache=None)
    assert "only 64 / 512" in error(rope_dim=128)
    assert "f16 / bf16" in error(dtype=_lib.FI_DTYPE_F32)
    assert "e4m3 / e5m2" in error(out_dtype=_lib.FI_DTYPE_BF16)
    assert "input rows must be 16-byte aligned" in error(q_nope_stride_h=516)
    assert "input rows must be 16-byte aligned" in error(k_rope=base + 8)
    assert "output rows must be 8-byte aligned" in error(k_nope_out_stride_n=516)
    assert "output rows must be 8-byte aligned" in error(q_rope_out=base + 4)


# ---- the reference the GPU tests compare against ----

@pytest.mark.parametrize("fp8_dtype", [E4M3, E5M2], ids=["e4m3", "e5m2"])
def test_numpy_fp8_rounding_is_torch_s_and_saturates(fp8_dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g, dtype=torch.float64) * s for s in (1e-3, 0.05, 1.0, 30.0)])
    finite = torch.arange(256, dtype=torch.uint8).view(fp8_dtype).double()
    finite = finite[torch.isfinite(finite)]
    ties = (finite[:-1] + finite[1:]) / 2  # halfway between neighbours (and across zero)
    x = torch.cat([x, finite, ties])
    big = 448.0 if fp8_dtype == E4M3 else 57344.0
    x = x[x.abs() <= big]  # torch does not saturate: compared below the largest finite value only
    got = fp8_round(x.numpy(), fp8_dtype)
    assert np.array_equal(got, x.to(fp8_dtype).double().numpy())
    assert np.array_equal(fp8_round(np.array([big * 1.07, -1e9, 2400.0 * 8 * 8]), fp8_dtype)[:2], [big, -big])
    order = fp8_order(np.sort(finite.numpy()), fp8_dtype)
    assert set(np.diff(order)) <= {0, 1} and order[0] == -order[-1]


def test_rope_quantize_ref_rotates_the_right_pairs():
    """Position p with cos = 0, sin = 1 turns (x0, x1) into (-x1, x0): NeoX pairs are (i, i + 32), the others (2i, 2i+1)."""
    cache = torch.cat([torch.zeros(4, 32), torch.ones(4, 32)], dim=1)
    x = torch.arange(1, 65, dtype=torch.float32).reshape(1, 64) / 8
    zeros = torch.zeros(1, 512)
    pos = torch.tensor([2])
    neox = rope_quantize_ref(x[:, None], x, zeros[:, None], zeros, cache, pos, True, E4M3, 1.0, 2.0)
    assert np.array_equal(neox[0][0, 0], torch.cat([-x[0, 32:], x[0, :32]]).to(E4M3).double().numpy())
    assert np.array_equal(neox[1][0], (2 * torch.cat([-x[0, 32:], x[0, :32]])).to(E4M3).double().numpy())
    gptj = rope_quantize_ref(x[:, None], x, zeros[:, None], zeros, cache, pos, False, E4M3, 1.0, 1.0)
    want = torch.stack([-x[0, 1::2], x[0, 0::2]], dim=1).reshape(64)
    assert np.array_equal(gptj[1][0], want.to(E4M3).double().numpy())


def test_graded_cache_covers_every_finite_code_and_poisons_the_rest():
    c = make_fp8_case([65, 3], 1, 16, 16, torch.bfloat16, seed=0)
    raw = c["cache8"].view(torch.uint8)
    assert c["cache"].isnan().any() and (raw == 0x7F).any() and not (raw == 0xFF).any()
    assert torch.equal(c["cache"].float()[~c["cache"].isnan()], c["cache8"].float()[~c["cache8"].float().isnan()])
