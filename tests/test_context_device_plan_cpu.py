"""flashinfer.prefill.trtllm_batch_context_with_kv_cache and fi_batch_prefill_plan_device without a GPU: the
signature, what is refused by name, the argument checks, the workspace sizes and the C entry's checks, none of which
launches anything."""
import ctypes as C
import inspect
import os

import pytest
import torch

from flashinfer import _lib
from flashinfer import prefill as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = inspect.Parameter.empty

# ref flashinfer/prefill.py:3314-3334: names, order, defaults
REFERENCE_PARAMETERS = [
    ("query", E), ("kv_cache", E), ("workspace_buffer", E), ("block_tables", E), ("seq_lens", E), ("max_q_len", E),
    ("max_kv_len", E), ("bmm1_scale", E), ("bmm2_scale", E), ("batch_size", E), ("cum_seq_lens_q", E),
    ("cum_seq_lens_kv", E), ("window_left", -1), ("out", None), ("out_dtype", None), ("o_sf_scale", None),
    ("o_sf_vec_size", None), ("enable_pdl", None), ("sinks", None),
]


def test_signature_is_the_reference_s():
    params = inspect.signature(P.trtllm_batch_context_with_kv_cache).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_PARAMETERS
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_it_lives_in_flashinfer_prefill_only():
    import flashinfer

    assert not hasattr(flashinfer, "trtllm_batch_context_with_kv_cache")


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def _args(B=3, rows=10, hq=32, hkv=8, d=128, ps=16, max_blocks=8, pages=12, ws_bytes=1 << 20, dtype=torch.float16,
          **over):
    args = dict(query=torch.zeros(rows, hq, d, dtype=dtype), kv_cache=torch.zeros(pages, 2, hkv, ps, d, dtype=dtype),
                workspace_buffer=torch.zeros(ws_bytes, dtype=torch.uint8),
                block_tables=torch.zeros(B, max_blocks, dtype=torch.int32), seq_lens=torch.ones(B, dtype=torch.int32),
                max_q_len=rows, max_kv_len=max_blocks * ps, bmm1_scale=d ** -0.5, bmm2_scale=1.0, batch_size=B,
                cum_seq_lens_q=torch.zeros(B + 1, dtype=torch.int32), cum_seq_lens_kv=None)
    args.update(over)
    return args


class _NotATensor:
    """Stands in for the reference's FP4Tensor: an ``out`` that is not a torch.Tensor."""


REFUSALS = [
    ("e5m2 query", dict(query=torch.zeros(10, 32, 128).to(torch.float8_e5m2))),
    ("nvfp4", dict(out_dtype="nvfp4")),
    ("o_sf_scale", dict(o_sf_scale=1.0)),
    ("o_sf_vec_size", dict(o_sf_vec_size=16)),
    ("FP4Tensor", dict(out=_NotATensor())),
    ("K and V shared", dict(kv_cache=torch.zeros(12, 1, 8, 16, 128, dtype=torch.float16))),
    ("fp8 output", dict(out_dtype=torch.float8_e4m3fn)),
    ("fp8 output", dict(out=torch.zeros(10, 32, 128).to(torch.float8_e4m3fn))),
]


@pytest.mark.parametrize("names,over", REFUSALS, ids=[f"{i}-{r[0]}" for i, r in enumerate(REFUSALS)])
def test_what_is_not_offered_is_refused_by_name_before_the_library(monkeypatch, names, over):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=names):
        P.trtllm_batch_context_with_kv_cache(**_args(**over))


def _fp8(*shape):
    return torch.zeros(*shape).to(torch.float8_e4m3fn)


def test_accepted_arguments_reach_the_library(monkeypatch):
    """A (k, v) tuple, uint32 lengths, a one-element sinks list, enable_pdl, a strided query, an fp8 cache under a
    16-bit query, an fp8 query with a 16-bit output named either way: all pass the Python checks."""
    _no_library(monkeypatch)
    kv = torch.zeros(12, 8, 16, 128, dtype=torch.float16)
    fp8 = dict(query=_fp8(10, 32, 128), kv_cache=_fp8(12, 2, 8, 16, 128))
    for over in (dict(), dict(kv_cache=(kv, kv.clone())), dict(seq_lens=torch.ones(3, dtype=torch.uint32)),
                 dict(sinks=[torch.zeros(32)]), dict(sinks=torch.zeros(32)), dict(enable_pdl=True),
                 dict(out_dtype=torch.float16), dict(out_dtype="float16"), dict(window_left=64),
                 dict(query=torch.zeros(10, 40, 128, dtype=torch.float16)[:, :32]),
                 dict(kv_cache=_fp8(12, 2, 8, 16, 128)), dict(cum_seq_lens_kv=torch.zeros(4, dtype=torch.int32)),
                 dict(out_dtype=torch.bfloat16, **fp8), dict(out=torch.zeros(10, 32, 128, dtype=torch.float16), **fp8)):
        with pytest.raises(AssertionError, match="the library was reached"):
            P.trtllm_batch_context_with_kv_cache(**_args(**over))


BAD = [
    dict(max_kv_len=8 * 16 + 1), dict(block_tables=torch.zeros(3, 8, dtype=torch.int64)),
    dict(seq_lens=torch.ones(4, dtype=torch.int32)), dict(sinks=[torch.zeros(31)]), dict(out_dtype=torch.bfloat16),
    dict(kv_cache=torch.zeros(12, 2, 8, 16, 64).half()), dict(batch_size=4),
    dict(cum_seq_lens_q=torch.zeros(3, dtype=torch.int32)), dict(cum_seq_lens_q=torch.zeros(4, dtype=torch.int64)),
    dict(query=torch.zeros(10, 32, 128)), dict(out=torch.zeros(9, 32, 128, dtype=torch.float16)),
    dict(out=torch.zeros(10, 32, 128, dtype=torch.float16), out_dtype=torch.bfloat16),
    # an fp8 query: no output dtype named; a 16-bit cache; sinks
    dict(query=_fp8(10, 32, 128), kv_cache=_fp8(12, 2, 8, 16, 128)),
    dict(query=_fp8(10, 32, 128), out_dtype=torch.float16),
    dict(query=_fp8(10, 32, 128), kv_cache=_fp8(12, 2, 8, 16, 128), out_dtype=torch.float16, sinks=torch.zeros(32)),
]


@pytest.mark.parametrize("over", BAD, ids=[f"{i}-{'-'.join(o)}" for i, o in enumerate(BAD)])
def test_bad_arguments_are_value_errors(monkeypatch, over):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        P.trtllm_batch_context_with_kv_cache(**_args(**over))


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="GPU"):
        P.trtllm_batch_context_with_kv_cache(**_args())


def _plan_params(B=3, rows=10, max_blocks=8, ps=16, hq=32, hkv=8, d=128, hint=64, **over):
    kw = dict(block_tables=None, seq_lens=None, cum_seq_lens_q=None, block_tables_stride=max_blocks, int_ws=None,
              int_ws_bytes=0, float_ws=None, float_ws_bytes=0, batch_size=B, max_blocks=max_blocks, page_size=ps,
              total_num_rows=rows, num_qo_heads=hq, num_kv_heads=hkv, head_dim=d, q_dtype=_lib.FI_DTYPE_F16,
              kv_dtype=_lib.FI_DTYPE_F16, window_left=-1, max_items_hint=hint)
    kw.update(over)
    return _lib.fi_batch_prefill_plan_device_params_t(**kw)


def _sizes(fi_lib, p):
    ib, fb = C.c_size_t(), C.c_size_t()
    assert fi_lib.fi_batch_prefill_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)) == 0, \
        fi_lib.fi_last_error()
    return ib.value, fb.value


def _a16(n):
    return (n + 15) // 16 * 16


def _int_bytes(capacity, rows, B, mb):
    n = 0
    for words in (capacity, capacity, capacity, rows + 1, 2, B + 1, B + 1, B + 1, B + 1, B):
        n = _a16(n) + 4 * words  # three lists, merge_indptr, chunk slot, qo / item / entry / page indptr, last_page_len
    return _a16(n) + 4 * B * mb  # indices


def test_workspace_sizes_follow_the_host_known_branch(fi_lib):
    """T0 = ceil(rows x group / 128).  Split (T0 <= max_items): the list holds max(max_items, T0 + B - 1) items and the
    partial states max_items x (ceil(128 / group) + 1) entries, lse first.  Unsplit: T0 + B - 1 items and no float
    workspace at all."""
    B, mb, hq, hkv, d = 3, 8, 32, 8, 128
    rows, group = 300, hq // hkv
    t0 = -(-rows * group // 128)  # 10
    entries = 64 * (128 // group + 1)
    assert _sizes(fi_lib, _plan_params(B, rows, mb, hint=64)) == (
        _int_bytes(64, rows, B, mb), _a16(4 * hq * entries) + 4 * hq * entries * d)
    # more q tiles than max_items can come out of the bound alone: capacity T0 + B - 1 in the split branch too
    assert _sizes(fi_lib, _plan_params(B, rows, mb, hint=t0))[0] == _int_bytes(t0 + B - 1, rows, B, mb)
    assert _sizes(fi_lib, _plan_params(B, rows, mb, hint=t0 - 1)) == (_int_bytes(t0 + B - 1, rows, B, mb), 0)


def test_too_small_a_workspace_is_a_value_error_with_the_size(monkeypatch, fi_lib):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)
    ib, fb = _sizes(fi_lib, _plan_params(hint=0))  # the call sizes max_items from the device, as hint 0 does
    assert fb > 0
    args = _args(ws_bytes=ib + 15)  # the int region alone (plus alignment slack): no room for the partial states
    slack = -args["workspace_buffer"].data_ptr() % 16
    need = slack + _a16(ib) + fb
    with pytest.raises(ValueError, match=rf"{need} bytes needed"):
        P.trtllm_batch_context_with_kv_cache(**args)


def test_c_entry_checks_before_any_launch(fi_lib):
    info, csr = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)(), (C.c_int64 * 4)()

    def error(p):
        assert fi_lib.fi_batch_prefill_plan_device(C.byref(p), info, csr, None) != 0
        return fi_lib.fi_last_error().decode()

    assert "null tensor" in error(_plan_params())
    buf = (C.c_char * 64)()
    fake = dict(block_tables=C.addressof(buf), seq_lens=C.addressof(buf), cum_seq_lens_q=C.addressof(buf),
                int_ws=C.addressof(buf), float_ws=C.addressof(buf))
    ib, fb = _sizes(fi_lib, _plan_params())
    assert f"int workspace too small (64 bytes, need {ib})" in error(_plan_params(int_ws_bytes=64, **fake))
    assert f"float workspace too small (64 bytes, need {fb})" in error(
        _plan_params(int_ws_bytes=ib, float_ws_bytes=64, **fake))
    assert "head_dim 96" in error(_plan_params(d=96, **fake))
    assert "q dtype" in error(_plan_params(q_dtype=_lib.FI_DTYPE_FP8_E5M2, **fake))
    assert "kv dtype 4" in error(_plan_params(kv_dtype=_lib.FI_DTYPE_F32, **fake))
    assert "kv dtype" in error(_plan_params(q_dtype=_lib.FI_DTYPE_FP8_E4M3, **fake))  # an fp8 q over a 16-bit cache
    assert "batch_size" in error(_plan_params(B=0, **fake))
    assert "total_num_rows" in error(_plan_params(rows=-1, **fake))
    assert "rows overlap" in error(_plan_params(block_tables_stride=7, **fake))
    assert "multiple of num_kv_heads" in error(_plan_params(hq=30, **fake))
    assert "31 bits" in error(_plan_params(max_blocks=1 << 27, ps=16, block_tables_stride=1 << 27, **fake))
    assert fi_lib.fi_batch_prefill_plan_device(None, info, csr, None) != 0


def test_new_sources_do_not_name_the_oracle():
    for rel in ("flashinfer-ai_amd/csrc/prefill_plan_device.hip", "flashinfer-ai_amd/csrc/prefill_plan.h",
                "flashinfer-ai_amd/csrc/plan_device.h", "flashinfer-ai_amd/flashinfer/_plan_free.py"):
        with open(os.path.join(ROOT, rel)) as f:
            assert "oracle" not in f.read(), rel
