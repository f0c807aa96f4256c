"""flashinfer.decode.trtllm_batch_decode_with_kv_cache and fi_batch_decode_plan_device without a GPU: the signature,
what is refused by name, the workspace carve and the C entry's checks, none of which launches anything."""
import ctypes as C
import inspect
import os

import pytest
import torch

from flashinfer import _lib
from flashinfer import decode as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ref flashinfer/decode.py:2054-2071: names, order, defaults
REFERENCE_PARAMETERS = [
    ("query", inspect.Parameter.empty), ("kv_cache", inspect.Parameter.empty),
    ("workspace_buffer", inspect.Parameter.empty), ("block_tables", inspect.Parameter.empty),
    ("seq_lens", inspect.Parameter.empty), ("max_seq_len", inspect.Parameter.empty),
    ("bmm1_scale", inspect.Parameter.empty), ("bmm2_scale", inspect.Parameter.empty), ("window_left", -1),
    ("out", None), ("out_dtype", None), ("o_sf_scale", None), ("o_sf_vec_size", None), ("sinks", None),
    ("enable_pdl", None), ("q_len_per_req", 1),
]


def test_signature_is_the_reference_s():
    params = inspect.signature(D.trtllm_batch_decode_with_kv_cache).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_PARAMETERS
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_it_lives_in_flashinfer_decode_only():
    import flashinfer

    assert not hasattr(flashinfer, "trtllm_batch_decode_with_kv_cache")


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def _args(B=3, hq=32, hkv=8, d=128, ps=16, max_blocks=8, pages=12, ws_bytes=1 << 20, dtype=torch.float16, **over):
    args = dict(query=torch.zeros(B, hq, d, dtype=dtype), kv_cache=torch.zeros(pages, 2, hkv, ps, d, dtype=dtype),
                workspace_buffer=torch.zeros(ws_bytes, dtype=torch.uint8),
                block_tables=torch.zeros(B, max_blocks, dtype=torch.int32), seq_lens=torch.ones(B, dtype=torch.int32),
                max_seq_len=max_blocks * ps, bmm1_scale=d ** -0.5, bmm2_scale=1.0)
    args.update(over)
    return args


class _NotATensor:
    """Stands in for the reference's FP4Tensor: an ``out`` that is not a torch.Tensor."""


REFUSALS = [
    ("q_len_per_req", dict(q_len_per_req=2)),
    ("fp8 query", dict(query=torch.zeros(3, 32, 128).to(torch.float8_e4m3fn))),
    ("nvfp4", dict(out_dtype="nvfp4")),
    ("o_sf_scale", dict(o_sf_scale=1.0)),
    ("o_sf_vec_size", dict(o_sf_vec_size=16)),
    ("FP4Tensor", dict(out=_NotATensor())),
    ("K and V shared", dict(kv_cache=torch.zeros(12, 1, 8, 16, 128, dtype=torch.float16))),
]


@pytest.mark.parametrize("names,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_what_is_not_offered_is_refused_by_name_before_the_library(monkeypatch, names, over):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=names):
        D.trtllm_batch_decode_with_kv_cache(**_args(**over))


def test_accepted_arguments_reach_the_library(monkeypatch):
    """A (k, v) tuple, uint32 lengths, a one-element sinks list, enable_pdl: all pass the Python checks."""
    _no_library(monkeypatch)
    kv = torch.zeros(12, 8, 16, 128, dtype=torch.float16)
    for over in (dict(), dict(kv_cache=(kv, kv.clone())), dict(seq_lens=torch.ones(3, dtype=torch.uint32)),
                 dict(sinks=[torch.zeros(32)]), dict(sinks=torch.zeros(32)), dict(enable_pdl=True),
                 dict(out_dtype=torch.float16), dict(out_dtype="float16"), dict(window_left=64)):
        with pytest.raises(AssertionError, match="the library was reached"):
            D.trtllm_batch_decode_with_kv_cache(**_args(**over))


@pytest.mark.parametrize("over", [dict(max_seq_len=8 * 16 + 1), dict(block_tables=torch.zeros(3, 8, dtype=torch.int64)),
                                  dict(seq_lens=torch.ones(4, dtype=torch.int32)), dict(sinks=[torch.zeros(31)]),
                                  dict(out_dtype=torch.bfloat16), dict(kv_cache=torch.zeros(12, 2, 8, 16, 64).half())])
def test_bad_arguments_are_value_errors(monkeypatch, over):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        D.trtllm_batch_decode_with_kv_cache(**_args(**over))


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="GPU"):
        D.trtllm_batch_decode_with_kv_cache(**_args())


def _plan_params(B=3, max_blocks=8, ps=16, hq=32, hkv=8, d=128, hint=0, **over):
    kw = dict(block_tables=None, seq_lens=None, block_tables_stride=max_blocks, int_ws=None, int_ws_bytes=0,
              float_ws=None, float_ws_bytes=0, batch_size=B, max_blocks=max_blocks, page_size=ps, num_qo_heads=hq,
              num_kv_heads=hkv, head_dim=d, q_dtype=_lib.FI_DTYPE_F16, kv_dtype=_lib.FI_DTYPE_F16, max_grid_hint=hint)
    kw.update(over)
    return _lib.fi_batch_decode_plan_device_params_t(**kw)


def _sizes(fi_lib, p):
    ib, fb = C.c_size_t(), C.c_size_t()
    assert fi_lib.fi_batch_decode_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)) == 0, \
        fi_lib.fi_last_error()
    return ib.value, fb.value


def _a16(n):
    return (n + 15) // 16 * 16


def test_workspace_sizes_follow_the_host_known_capacity(fi_lib):
    """Split branch (B * gdy < max_grid): the list holds max(max_grid / gdy, B) entries, as a host graph plan whose
    list is no longer; unsplit: B, no partial states."""
    B, mb, hq, hkv, d = 3, 8, 32, 8, 128
    padded = max(256 // 8, B)
    ints = _a16(4 * padded)  # request_indices
    ints = _a16(ints + 4 * padded)  # kv_tile_indices
    ints = _a16(ints + 4 * (B + 1))  # o_indptr
    ints = _a16(ints + 8)  # chunk size, work items
    ints = _a16(ints + padded)  # mask
    ints = _a16(ints + 4 * (B + 1))  # CSR indptr
    ints = _a16(ints + 4 * B)  # last_page_len
    ints = ints + 4 * B * mb  # indices
    assert _sizes(fi_lib, _plan_params(B, mb, hint=256)) == (ints, _a16(4 * hq * padded * d) + 4 * hq * padded)
    ib, fb = _sizes(fi_lib, _plan_params(B, mb, hint=24))  # 3 requests x 8 kv heads fill a grid of 24
    assert fb == 0 and ib < ints


def test_too_small_a_workspace_is_a_value_error_with_the_size(monkeypatch, fi_lib):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)
    ib, fb = _sizes(fi_lib, _plan_params())
    args = _args(ws_bytes=ib + 15)  # the int region alone (plus alignment slack): no room for the partial states
    slack = -args["workspace_buffer"].data_ptr() % 16
    need = slack + _a16(ib) + fb
    with pytest.raises(ValueError, match=rf"{need} bytes needed"):
        D.trtllm_batch_decode_with_kv_cache(**args)


def test_c_entry_checks_before_any_launch(fi_lib):
    info, csr = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)(), (C.c_int64 * 3)()

    def error(p):
        assert fi_lib.fi_batch_decode_plan_device(C.byref(p), info, csr, None) != 0
        return fi_lib.fi_last_error().decode()

    assert "null tensor" in error(_plan_params())
    buf = (C.c_char * 64)()
    fake = dict(block_tables=C.addressof(buf), seq_lens=C.addressof(buf), int_ws=C.addressof(buf), float_ws=C.addressof(buf))
    ib, fb = _sizes(fi_lib, _plan_params())
    assert f"int workspace too small (64 bytes, need {ib})" in error(_plan_params(int_ws_bytes=64, **fake))
    assert f"float workspace too small (64 bytes, need {fb})" in error(
        _plan_params(int_ws_bytes=ib, float_ws_bytes=64, **fake))
    assert "head_dim 96" in error(_plan_params(d=96, **fake))
    assert "q dtype" in error(_plan_params(q_dtype=_lib.FI_DTYPE_FP8_E4M3, **fake))
    assert "kv dtype 4" in error(_plan_params(kv_dtype=_lib.FI_DTYPE_F32, **fake))
    assert "batch_size" in error(_plan_params(B=0, **fake))
    assert fi_lib.fi_batch_decode_plan_device(None, info, csr, None) != 0


def test_new_sources_do_not_name_the_oracle():
    for rel in ("flashinfer-ai_amd/flashinfer/decode.py", "flashinfer-ai_amd/csrc/decode_plan_device.hip",
                "flashinfer-ai_amd/csrc/decode_plan.h", "flashinfer-ai_amd/csrc/plan_device.h",
                "flashinfer-ai_amd/flashinfer/_plan_free.py"):
        with open(os.path.join(ROOT, rel)) as f:
            assert "oracle" not in f.read(), rel
