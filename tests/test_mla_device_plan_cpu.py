"""flashinfer.decode.trtllm_batch_decode_with_kv_cache_mla and fi_batch_mla_plan_device without a GPU: the signature,
what is refused by name, the argument checks, the workspace carve and the C entry's checks, none of which launches
anything."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from flashinfer import _lib
from flashinfer import decode as D
from mla_plan_free_inputs import plan_params, workspace_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fi_batch_mla_plan_device", "fi_batch_mla_plan_device_workspace")

# ref flashinfer/decode.py:2298-2315: names, order, defaults
REFERENCE_PARAMETERS = [
    ("query", inspect.Parameter.empty), ("kv_cache", inspect.Parameter.empty),
    ("workspace_buffer", inspect.Parameter.empty), ("qk_nope_head_dim", inspect.Parameter.empty),
    ("kv_lora_rank", inspect.Parameter.empty), ("qk_rope_head_dim", inspect.Parameter.empty),
    ("block_tables", inspect.Parameter.empty), ("seq_lens", inspect.Parameter.empty),
    ("max_seq_len", inspect.Parameter.empty), ("out", None), ("bmm1_scale", 1.0), ("bmm2_scale", 1.0),
    ("bmm1_scale_log2_tensor", None), ("bmm2_scale_tensor", None), ("sinks", None), ("enable_pdl", None),
]


def test_signature_is_the_reference_s():
    params = inspect.signature(D.trtllm_batch_decode_with_kv_cache_mla).parameters.values()
    assert [(p.name, p.default) for p in params] == REFERENCE_PARAMETERS
    assert all(p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params)


def test_it_lives_in_flashinfer_decode_only():
    import flashinfer

    assert not hasattr(flashinfer, "trtllm_batch_decode_with_kv_cache_mla")


def _no_library(monkeypatch):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def _args(B=3, q_len=2, H=16, ps=16, max_blocks=8, pages=12, ws_bytes=1 << 20, dtype=torch.float16, **over):
    args = dict(query=torch.zeros(B, q_len, H, 576, dtype=dtype), kv_cache=torch.zeros(pages, 1, ps, 576, dtype=dtype),
                workspace_buffer=torch.zeros(ws_bytes, dtype=torch.uint8), qk_nope_head_dim=128, kv_lora_rank=512,
                qk_rope_head_dim=64, block_tables=torch.zeros(B, max_blocks, dtype=torch.int32),
                seq_lens=torch.ones(B, dtype=torch.int32), max_seq_len=max_blocks * ps)
    args.update(over)
    return args


REFUSALS = [
    ("fp8 query", dict(query=torch.zeros(3, 2, 16, 576).to(torch.float8_e4m3fn))),
    ("fp8 query or kv_cache", dict(kv_cache=torch.zeros(12, 16, 576).to(torch.float8_e4m3fn))),
    ("bmm1_scale_log2_tensor", dict(bmm1_scale_log2_tensor=torch.ones(1))),
    ("bmm2_scale_tensor", dict(bmm2_scale_tensor=torch.ones(1))),
    ("sinks", dict(sinks=[torch.zeros(16)])),
]


@pytest.mark.parametrize("names,over", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_what_is_not_offered_is_refused_by_name_before_the_library(monkeypatch, names, over):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=names):
        D.trtllm_batch_decode_with_kv_cache_mla(**_args(**over))


def test_accepted_arguments_reach_the_library(monkeypatch):
    """Both cache shapes, any page size, uint32 lengths, views of wider tensors, both out shapes, enable_pdl, one
    request, one token: all pass the Python checks."""
    _no_library(monkeypatch)
    wide_q = torch.zeros(3, 2, 16, 640, dtype=torch.float16)[..., :576]
    wide_kv = torch.zeros(12, 16, 640, dtype=torch.float16)[..., :576]
    for over in (dict(), dict(kv_cache=torch.zeros(12, 16, 576, dtype=torch.float16)),
                 dict(kv_cache=torch.zeros(12, 1, 5, 576, dtype=torch.float16), max_seq_len=40),
                 dict(seq_lens=torch.ones(3, dtype=torch.uint32)), dict(query=wide_q), dict(kv_cache=wide_kv),
                 dict(enable_pdl=True), dict(out=torch.zeros(3, 2, 16, 512, dtype=torch.float16)),
                 dict(q_len=1, out=torch.zeros(3, 16, 512, dtype=torch.float16)),
                 dict(q_len=1, out=torch.zeros(3, 1, 16, 512, dtype=torch.float16)),
                 dict(query=torch.zeros(3, 4, 16, 576, dtype=torch.float16)[:, :1]),  # q_len 1: any batch stride
                 dict(query=torch.zeros(2, 4, 16, 576, dtype=torch.float16)[:1, :2],  # one request: any batch stride
                      block_tables=torch.zeros(1, 8, dtype=torch.int32), seq_lens=torch.ones(1, dtype=torch.int32)),
                 dict(dtype=torch.bfloat16), dict(bmm1_scale=0.1, bmm2_scale=0.5)):
        with pytest.raises(AssertionError, match="the library was reached"):
            D.trtllm_batch_decode_with_kv_cache_mla(**_args(**over))


BAD = {
    "qk_nope_head_dim": dict(qk_nope_head_dim=64),
    "kv_lora_rank": dict(kv_lora_rank=256),
    "qk_rope_head_dim": dict(qk_rope_head_dim=32),
    "query_3d": dict(query=torch.zeros(3, 16, 576, dtype=torch.float16)),
    "query_f32": dict(query=torch.zeros(3, 2, 16, 576)),
    "query_head_dim": dict(query=torch.zeros(3, 2, 16, 512, dtype=torch.float16)),
    "query_last_dim_strided": dict(query=torch.zeros(3, 2, 16, 1152, dtype=torch.float16)[..., ::2]),
    "query_does_not_flatten": dict(query=torch.zeros(3, 4, 16, 576, dtype=torch.float16)[:, :2]),
    "query_stride_not_8": dict(query=torch.zeros(3, 2, 16, 580, dtype=torch.float16)[..., :576]),
    "query_misaligned": dict(query=torch.zeros(3 * 2 * 16 * 576 + 8, dtype=torch.float16)[4:-4].view(3, 2, 16, 576)),
    "cache_dtype": dict(kv_cache=torch.zeros(12, 16, 576, dtype=torch.bfloat16)),
    "cache_head_dim": dict(kv_cache=torch.zeros(12, 16, 512, dtype=torch.float16)),
    "cache_5d": dict(kv_cache=torch.zeros(12, 2, 1, 16, 576, dtype=torch.float16)),
    "cache_stride_not_8": dict(kv_cache=torch.zeros(12, 16, 580, dtype=torch.float16)[..., :576]),
    "max_seq_len": dict(max_seq_len=8 * 16 + 1),
    "block_tables_int64": dict(block_tables=torch.zeros(3, 8, dtype=torch.int64)),
    "block_tables_batch": dict(block_tables=torch.zeros(4, 8, dtype=torch.int32)),
    "seq_lens_shape": dict(seq_lens=torch.ones(4, dtype=torch.int32)),
    "workspace_strided": dict(workspace_buffer=torch.zeros(2 << 20, dtype=torch.uint8)[::2]),
    "out_dtype": dict(out=torch.zeros(3, 2, 16, 512, dtype=torch.bfloat16)),
    "out_shape": dict(out=torch.zeros(3, 2, 16, 576, dtype=torch.float16)),
    "out_3d_with_q_len_2": dict(out=torch.zeros(3, 16, 512, dtype=torch.float16)),
    "out_strided": dict(out=torch.zeros(3, 2, 16, 1024, dtype=torch.float16)[..., :512]),
}


@pytest.mark.parametrize("case", BAD)
def test_bad_arguments_are_value_errors(monkeypatch, case):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        D.trtllm_batch_decode_with_kv_cache_mla(**_args(**BAD[case]))


def test_cpu_tensors_are_refused():
    with pytest.raises(RuntimeError, match="GPU"):
        D.trtllm_batch_decode_with_kv_cache_mla(**_args())


def test_new_symbols_are_in_the_header_the_library_and_the_binding(fi_lib):
    with open(os.path.join(ROOT, "include", "fi_mi355.h")) as f:
        header = f.read()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"FI_API int {sym}\(", header), sym
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, sym), sym
    assert "} fi_batch_mla_plan_device_params_t;" in header
    fields = [name for name, _ in _lib.fi_batch_mla_plan_device_params_t._fields_]
    assert fields == ["block_tables", "seq_lens", "block_tables_stride", "int_ws", "int_ws_bytes", "float_ws",
                      "float_ws_bytes", "batch_size", "max_blocks", "page_size", "num_heads", "q_len_per_request",
                      "head_dim_ckv", "head_dim_kpe", "q_dtype", "kv_dtype", "max_items_hint"]


def _a32(n):
    return (n + 31) // 32 * 32


def test_workspace_sizes_follow_the_host_known_capacity(fi_lib):
    """Header, merge indptr [rows + 1], the list at max(max_items, batch x tiles) items of 32 bytes, then the planner's
    two scans [batch + 1] and its chunk size.  No float bytes are required: a plan that cannot split is correct."""
    B, H, q_len = 3, 16, 2
    rows, tiles = B * q_len * H, 2
    for hint, capacity in ((64, 64), (B * tiles, B * tiles), (4, B * tiles)):
        want = _a32(64 + 4 * (rows + 1)) + 32 * capacity + 4 * (2 * (B + 1) + 1)
        assert workspace_sizes(fi_lib, plan_params(B, H=H, q_len=q_len, hint=hint)) == (want, 0)
    # 8 heads, 3 tokens: 24 packed rows are two tiles, the second half empty
    assert workspace_sizes(fi_lib, plan_params(1, H=8, q_len=3, hint=1))[0] == _a32(64 + 4 * 25) + 32 * 2 + 4 * 5
    # hint 0: sized from the device, as fi_batch_mla_plan does
    cus = fi_lib.fi_num_compute_units()
    assert workspace_sizes(fi_lib, plan_params(B, H=H, q_len=q_len))[0] == \
        _a32(64 + 4 * (rows + 1)) + 32 * max(cus, B * tiles) + 4 * (2 * (B + 1) + 1)


def test_too_small_a_workspace_is_a_value_error_with_the_size(monkeypatch, fi_lib):
    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)
    ib, fb = workspace_sizes(fi_lib, plan_params(3, H=16, q_len=2))
    assert fb == 0
    args = _args(ws_bytes=ib - 1)
    need = -args["workspace_buffer"].data_ptr() % 16 + (ib + 15) // 16 * 16
    with pytest.raises(ValueError, match=rf"{need} bytes needed"):
        D.trtllm_batch_decode_with_kv_cache_mla(**args)


def test_c_entry_checks_before_any_launch(fi_lib):
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()

    def error(p):
        assert fi_lib.fi_batch_mla_plan_device(C.byref(p), info, None) != 0
        return fi_lib.fi_last_error().decode()

    assert "null tensor" in error(plan_params())
    buf = (C.c_char * 64)()
    fake = dict(block_tables=C.addressof(buf), seq_lens=C.addressof(buf), int_ws=C.addressof(buf),
                float_ws=C.addressof(buf))
    ib, _ = workspace_sizes(fi_lib, plan_params())
    assert f"int workspace too small (64 bytes, need {ib})" in error(plan_params(int_ws_bytes=64, **fake))
    assert "head_dim_ckv 256" in error(plan_params(head_dim_ckv=256, **fake))
    assert "head_dim_kpe 32" in error(plan_params(head_dim_kpe=32, **fake))
    assert "dtype mismatch" in error(plan_params(kv_dtype=_lib.FI_DTYPE_F16, **fake))
    assert "unsupported dtype" in error(plan_params(q_dtype=_lib.FI_DTYPE_FP8_E4M3, kv_dtype=_lib.FI_DTYPE_FP8_E4M3,
                                                    **fake))
    assert "unsupported dtype" in error(plan_params(q_dtype=_lib.FI_DTYPE_F32, kv_dtype=_lib.FI_DTYPE_F32, **fake))
    assert "batch_size (0)" in error(plan_params(B=0, **fake))
    assert "q_len_per_request (0)" in error(plan_params(q_len=0, **fake))
    assert "num_heads (0)" in error(plan_params(H=0, **fake))
    assert "rows overlap" in error(plan_params(stride=7, int_ws_bytes=ib, **fake))
    assert "block_tables_stride must fit 31 bits" in error(plan_params(stride=1 << 30, int_ws_bytes=ib, **fake))
    assert "max_blocks x page_size" in error(plan_params(max_blocks=1 << 27, **fake))
    assert "max_items_hint" in error(plan_params(hint=1 << 22, **fake))
    assert fi_lib.fi_batch_mla_plan_device(None, info, None) != 0
    # the same checks guard the sizing entry
    sizes = (C.c_size_t(), C.c_size_t())
    assert fi_lib.fi_batch_mla_plan_device_workspace(C.byref(plan_params(head_dim_ckv=256)), C.byref(sizes[0]),
                                                     C.byref(sizes[1])) != 0
    assert "head_dim_ckv 256" in fi_lib.fi_last_error().decode()


def test_new_sources_do_not_name_the_oracle():
    for rel in ("flashinfer-ai_amd/csrc/mla_plan_device.hip", "flashinfer-ai_amd/csrc/mla_plan.h",
                "flashinfer-ai_amd/csrc/plan_device.h", "flashinfer-ai_amd/flashinfer/_plan_free.py"):
        with open(os.path.join(ROOT, rel)) as f:
            assert "oracle" not in f.read(), rel
