"""CPU: attention sinks.  The test oracle (tests/sink_ref.py: the attention oracle, then a merge with the state
(0, sink * log2 e)) against vectors of the reference's own pure-torch statement, sink_attention_unified
(tests/golden/attention_sink_golden.npz, written by tools/make_attention_sink_golden.py from
tests/test_helpers/sink_attention_reference.py); the Python signatures against the reference's
(tests/golden/attention_sink_signatures.json); the new exports; and the host-side refusals of the two *_run_sinks
entry points, which need no device."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import sink_ref as S

HERE = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = {"h8x2d64": (8, 2, 64), "h4x4d128": (4, 4, 128)}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "attention_sink_golden.npz"), allow_pickle=False)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def requests(gold, mode, shape):
    """[(q, k, v)] per request of a golden case, float32, and the output rows the fixture keeps (None: all).  Every
    mode reads its rows from the shape's one q [18, Hq, D] and k / v [2, 20, Hkv, D], as
    tools/make_attention_sink_golden.py lays out."""
    q, k, v = (t(gold[f"{shape}_{n}"]).float() for n in "qkv")
    if mode == "incremental":  # one query per request, over all of its keys
        return [(q[b][None], k[b], v[b]) for b in range(k.shape[0])], None
    if mode == "prefill":
        return [(q[:18], k[0, :18], v[0, :18])], [0, 1, 9, 16, 17]
    if mode == "chunk":
        return [(q[:2], k[0], v[0])], None
    return [(q[0:1], k[0, :18], v[0, :18]), (q[1:4], k[1], v[1])], None  # varlen


@pytest.mark.parametrize("window_left", [-1, 16])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["incremental", "prefill", "chunk", "varlen"])
def test_oracle_matches_the_reference_statement(gold, mode, shape, causal, window_left):
    """1e-5, the bar tests/test_oracle_ref_golden.py holds oracle/ to: the reference statement runs in float32 (einsum
    + softmax over a few dozen keys, rounding ~1e-6); the oracle runs in float64."""
    sink = t(gold[f"{shape}_sink"])
    reqs, rows = requests(gold, mode, shape)
    assert sink.shape == (SHAPES[shape][0],) and float(sink[0]) == -4.0 and float(sink[-1]) == 6.0
    # decode (incremental mode) has no causal mask to apply: the single query is the last position
    outs = [S.attention_sink_ref(q, k, v, sink, causal=causal and mode != "incremental", window_left=window_left)[0]
            for q, k, v in reqs]
    have = torch.cat(outs).float()
    want = t(gold[f"{mode}_{shape}_o_c{int(causal)}_w{window_left}"])
    torch.testing.assert_close(have if rows is None else have[rows], want, rtol=1e-5, atol=1e-5)


def test_oracle_fold_conventions():
    """The test oracle's own fold (tests/sink_ref.py), not the library: it follows the conventions the GPU tests then
    hold the kernels to -- empty row + finite sink -> (0, sink log2 e); sink = -inf leaves the state alone, the empty
    one included; lse' = log2(2^lse + 2^(sink log2 e)).  It passes without the feature."""
    o = torch.tensor([[[1.0, -2.0]], [[0.0, 0.0]]], dtype=torch.float64)  # rows: a real one, an empty one
    lse = torch.tensor([[3.0], [-5.0e4]], dtype=torch.float64)
    o2, lse2 = S.fold_sink(o, lse, torch.tensor([2.0]))
    s2 = 2.0 * S.LOG2E
    w = 2.0 ** 3.0 / (2.0 ** 3.0 + 2.0 ** s2)
    torch.testing.assert_close(o2[0], o[0] * w)
    torch.testing.assert_close(lse2[0, 0], torch.log2(torch.tensor(2.0 ** 3.0 + 2.0 ** s2, dtype=torch.float64)))
    assert torch.equal(o2[1], torch.zeros(1, 2, dtype=torch.float64)) and float(lse2[1, 0]) == pytest.approx(s2)
    o3, lse3 = S.fold_sink(o, lse, torch.tensor([float("-inf")]))
    assert torch.equal(o3, o) and torch.equal(lse3, lse)


def test_signatures_match_the_reference():
    import flashinfer

    with open(os.path.join(HERE, "attention_sink_signatures.json")) as f:
        want = json.load(f)
    assert len(want) == 3
    for path, names in want.items():
        obj = flashinfer
        for part in path.split(".")[1:]:
            obj = getattr(obj, part)
        have = list(inspect.signature(obj).parameters)
        # the paged prefill run() carries this library's per-head fp8 scale keywords behind the reference's parameters
        extensions = ["scale_q", "scale_k", "scale_v"] if path.endswith("BatchPrefillWithPagedKVCacheWrapper.run") else []
        assert have == names + extensions, path
    assert "sinks" in want["flashinfer.decode.BatchDecodeWithPagedKVCacheWrapper.run"]
    assert "sinks" in want["flashinfer.prefill.BatchPrefillWithPagedKVCacheWrapper.run"]
    assert issubclass(flashinfer.BatchAttentionWithAttentionSinkWrapper, flashinfer.BatchPrefillWithPagedKVCacheWrapper)
    assert flashinfer.BatchAttentionWithAttentionSinkWrapper is flashinfer.attention.BatchAttentionWithAttentionSinkWrapper


def test_exports_and_abi_version(fi_lib):
    from flashinfer import _lib

    for name in ("fi_batch_decode_run_sinks", "fi_batch_prefill_paged_run_sinks"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, name)
    assert fi_lib.fi_abi_version() == 2  # additive: no existing struct or function changed
    with open(os.path.join(os.path.dirname(HERE), "..", "include", "fi_mi355.h")) as f:
        header = f.read()
    assert "fi_batch_decode_run_sinks(" in header and "fi_batch_prefill_paged_run_sinks(" in header
    assert "variants.py:17-53" in header


def test_jit_args_only_for_the_attention_sink_variant():
    from flashinfer._wrapper import is_attention_sink_variant

    sink_args = ["uri", torch.float16, torch.float16, torch.float16, torch.int32, 128, 128, ["sink"], ["float"],
                 ["sm_scale"], ["double"], "AttentionSink", "struct AttentionSink { ... };"]
    assert is_attention_sink_variant(sink_args) and is_attention_sink_variant(tuple(sink_args))
    assert not is_attention_sink_variant(None)
    assert not is_attention_sink_variant(sink_args[:11] + ["FlashSigmoid", ""])
    assert not is_attention_sink_variant(["AttentionSink"])


@pytest.mark.parametrize("q_dtype", [2, 3])  # FI_DTYPE_FP8_E4M3, FI_DTYPE_FP8_E5M2
def test_run_sinks_entry_points_refuse_fp8_queries_before_any_launch(fi_lib, q_dtype):
    """No plan, no workspace, no tensor and no device: the refusal is the first thing the entry point says, so nothing
    can have been launched.  Without sinks the same calls fail on the missing plan instead."""
    from flashinfer import _lib

    sink = (C.c_float * 8)()
    dp = _lib.fi_batch_decode_params_t(num_qo_heads=8, q_dtype=q_dtype)
    assert fi_lib.fi_batch_decode_run_sinks(None, 0, None, 0, None, 0, C.byref(dp), sink, None) != 0
    assert b"attention sinks need f16 / bf16 queries" in fi_lib.fi_last_error()
    assert fi_lib.fi_batch_decode_run_sinks(None, 0, None, 0, None, 0, C.byref(dp), None, None) != 0
    assert b"not a decode plan" in fi_lib.fi_last_error()
    pp = _lib.fi_batch_prefill_params_t(num_qo_heads=8, q_dtype=q_dtype, o_dtype=1)
    assert fi_lib.fi_batch_prefill_paged_run_sinks(None, 0, None, 0, None, 0, C.byref(pp), sink, None) != 0
    assert b"attention sinks need f16 / bf16 queries" in fi_lib.fi_last_error()
    assert fi_lib.fi_batch_prefill_paged_run_sinks(None, 0, None, 0, None, 0, C.byref(pp), None, None) != 0
    assert b"not a prefill plan" in fi_lib.fi_last_error()


def test_run_sinks_refuses_a_192_128_plan(fi_lib):
    from flashinfer import _lib

    info = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)()
    info[15] = 0x4649514b564f  # FI_PREFILL_QKVO_PLAN_MAGIC
    sink = (C.c_float * 8)()
    pp = _lib.fi_batch_prefill_params_t(num_qo_heads=8, q_dtype=1, o_dtype=1)
    assert fi_lib.fi_batch_prefill_paged_run_sinks(None, 0, None, 0, info, len(info), C.byref(pp), sink, None) != 0
    assert b"192 / head_dim_vo 128" in fi_lib.fi_last_error()
