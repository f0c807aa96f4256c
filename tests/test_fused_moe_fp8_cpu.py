"""CPU: flashinfer.fused_moe_fp8.trtllm_fp8_block_scale_moe has the reference's signature and refuses what is not provided by
name before any device access; the new fi_* entry points validate on the host without a launch; and the fp64 oracle of
the GPU tests (tests/moe_fp8_ref.py) agrees with the reference test's dequantisation written out as a formula and with
hand-made blocks of the quantisation rule."""
import ctypes as C
import inspect
import os

import pytest
import torch

import moe_fp8_ref as R8
from flashinfer import fp8_quantization as Q
from flashinfer import fused_moe as F
from flashinfer import fused_moe_fp8 as F8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3 = torch.float8_e4m3fn


def _fp8_zeros(*shape):
    return torch.zeros(*shape, dtype=torch.uint8).view(E4M3)


def _layer_args(T=3, E=8, top_k=2, H=256, I=128, G=None, offset=0, **over):
    """Arguments of trtllm_fp8_block_scale_moe on CPU tensors of valid shapes and dtypes (Default routing)."""
    G = E if G is None else G
    a = dict(
        routing_logits=torch.zeros(T, E), routing_bias=None, hidden_states=_fp8_zeros(T, H),
        hidden_states_scale=torch.ones(H // 128, T), gemm1_weights=_fp8_zeros(G, 2 * I, H),
        gemm1_weights_scale=torch.ones(G, 2 * I // 128, H // 128), gemm2_weights=_fp8_zeros(G, H, I),
        gemm2_weights_scale=torch.ones(G, H // 128, I // 128), num_experts=E, top_k=top_k, n_group=None, topk_group=None,
        intermediate_size=I, local_expert_offset=offset, local_num_experts=G, routed_scaling_factor=None)
    a.update(over)
    return a


def _no_device(monkeypatch):
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def test_signature_is_the_references_and_the_call_is_exported():
    import flashinfer

    # ref: flashinfer/fused_moe/core.py:1742-1764
    want = [("routing_logits",), ("routing_bias",), ("hidden_states",), ("hidden_states_scale",), ("gemm1_weights",),
            ("gemm1_weights_scale",), ("gemm2_weights",), ("gemm2_weights_scale",), ("num_experts",), ("top_k",),
            ("n_group",), ("topk_group",), ("intermediate_size",), ("local_expert_offset",), ("local_num_experts",),
            ("routed_scaling_factor",), ("tile_tokens_dim", 8), ("routing_method_type", 0), ("use_shuffled_weight", False),
            ("weight_layout", 0), ("enable_pdl", None)]
    got = [(p.name,) if p.default is inspect.Parameter.empty else (p.name, p.default)
           for p in inspect.signature(F8.trtllm_fp8_block_scale_moe).parameters.values()]
    assert got == want
    # the call is a module of its own: flashinfer.fused_moe and the top level keep the MXFP4 layer's names only
    assert flashinfer.fused_moe_fp8 is F8 and F8.__name__ == "flashinfer.fused_moe_fp8"
    assert not hasattr(flashinfer, "trtllm_fp8_block_scale_moe") and not hasattr(F, "trtllm_fp8_block_scale_moe")
    assert flashinfer.fp8_quantization.fp8_quantize_1x128 is Q.fp8_quantize_1x128
    for fn in (F.moe_permute_fp8_block, F.moe_gated_act_fp8_block, Q.fp8_quantize_1x128):
        assert "Not part of the reference" in fn.__doc__
    assert not hasattr(F8, "trtllm_fp8_per_tensor_scale_moe")  # stays out


REFUSALS = [
    (NotImplementedError, "use_shuffled_weight", dict(use_shuffled_weight=True)),
    (NotImplementedError, "weight_layout", dict(weight_layout=1)),
    (NotImplementedError, "weight_layout", dict(weight_layout=2)),
    (ValueError, "tile_tokens_dim", dict(tile_tokens_dim=0)),
    (ValueError, "tile_tokens_dim", dict(tile_tokens_dim="8")),
    (ValueError, "enable_pdl", dict(enable_pdl=1)),
    (NotImplementedError, "routing_method_type", dict(routing_method_type=6)),
    (NotImplementedError, "routing_method_type", dict(routing_method_type=9)),
    (NotImplementedError, "routing_method_type DeepSeekV3", dict(routing_method_type=2)),
    (NotImplementedError, "routing_method_type Llama4", dict(routing_method_type=3)),
    (NotImplementedError, "routing_bias", dict(routing_bias=torch.zeros(8))),
    (NotImplementedError, "n_group", dict(n_group=4, topk_group=2)),
    (NotImplementedError, "routed_scaling_factor", dict(routed_scaling_factor=2.5)),
    (ValueError, "topk_group", dict(routing_method_type=2, routing_bias=torch.zeros(8), n_group=4, topk_group=5)),
    (NotImplementedError, "top_k", dict(top_k=9, num_experts=16, routing_logits=torch.zeros(3, 16), local_num_experts=8)),
    (NotImplementedError, "num_experts", dict(num_experts=513, routing_logits=torch.zeros(3, 513))),
    (NotImplementedError, "hidden_states has dtype", dict(hidden_states=torch.zeros(3, 256, dtype=torch.bfloat16))),
    (NotImplementedError, "hidden size 192", dict(hidden_states=_fp8_zeros(3, 192))),
    (NotImplementedError, "hidden_states_scale", dict(hidden_states_scale=None)),
    (NotImplementedError, "hidden_states_scale", dict(hidden_states_scale=torch.ones(2, 3, dtype=torch.bfloat16))),
    (ValueError, "hidden_states_scale", dict(hidden_states_scale=torch.ones(3, 2))),  # [T, H / 128]: pass its .t()
    (NotImplementedError, "intermediate_size", dict(intermediate_size=96)),
    (NotImplementedError, "gemm1_weights ", dict(gemm1_weights=torch.zeros(8, 256, 256, dtype=torch.uint8))),
    (NotImplementedError, "gemm1_weights ", dict(gemm1_weights=_fp8_zeros(8, 128, 256))),
    (NotImplementedError, "gemm1_weights_scale", dict(gemm1_weights_scale=torch.ones(8, 2, 2, dtype=torch.bfloat16))),
    (NotImplementedError, "gemm1_weights_scale", dict(gemm1_weights_scale=torch.ones(8, 2, 1))),
    (NotImplementedError, "gemm2_weights ", dict(gemm2_weights=_fp8_zeros(8, 128, 256))),
    (NotImplementedError, "gemm2_weights_scale", dict(gemm2_weights_scale=torch.ones(8, 1, 2))),
    (ValueError, "gemm2_weights must be contiguous", dict(gemm2_weights=_fp8_zeros(8, 128, 256).transpose(1, 2))),
    (ValueError, "local experts", dict(G=4, offset=6)),
    (ValueError, "routing_logits", dict(routing_logits=torch.zeros(3, 7))),
    (NotImplementedError, "routing_logits", dict(routing_logits=torch.zeros(3, 8, dtype=torch.float16))),
]


@pytest.mark.parametrize("kind,match,over", REFUSALS, ids=[f"{i}-{m.split()[0]}" for i, (_, m, _) in enumerate(REFUSALS)])
def test_refusals_happen_before_any_device_access(kind, match, over, monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(kind, match=match):
        F8.trtllm_fp8_block_scale_moe(**_layer_args(**over))


def test_accepted_spellings_reach_the_first_stage(monkeypatch):
    _no_device(monkeypatch)

    def reached(*args, **kwargs):
        raise AssertionError("the first stage was reached")

    monkeypatch.setattr(F8, "moe_route", reached)
    transposed = torch.ones(3, 2).t()  # the reference test's spelling: [T, H / 128] transposed, strides (1, 2)
    assert transposed.stride() == (1, 2)
    for over in (dict(), dict(hidden_states_scale=transposed), dict(tile_tokens_dim=64, enable_pdl=True),
                 dict(n_group=0, topk_group=0, routed_scaling_factor=1.0), dict(routing_method_type=1), dict(G=3, offset=2),
                 dict(routing_logits=torch.zeros(3, 8, dtype=torch.bfloat16), routing_method_type=5),
                 dict(routing_method_type=2, routing_bias=torch.zeros(8), n_group=4, topk_group=2, routed_scaling_factor=2.5),
                 dict(routing_method_type=3, top_k=1), dict(weight_layout=0, use_shuffled_weight=False)):
        with pytest.raises(AssertionError, match="the first stage was reached"):
            F8.trtllm_fp8_block_scale_moe(**_layer_args(**over))


def test_an_empty_batch_returns_an_empty_tensor_without_a_launch(monkeypatch):
    _no_device(monkeypatch)
    out = F8.trtllm_fp8_block_scale_moe(**_layer_args(T=0))
    assert isinstance(out, torch.Tensor) and out.shape == (0, 256) and out.dtype == torch.bfloat16


def test_device_ops_fail_loudly_on_cpu_tensors():
    args = _layer_args()
    ids = torch.zeros(3, 2, dtype=torch.int32)
    calls = [
        lambda: F8.trtllm_fp8_block_scale_moe(**args),
        lambda: F.moe_permute_fp8_block(ids, args["hidden_states"], args["hidden_states_scale"], 0, 8),
        lambda: F.moe_gated_act_fp8_block(torch.zeros(4, 256, dtype=torch.bfloat16), torch.zeros(9, dtype=torch.int32)),
        lambda: Q.fp8_quantize_1x128(torch.zeros(3, 128, dtype=torch.bfloat16)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_stage_functions_check_their_arguments(monkeypatch):
    _no_device(monkeypatch)
    ids = torch.zeros(3, 2, dtype=torch.int32)
    x, s = _fp8_zeros(3, 256), torch.ones(2, 3)
    for call, kind, match in (
            (lambda: F.moe_permute_fp8_block(ids.long(), x, s, 0, 8), ValueError, "topk_ids"),
            (lambda: F.moe_permute_fp8_block(ids, x, torch.ones(3, 2), 0, 8), ValueError, "hidden_states_scale"),
            (lambda: F.moe_permute_fp8_block(ids, x, s.double(), 0, 8), NotImplementedError, "hidden_states_scale"),
            (lambda: F.moe_permute_fp8_block(ids[:2], x, s, 0, 8), ValueError, "rows"),
            (lambda: F.moe_permute_fp8_block(ids, x, s, 0, 513), NotImplementedError, "local_num_experts"),
            (lambda: F.moe_gated_act_fp8_block(torch.zeros(4, 256), torch.zeros(9, dtype=torch.int32)), ValueError, "bfloat16"),
            (lambda: F.moe_gated_act_fp8_block(torch.zeros(4, 192, dtype=torch.bfloat16), torch.zeros(9, dtype=torch.int32)),
             NotImplementedError, "multiple of 128"),
            (lambda: F.moe_gated_act_fp8_block(torch.zeros(4, 256, dtype=torch.bfloat16), torch.zeros(9)), ValueError, "m_indptr"),
            (lambda: Q.fp8_quantize_1x128(torch.zeros(3, 128)), ValueError, "dtype"),
            (lambda: Q.fp8_quantize_1x128(torch.zeros(3, 96, dtype=torch.bfloat16)), ValueError, "multiple of 128"),
            (lambda: Q.fp8_quantize_1x128(torch.zeros(128, dtype=torch.bfloat16)), ValueError, "2D")):
        with pytest.raises(kind, match=match):
            call()
    # empty problems return their shapes without a launch
    q, sc = Q.fp8_quantize_1x128(torch.zeros(0, 256, dtype=torch.bfloat16))
    assert (q.shape, sc.shape, q.dtype, sc.dtype) == ((0, 256), (2, 0), E4M3, torch.float32)
    q, sc = F.moe_gated_act_fp8_block(torch.zeros(0, 256, dtype=torch.bfloat16), torch.zeros(9, dtype=torch.int32))
    assert (q.shape, sc.shape) == ((0, 128), (0, 1))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
SYMBOLS = {"fi_moe_permute_fp8_block": "fi_moe_permute_fp8_block_params_t",
           "fi_moe_gated_act_fp8_block": "fi_moe_gated_act_fp8_block_params_t",
           "fi_fp8_quantize_1x128": "fi_fp8_quantize_1x128_params_t"}


def test_symbols_are_declared_bound_and_exported(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    for name, struct in SYMBOLS.items():
        assert f"FI_API int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, name), name
        assert getattr(fi_lib, name).argtypes[0] is C.POINTER(getattr(_lib, struct))
    assert fi_lib.fi_abi_version() == 2  # the change is additive
    makefile = open(os.path.join(ROOT, "flashinfer-ai_amd", "csrc", "Makefile")).read()
    assert " fp8_block_quantize" in [l for l in makefile.splitlines() if l.startswith("PLAIN_SRCS")][0]


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error

    def refused(fn, params, message):
        assert fn(C.byref(params), None) != 0 and message in err(), (message, err())

    # ---- permute: 4 tokens x top_k 2, 3 local experts
    def permute(**kw):
        base = dict(topk_ids=a, x=a, x_scale=a, m_indptr=a, expanded_to_permuted=a, x_permuted=a, scale_permuted=a,
                    unpacked_weights=None, workspace=a, scale_stride_kb=4, scale_stride_t=1, workspace_bytes=1 << 20,
                    num_tokens=4, top_k=2, hidden=128, local_expert_offset=0, local_num_experts=3, packed=0)
        base.update(kw)
        return _lib.fi_moe_permute_fp8_block_params_t(**base)

    fn = fi_lib.fi_moe_permute_fp8_block
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("topk_ids", "x", "x_scale", "m_indptr", "expanded_to_permuted", "x_permuted", "scale_permuted", "workspace"):
        refused(fn, permute(**{field: None}), b"null tensor")
    for field in ("num_tokens", "top_k", "hidden", "local_expert_offset", "local_num_experts"):
        refused(fn, permute(**{field: -1}), b"negative")
    for field in ("scale_stride_kb", "scale_stride_t"):
        refused(fn, permute(**{field: -1}), b"negative stride")
    refused(fn, permute(local_num_experts=513), b"local_num_experts 513")
    refused(fn, permute(top_k=9), b"top_k 9")
    refused(fn, permute(top_k=0), b"top_k 0")
    for hidden in (0, 96, 160):
        refused(fn, permute(hidden=hidden), b"multiple of 128")
    refused(fn, permute(x=a + 8), b"aligned")
    refused(fn, permute(x_permuted=a + 8), b"aligned")
    refused(fn, permute(x_scale=a + 2), b"aligned")
    refused(fn, permute(workspace_bytes=43), b"workspace holds 43 bytes, 44 needed")  # (1 block * 3 + 8) * 4
    none = dict(topk_ids=None, x=None, x_scale=None, m_indptr=None, expanded_to_permuted=None, x_permuted=None,
                scale_permuted=None, workspace=None)
    assert fn(C.byref(permute(num_tokens=0, **none)), None) == 0

    # ---- gated activation
    def act(**kw):
        base = dict(x=a, m_indptr=a, q=a, scale=a, cum_m=8, intermediate=256, num_groups=3)
        base.update(kw)
        return _lib.fi_moe_gated_act_fp8_block_params_t(**base)

    fn = fi_lib.fi_moe_gated_act_fp8_block
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("x", "m_indptr", "q", "scale"):
        refused(fn, act(**{field: None}), b"null tensor")
    for field in ("cum_m", "intermediate", "num_groups"):
        refused(fn, act(**{field: -1}), b"negative")
    refused(fn, act(num_groups=0), b"num_groups 0")
    refused(fn, act(num_groups=513), b"num_groups 513")
    for inter in (0, 64, 192):
        refused(fn, act(intermediate=inter), b"multiple of 128")
    refused(fn, act(x=a + 8), b"aligned")
    refused(fn, act(q=a + 4), b"aligned")
    assert fn(C.byref(act(cum_m=0, x=None, m_indptr=None, q=None, scale=None)), None) == 0

    # ---- quantiser
    def quant(**kw):
        base = dict(input=a, q=a, scale=a, input_stride=256, m=4, k=256, dtype=_lib.FI_DTYPE_BF16)
        base.update(kw)
        return _lib.fi_fp8_quantize_1x128_params_t(**base)

    fn = fi_lib.fi_fp8_quantize_1x128
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("input", "q", "scale"):
        refused(fn, quant(**{field: None}), b"null tensor")
    for field in ("m", "k"):
        refused(fn, quant(**{field: -1}), b"negative")
    refused(fn, quant(k=96, input_stride=96), b"multiple of 128")
    refused(fn, quant(dtype=_lib.FI_DTYPE_F32), b"dtype")
    refused(fn, quant(input_stride=128), b"stride")
    refused(fn, quant(input_stride=260), b"aligned")
    refused(fn, quant(input=a + 8), b"aligned")
    assert fn(C.byref(quant(m=0, input=None, q=None, scale=None)), None) == 0


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_oracle_dequantisation_is_the_reference_tests_formula():
    """dequant_reference_dsfp8 (tests/moe/test_trtllm_gen_fused_moe.py:1458-1481, used at :1720-1734): a weight element
    times the scale of its 128 x 128 block; an activation element times scale[column / 128, token] (the scale tensor is
    [H / 128, T] and transposed before use).  Written out element by element on a 2-expert case."""
    g = torch.Generator().manual_seed(1)
    G, n, k, T = 2, 256, 384, 5
    w = torch.randint(0, 256, (G, n, k), dtype=torch.uint8, generator=g)
    w[(w & 0x7F) == 0x7F] = 0  # no NaN bytes
    w = w.view(E4M3)
    ws = torch.rand(G, n // 128, k // 128, generator=g) + 0.5
    got = R8.dequant_weights(w, ws)
    wf = w.to(torch.float32).double()
    for e in range(G):
        for i in (0, 1, 127, 128, 255):
            for j in (0, 127, 128, 129, 255, 256, 383):
                assert got[e, i, j].item() == wf[e, i, j].item() * float(ws[e, i // 128, j // 128])
    x = torch.randint(0, 120, (T, k), dtype=torch.uint8, generator=g).view(E4M3)
    # the scales as the reference's test holds them: a [T, H / 128] tensor, passed as its transposed view
    xs_tk = torch.rand(T, k // 128, generator=g) + 0.5
    for scale in (xs_tk.t(), xs_tk.t().contiguous()):
        got = R8.dequant_activations(x, scale)
        xf = x.to(torch.float32).double()
        for t in range(T):
            for j in (0, 127, 128, 255, 256, 383):
                assert got[t, j].item() == xf[t, j].item() * float(xs_tk[t, j // 128])
    # row-major scales of a permuted operand
    rows = R8.dequant_rows(x, xs_tk)
    assert torch.equal(rows, R8.dequant_activations(x, xs_tk.t()))


def _bytes(q):
    return q.view(torch.uint8)


def test_block_rule_on_hand_made_blocks():
    """s = max(amax / 448, 2^-126), q = e4m3(clamp(x / s, -448, 448)) per row and 128 columns."""
    x = torch.zeros(6, 256, dtype=torch.float64)
    # row 0: an all-zero block beside a live one
    x[0, 128:] = 1.0
    # row 1: amax exactly 448 * 2^e (e = -3 and e = 5): the scale is the power of two, the maximum becomes 448 = 0x7E
    x[1, 5], x[1, 6] = 448 * 2.0 ** -3, -2.0 ** -3
    x[1, 128 + 9], x[1, 128 + 10] = -448 * 2.0 ** 5, 3 * 2.0 ** 5
    # row 2: a value whose quotient rounds up to 448: amax 7, the value 6.9 -> 6.9 / (7 / 448) = 441.6, between 416 and 448
    x[2, 0], x[2, 1], x[2, 2] = 7.0, 6.9, 6.7  # 6.7 -> 428.8 rounds down to 416
    # row 3: bf16-sized inputs whose amax / 448 is no power of two
    x[3, :128] = torch.arange(128, dtype=torch.float64) / 64 - 1
    # row 4: a tiny block: amax / 448 is below the floor, the scale is 2^-126 and the bytes are subnormal or zero
    x[4, 3] = 2.0 ** -130
    x[4, 128 + 3] = 2.0 ** -118
    q, s = R8.block_quantize_ref(x)
    qb = _bytes(q)
    assert s.dtype == torch.float64 and s.shape == (6, 2) and q.dtype == E4M3
    assert s[0, 0].item() == 2.0 ** -126 and not qb[0, :128].any()
    assert s[0, 1].item() == 1 / 448 and bool((qb[0, 128:] == 0x7E).all())
    assert s[1, 0].item() == 2.0 ** -3 and qb[1, 5].item() == 0x7E and q[1, 6].float().item() == -1.0
    assert s[1, 1].item() == 2.0 ** 5 and qb[1, 128 + 9].item() == 0xFE and q[1, 128 + 10].float().item() == 3.0
    assert s[2, 0].item() == 7 / 448 and qb[2, 0].item() == 0x7E and qb[2, 1].item() == 0x7E and q[2, 2].float().item() == 416.0
    assert s[3, 0].item() == 1 / 448 and q[3, 0].float().item() == -448.0 and s[3, 1].item() == 2.0 ** -126
    assert s[4, 0].item() == 2.0 ** -126 and q[4, 3].float().item() == 2.0 ** -4
    assert s[4, 1].item() == 2.0 ** -126 and q[4, 128 + 3].float().item() == 256.0
    assert s[5].tolist() == [2.0 ** -126] * 2 and not qb[5].any()
    assert not bool(((qb & 0x7F) == 0x7F).any())  # no NaN byte anywhere
    # the f32 scale of the device: the correctly rounded quotient of the exact amax
    q32, s32 = R8.block_quantize_ref(x, torch.float32)
    assert s32.dtype == torch.float32 and s32[2, 0].item() == (torch.tensor(7.0) / 448).item()
    assert torch.equal(s32.double()[[1, 4, 5]], s[[1, 4, 5]])  # powers of two are exact in both
    # a quotient one ulp above 448 is clamped, not NaN: 448 / s32 with s32 rounded down
    y = torch.tensor([448.0000001, -449.0, 1e9])
    assert _bytes(R8.to_e4m3(y.double())).tolist() == [0x7E, 0xFE, 0x7E]


def test_near_rounding_boundary_marks_the_midpoints_only():
    # e4m3 around 17: values 16, 18 (step 2); the midpoint is 17
    y = torch.tensor([17.0, 17.0 * (1 + 2.0 ** -21), 17.0 * (1 + 2.0 ** -18), 16.0, 18.0, 0.0, 2.0 ** -10, 447.999999, 432.0],
                     dtype=torch.float64)
    assert R8.near_rounding_boundary(y).tolist() == [True, True, False, False, False, False, True, False, True]
    assert R8.e4m3_step(torch.tensor([0.001, 2.0 ** -6, 1.0, 17.0, 448.0], dtype=torch.float64)).tolist() == [
        2.0 ** -9, 2.0 ** -9, 0.125, 2.0, 32.0]


def test_quantiser_inputs_keep_clear_of_the_rounding_boundaries():
    """The oracle side of the GPU test of fp8_quantize_1x128: with the scale bit-equal, the device's byte may differ from
    the oracle's only where the fp64 quotient lies within 2^-20 of a rounding boundary; on the chosen inputs that is at
    most 1 % of the elements (bf16 inputs make exact ties likelier than real data would: x / s with s = amax / 448)."""
    for T, H in R8.QUANT_SHAPES:
        x = R8.quantiser_input(T, H)
        q, s = R8.block_quantize_ref(x, torch.float32)
        y = x.double().view(T, H // 128, 128) / s.double().unsqueeze(-1)
        share = R8.near_rounding_boundary(y).double().mean().item()
        assert share <= 0.01, (T, H, share)
        assert torch.equal(s, torch.clamp(x.float().view(T, H // 128, 128).abs().amax(-1) / 448, min=2.0 ** -126))

