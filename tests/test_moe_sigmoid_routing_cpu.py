"""CPU: the sigmoid routing methods (DeepSeekV3, Llama4) are declared, exported and bound, fi_moe_route_sigmoid validates
on the host without a launch, the Python checks of flashinfer.fused_moe accept and refuse what they should before any
launch, and the oracle and input generator of the GPU tests (tests/moe_sigmoid_ref.py) are sound."""
import ctypes as C
import math
import os

import pytest
import torch

import moe_sigmoid_ref as S
from flashinfer import fused_moe as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_bound_and_exported(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    assert "FI_API int fi_moe_route_sigmoid(" in header
    assert "fi_moe_route_sigmoid" in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, "fi_moe_route_sigmoid")
    assert fi_lib.fi_moe_route_sigmoid.argtypes[0] is C.POINTER(_lib.fi_moe_route_sigmoid_params_t)
    fields = dict(_lib.fi_moe_route_sigmoid_params_t._fields_)
    assert list(fields) == ["logits", "bias", "topk_ids", "topk_weights", "num_tokens", "num_experts", "top_k", "n_group",
                            "topk_group", "routed_scaling_factor", "method", "dtype", "bias_dtype"]
    assert fields["routed_scaling_factor"] is C.c_float
    assert fi_lib.fi_abi_version() == 2  # the change is additive
    assert (_lib.FI_MOE_ROUTING_DEEPSEEK_V3, _lib.FI_MOE_ROUTING_LLAMA4) == (
        int(F.RoutingMethodType.DeepSeekV3), int(F.RoutingMethodType.Llama4)) == (2, 3)


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error
    fn = fi_lib.fi_moe_route_sigmoid

    def params(**kw):
        base = dict(logits=a, bias=a, topk_ids=a, topk_weights=a, num_tokens=4, num_experts=16, top_k=4, n_group=4,
                    topk_group=2, routed_scaling_factor=2.5, method=_lib.FI_MOE_ROUTING_DEEPSEEK_V3,
                    dtype=_lib.FI_DTYPE_F32, bias_dtype=_lib.FI_DTYPE_BF16)
        base.update(kw)
        return _lib.fi_moe_route_sigmoid_params_t(**base)

    def refused(p, message):
        assert fn(C.byref(p), None) != 0 and message in err(), (message, err())

    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("logits", "bias", "topk_ids", "topk_weights"):
        refused(params(**{field: None}), b"null tensor")
    for field in ("num_tokens", "num_experts", "top_k", "n_group", "topk_group"):
        refused(params(**{field: -1}), b"negative")
    refused(params(num_experts=513, n_group=0), b"num_experts 513")
    refused(params(num_experts=0), b"num_experts 0")
    refused(params(top_k=0), b"top_k 0")
    refused(params(top_k=9), b"top_k 9")
    refused(params(top_k=5, num_experts=4, n_group=0), b"top_k 5")
    refused(params(n_group=3), b"num_experts 16 is not a multiple of n_group 3")
    refused(params(n_group=16, topk_group=4), b"num_experts 16 / n_group 16")  # one expert per group
    refused(params(num_experts=130, n_group=65), b"n_group 65")
    refused(params(topk_group=0), b"topk_group 0")
    refused(params(topk_group=5), b"topk_group 5 is not in [1, n_group 4]")
    refused(params(top_k=5, topk_group=1), b"top_k 5 exceeds the 4 experts")
    refused(params(method=_lib.FI_MOE_ROUTING_LLAMA4, top_k=2), b"Llama4 routing takes top_k 1, not 2")
    refused(params(bias=None), b"DeepSeekV3 routing reads bias")
    refused(params(dtype=_lib.FI_DTYPE_F16), b"dtype")
    refused(params(bias_dtype=_lib.FI_DTYPE_F16), b"bias_dtype")
    for method in (0, 1, 4, 5, 6):
        refused(params(method=method), b"routing method")
    # an empty batch returns 0 without a launch and tolerates null pointers, for both methods
    none = dict(logits=None, bias=None, topk_ids=None, topk_weights=None)
    assert fn(C.byref(params(num_tokens=0, **none)), None) == 0
    assert fn(C.byref(params(num_tokens=0, method=_lib.FI_MOE_ROUTING_LLAMA4, top_k=1, **none)), None) == 0
    # fi_moe_route keeps refusing the sigmoid methods: they have an entry point of their own
    route = _lib.fi_moe_route_params_t(logits=a, topk_ids=a, topk_weights=a, num_tokens=4, num_experts=8, top_k=1, method=2,
                                       dtype=_lib.FI_DTYPE_F32)
    assert fi_lib.fi_moe_route(C.byref(route), None) != 0 and b"routing method" in err()


# ---- the Python checks, with the library monkeypatched away -----------------------------------------------------------
def _layer_args(T=3, E=16, top_k=4, H=128, I=128, **over):
    a = dict(
        routing_logits=torch.zeros(T, E), routing_bias=None,
        hidden_states=torch.zeros(T, H, dtype=torch.uint8).view(torch.float8_e4m3fn),
        hidden_states_scale=torch.zeros(T, H // 32, dtype=torch.uint8),
        gemm1_weights=torch.zeros(E, 2 * I, H // 2, dtype=torch.uint8),
        gemm1_weights_scale=torch.zeros(E, (2 * I + 127) // 128 * 128, H // 32, dtype=torch.uint8),
        gemm1_bias=None, gemm1_alpha=None, gemm1_beta=None, gemm1_clamp_limit=None,
        gemm2_weights=torch.zeros(E, H, I // 2, dtype=torch.uint8),
        gemm2_weights_scale=torch.zeros(E, (H + 127) // 128 * 128, I // 32, dtype=torch.uint8),
        gemm2_bias=None, output1_scale_scalar=None, output1_scale_gate_scalar=None, output2_scale_scalar=None,
        num_experts=E, top_k=top_k, n_group=None, topk_group=None, intermediate_size=I, local_expert_offset=0,
        local_num_experts=E, routed_scaling_factor=None)
    a.update(over)
    return a


def _no_library(monkeypatch):
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


class _Reached(Exception):
    pass


BIAS = torch.zeros(16)
ACCEPTED = [
    dict(routing_method_type=2, routing_bias=BIAS, n_group=4, topk_group=2, routed_scaling_factor=2.5),
    dict(routing_method_type=F.RoutingMethodType.DeepSeekV3, routing_bias=BIAS.to(torch.bfloat16), n_group=8, topk_group=8),
    dict(routing_method_type=2, routing_bias=BIAS),                                        # no groups
    dict(routing_method_type=2, routing_bias=BIAS, n_group=0, topk_group=0, routed_scaling_factor=1.0),
    dict(routing_method_type=2, routing_bias=BIAS, n_group=1, topk_group=1, top_k=8),      # Kimi-K2's spelling
    dict(routing_method_type=2, routing_bias=BIAS, n_group=4, topk_group=1, top_k=4),      # top_k == topk_group * epg
    dict(routing_method_type=3, top_k=1),
    dict(routing_method_type=F.RoutingMethodType.Llama4, top_k=1, routed_scaling_factor=1.0,
         routing_logits=torch.zeros(3, 16, dtype=torch.bfloat16)),
]


@pytest.mark.parametrize("over", ACCEPTED, ids=[str(i) for i in range(len(ACCEPTED))])
def test_accepted_spellings_reach_moe_route_with_the_arguments_passed_through(over, monkeypatch):
    _no_library(monkeypatch)
    seen = {}

    def reached(routing_logits, top_k, routing_method_type, **kwargs):
        seen.update(kwargs, top_k=top_k, method=int(routing_method_type), logits=routing_logits)
        raise _Reached

    monkeypatch.setattr(F, "moe_route", reached)
    args = _layer_args(**over)
    with pytest.raises(_Reached):
        F.trtllm_fp4_block_scale_moe(**args)
    assert seen["logits"] is args["routing_logits"] and seen["top_k"] == args["top_k"]
    assert seen["method"] == int(args["routing_method_type"])
    assert seen["routing_bias"] is args["routing_bias"]
    assert (seen["n_group"], seen["topk_group"], seen["routed_scaling_factor"]) == (
        args["n_group"], args["topk_group"], args["routed_scaling_factor"])
    assert sorted(seen) == ["logits", "method", "n_group", "routed_scaling_factor", "routing_bias", "top_k", "topk_group"]


DS = dict(routing_method_type=2, routing_bias=BIAS)
VALUE_ERRORS = [
    ("multiple of n_group", dict(DS, n_group=3, topk_group=2)),
    ("topk_group 5", dict(DS, n_group=4, topk_group=5)),
    ("topk_group 0", dict(DS, n_group=4, topk_group=None)),
    ("top_k 5 exceeds", dict(DS, n_group=4, topk_group=1, top_k=5)),
    ("routing_bias", dict(DS, routing_bias=torch.zeros(15))),
    ("routing_bias", dict(DS, routing_bias=torch.zeros(1, 16))),
    ("routing_bias", dict(DS, routing_bias=torch.zeros(16, dtype=torch.float16))),
    ("without expert groups", dict(DS, topk_group=2)),
    ("without expert groups", dict(DS, n_group=1, topk_group=2)),
    ("negative", dict(DS, n_group=-4, topk_group=2)),
]


@pytest.mark.parametrize("what,over", VALUE_ERRORS, ids=[f"{i}-{w.split()[0]}" for i, (w, _) in enumerate(VALUE_ERRORS)])
def test_inconsistent_routing_arguments_are_value_errors_before_any_launch(what, over, monkeypatch):
    _no_library(monkeypatch)
    args = _layer_args(**over)
    with pytest.raises(ValueError, match=what):
        F.trtllm_fp4_block_scale_moe(**args)
    with pytest.raises(ValueError, match=what):
        F.moe_route(args["routing_logits"], args["top_k"], 2, args["routing_bias"], args["n_group"], args["topk_group"])


REFUSALS = [
    ("routing_method_type DeepSeekV3 needs routing_bias", dict(routing_method_type=2, n_group=4, topk_group=2)),
    ("routing_method_type Llama4", dict(routing_method_type=3, top_k=2)),
    ("routing_bias", dict(routing_method_type=3, top_k=1, routing_bias=BIAS)),
    ("n_group / topk_group", dict(routing_method_type=3, top_k=1, n_group=4)),
    ("n_group / topk_group", dict(routing_method_type=1, topk_group=2)),
    ("routed_scaling_factor", dict(routing_method_type=3, top_k=1, routed_scaling_factor=2.5)),
    ("routing_bias", dict(routing_method_type=0, routing_bias=BIAS)),
    ("n_group 65", dict(DS, n_group=65, topk_group=2, num_experts=130, routing_logits=torch.zeros(3, 130),
                        routing_bias=torch.zeros(130), local_num_experts=16)),
    ("1 expert per group", dict(DS, n_group=16, topk_group=8)),
    ("routing_method_type Unspecified", dict(routing_method_type=6)),
]


@pytest.mark.parametrize("what,over", REFUSALS, ids=[f"{i}-{w.split()[0]}" for i, (w, _) in enumerate(REFUSALS)])
def test_what_is_not_provided_is_refused_by_name_before_any_launch(what, over, monkeypatch):
    _no_library(monkeypatch)
    args = _layer_args(**over)
    with pytest.raises(NotImplementedError, match=what):
        F.trtllm_fp4_block_scale_moe(**args)
    with pytest.raises(NotImplementedError, match=what):
        F.moe_route(args["routing_logits"], args["top_k"], args["routing_method_type"], args["routing_bias"],
                    args["n_group"], args["topk_group"], args["routed_scaling_factor"])


def test_the_routed_call_refuses_the_deepseek_arguments(monkeypatch):
    """No routing runs there, so there is nothing a bias, groups or a scaling factor could act on."""
    _no_library(monkeypatch)
    ids = torch.zeros(3, 4, dtype=torch.int32)
    for what, over in (("routing_bias", dict(routing_bias=BIAS)), ("n_group", dict(n_group=4)),
                       ("n_group / topk_group", dict(topk_group=2)), ("routed_scaling_factor", dict(routed_scaling_factor=2.5))):
        args = _layer_args(routing_method_type=2, **over)
        del args["routing_logits"]
        with pytest.raises(NotImplementedError, match=what):
            F.trtllm_fp4_block_scale_routed_moe(ids, **args)


def test_moe_route_fails_loudly_on_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        F.moe_route(torch.zeros(3, 16), 4, 2, BIAS, 4, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        F.moe_route(torch.zeros(3, 16), 1, 3)


# ---- the oracle and the generator ---------------------------------------------------------------------------------------
def _transcription(logits, bias, n_group, topk_group, top_k, scale):
    """DeepSeekV3 as the formulas read, one row and one expert at a time, in Python floats (fp64)."""
    ids, weights = [], []
    for row in logits.double().tolist():
        E = len(row)
        s = [0.0 if math.isnan(x) else 1.0 / (1.0 + math.exp(-x)) if x > -700 else 0.0 for x in row]
        b = [s[e] + float(bias[e]) for e in range(E)]
        candidates = list(range(E))
        if n_group is not None and n_group > 1:
            epg = E // n_group
            score = []
            for g in range(n_group):
                top = sorted(b[g * epg:(g + 1) * epg], reverse=True)
                score.append(top[0] + top[1])
            kept = sorted(range(n_group), key=lambda g: (-score[g], g))[:topk_group]
            candidates = [e for e in range(E) if e // epg in kept]
        chosen = sorted(candidates, key=lambda e: (-b[e], e))[:top_k]
        total = sum(s[e] for e in chosen)
        ids.append(chosen)
        weights.append([s[e] * (1.0 if scale is None else scale) / (total + 1e-20) for e in chosen])
    return ids, weights


@pytest.mark.parametrize("E,n_group,topk_group,top_k", [(8, 4, 2, 2), (12, 4, 2, 3), (72, 8, 3, 8), (64, None, None, 8),
                                                        (16, 1, 1, 4)])
def test_oracle_agrees_with_a_transcription_of_the_formulas(E, n_group, topk_group, top_k):
    logits, bias, _ = S.sigmoid_case(3, E, n_group, seed=E)
    for scale in (None, 2.5):
        ids, w = S.route_sigmoid_ref(logits, bias, n_group, topk_group, top_k, scale, S.DEEPSEEK_V3)
        want_ids, want_w = _transcription(logits, bias, n_group, topk_group, top_k, scale)
        assert ids.dtype == torch.int32 and ids.tolist() == want_ids
        torch.testing.assert_close(w, torch.tensor(want_w, dtype=torch.float64), rtol=1e-13, atol=0)


def test_oracle_hand_worked():
    ln3 = math.log(3.0)  # sigmoid(ln 3) = 3/4, sigmoid(-ln 3) = 1/4, sigmoid(0) = 1/2
    logits = torch.tensor([[ln3, 0.0, -ln3, 0.0, ln3, ln3, float("nan"), -ln3]], dtype=torch.float64)
    bias = torch.tensor([0.0, 0.0, 1.0, 0.0, -0.5, -0.5, 0.25, 0.0], dtype=torch.float64)
    # b:    3/4  1/2  5/4  1/2 | 1/4  1/4  1/4 (NaN: s = 0)  1/4;   groups of 2: scores 5/4, 7/4, 1/2, 1/2
    ids, w = S.route_sigmoid_ref(logits, bias, 4, 2, 3, 2.0, S.DEEPSEEK_V3)
    assert ids.tolist() == [[2, 0, 1]]  # groups 1 and 0 are kept; 1 and 3 tie at 1/2: the lower expert
    torch.testing.assert_close(w, torch.tensor([[0.25, 0.75, 0.5]], dtype=torch.float64) * 2.0 / 1.5, rtol=1e-14, atol=0)
    # groups 2 and 3 tie: the lower group; its experts 4 and 5 tie: the lower expert; the NaN expert has s = 0
    ids, w = S.route_sigmoid_ref(logits, bias, 4, 3, 6, None, S.DEEPSEEK_V3)
    assert ids.tolist() == [[2, 0, 1, 3, 4, 5]]
    # without groups all 8 are candidates
    ids, _ = S.route_sigmoid_ref(logits, bias, None, None, 8, None, S.DEEPSEEK_V3)
    assert ids.tolist() == [[2, 0, 1, 3, 4, 5, 6, 7]]
    # a bias of -2 on the kept groups makes every candidate negative; groups 1 and 3 are dropped for their second expert
    # and their first, at b = 1/2 and 3/4, still never wins.  top_k = topk_group * epg takes every candidate.
    zeros = torch.zeros(1, 8, dtype=torch.float64)
    bias2 = torch.tensor([-2.0, -2.0, 0.0, -10.0, -2.0, -2.25, 0.25, -20.0], dtype=torch.float64)
    ids, w = S.route_sigmoid_ref(zeros, bias2, 4, 2, 4, None, S.DEEPSEEK_V3)
    assert ids.tolist() == [[0, 1, 4, 5]] and w.tolist() == [[0.25] * 4]
    # Llama4: the largest logit, ties to the lower index, NaN as -inf; the weight is its sigmoid
    ids, w = S.route_sigmoid_ref(logits, None, None, None, 1, None, S.LLAMA4)
    assert ids.tolist() == [[0]] and w.tolist() == [[pytest.approx(0.75, rel=1e-15)]]


CASES = [(8, 4), (12, 4), (16, 4), (72, 8), (256, 8), (384, 12), (512, 4), (512, 16), (128, 64), (128, 2), (384, 1),
         (512, None)]


@pytest.mark.parametrize("E,n_group", CASES)
def test_generated_inputs_keep_the_margin(E, n_group):
    T = 5
    logits, bias, draws = S.sigmoid_case(T, E, n_group, seed=E)
    assert logits.shape == (T, E) and logits.dtype == torch.float32 and bias.shape == (E,) and bias.dtype == torch.float32
    assert torch.equal(bias.to(torch.bfloat16).float(), bias) and bool((bias.abs() <= 0.125).all())
    experts, groups = S.decision_gaps(logits, bias, n_group)
    assert experts >= S.MARGIN and (groups is None) == (not S.grouped(n_group)) and (groups is None or groups >= S.MARGIN)
    assert draws <= (40 if n_group == 64 else 3) * T  # the margin costs few draws: the inputs are not cherry-picked
    again = S.sigmoid_case(T, E, n_group, seed=E)
    assert torch.equal(again[0], logits) and torch.equal(again[1], bias)  # deterministic
    # a torch f32 evaluation of the scores picks the oracle's experts
    b32 = torch.sigmoid(logits) + bias
    assert b32.dtype == torch.float32
    topk_group = max(1, n_group // 2) if S.grouped(n_group) else None
    want = S.choose_ref(S.scores_ref(logits, bias)[1], n_group, topk_group, 2)
    assert torch.equal(S.choose_ref(b32, n_group, topk_group, 2), want)


def test_generated_bf16_inputs_keep_the_margin():
    for E, n_group in ((64, 8), (16, 4)):
        logits, bias, _ = S.sigmoid_case(5, E, n_group, seed=E, dtype=torch.bfloat16)
        assert logits.dtype == torch.bfloat16
        experts, groups = S.decision_gaps(logits, bias, n_group)
        assert experts >= S.MARGIN and groups >= S.MARGIN
