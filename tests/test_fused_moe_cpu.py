"""CPU: flashinfer.fused_moe has the reference's surface for its MXFP8 x MXFP4 mode and refuses the rest by name before
any launch, every fi_moe_* entry point validates on the host without a launch, and the fp64 oracle of the GPU tests
(tests/moe_ref.py) agrees with hand-worked cases."""
import ctypes as C
import inspect
import json
import math
import os

import pytest
import torch

import moe_ref as M
from flashinfer import fused_moe as F  # the module under test: without it nothing here is collected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fused_moe_signatures.json")
NAMES = ["GatedActType", "RoutingMethodType", "trtllm_fp4_block_scale_moe", "trtllm_fp4_block_scale_routed_moe"]
SYMBOLS = ("fi_moe_route", "fi_moe_permute_mxfp8", "fi_moe_gated_act_mxfp8", "fi_moe_finalize")


def _params(fn):
    return [
        {"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
        for p in inspect.signature(fn).parameters.values()
    ]


def test_signatures_and_enums_match_the_reference():
    import flashinfer

    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == ["fused_moe"]
    entry = g["fused_moe"]
    assert flashinfer.fused_moe is F and F.__name__ == "flashinfer.fused_moe"
    assert sorted(entry["functions"]) == NAMES[2:] and entry["top_level"] == NAMES
    for name, params in entry["functions"].items():
        assert _params(getattr(F, name)) == params, name
        assert len(params) == 31 and [p["name"] for p in params[-7:]] == [
            "tile_tokens_dim", "routing_method_type", "do_finalize", "enable_pdl", "gated_act_type", "output",
            "tune_max_num_tokens"]
    assert _params(F.trtllm_fp4_block_scale_moe)[0] == {"name": "routing_logits"}
    assert _params(F.trtllm_fp4_block_scale_routed_moe)[0] == {"name": "topk_ids"}
    assert _params(F.trtllm_fp4_block_scale_moe)[1:] == _params(F.trtllm_fp4_block_scale_routed_moe)[1:]
    for name, members in entry["enums"].items():
        enum = getattr(F, name)
        assert {m.name: int(m) for m in enum} == members, name
    assert {m.name: int(m) for m in F.RoutingMethodType} == {
        "Default": 0, "Renormalize": 1, "DeepSeekV3": 2, "Llama4": 3, "RenormalizeNaive": 4, "TopK": 5, "Unspecified": 6}
    assert {m.name: int(m) for m in F.GatedActType} == {"SwiGlu": 0, "GeGlu": 1}
    for name in NAMES:
        assert getattr(flashinfer, name) is getattr(F, name), name
    for name in ("moe_route", "moe_permute_mxfp8", "moe_gated_act_mxfp8", "moe_finalize"):
        assert callable(getattr(F, name)) and "Not part of the reference" in getattr(F, name).__doc__, name
    for name in ("cutlass_fused_moe", "trtllm_fp8_block_scale_moe", "trtllm_fp8_per_tensor_scale_moe",
                 "reorder_rows_for_gated_act_gemm", "shuffle_matrix_a", "shuffle_matrix_sf_a"):
        assert not hasattr(flashinfer, name) and not hasattr(F, name), name


def _layer_args(T=3, E=8, top_k=2, H=128, I=128, G=None, offset=0, **over):
    """Positional arguments of trtllm_fp4_block_scale_moe on CPU tensors of valid shapes and dtypes."""
    G = E if G is None else G
    a = dict(
        routing_logits=torch.zeros(T, E), routing_bias=None,
        hidden_states=torch.zeros(T, H, dtype=torch.uint8).view(torch.float8_e4m3fn),
        hidden_states_scale=torch.zeros(T, H // 32, dtype=torch.uint8),
        gemm1_weights=torch.zeros(G, 2 * I, H // 2, dtype=torch.uint8),
        gemm1_weights_scale=torch.zeros(G, (2 * I + 127) // 128 * 128, H // 32, dtype=torch.uint8),
        gemm1_bias=None, gemm1_alpha=None, gemm1_beta=None, gemm1_clamp_limit=None,
        gemm2_weights=torch.zeros(G, H, I // 2, dtype=torch.uint8),
        gemm2_weights_scale=torch.zeros(G, (H + 127) // 128 * 128, I // 32, dtype=torch.uint8),
        gemm2_bias=None, output1_scale_scalar=None, output1_scale_gate_scalar=None, output2_scale_scalar=None,
        num_experts=E, top_k=top_k, n_group=None, topk_group=None, intermediate_size=I, local_expert_offset=offset,
        local_num_experts=G, routed_scaling_factor=None)
    a.update(over)
    return a


def _no_library(monkeypatch):
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


REFUSALS = [
    ("routing_bias", dict(routing_bias=torch.zeros(8))),
    ("n_group", dict(n_group=2)),
    ("n_group / topk_group", dict(topk_group=1)),
    ("routed_scaling_factor", dict(routed_scaling_factor=2.5)),
    ("output1_scale_scalar", dict(output1_scale_scalar=torch.ones(8))),
    ("output1_scale_gate_scalar", dict(output1_scale_gate_scalar=torch.ones(8))),
    ("output2_scale_scalar", dict(output2_scale_scalar=torch.ones(8))),
    ("gated_act_type", dict(gated_act_type=1)),
    ("routing_method_type DeepSeekV3", dict(routing_method_type=2)),
    ("routing_method_type Llama4", dict(routing_method_type=3)),
    ("routing_method_type", dict(routing_method_type=6)),
    ("routing_method_type", dict(routing_method_type=9)),
    ("hidden_states in bfloat16.*mxfp8_quantize", dict(hidden_states=torch.zeros(3, 128, dtype=torch.bfloat16))),
    ("hidden_states.*nvfp4", dict(hidden_states=torch.zeros(3, 64, dtype=torch.uint8))),
    ("hidden_states_scale", dict(hidden_states_scale=None)),
    ("hidden_states_scale", dict(hidden_states_scale=torch.zeros(3, 4))),
    ("hidden_states", dict(hidden_states=torch.zeros(3, 96, dtype=torch.uint8).view(torch.float8_e4m3fn),
                           hidden_states_scale=torch.zeros(3, 3, dtype=torch.uint8))),
    ("intermediate_size", dict(intermediate_size=96)),
    ("num_experts", dict(num_experts=513, routing_logits=torch.zeros(3, 513))),
    ("top_k", dict(top_k=9, num_experts=16, routing_logits=torch.zeros(3, 16), local_num_experts=8)),
    ("top_k", dict(top_k=0)),
    ("routing_logits", dict(routing_logits=torch.zeros(3, 8, dtype=torch.float16))),
    ("gemm1_weights ", dict(gemm1_weights=torch.zeros(8, 256, 64, dtype=torch.int8))),
    ("gemm1_weights_scale", dict(gemm1_weights_scale=torch.zeros(8, 256, 4))),
    ("gemm2_weights ", dict(gemm2_weights=torch.zeros(8, 128, 128, dtype=torch.uint8))),
    ("gemm2_weights_scale", dict(gemm2_weights_scale=torch.zeros(8, 128, 2, dtype=torch.uint8))),
    ("gemm2_bias", dict(gemm2_bias=torch.zeros(8, 128), do_finalize=False)),
]


@pytest.mark.parametrize("names,over", REFUSALS, ids=[f"{i}-{n.split('.')[0].strip()}" for i, (n, _) in enumerate(REFUSALS)])
def test_everything_else_is_refused_by_name_before_any_launch(names, over, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=names):
        F.trtllm_fp4_block_scale_moe(**_layer_args(**over))
    if "routing_method_type" in over or "routing_logits" in over:
        return  # the routed call has no logits and does not use the method
    args = _layer_args(**over)
    del args["routing_logits"]
    with pytest.raises(NotImplementedError, match=names):
        F.trtllm_fp4_block_scale_routed_moe(torch.zeros(3, args["top_k"], dtype=torch.int32), **args)


def test_accepted_spellings_reach_the_library(monkeypatch):
    """routed_scaling_factor 1.0, scale bytes as float8_e4m3fn, a flat scale tensor, the ignored tuning knobs: all pass the
    Python checks (the first stage is reached)."""
    _no_library(monkeypatch)

    def reached(*args, **kwargs):
        raise AssertionError("the first stage was reached")

    monkeypatch.setattr(F, "moe_route", reached)
    sf8 = torch.zeros(3 * 4, dtype=torch.uint8).view(torch.float8_e4m3fn)
    for over in (dict(), dict(routed_scaling_factor=1.0), dict(hidden_states_scale=sf8), dict(tile_tokens_dim=64),
                 dict(tune_max_num_tokens=1, enable_pdl=True), dict(routing_method_type=F.RoutingMethodType.TopK),
                 dict(routing_logits=torch.zeros(3, 8, dtype=torch.bfloat16), routing_method_type=4),
                 dict(G=3, offset=2), dict(gemm1_bias=torch.zeros(8, 256), gemm1_alpha=torch.ones(8),
                                          gemm1_beta=torch.ones(8), gemm1_clamp_limit=torch.ones(8),
                                          gemm2_bias=torch.zeros(8, 128))):
        with pytest.raises(AssertionError, match="the first stage was reached"):
            F.trtllm_fp4_block_scale_moe(**_layer_args(**over))
    # shapes are checked too, as ValueError
    for over, what in ((dict(routing_logits=torch.zeros(3, 7)), "routing_logits"),
                       (dict(gemm1_bias=torch.zeros(8, 128)), "gemm1_bias"),
                       (dict(gemm1_alpha=torch.ones(7)), "gemm1_alpha"),
                       (dict(gemm2_bias=torch.zeros(8, 128, dtype=torch.bfloat16)), "gemm2_bias"),
                       (dict(output=torch.zeros(3, 128)), "output"),
                       (dict(G=4, offset=6), "local experts"),
                       (dict(hidden_states_scale=torch.zeros(3, 5, dtype=torch.uint8)), "hidden_states_scale")):
        with pytest.raises(ValueError, match=what):
            F.trtllm_fp4_block_scale_moe(**_layer_args(**over))


def test_an_empty_batch_returns_empty_tensors_without_a_launch(monkeypatch):
    _no_library(monkeypatch)
    (out,) = F.trtllm_fp4_block_scale_moe(**_layer_args(T=0))
    assert out.shape == (0, 128) and out.dtype == torch.bfloat16
    y, w, emap = F.trtllm_fp4_block_scale_moe(**_layer_args(T=0), do_finalize=False)
    assert (y.shape, w.shape, emap.shape) == ((0, 128), (0, 2), (0,))
    assert (y.dtype, w.dtype, emap.dtype) == (torch.bfloat16, torch.bfloat16, torch.int32)
    given = torch.zeros(0, 128, dtype=torch.bfloat16)
    assert F.trtllm_fp4_block_scale_moe(**_layer_args(T=0), output=given)[0] is given


def test_device_ops_fail_loudly_on_cpu_tensors():
    args = _layer_args()
    ids = torch.zeros(3, 2, dtype=torch.int32)
    calls = [
        lambda: F.trtllm_fp4_block_scale_moe(**args),
        lambda: F.trtllm_fp4_block_scale_routed_moe(ids, **{k: v for k, v in args.items() if k != "routing_logits"}),
        lambda: F.moe_route(torch.zeros(3, 8), 2),
        lambda: F.moe_permute_mxfp8(ids, args["hidden_states"], args["hidden_states_scale"], 0, 8),
        lambda: F.moe_gated_act_mxfp8(torch.zeros(4, 256, dtype=torch.bfloat16), torch.zeros(9, dtype=torch.int32)),
        lambda: F.moe_finalize(torch.zeros(6, 128, dtype=torch.bfloat16), torch.zeros(3, 2, dtype=torch.bfloat16),
                               torch.zeros(6, dtype=torch.int32)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_symbols_are_declared_bound_and_exported(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    for name in SYMBOLS:
        assert f"FI_API int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, name), name
    for name, struct in zip(SYMBOLS, ("fi_moe_route_params_t", "fi_moe_permute_params_t", "fi_moe_gated_act_params_t",
                                      "fi_moe_finalize_params_t")):
        assert getattr(fi_lib, name).argtypes[0] is C.POINTER(getattr(_lib, struct))
    assert fi_lib.fi_abi_version() == 2  # the change is additive
    assert (_lib.FI_MOE_MAX_EXPERTS, _lib.FI_MOE_MAX_TOP_K, _lib.FI_MOE_SORT_BLOCK) == (512, 8, 256)
    assert (_lib.FI_MOE_ROUTING_DEFAULT, _lib.FI_MOE_ROUTING_RENORMALIZE, _lib.FI_MOE_ROUTING_RENORMALIZE_NAIVE,
            _lib.FI_MOE_ROUTING_TOPK) == tuple(int(F.RoutingMethodType[n]) for n in
                                               ("Default", "Renormalize", "RenormalizeNaive", "TopK"))
    makefile = open(os.path.join(ROOT, "flashinfer-ai_amd", "csrc", "Makefile")).read()
    assert " moe" in [l for l in makefile.splitlines() if l.startswith("PLAIN_SRCS")][0]


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error

    def refused(fn, params, message):
        assert fn(C.byref(params), None) != 0 and message in err(), (message, err())

    # ---- route
    def route(**kw):
        base = dict(logits=a, topk_ids=a, topk_weights=a, num_tokens=4, num_experts=8, top_k=2, method=0,
                    dtype=_lib.FI_DTYPE_F32)
        base.update(kw)
        return _lib.fi_moe_route_params_t(**base)

    fn = fi_lib.fi_moe_route
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("logits", "topk_ids", "topk_weights"):
        refused(fn, route(**{field: None}), b"null tensor")
    for field in ("num_tokens", "num_experts", "top_k"):
        refused(fn, route(**{field: -1}), b"negative")
    refused(fn, route(num_experts=513), b"num_experts 513")
    refused(fn, route(num_experts=0), b"num_experts 0")
    for top_k, experts in ((0, 8), (9, 16), (5, 4)):
        refused(fn, route(top_k=top_k, num_experts=experts), b"top_k")
    for method in (2, 3, 6):
        refused(fn, route(method=method), b"routing method")
    refused(fn, route(dtype=_lib.FI_DTYPE_F16), b"dtype")
    assert fn(C.byref(route(num_tokens=0, logits=None, topk_ids=None, topk_weights=None)), None) == 0

    # ---- permute: 4 tokens x top_k 2, 3 local experts: (8 + 127 * 3) / 128 * 128 = 384 scale rows of 4 bytes
    def permute(**kw):
        base = dict(topk_ids=a, x=a, x_sf=a, m_indptr=a, expanded_to_permuted=a, x_permuted=a, sf_permuted=a,
                    unpacked_weights=None, workspace=a, sf_bytes=1 << 20, workspace_bytes=1 << 20, num_tokens=4, top_k=2,
                    hidden=128, local_expert_offset=0, local_num_experts=3, packed=0)
        base.update(kw)
        return _lib.fi_moe_permute_params_t(**base)

    fn = fi_lib.fi_moe_permute_mxfp8
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("topk_ids", "x", "x_sf", "m_indptr", "expanded_to_permuted", "x_permuted", "sf_permuted", "workspace"):
        refused(fn, permute(**{field: None}), b"null tensor")
    for field in ("num_tokens", "top_k", "hidden", "local_expert_offset", "local_num_experts"):
        refused(fn, permute(**{field: -1}), b"negative")
    refused(fn, permute(local_num_experts=513), b"local_num_experts 513")
    refused(fn, permute(top_k=9), b"top_k 9")
    refused(fn, permute(top_k=0), b"top_k 0")
    for hidden in (0, 96, 160):
        refused(fn, permute(hidden=hidden), b"multiple of 128")
    refused(fn, permute(x=a + 8), b"aligned")
    refused(fn, permute(x_sf=a + 2), b"aligned")
    refused(fn, permute(sf_bytes=384 * 4 - 1), b"sf_permuted holds 1535 bytes, 1536 needed")
    refused(fn, permute(workspace_bytes=43), b"workspace holds 43 bytes, 44 needed")  # (1 block * 3 + 8) * 4
    refused(fn, permute(num_tokens=200, workspace_bytes=1623), b"1624 needed")       # (2 blocks * 3 + 400) * 4
    none = dict(topk_ids=None, x=None, x_sf=None, m_indptr=None, expanded_to_permuted=None, x_permuted=None,
                sf_permuted=None, workspace=None)
    assert fn(C.byref(permute(num_tokens=0, **none)), None) == 0

    # ---- gated activation: cum_m 8, 3 groups: 384 scale rows of 8 bytes at intermediate 256
    def act(**kw):
        base = dict(x=a, m_indptr=a, bias=None, alpha=None, beta=None, limit=None, q=a, sf=a, sf_bytes=1 << 20, cum_m=8,
                    intermediate=256, num_groups=3)
        base.update(kw)
        return _lib.fi_moe_gated_act_params_t(**base)

    fn = fi_lib.fi_moe_gated_act_mxfp8
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("x", "m_indptr", "q", "sf"):
        refused(fn, act(**{field: None}), b"null tensor")
    for field in ("cum_m", "intermediate", "num_groups"):
        refused(fn, act(**{field: -1}), b"negative")
    refused(fn, act(num_groups=513), b"num_groups 513")
    refused(fn, act(num_groups=0), b"num_groups 0")
    for inter in (0, 64, 192):
        refused(fn, act(intermediate=inter), b"multiple of 128")
    refused(fn, act(x=a + 2), b"aligned")
    refused(fn, act(bias=a + 4), b"aligned")
    refused(fn, act(sf_bytes=384 * 8 - 1), b"sf holds 3071 bytes, 3072 needed")
    assert fn(C.byref(act(cum_m=0, x=None, m_indptr=None, q=None, sf=None)), None) == 0

    # ---- finalize
    def fin(**kw):
        base = dict(y=a, weights=a, expanded_to_permuted=a, bias=None, m_indptr=None, out=a, num_tokens=4, top_k=2,
                    hidden=128, num_groups=0, rows=8)
        base.update(kw)
        return _lib.fi_moe_finalize_params_t(**base)

    fn = fi_lib.fi_moe_finalize
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("y", "weights", "expanded_to_permuted", "out"):
        refused(fn, fin(**{field: None}), b"null tensor")
    for field in ("num_tokens", "top_k", "hidden", "num_groups", "rows"):
        refused(fn, fin(**{field: -1}), b"negative")
    refused(fn, fin(top_k=9), b"top_k 9")
    refused(fn, fin(hidden=12), b"multiple of 8")
    refused(fn, fin(bias=a, m_indptr=None, num_groups=3), b"m_indptr")
    refused(fn, fin(bias=a, m_indptr=a, num_groups=0), b"num_groups 0")
    refused(fn, fin(bias=a, m_indptr=a, num_groups=513), b"num_groups 513")
    refused(fn, fin(y=a + 2), b"aligned")
    refused(fn, fin(out=a + 8), b"aligned")
    assert fn(C.byref(fin(num_tokens=0, y=None, weights=None, expanded_to_permuted=None, out=None)), None) == 0


# ---- the oracle against hand-worked cases ------------------------------------------------------------------------------
# 3 tokens, 4 experts, top_k 2.  ln 2, ln 3 make the softmax weights fractions one can write down.
L2, L3 = math.log(2.0), math.log(3.0)
HAND_LOGITS = torch.tensor([[0.0, L2, L3, -50.0],     # exp: 1, 2, 3, ~0  -> experts 2, 1
                            [L3, -50.0, 0.0, L2],     # exp: 3, ~0, 1, 2  -> experts 0, 3
                            [L2, L2 + L3, -50.0, 0.0]],  # exp: 2, 6, ~0, 1  -> experts 1, 0
                           dtype=torch.float64)
HAND_IDS = [[2, 1], [0, 3], [1, 0]]


@pytest.mark.parametrize("method", M.METHODS)
def test_oracle_routing_hand_worked(method):
    ids, w = M.route_ref(HAND_LOGITS, 2, method)
    assert ids.dtype == torch.int32 and ids.tolist() == HAND_IDS
    tiny = math.exp(-50.0)
    want = {
        M.DEFAULT: [[3 / (6 + tiny), 2 / (6 + tiny)], [3 / (6 + tiny), 2 / (6 + tiny)], [6 / (9 + tiny), 2 / (9 + tiny)]],
        M.RENORMALIZE: [[3 / 5, 2 / 5], [3 / 5, 2 / 5], [6 / 8, 2 / 8]],
        M.RENORMALIZE_NAIVE: [[3 / 5, 2 / 5], [3 / 5, 2 / 5], [6 / 8, 2 / 8]],
        M.TOPK: [[L3, L2], [L3, L2], [L2 + L3, L2]],
    }[method]
    torch.testing.assert_close(w, torch.tensor(want, dtype=torch.float64), rtol=1e-13, atol=0)


def test_oracle_routing_ties_go_to_the_lower_expert():
    ids, _ = M.route_ref(torch.tensor([[1.0, 2.0, 2.0, 1.0, 2.0]]), 4, M.TOPK)
    assert ids.tolist() == [[1, 2, 4, 0]]


def test_oracle_logits_are_tie_free_and_exact_in_bf16():
    for E in (4, 6, 65, 512):
        x = M.tie_free_logits(5, E, seed=E)
        assert x.shape == (5, E)
        for row in x.double():
            assert sorted(row.tolist()) == [(k - E // 2) / 8 for k in range(E)]
        assert torch.equal(M.tie_free_logits(5, E, seed=E, dtype=torch.bfloat16).float(), x)


def test_oracle_permutation_hand_worked():
    ids = torch.tensor(HAND_IDS, dtype=torch.int32)
    # expanded index:      0  1  2  3  4  5
    # expert:              2  1  0  3  1  0     -> expert 0: rows 0, 1 (indices 2, 5); expert 1: rows 2, 3 (indices 1, 4);
    #                                              expert 2: row 4 (index 0); expert 3: row 5 (index 3)
    indptr, emap, inverse = M.permute_ref(ids, 0, 4)
    assert indptr.tolist() == [0, 2, 4, 5, 6]
    assert emap.tolist() == [4, 2, 0, 5, 3, 1]
    assert inverse == [2, 5, 1, 4, 0, 3]
    # the local window [1, 3): experts 1 and 2 only; the slots on experts 0 and 3 get no row
    indptr, emap, inverse = M.permute_ref(ids, 1, 2)
    assert indptr.tolist() == [0, 2, 3]
    assert emap.tolist() == [2, 0, -1, -1, 1, -1]
    assert inverse == [1, 4, 0]
    assert M.segments(indptr) == (2, 1)
    # token 1 (indices 2, 3) has no local slot: finalize gives it zeros
    y = torch.tensor([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]])
    w = torch.tensor([[0.5, 0.25], [0.5, 0.5], [2.0, 1.0]])
    out, mag = M.finalize_ref(y, w, emap, 2)
    assert out.tolist() == [[0.5 * 100 + 0.25 * 1, 0.5 * 200 + 0.25 * 2], [0.0, 0.0], [2.0 * 10, 2.0 * 20]]
    assert torch.equal(out, mag)
    bias = torch.tensor([[1.0, 1.0], [-1000.0, 0.0]])  # group 0 (expert 1) rows 0, 1; group 1 (expert 2) row 2
    out, mag = M.finalize_ref(y, w, emap, 2, bias, indptr)
    assert out.tolist() == [[0.5 * -900 + 0.25 * 2, 0.5 * 200 + 0.25 * 3], [0.0, 0.0], [2.0 * 11, 2.0 * 21]]
    assert mag[0].tolist() == [450.5, 100.75]


def test_oracle_packing_round_trips():
    ids = torch.tensor([[511, 0], [3, 65]], dtype=torch.int32)
    w = torch.tensor([[0.75, -2.0], [1e-3, 3.0]]).to(torch.bfloat16)
    packed = M.pack_topk_ids(ids, w)
    assert packed.dtype == torch.int32
    assert torch.equal(packed & 0xFFFF, ids)
    assert torch.equal((packed >> 16).to(torch.int16).view(torch.bfloat16), w)
    assert packed[0, 1].item() == (0xC000 << 16) - 2 ** 32  # -2.0 is 0xC000: the sign bit makes the int32 negative


def test_oracle_activation_hand_worked():
    I = 32
    x = torch.zeros(3, 2 * I, dtype=torch.float64)
    x[:, 0], x[:, I] = torch.tensor([2.0, -3.0, 10.0]), torch.tensor([1.0, 5.0, -1.0])  # x1 (linear), x2 (gate)
    indptr = [0, 2, 3]
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))  # noqa: E731
    plain = M.gated_act_ref(x, indptr)
    assert plain.shape == (3, I)
    torch.testing.assert_close(plain[:, 0], torch.tensor([1 * sig(1) * 2, 5 * sig(5) * -3, -1 * sig(-1) * 10],
                                                         dtype=torch.float64), rtol=1e-14, atol=0)
    assert not plain[:, 1:].any()
    bias = torch.zeros(2, 2 * I)
    bias[0, 0], bias[0, I], bias[1, 0], bias[1, I] = 0.5, 1.0, -20.0, 0.25
    full = M.gated_act_ref(x, indptr, bias, alpha=torch.tensor([1.5, 2.0]), beta=torch.tensor([1.0, 0.5]),
                           limit=torch.tensor([4.0, 7.0]))
    want = [
        2.0 * sig(1.5 * 2.0) * (2.5 + 1.0),            # gate 1 + 1 = 2; linear 2 + 0.5
        4.0 * sig(1.5 * 4.0) * (-2.5 + 1.0),           # gate 5 + 1 = 6 -> 4; linear -3 + 0.5
        -0.75 * sig(2.0 * -0.75) * (-7.0 + 0.5),         # group 1: gate -1 + 0.25; linear 10 - 20 -> clamp -7
    ]
    torch.testing.assert_close(full[:, 0], torch.tensor(want, dtype=torch.float64), rtol=1e-14, atol=0)
    # the other columns: gate 0 + bias 0 -> 0
    assert not full[:, 1:].any()
    q, sf = M.quantize_act_ref(full)
    assert q.shape == (3, I) and sf.shape == (3, 1)
    # |want[0]| = 6.77...: 448 * 2^-7 = 3.5 < 6.77 <= 448 * 2^-6 = 7
    assert sf[0, 0].item() == 127 - 6
