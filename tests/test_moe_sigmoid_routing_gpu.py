"""GPU: the sigmoid routing methods, DeepSeekV3 and Llama4 (fi_moe_route_sigmoid, csrc/moe.hip), against the fp64 oracle of
tests/moe_sigmoid_ref.py -- ids exact, weights within one bf16 ulp -- then the MoE layer with them: bit-identical to its
stages called by hand, to the routed call on the packed output of moe_route, and to its graph replay.

T = 1, 3, 67: one wave, a partly filled workgroup, many workgroups with a ragged last one."""
import functools

import pytest
import torch

import moe_ref as M
import moe_sigmoid_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOKENS = (1, 3, 67)


def _fm():
    from flashinfer import fused_moe

    return fused_moe


def _check(ids, w, want_ids, want_w, what):
    assert ids.dtype == torch.int32 and w.dtype == torch.bfloat16 and ids.shape == w.shape == want_ids.shape
    assert torch.equal(ids.cpu(), want_ids), what
    want_bf16 = want_w.to(torch.bfloat16).double()
    err = (w.cpu().double() - want_bf16).abs()
    # the f32 error of the weight is far below a bf16 ulp: only a flip of the final rounding is allowed for
    assert bool((err <= M.bf16_ulp(want_bf16)).all()), (what, err.max().item())


# ---- DeepSeekV3 against the oracle ----------------------------------------------------------------------------------------
# (E, n_group, topk_group, top_k): what the kernel can get wrong at it
DEEPSEEK_CASES = [
    (8, 4, 2, 2),         # epg 2: the top-2 is the whole group
    (12, 4, 2, 3),        # epg 3: not a power of two, below one slot
    (16, 4, 2, 4),        # a small power-of-two group
    (72, 8, 3, 8),        # epg 9: E not a multiple of 64, groups straddle a slot
    (256, 8, 4, 8),       # DeepSeek-V3's own shape
    (384, 12, 4, 8),      # a further grouped shape
    (512, 4, 2, 8),       # epg 128: a group spans two slots
    (512, 16, 4, 8),      # 16 groups at the expert limit
    (128, 64, 4, 8),      # the group-count limit
    (128, 2, 1, 8),       # epg 64: a group is one whole slot, the widest shuffle reduction
    (384, 1, 1, 8),       # no groups: Kimi-K2's shape as it spells it
    (512, None, None, 8),  # no groups
]
BF16_CASES = [(64, 8, 4, 8), (16, 4, 2, 4)]
ALL_CASES = [(c, torch.float32) for c in DEEPSEEK_CASES] + [(c, torch.bfloat16) for c in BF16_CASES]


@functools.lru_cache(maxsize=None)
def _inputs(T, E, n_group, dtype):
    logits, bias, _ = S.sigmoid_case(T, E, n_group, seed=1000 * E + 10 * T + (n_group or 0), dtype=dtype)
    return logits, bias, S.decision_gaps(logits, bias, n_group)


@functools.lru_cache(maxsize=None)
def _oracle(T, E, n_group, topk_group, top_k, scale, dtype):
    logits, bias, _ = _inputs(T, E, n_group, dtype)
    return S.route_sigmoid_ref(logits, bias, n_group, topk_group, top_k, scale, S.DEEPSEEK_V3)


@pytest.mark.parametrize("scale", [None, 2.5], ids=["unscaled", "scale2.5"])
@pytest.mark.parametrize("bias_dtype", [torch.bfloat16, torch.float32], ids=["bias_bf16", "bias_f32"])
@pytest.mark.parametrize("case,dtype", ALL_CASES,
                         ids=["E{}_g{}_k{}_top{}_{}".format(*c, "f32" if d == torch.float32 else "bf16") for c, d in ALL_CASES])
def test_deepseek_v3_matches_the_oracle(case, dtype, bias_dtype, scale):
    F = _fm()
    E, n_group, topk_group, top_k = case
    for T in TOKENS:
        logits, bias, (expert_gap, group_gap) = _inputs(T, E, n_group, dtype)
        assert expert_gap >= S.MARGIN and (group_gap is None or group_gap >= S.MARGIN), (T, expert_gap, group_gap)
        assert (group_gap is None) == (not S.grouped(n_group))
        want_ids, want_w = _oracle(T, E, n_group, topk_group, top_k, scale, dtype)
        dev_bias = bias.to(bias_dtype).to(DEV)
        assert torch.equal(dev_bias.float().cpu(), bias)  # the bias is exact in bf16
        ids, w = F.moe_route(logits.to(DEV), top_k, F.RoutingMethodType.DeepSeekV3, routing_bias=dev_bias, n_group=n_group,
                             topk_group=topk_group, routed_scaling_factor=scale)
        _check(ids, w, want_ids, want_w, (T, case))


# ---- hand-made rows -------------------------------------------------------------------------------------------------------
def _route(logits, bias, n_group, topk_group, top_k, scale=None):
    F = _fm()
    logits = torch.as_tensor(logits, dtype=torch.float32)
    bias = torch.as_tensor(bias, dtype=torch.float32)
    ids, w = F.moe_route(logits.to(DEV), top_k, 2, bias.to(DEV), n_group, topk_group, scale)
    want_ids, want_w = S.route_sigmoid_ref(logits, bias, n_group, topk_group, top_k, scale, S.DEEPSEEK_V3)
    _check(ids, w, want_ids, want_w, "hand-made")
    return ids.cpu().tolist(), w.cpu().float().tolist()


def test_equal_scores_go_to_the_lower_expert():
    # sigmoid(0) = 1/2 exactly on the device, and the biases are exact: the ties are ties in f32 too
    ids, w = _route(torch.zeros(2, 70), torch.zeros(70), None, None, 4)
    assert ids == [[0, 1, 2, 3]] * 2 and w == [[0.25] * 4] * 2
    bias = torch.zeros(130)
    bias[[5, 69, 129]] = 0.25  # one tie over three slots of lane 5 ...
    bias[[7, 70]] = 0.125      # ... and one over two lanes
    ids, _ = _route(torch.zeros(1, 130), bias, None, None, 6)
    assert ids == [[5, 69, 129, 7, 70, 0]]
    # inside the kept groups, through both group forms (epg 2: shuffles, epg 3: LDS)
    ids, _ = _route(torch.zeros(1, 8), [0, 0, 0, 0, 0.5, 0.5, 0.5, 0.5], 4, 2, 3)
    assert ids == [[4, 5, 6]]
    ids, _ = _route(torch.zeros(1, 12), [0] * 6 + [0.5] * 6, 4, 2, 4)
    assert ids == [[6, 7, 8, 9]]


def test_equal_group_scores_go_to_the_lower_group():
    for E, n_group in ((8, 4), (12, 4), (128, 64), (512, 4)):  # epg 2 and 64 lanes apart by shuffles, 3 and 128 through LDS
        epg = E // n_group
        ids, _ = _route(torch.zeros(3, E), torch.zeros(E), n_group, 2, min(8, 2 * epg))
        assert ids == [list(range(min(8, 2 * epg)))] * 3
        # all groups equal but for the last, which is ahead: it comes first, then the lowest
        bias = torch.zeros(E)
        bias[E - epg:] = 0.125
        ids, _ = _route(torch.zeros(1, E), bias, n_group, 2, 4)
        assert ids == [(list(range(E - epg, E)) + [0, 1])[:4] if epg < 4 else list(range(E - epg, E - epg + 4))]


def test_an_expert_of_a_dropped_group_never_wins_against_negative_scores():
    """A bias of -2 (and below) on every expert of the kept groups makes all their b negative.  Groups 1 and 3 are dropped
    for their other experts, and their first expert, at b = 1/2 and 3/4, is larger than every candidate: it is still not
    chosen.  top_k == topk_group * epg: every candidate is taken."""
    ids, w = _route(torch.zeros(3, 8), [-2, -2, 0, -10, -2, -2.25, 0.25, -20], 4, 2, 4)       # epg 2: shuffles
    assert ids == [[0, 1, 4, 5]] * 3 and w == [[0.25] * 4] * 3
    ids, w = _route(torch.zeros(3, 12), [-2, -2, -2, 0, -10, -10, -2, -2.25, -2.5, 0.25, -20, -20], 4, 2, 6, 3.0)  # epg 3: LDS
    assert ids == [[0, 1, 2, 6, 7, 8]] * 3 and w == [[0.5] * 6] * 3
    # without groups the same scores are plain candidates
    ids, _ = _route(torch.zeros(1, 8), [-2, -2, 0, -10, -2, -2.25, 0.25, -20], None, None, 2)
    assert ids == [[6, 2]]


def test_a_nan_logit_counts_as_minus_infinity():
    F = _fm()
    bias = torch.tensor([0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 0.0])
    nan = torch.zeros(2, 8)
    nan[:, 3] = float("nan")
    ids, w = _route(nan, bias, None, None, 8)
    assert ids == [[0, 1, 2, 4, 5, 6, 7, 3]] * 2 and w[0][7] == 0.0  # s = 0, b = the bias alone
    inf = torch.zeros(2, 8)
    inf[:, 3] = float("-inf")
    ids2, w2 = F.moe_route(inf.to(DEV), 8, 2, bias.to(DEV))
    assert ids2.cpu().tolist() == ids and w2.cpu().float().tolist() == w
    # with groups: the NaN expert still counts towards its group's score with b = its bias
    ids, _ = _route(nan, bias, 4, 1, 2)
    assert ids == [[0, 1]] * 2
    ids, _ = _route(nan, bias + torch.tensor([0, 0, 0.5, 0.5, 0, 0, 0, 0]), 4, 1, 2)  # group 1: 1.0 + 0.75
    assert ids == [[2, 3]] * 2


# ---- Llama4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("E", [4, 65, 128, 512])
def test_llama4_is_the_argmax_and_its_sigmoid(E, dtype):
    F = _fm()
    for T in TOKENS:
        logits = M.tie_free_logits(T, E, seed=3000 * E + T, dtype=dtype)
        ids, w = F.moe_route(logits.to(DEV), 1, F.RoutingMethodType.Llama4)
        want_ids, want_w = S.route_sigmoid_ref(logits, None, None, None, 1, None, S.LLAMA4)
        assert torch.equal(want_ids[:, 0].long(), logits.double().argmax(-1))
        assert torch.equal(want_w, torch.sigmoid(logits.double().amax(-1, keepdim=True)))
        _check(ids, w, want_ids, want_w, (T, E))


def test_llama4_ties_go_to_the_lower_index():
    F = _fm()
    rows = torch.zeros(4, 130)
    rows[0, [1, 2, 4]] = 2.0
    rows[0, [0, 3]] = 1.0
    rows[2, [69, 129]] = 3.0               # the same lane, two slots
    rows[3, 0] = float("nan")              # as -inf: not the maximum
    rows[3, 1:] = -1.0
    ids, w = F.moe_route(rows.to(DEV), 1, 3)
    assert ids.cpu().tolist() == [[1], [0], [69], [1]]
    want = torch.sigmoid(torch.tensor([[2.0], [0.0], [3.0], [-1.0]], dtype=torch.float64))
    _check(ids, w, torch.tensor([[1], [0], [69], [1]], dtype=torch.int32), want, "ties")


# ---- the layer ------------------------------------------------------------------------------------------------------------
E_L, GROUPS_L, TOPK_GROUP_L, H_L, I_L = 16, 4, 2, 256, 128


@functools.lru_cache(maxsize=None)
def _layer_case(T, offset, G, method):
    """Inputs made as tests/test_fused_moe_gpu.py::_layer_case makes them, with the routing arguments of ``method``."""
    import flashinfer

    E, H, I = E_L, H_L, I_L
    g = torch.Generator().manual_seed(100 * T + 10 * offset + G)
    logits, bias, _ = S.sigmoid_case(T, E, GROUPS_L, seed=T + offset)
    if method == S.LLAMA4:  # the logits of sigmoid_case order the experts by their bias, the same for every token
        logits = M.tie_free_logits(T, E, seed=T + offset)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(G, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    w2 = (4 * torch.randn(G, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)
    x_q, x_sf = flashinfer.mxfp8_quantize(x.to(DEV), False)
    w1_q, w1_sf = flashinfer.mxfp4_quantize_grouped(w1.to(DEV))
    w2_q, w2_sf = flashinfer.mxfp4_quantize_grouped(w2.to(DEV))
    p = dict(bias1=0.5 * torch.randn(G, 2 * I, generator=g), alpha=torch.full((G,), 1.702), beta=torch.ones(G),
             limit=torch.full((G,), 2.0), bias2=0.5 * torch.randn(G, H, generator=g))
    dev = {k: v.to(DEV) for k, v in p.items()}
    deepseek = method == S.DEEPSEEK_V3
    return dict(
        routing_logits=logits.to(DEV), routing_bias=bias.to(torch.bfloat16).to(DEV) if deepseek else None, hidden_states=x_q,
        hidden_states_scale=x_sf.view(T, H // 32), gemm1_weights=w1_q, gemm1_weights_scale=w1_sf, gemm1_bias=dev["bias1"],
        gemm1_alpha=dev["alpha"], gemm1_beta=dev["beta"], gemm1_clamp_limit=dev["limit"], gemm2_weights=w2_q,
        gemm2_weights_scale=w2_sf, gemm2_bias=dev["bias2"], output1_scale_scalar=None, output1_scale_gate_scalar=None,
        output2_scale_scalar=None, num_experts=E, top_k=4 if deepseek else 1, n_group=GROUPS_L if deepseek else None,
        topk_group=TOPK_GROUP_L if deepseek else None, intermediate_size=I, local_expert_offset=offset,
        local_num_experts=G, routed_scaling_factor=2.5 if deepseek else None, routing_method_type=method)


def _bits(t):
    return t.view(torch.int16)


def _check_layer(T, offset, G, method):
    F = _fm()
    from flashinfer.gemm import _group_gemm_mxfp4_into

    args = _layer_case(T, offset, G, method)
    H, I, top_k = H_L, I_L, args["top_k"]
    (out,) = F.trtllm_fp4_block_scale_moe(**args)
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    # 1. the stages by hand, moe_route with the new arguments
    ids, w = F.moe_route(args["routing_logits"], top_k, method, routing_bias=args["routing_bias"], n_group=args["n_group"],
                         topk_group=args["topk_group"], routed_scaling_factor=args["routed_scaling_factor"])
    m_indptr, emap, x_perm, sf_perm = F.moe_permute_mxfp8(ids, args["hidden_states"], args["hidden_states_scale"], offset, G)
    y1 = torch.empty(T * top_k, 2 * I, dtype=torch.bfloat16, device=DEV)
    _group_gemm_mxfp4_into(x_perm, args["gemm1_weights"], sf_perm, args["gemm1_weights_scale"], y1, m_indptr, 2 * I, H)
    act, act_sf = F.moe_gated_act_mxfp8(y1, m_indptr, args["gemm1_bias"], args["gemm1_alpha"], args["gemm1_beta"],
                                        args["gemm1_clamp_limit"])
    y2 = torch.empty(T * top_k, H, dtype=torch.bfloat16, device=DEV)
    _group_gemm_mxfp4_into(act, args["gemm2_weights"], act_sf, args["gemm2_weights_scale"], y2, m_indptr, H, I)
    by_hand = F.moe_finalize(y2, w, emap, args["gemm2_bias"], m_indptr)
    assert torch.equal(_bits(out), _bits(by_hand))
    if G < E_L and T > 1:  # the window drops slots, and not all of them
        local = emap.cpu() >= 0
        assert bool(local.any()) and not bool(local.all())
    # 2. the routed call on the packed output of moe_route: the default method, no bias, no groups, no factor
    routed_args = {k: v for k, v in args.items() if k != "routing_logits"}
    routed_args.update(routing_bias=None, n_group=None, topk_group=None, routed_scaling_factor=None, routing_method_type=0)
    packed = M.pack_topk_ids(ids.cpu(), w.cpu()).to(DEV)
    (routed,) = F.trtllm_fp4_block_scale_routed_moe(packed, **routed_args)
    assert torch.equal(_bits(out), _bits(routed))
    # 3. do_finalize=False returns the same weights and map
    triple = F.trtllm_fp4_block_scale_moe(**{**args, "gemm2_bias": None}, do_finalize=False)
    assert [tuple(t.shape) for t in triple] == [(T * top_k, H), (T, top_k), (T * top_k,)]
    assert torch.equal(triple[2], emap) and torch.equal(_bits(triple[1]), _bits(w))
    again = F.moe_finalize(triple[0], triple[1], triple[2], args["gemm2_bias"], m_indptr)
    assert torch.equal(_bits(out), _bits(again))


@pytest.mark.parametrize("offset,G", [(0, 16), (4, 8)], ids=["all_local", "local_window"])
@pytest.mark.parametrize("T", [1, 67])
def test_layer_with_deepseek_v3_routing_is_its_stages(T, offset, G):
    _check_layer(T, offset, G, S.DEEPSEEK_V3)


def test_layer_with_llama4_routing_is_its_stages():
    _check_layer(67, 4, 8, S.LLAMA4)


# ---- graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    F = _fm()
    args_a = _layer_case(67, 0, 16, S.DEEPSEEK_V3)
    args_b = _layer_case(67, 4, 8, S.DEEPSEEK_V3)  # other logits and activations of the same shapes
    static = dict(args_a)
    for name in ("routing_logits", "hidden_states", "hidden_states_scale"):
        static[name] = args_a[name].clone()
    (eager_a,) = F.trtllm_fp4_block_scale_moe(**static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        (captured,) = F.trtllm_fp4_block_scale_moe(**static)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(captured), _bits(eager_a))
    for name in ("routing_logits", "hidden_states", "hidden_states_scale"):
        static[name].view(torch.uint8).copy_(args_b[name].view(torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    replayed = captured.clone()
    (eager_b,) = F.trtllm_fp4_block_scale_moe(**static)
    torch.cuda.synchronize()
    assert torch.equal(_bits(replayed), _bits(eager_b))
    assert not torch.equal(_bits(eager_a), _bits(eager_b))
