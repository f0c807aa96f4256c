"""GPU: the MoE layer (flashinfer.fused_moe, csrc/moe.hip) stage by stage against the fp64 oracle of tests/moe_ref.py, each
stage on the device's own previous-stage output and exact where exactness is possible, then the whole layer: bit-identical
to its stages called by hand, and against the oracle at the reference's own bar for this mode.

Shapes are the smallest at which each kernel can still go wrong: H = I = 128 (one k tile) unless two tiles matter, and
one size past the 256-thread row team (H = 4224, I = 2176, H = 2056) for its second pass."""
import functools

import pytest
import torch

import moe_ref as M
import mx_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
METHOD_NAMES = {M.DEFAULT: "default", M.RENORMALIZE: "renormalize", M.RENORMALIZE_NAIVE: "naive", M.TOPK: "topk"}


def _fm():
    from flashinfer import fused_moe

    return fused_moe


# ---- routing ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", M.METHODS, ids=METHOD_NAMES.get)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("E", [4, 6, 64, 65, 128, 512])
def test_routing_matches_the_oracle(E, dtype, method):
    F = _fm()
    for T in (1, 3, 67):
        logits = M.tie_free_logits(T, E, seed=1000 * E + T, dtype=dtype)
        dev_logits = logits.to(DEV)
        for top_k in (k for k in (1, 2, 4, 8) if k <= E):
            ids, w = F.moe_route(dev_logits, top_k, method)
            assert ids.dtype == torch.int32 and w.dtype == torch.bfloat16 and ids.shape == w.shape == (T, top_k)
            want_ids, want_w = M.route_ref(logits, top_k, method)
            assert torch.equal(ids.cpu(), want_ids), (T, top_k)
            want_bf16 = want_w.to(torch.bfloat16).double()
            err = (w.cpu().double() - want_bf16).abs()
            # f32 softmax error is far below a bf16 ulp: only a flip of the final rounding is allowed for
            assert bool((err <= M.bf16_ulp(want_bf16)).all()), (T, top_k, err.max().item())


def test_routing_ties_go_to_the_lower_expert():
    F = _fm()
    logits = torch.tensor([[1.0, 2.0, 2.0, 1.0, 2.0] + [0.0] * 65, [0.0] * 70], dtype=torch.float32)
    ids, w = F.moe_route(logits.to(DEV), 4, M.TOPK)
    assert ids.cpu().tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]]
    assert w.cpu().float().tolist() == [[2.0, 2.0, 2.0, 1.0], [0.0] * 4]


# ---- permute ------------------------------------------------------------------------------------------------------------
def _activations(T, H, seed):
    """MXFP8 activations made on the device: (x_q [T, H] e4m3, x_sf [T, H / 32] bytes), and their CPU copies."""
    import flashinfer

    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, H, generator=g) * torch.exp2(torch.randint(-3, 4, (T, 1), generator=g).float())).to(torch.bfloat16)
    q, sf = flashinfer.mxfp8_quantize(x.to(DEV), False)
    return q, sf.view(T, H // 32)


def _routed_ids(T, E, top_k, seed):
    return M.route_ref(M.tie_free_logits(T, E, seed), top_k, M.TOPK)[0]


PERMUTE_CASES = {
    # name: (ids [T, top_k] builder, offset, E_local)
    "empty_expert": (lambda: torch.tensor([[0, 1], [2, 4], [5, 7], [6, 0], [1, 2]], dtype=torch.int32), 0, 8),
    "one_expert_crosses_a_scale_tile": (lambda: torch.full((130, 1), 2, dtype=torch.int32), 0, 4),
    "ragged_boundaries": (lambda: _routed_ids(67, 8, 4, 3), 0, 8),
    "several_placement_blocks": (lambda: _routed_ids(300, 8, 4, 4), 0, 8),
    "local_window": (lambda: _routed_ids(67, 8, 2, 5), 2, 3),
    "512_experts": (lambda: _routed_ids(40, 512, 8, 6), 0, 512),
    # wave boundaries of the scan over the experts inside the window, the last wave partly filled (8 of 64)
    "local_window_of_200": (lambda: _routed_ids(40, 512, 8, 8), 100, 200),
}


def _check_permute(ids, offset, G, packed_weights=None, H=128):
    F = _fm()
    T, top_k = ids.shape
    x_q, x_sf = _activations(T, H, seed=T)
    n = T * top_k
    dev_ids = ids if packed_weights is None else M.pack_topk_ids(ids, packed_weights)
    res = F.moe_permute_mxfp8(dev_ids.to(DEV), x_q, x_sf, offset, G, packed=packed_weights is not None)
    m_indptr, emap, x_perm, sf_perm = res[:4]
    # once more into prefilled buffers: every byte of the scale tensor is written, rows past the local count are not
    x2 = torch.full((n, H), 0x55, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    sf2 = torch.full_like(sf_perm, 0xFF)
    F._permute_into(dev_ids.to(DEV), x_q, x_sf, offset, G, packed_weights is not None, torch.empty_like(m_indptr),
                    torch.empty_like(emap), x2, sf2, None if packed_weights is None else torch.empty_like(res[4]))
    torch.cuda.synchronize()
    want_indptr, want_map, inverse = M.permute_ref(ids, offset, G)
    assert torch.equal(m_indptr.cpu(), want_indptr)
    assert torch.equal(emap.cpu(), want_map)
    cum = int(want_indptr[-1])
    tokens = torch.tensor([i // top_k for i in inverse], dtype=torch.long)
    xq_cpu, xsf_cpu = x_q.cpu().view(torch.uint8), x_sf.cpu()
    assert torch.equal(x_perm.cpu().view(torch.uint8)[:cum], xq_cpu[tokens])
    assert torch.equal(x2.cpu().view(torch.uint8)[:cum], xq_cpu[tokens])
    assert bool((x2.cpu().view(torch.uint8)[cum:] == 0x55).all())
    want_sf = R.group_swizzle_a(xsf_cpu[tokens], M.segments(want_indptr))
    rows = (n + 127 * G) // 128 * 128
    assert sf_perm.shape == (rows, H // 32) and want_sf.shape[0] <= rows
    full = torch.zeros(rows, H // 32, dtype=torch.uint8)
    full[:want_sf.shape[0]] = want_sf
    assert torch.equal(sf_perm.cpu(), full)
    assert torch.equal(sf2.cpu(), full)
    if packed_weights is not None:
        assert torch.equal(res[4].cpu().view(torch.int16), packed_weights.view(torch.int16))
    return m_indptr, emap, x_perm, sf_perm


@pytest.mark.parametrize("case", sorted(PERMUTE_CASES))
def test_permute_is_exact(case):
    build, offset, G = PERMUTE_CASES[case]
    ids = build()
    if case == "empty_expert":
        assert 3 not in ids.tolist()
    if case == "local_window_of_200":
        rows = torch.tensor(M.segments(M.permute_ref(ids, offset, G)[0]))
        for part in rows.split(64):  # every 64-expert range of the window has an empty and a non-empty expert
            assert bool((part == 0).any()) and bool((part > 0).any())
    _check_permute(ids, offset, G)
    if case in ("empty_expert", "one_expert_crosses_a_scale_tile"):
        # 264 sixteen-byte chunks, more than the 256-thread row team: its second pass writes the scale dword at k block 128
        _check_permute(ids, offset, G, H=4224)


def test_permute_takes_packed_ids():
    ids = _routed_ids(67, 8, 4, 7)
    g = torch.Generator().manual_seed(8)
    weights = torch.randn(67, 4, generator=g).to(torch.bfloat16)  # negative weights too: the packed int32 is negative
    _check_permute(ids, 2, 3, packed_weights=weights)
    _check_permute(ids, 0, 8, packed_weights=weights)


# ---- gated activation ---------------------------------------------------------------------------------------------------
ACT_SEGMENTS = {"ragged": (4, 132, 0, 260), "one_group": (130,), "small": (3, 0, 1, 2, 0, 5, 1, 1)}
# I = 2176: 272 chunks of 8 columns, a partial second pass of the 256-thread row team
ACT_CASES = [(s, I) for s in sorted(ACT_SEGMENTS) for I in (128, 256)] + [("ragged", 2176), ("small", 2176)]


def _e4m3_step(v: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 at |v| <= 448 (fp64): 2^(floor(log2 |v|) - 3), the subnormal spacing 2^-9 below 2^-6."""
    e = torch.frexp(v.abs().clamp(min=2.0 ** -6))[1] - 1
    return torch.exp2(e.double() - 3)


@functools.lru_cache(maxsize=None)
def _act_case(segments, I, with_params):
    G, cum = len(segments), sum(segments)
    g = torch.Generator().manual_seed(cum + I + int(with_params))
    extra = 8  # rows past m_indptr[-1]
    x = (torch.randn(cum + extra, 2 * I, generator=g) * 2).to(torch.bfloat16)
    indptr = torch.tensor([0] + list(torch.tensor(segments).cumsum(0)), dtype=torch.int32)
    params = {}
    if with_params:
        params = dict(bias=torch.randn(G, 2 * I, generator=g), alpha=torch.full((G,), 1.702) + 0.1 * torch.arange(G),
                      beta=torch.ones(G) - 0.25 * torch.arange(G), limit=torch.full((G,), 1.5) + 0.5 * torch.arange(G))
    want = M.gated_act_ref(x[:cum], indptr, params.get("bias"), params.get("alpha"), params.get("beta"), params.get("limit"))
    return x, indptr, params, want


@pytest.mark.parametrize("with_params", [False, True], ids=["plain", "bias_alpha_beta_limit"])
@pytest.mark.parametrize("segments,I", ACT_CASES)
def test_gated_activation_against_the_oracle(segments, I, with_params):
    F = _fm()
    segs = ACT_SEGMENTS[segments]
    x, indptr, params, want = _act_case(segs, I, with_params)
    G, cum, nkb = len(segs), sum(segs), I // 32
    if with_params:  # the clamp binds on some elements, on both halves
        xd, b = x[:cum].double(), params["bias"].double()
        lim = torch.repeat_interleave(params["limit"].double(), torch.tensor(segs)).unsqueeze(-1)
        bias_rows = torch.repeat_interleave(b, torch.tensor(segs), dim=0)
        assert bool(((xd[:, I:] + bias_rows[:, I:]) > lim).any()) and bool(((xd[:, :I] + bias_rows[:, :I]).abs() > lim).any())
    # oracle side first: the blocks whose amax sits on a scale threshold (448 * 2^e) within 2^-20 relative may take the
    # neighbouring scale in f32; they are rare
    want_q, want_sf = M.quantize_act_ref(want)
    amax = want.view(cum, nkb, 32).abs().amax(-1)
    mant = torch.frexp(amax)[0] * 2  # in [1, 2)
    near = ((mant / 1.75 - 1).abs() <= 2.0 ** -20) & (amax > 0)
    assert near.double().mean().item() <= 0.01

    dev = {k: v.to(DEV) for k, v in params.items()}
    q, sf = F.moe_gated_act_mxfp8(x.to(DEV), indptr.to(DEV), dev.get("bias"), dev.get("alpha"), dev.get("beta"),
                                  dev.get("limit"))
    rows = (cum + 8 + 127 * G) // 128 * 128
    assert q.shape == (cum + 8, I) and q.dtype == torch.float8_e4m3fn and sf.shape == (rows, nkb) and sf.dtype == torch.uint8
    # again into prefilled buffers: rows past m_indptr[-1] are untouched, every scale byte is written
    q2 = torch.full((cum + 8, I), 0x55, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
    sf2 = torch.full_like(sf, 0xFF)
    F._gated_act_into(x.to(DEV), indptr.to(DEV), dev.get("bias"), dev.get("alpha"), dev.get("beta"), dev.get("limit"), q2, sf2)
    torch.cuda.synchronize()
    q, sf, q2, sf2 = q.cpu(), sf.cpu(), q2.cpu(), sf2.cpu()
    assert torch.equal(sf, sf2) and torch.equal(q.view(torch.uint8)[:cum], q2.view(torch.uint8)[:cum])
    assert bool((q2.view(torch.uint8)[cum:] == 0x55).all())
    # the scale bytes: un-swizzle every group, compare, and the padding is 0
    off = R.sf_row_offsets(segs)
    got_sf = torch.zeros(cum, nkb, dtype=torch.uint8)
    begin = 0
    for gi, m in enumerate(segs):
        got_sf[begin:begin + m] = R.unswizzle(sf.reshape(-1)[off[gi] * nkb:], m, nkb)
        begin += m
    full = torch.zeros(rows, nkb, dtype=torch.uint8)
    regrouped = R.group_swizzle_a(got_sf, segs)
    full[:regrouped.shape[0]] = regrouped
    assert torch.equal(sf, full)
    diff = (got_sf.int() - want_sf.int()).abs()
    assert bool((diff[~near] == 0).all()), f"{int((diff[~near] != 0).sum())} scale bytes differ off the thresholds"
    assert bool((diff[near] <= 1).all())
    # the values: within one e4m3 step at the oracle's block scale of the fp64 activation -- half a step is the format's
    # rounding, the other half lets f32 sigmoid rounding move a value across a rounding boundary
    scale = R.scale_f64(want_sf).unsqueeze(-1)
    got = R.dequantize(R.fp8_to_f64(q[:cum]), got_sf).view(cum, nkb, 32)
    want_b = want.view(cum, nkb, 32)
    step = _e4m3_step(torch.maximum(want_b.abs(), got.abs()) / scale) * scale
    bad = (got - want_b).abs() > step
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements are off by more than one step"
    # and off the thresholds nearly every byte is the oracle's own: an f32 result rounds differently only when the fp64 one
    # lies within ~2^-20 of a rounding boundary, relative to a step of 2^-4 or more -- about one byte in 10^4, so one in
    # 10^2 would be a conversion that does not round to nearest
    keep = ~near.unsqueeze(-1).expand(cum, nkb, 32).reshape(cum, I)
    same = (q.view(torch.uint8)[:cum] == want_q.view(torch.uint8))[keep].double().mean().item() if cum else 1.0
    assert same >= 0.99, same


# ---- the layer ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_case(T, offset, G, with_params, method=M.RENORMALIZE, logits_dtype=torch.float32):
    """Inputs on the CPU and on the device, and the oracle's result.  E = 8, top_k = 2, H = 256, I = 128."""
    import flashinfer

    E, top_k, H, I = 8, 2, 256, 128
    g = torch.Generator().manual_seed(100 * T + 10 * offset + G + int(with_params))
    logits = M.tie_free_logits(T, E, seed=T + offset, dtype=logits_dtype)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    w1 = (torch.randn(G, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    w2 = (4 * torch.randn(G, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)  # outputs of order 1: well above the atol
    x_q, x_sf = flashinfer.mxfp8_quantize(x.to(DEV), False)
    w1_q, w1_sf = flashinfer.mxfp4_quantize_grouped(w1.to(DEV))
    w2_q, w2_sf = flashinfer.mxfp4_quantize_grouped(w2.to(DEV))
    p = dict(bias1=None, alpha=None, beta=None, limit=None, bias2=None)
    if with_params:
        p = dict(bias1=0.5 * torch.randn(G, 2 * I, generator=g), alpha=torch.full((G,), 1.702), beta=torch.ones(G),
                 limit=torch.full((G,), 2.0), bias2=0.5 * torch.randn(G, H, generator=g))
    lin = lambda sf, n, nkb: torch.stack([R.unswizzle(sf[i].cpu().reshape(-1), n, nkb) for i in range(G)])  # noqa: E731
    want = M.moe_ref(logits, x_q.cpu(), x_sf.cpu().view(T, H // 32), w1_q.cpu(), lin(w1_sf, 2 * I, H // 32), w2_q.cpu(),
                     lin(w2_sf, H, I // 32), top_k, method, offset, G, **p)
    dev = {k: None if v is None else v.to(DEV) for k, v in p.items()}
    args = dict(
        routing_logits=logits.to(DEV), routing_bias=None, hidden_states=x_q, hidden_states_scale=x_sf.view(T, H // 32),
        gemm1_weights=w1_q, gemm1_weights_scale=w1_sf, gemm1_bias=dev["bias1"], gemm1_alpha=dev["alpha"],
        gemm1_beta=dev["beta"], gemm1_clamp_limit=dev["limit"], gemm2_weights=w2_q, gemm2_weights_scale=w2_sf,
        gemm2_bias=dev["bias2"], output1_scale_scalar=None, output1_scale_gate_scalar=None, output2_scale_scalar=None,
        num_experts=E, top_k=top_k, n_group=None, topk_group=None, intermediate_size=I, local_expert_offset=offset,
        local_num_experts=G, routed_scaling_factor=None, routing_method_type=method)
    return args, want


def check_accuracy(a, b, atol, rtol, percent):
    """The reference's check (tests/moe/test_trtllm_gen_fused_moe.py:1262-1284): a the oracle, b the result."""
    assert not torch.isnan(a).any() and not torch.isnan(b).any() and not torch.isinf(a).any() and not torch.isinf(b).any()
    assert a.shape == b.shape
    mismatch = ((a - b).abs() > atol + rtol * b.abs()).double().mean().item()
    assert mismatch <= 1 - percent, f"mismatch {mismatch:.4f} over {1 - percent:.4f}"


LAYER_CASES = [(1, 0, 8, False), (67, 0, 8, False), (67, 0, 8, True), (67, 2, 3, True)]
LAYER_IDS = ["T1", "T67", "T67_params", "T67_local_window"]


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("T,offset,G,with_params", LAYER_CASES, ids=LAYER_IDS)
def test_layer_is_its_stages_and_meets_the_reference_bar(T, offset, G, with_params):
    F = _fm()
    from flashinfer.gemm import _group_gemm_mxfp4_into

    args, want = _layer_case(T, offset, G, with_params)
    (out,) = F.trtllm_fp4_block_scale_moe(**args)
    assert out.shape == (T, 256) and out.dtype == torch.bfloat16
    # 1. the stages and the GEMM by hand
    H, I, top_k = 256, 128, args["top_k"]
    ids, w = F.moe_route(args["routing_logits"], top_k, args["routing_method_type"])
    m_indptr, emap, x_perm, sf_perm = F.moe_permute_mxfp8(ids, args["hidden_states"], args["hidden_states_scale"], offset, G)
    y1 = torch.empty(T * top_k, 2 * I, dtype=torch.bfloat16, device=DEV)
    _group_gemm_mxfp4_into(x_perm, args["gemm1_weights"], sf_perm, args["gemm1_weights_scale"], y1, m_indptr, 2 * I, H)
    act, act_sf = F.moe_gated_act_mxfp8(y1, m_indptr, args["gemm1_bias"], args["gemm1_alpha"], args["gemm1_beta"],
                                        args["gemm1_clamp_limit"])
    y2 = torch.empty(T * top_k, H, dtype=torch.bfloat16, device=DEV)
    _group_gemm_mxfp4_into(act, args["gemm2_weights"], act_sf, args["gemm2_weights_scale"], y2, m_indptr, H, I)
    by_hand = F.moe_finalize(y2, w, emap, args["gemm2_bias"], m_indptr)
    assert torch.equal(_bits(out), _bits(by_hand))
    # 2. finalize on the do_finalize=False triple (the bias belongs to finalize)
    triple = F.trtllm_fp4_block_scale_moe(**{**args, "gemm2_bias": None}, do_finalize=False)
    assert [t.dtype for t in triple] == [torch.bfloat16, torch.bfloat16, torch.int32]
    assert [tuple(t.shape) for t in triple] == [(T * top_k, H), (T, top_k), (T * top_k,)]
    assert torch.equal(triple[2], emap) and torch.equal(_bits(triple[1]), _bits(w))
    again = F.moe_finalize(triple[0], triple[1], triple[2], args["gemm2_bias"], m_indptr)
    assert torch.equal(_bits(out), _bits(again))
    # 3. the routed call on the packed output of moe_route
    routed_args = {k: v for k, v in args.items() if k != "routing_logits"}
    packed = M.pack_topk_ids(ids.cpu(), w.cpu()).to(DEV)
    (routed,) = F.trtllm_fp4_block_scale_routed_moe(packed, **routed_args)
    assert torch.equal(_bits(out), _bits(routed))
    # 4. the oracle, at the reference's bar for this mode: wiring (halves, experts, scale rows), not rounding
    torch.cuda.synchronize()
    check_accuracy(want, out.cpu().double(), atol=0.1, rtol=0.85, percent=0.925)


@pytest.mark.parametrize("method", [M.DEFAULT, M.RENORMALIZE_NAIVE, M.TOPK], ids=METHOD_NAMES.get)
def test_layer_with_the_other_routing_methods_and_bf16_logits(method):
    F = _fm()
    args, want = _layer_case(67, 0, 8, True, method, torch.bfloat16)
    (out,) = F.trtllm_fp4_block_scale_moe(**args)
    torch.cuda.synchronize()
    check_accuracy(want, out.cpu().double(), atol=0.1, rtol=0.85, percent=0.925)


# ---- finalize -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,offset,G,with_params", LAYER_CASES, ids=LAYER_IDS)
def test_finalize_on_the_devices_own_outputs(T, offset, G, with_params):
    F = _fm()
    args, _ = _layer_case(T, offset, G, with_params)
    top_k, H = args["top_k"], 256
    y2, w, emap = F.trtllm_fp4_block_scale_moe(**{**args, "gemm2_bias": None}, do_finalize=False)
    ids, _ = F.moe_route(args["routing_logits"], top_k, args["routing_method_type"])
    m_indptr = F.moe_permute_mxfp8(ids, args["hidden_states"], args["hidden_states_scale"], offset, G)[0]
    given = torch.full((T, H), 7.0, dtype=torch.bfloat16, device=DEV)
    out = F.moe_finalize(y2, w, emap, args["gemm2_bias"], m_indptr, output=given)
    assert out is given  # written in place
    torch.cuda.synchronize()
    cum = int(m_indptr[-1])
    y_cpu = y2.cpu()
    y_cpu[cum:] = 0  # rows past the local count are unwritten and never read
    bias = None if args["gemm2_bias"] is None else args["gemm2_bias"].cpu()
    want, mag = M.finalize_ref(y_cpu, w.cpu(), emap.cpu(), top_k, bias, m_indptr.cpu())
    # bf16 rounding of the result plus f32 accumulation of at most 8 terms
    err = (out.cpu().double() - want).abs()
    assert bool((err <= 2.0 ** -8 * mag).all()), (err - 2.0 ** -8 * mag).max().item()
    no_local = (emap.cpu().view(T, top_k) < 0).all(dim=1)
    if G < 8:
        assert no_local.any() and not no_local.all()
    assert not out.cpu()[no_local].view(torch.int16).any()  # exact zeros, +0
    # without a bias no m_indptr is needed
    plain = F.moe_finalize(y2, w, emap)
    want0, mag0 = M.finalize_ref(y_cpu, w.cpu(), emap.cpu(), top_k)
    assert bool(((plain.cpu().double() - want0).abs() <= 2.0 ** -8 * mag0).all())


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("H", [8, 2056])
def test_finalize_on_made_up_inputs(H, with_bias):
    """The row team at its ends: H = 8 is one chunk of 8 columns (a one-quad team with three idle lanes), H = 2056 is 257
    chunks (one lane of the 256-thread team takes a second pass).  T = 5, top_k = 2, G = 3 with an empty group; token 3
    has no local slot."""
    F = _fm()
    T, top_k = 5, 2
    g = torch.Generator().manual_seed(H + int(with_bias))
    emap = torch.tensor([0, 3, -1, 4, 1, -1, -1, -1, 5, 2], dtype=torch.int32)
    m_indptr = torch.tensor([0, 3, 3, 6], dtype=torch.int32)
    y = torch.randn(T * top_k, H, generator=g).to(torch.bfloat16)  # rows 6 .. 9 are past the local count: never read
    w = torch.randn(T, top_k, generator=g).to(torch.bfloat16)
    bias = torch.randn(3, H, generator=g) if with_bias else None
    out = F.moe_finalize(y.to(DEV), w.to(DEV), emap.to(DEV), None if bias is None else bias.to(DEV),
                         m_indptr.to(DEV) if with_bias else None)
    torch.cuda.synchronize()
    assert out.shape == (T, H) and out.dtype == torch.bfloat16
    want, mag = M.finalize_ref(y, w, emap, top_k, bias, m_indptr if with_bias else None)
    err = (out.cpu().double() - want).abs()
    assert bool((err <= 2.0 ** -8 * mag).all()), (err - 2.0 ** -8 * mag).max().item()
    assert mag[[0, 1, 2, 4]].all() and not out.cpu()[3].view(torch.int16).any()  # exact zeros, +0


# ---- graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    F = _fm()
    args_a, _ = _layer_case(67, 0, 8, True)
    args_b, _ = _layer_case(67, 2, 3, True)  # other logits and activations of the same shapes
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
