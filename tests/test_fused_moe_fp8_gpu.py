"""GPU: the fp8 block-scale MoE layer (flashinfer.fused_moe_fp8.trtllm_fp8_block_scale_moe; csrc/moe.hip,
csrc/fp8_block_quantize.hip) stage by stage against the fp64 oracle of tests/moe_fp8_ref.py, exact where exactness is
possible, then the whole layer: bit-identical to its stages called by hand, and against the oracle at the reference's own bar
for this mode.

Shapes are the smallest at which each kernel can still go wrong: E = 8, top_k = 2, H = 256 (two k blocks with T != H / 128,
so a transposed or mis-strided scale read shows), I = 128, and one size past the 256-thread row team (H = 4224, I = 2176)
for its further passes.  The ids of the permutation and the segments of the activation are the existing MXFP8 test's."""
import functools

import pytest
import torch

import moe_fp8_ref as R8
import moe_ref as M
import moe_sigmoid_ref as S
from test_fused_moe_gpu import ACT_SEGMENTS, PERMUTE_CASES, check_accuracy

pytestmark = pytest.mark.gpu

DEV = "cuda"
E4M3 = torch.float8_e4m3fn


def _fm():
    from flashinfer import fused_moe

    return fused_moe


def _layer():
    from flashinfer import fused_moe_fp8

    return fused_moe_fp8.trtllm_fp8_block_scale_moe


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- permute, and the grouped GEMM on its output ----------------------------------------------------------------------------
FP8_PERMUTE_CASES = ["empty_expert", "one_expert_crosses_a_scale_tile", "local_window", "512_experts"]


def _random_activations(T, H, seed):
    """Any bytes but NaN, any positive normal scales: the gather moves them, nothing computes with them.  The scales are
    made [T, H / 128], as the reference's test holds them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (T, H), dtype=torch.uint8, generator=g)
    x[(x & 0x7F) == 0x7F] = 0
    scale_tk = torch.rand(T, H // 128, generator=g) + 0.25
    return x.view(E4M3), scale_tk


def _check_permute(ids, offset, G, x_q, scale_tk):
    """x_q e4m3 [T, H] and its scales [T, H / 128] on the CPU.  Returns the device's outputs of the contiguous run."""
    F = _fm()
    T, top_k = ids.shape
    H = x_q.shape[1]
    n, nkb = T * top_k, H // 128
    dev_ids, dev_x = ids.to(DEV), x_q.to(DEV)
    as_view = scale_tk.to(DEV).t()                 # [H / 128, T] with strides (1, H / 128): the reference test's spelling
    contiguous = scale_tk.t().contiguous().to(DEV)  # [H / 128, T] with strides (T, 1)
    assert as_view.shape == contiguous.shape == (nkb, T) and (nkb == 1 or T == 1 or as_view.stride() != contiguous.stride())
    want_indptr, want_map, inverse = M.permute_ref(ids, offset, G)
    cum = int(want_indptr[-1])
    tokens = torch.tensor([i // top_k for i in inverse], dtype=torch.long)
    mx = F.moe_permute_mxfp8(dev_ids, dev_x, torch.zeros(T, H // 32, dtype=torch.uint8, device=DEV), offset, G)
    results = []
    for scale in (contiguous, as_view):
        m_indptr, emap, x_perm, s_perm = F.moe_permute_fp8_block(dev_ids, dev_x, scale, offset, G)
        assert x_perm.shape == (n, H) and x_perm.dtype == E4M3 and s_perm.shape == (n, nkb) and s_perm.dtype == torch.float32
        assert s_perm.is_contiguous()
        # the same sort as the MXFP8 permutation, and the oracle's
        assert torch.equal(m_indptr, mx[0]) and torch.equal(emap, mx[1])
        assert torch.equal(m_indptr.cpu(), want_indptr) and torch.equal(emap.cpu(), want_map)
        # once more into prefilled buffers: x rows past the local count are untouched, scale rows there are 1.0
        x2 = torch.full((n, H), 0x55, dtype=torch.uint8, device=DEV).view(E4M3)
        s2 = torch.full((n, nkb), float("nan"), dtype=torch.float32, device=DEV)
        F._permute_fp8_block_into(dev_ids, dev_x, scale, offset, G, False, torch.empty_like(m_indptr), torch.empty_like(emap),
                                  x2, s2, None)
        torch.cuda.synchronize()
        for xp, sp in ((x_perm, s_perm), (x2, s2)):
            assert torch.equal(_u8(xp.cpu())[:cum], _u8(x_q)[tokens])
            assert torch.equal(_bits(sp.cpu())[:cum], _bits(scale_tk[tokens].contiguous()))
            assert bool((sp.cpu()[cum:] == 1.0).all())
        assert bool((_u8(x2.cpu())[cum:] == 0x55).all())
        results.append((m_indptr, emap, x2, s2))
    # both spellings of the scales give identical bytes
    assert torch.equal(_u8(results[0][2]), _u8(results[1][2])) and torch.equal(_bits(results[0][3]), _bits(results[1][3]))
    return results[0]


@pytest.mark.parametrize("case", FP8_PERMUTE_CASES)
def test_permute_is_exact(case):
    build, offset, G = PERMUTE_CASES[case]
    ids = build()
    T = ids.shape[0]
    assert T != 2  # T != H / 128 at H = 256
    _check_permute(ids, offset, G, *_random_activations(T, 256, seed=T))
    if case == "empty_expert":
        # 264 sixteen-byte chunks, more than the 256-thread row team: its second pass moves the scale of k block 32
        _check_permute(ids, offset, G, *_random_activations(T, 4224, seed=T + 1))


def test_grouped_gemm_on_the_permuted_rows_of_a_local_window():
    """_group_gemm_fp8_into with a.shape[0] > m_indptr[-1], which a local expert window produces: live rows are exact
    against fp64 (small integers, power-of-two scales: every product and sum is exact in f32 and the results in bf16),
    rows of a prefilled `out` past the local count are untouched.  The rows of x_permuted past the count hold 0x55 bytes
    and those of `out` a pattern: were they loaded or stored it would show."""
    from flashinfer.gemm import _group_gemm_fp8_into

    build, offset, G = PERMUTE_CASES["local_window"]
    ids = build()
    T, top_k = ids.shape
    H, N = 256, 128
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-1, 2, (T, H), generator=g).float().to(E4M3)
    scale_tk = torch.exp2(torch.randint(0, 2, (T, H // 128), generator=g).float())
    w = torch.randint(-1, 2, (G, N, H), generator=g).float().to(E4M3)
    w_scale = torch.exp2(torch.randint(-1, 1, (G, N // 128, H // 128), generator=g).float())
    m_indptr, emap, x_perm, s_perm = _check_permute(ids, offset, G, x, scale_tk)
    cum = int(m_indptr[-1])
    n = T * top_k
    assert 0 < cum < n
    want = torch.zeros(cum, N, dtype=torch.float64)
    a = R8.dequant_rows(x_perm.cpu()[:cum], s_perm.cpu()[:cum])
    b = R8.dequant_weights(w, w_scale)
    for gi, (lo, hi) in enumerate(zip(m_indptr.cpu().tolist()[:-1], m_indptr.cpu().tolist()[1:])):
        want[lo:hi] = a[lo:hi] @ b[gi].T
    assert torch.equal(want.to(torch.bfloat16).double(), want) and want.abs().max() > 8  # exact in bf16, and not trivial
    out = torch.full((n, N), -7.0, dtype=torch.bfloat16, device=DEV)
    _group_gemm_fp8_into(x_perm, w.to(DEV), s_perm, w_scale.to(DEV), out, m_indptr)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu()[:cum].double(), want)
    assert bool((out.cpu()[cum:] == -7.0).all())
    with pytest.raises(ValueError, match="contiguous"):
        _group_gemm_fp8_into(x_perm, w.to(DEV), s_perm, w_scale.to(DEV), out.t(), m_indptr)


# ---- gated activation ---------------------------------------------------------------------------------------------------
ACT_CASES = [(s, I) for s in sorted(ACT_SEGMENTS) for I in (128, 256)] + [("ragged", 2176), ("small", 2176)]
EXTRA = 8  # rows past m_indptr[-1]


@functools.lru_cache(maxsize=None)
def _act_case(segments, I):
    cum = sum(segments)
    g = torch.Generator().manual_seed(cum + I)
    x = (torch.randn(cum + EXTRA, 2 * I, generator=g) * 2).to(torch.bfloat16)
    if cum:
        x[0, :128] = 0  # the linear half of block 0 of row 0: an all-zero block of the activation
    indptr = torch.tensor([0] + list(torch.tensor(segments).cumsum(0)), dtype=torch.int32)
    want = M.gated_act_ref(x[:cum], indptr)
    return x, indptr, want


@pytest.mark.parametrize("segments,I", ACT_CASES)
def test_gated_activation_against_the_oracle(segments, I):
    F = _fm()
    segs = ACT_SEGMENTS[segments]
    x, indptr, want = _act_case(segs, I)
    cum, nkb = sum(segs), I // 128
    want_q, want_s = R8.block_quantize_ref(want)
    q, s = F.moe_gated_act_fp8_block(x.to(DEV), indptr.to(DEV))
    assert q.shape == (cum + EXTRA, I) and q.dtype == E4M3 and s.shape == (cum + EXTRA, nkb) and s.dtype == torch.float32
    # again into prefilled buffers: rows of q past m_indptr[-1] are untouched, every scale is written, 1.0 past the count
    q2 = torch.full((cum + EXTRA, I), 0x55, dtype=torch.uint8, device=DEV).view(E4M3)
    s2 = torch.full((cum + EXTRA, nkb), float("nan"), dtype=torch.float32, device=DEV)
    F._gated_act_fp8_block_into(x.to(DEV), indptr.to(DEV), q2, s2)
    torch.cuda.synchronize()
    q, s, q2, s2 = q.cpu(), s.cpu(), q2.cpu(), s2.cpu()
    assert torch.equal(_bits(s), _bits(s2)) and torch.equal(_u8(q)[:cum], _u8(q2)[:cum])
    assert bool((_u8(q2)[cum:] == 0x55).all()) and bool((s[cum:] == 1.0).all())
    assert not bool(((_u8(q)[:cum] & 0x7F) == 0x7F).any())  # no NaN byte
    # the all-zero block (a negative gate times the zero linear half is -0: the byte is 0x00 or 0x80)
    assert not (_u8(q)[0, :128] & 0x7F).any() and s[0, 0].item() == 2.0 ** -126 and want_s[0, 0].item() == 2.0 ** -126
    # the scale: f32 SwiGLU against fp64 within relative 2^-20, the margin the MXFP8 test grants it, and the division
    got_s = s[:cum].double()
    rel = ((got_s - want_s).abs() / want_s).max().item()
    print(f"scale: max relative error {rel:.3e} (bar {2.0 ** -20:.3e})")
    assert rel <= 2.0 ** -20
    # the values: within one e4m3 step, at the oracle's scale, of the fp64 activation -- half a step is the format's
    # rounding, the other half lets f32 rounding move a value across a rounding boundary
    scale = want_s.unsqueeze(-1)
    got = (q[:cum].float().double().view(cum, nkb, 128) * got_s.unsqueeze(-1))
    want_b = want.view(cum, nkb, 128)
    step = R8.e4m3_step(torch.maximum(want_b.abs(), got.abs()) / scale) * scale
    bad = (got - want_b).abs() > step
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements are off by more than one step"
    # nearly every byte is the oracle's own.  The MXFP8 test sets aside the blocks whose amax sits on a scale threshold;
    # this format has none (the scale is amax / 448, continuous in amax), so every block counts.  An f32 quotient is
    # within ~2^-21 of the fp64 one, a rounding boundary is 1 / 32 to 1 / 16 of a value away: about one byte in 10^4
    # may differ, so one in 10^2 would be a conversion that does not round to nearest.
    same = (_u8(q)[:cum] == _u8(want_q)).double().mean().item()
    print(f"bytes equal to the oracle's: {same:.6f}")
    assert same >= 0.99, same


def test_gated_activation_on_hand_made_rows():
    """Blocks whose result is known exactly: gate 0 gives act 0 whatever the linear half (an all-zero block: q = 0,
    s = 2^-126, no NaN byte); a row whose act is the same value everywhere gets that value / 448 as its scale and 0x7E."""
    F = _fm()
    I = 256
    x = torch.zeros(3, 2 * I, dtype=torch.bfloat16)
    x[0, :I] = 3.0               # gate 0: act = 0 * 0.5 * 3 = 0 in both blocks
    x[1, :I], x[1, I:] = 2.0, 0.0
    x[1, 5], x[1, I + 5] = 4.0, 1.0  # one live element in block 0 of row 1: act = sigmoid(1) * 4
    x[2, :I], x[2, I:] = -1.5, 2.0   # act = 2 sigmoid(2) * -1.5 everywhere
    indptr = torch.tensor([0, 2, 3], dtype=torch.int32)
    q, s = F.moe_gated_act_fp8_block(x.to(DEV), indptr.to(DEV))
    torch.cuda.synchronize()
    q, s = q.cpu(), s.cpu()
    assert not _u8(q)[0].any() and s[0].tolist() == [2.0 ** -126] * 2
    live = torch.zeros(I, dtype=torch.uint8)
    live[5] = 0x7E
    assert torch.equal(_u8(q)[1], live) and s[1, 1].item() == 2.0 ** -126
    assert abs(s[1, 0].item() / (4 / (1 + torch.exp(torch.tensor(-1.0, dtype=torch.float64))).item() / 448) - 1) <= 2.0 ** -20
    assert bool((_u8(q)[2] == 0xFE).all()) and s[2, 0].item() == s[2, 1].item()
    assert not bool(((_u8(q) & 0x7F) == 0x7F).any())


# ---- the quantiser --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,H", R8.QUANT_SHAPES)
def test_fp8_quantize_1x128(T, H):
    from flashinfer.fp8_quantization import fp8_quantize_1x128

    x = R8.quantiser_input(T, H)
    q, s = fp8_quantize_1x128(x.to(DEV))
    torch.cuda.synchronize()
    nkb = H // 128
    assert q.shape == (T, H) and q.dtype == E4M3 and s.shape == (nkb, T) and s.dtype == torch.float32 and s.is_contiguous()
    q, s = q.cpu(), s.cpu()
    # scales: the amax of bf16 values is exact and IEEE division is correctly rounded -- bit-equal to f32 torch
    want_s = torch.clamp(x.float().view(T, nkb, 128).abs().amax(-1) / 448, min=2.0 ** -126)
    assert torch.equal(_bits(s.t().contiguous()), _bits(want_s))
    if H > 128:
        assert s[1, 0].item() == 2.0 ** -126 and not _u8(q)[0, 128:256].any()  # the all-zero block
    # bytes: the oracle's, except where the fp64 quotient lies within 2^-20 of a rounding boundary
    want_q, s32 = R8.block_quantize_ref(x, torch.float32)
    assert torch.equal(s32, want_s)
    y = x.double().view(T, nkb, 128) / want_s.double().unsqueeze(-1)
    near = R8.near_rounding_boundary(y).view(T, H)
    assert near.double().mean().item() <= 0.01
    differ = _u8(q) != _u8(want_q)
    assert not bool((differ & ~near).any()), f"{int((differ & ~near).sum())} bytes differ off the rounding boundaries"
    assert not bool(((_u8(q) & 0x7F) == 0x7F).any())
    # f16 input and a strided view go the same way
    if (T, H) == (67, 128):
        wide = torch.zeros(T, 3 * H, dtype=torch.bfloat16)
        wide[:, H:2 * H] = x
        q2, s2 = fp8_quantize_1x128(wide.to(DEV)[:, H:2 * H])
        assert torch.equal(_u8(q2.cpu()), _u8(q)) and torch.equal(_bits(s2.cpu()), _bits(s))
        xh = x.to(torch.float16)
        qh, sh = fp8_quantize_1x128(xh.to(DEV))
        assert torch.equal(_bits(sh.cpu().t().contiguous()),
                           _bits(torch.clamp(xh.float().view(T, nkb, 128).abs().amax(-1) / 448, min=2.0 ** -126)))


def test_fp8_quantize_1x128_on_hand_made_blocks():
    """amax exactly 448 * 2^e: the scale is 2^e and the maximum becomes 0x7E; a value whose quotient rounds to 448; an all-zero
    block.  The oracle's answers to these are checked on the CPU (test_block_rule_on_hand_made_blocks)."""
    from flashinfer.fp8_quantization import fp8_quantize_1x128

    x = torch.zeros(3, 256, dtype=torch.bfloat16)
    x[0, 5], x[0, 6] = 448 * 2.0 ** -3, -2.0 ** -3
    x[0, 128 + 9], x[0, 128 + 10] = -448 * 2.0 ** 5, 3 * 2.0 ** 5
    x[1, 0], x[1, 1], x[1, 2] = 7.0, 6.90625, 6.6875  # bf16-exact; 442 and 428 of 448: up to 448, down to 416
    x[2, 128:] = 1.0
    q, s = fp8_quantize_1x128(x.to(DEV))
    torch.cuda.synchronize()
    want_q, want_s = R8.block_quantize_ref(x, torch.float32)
    assert torch.equal(_u8(q.cpu()), _u8(want_q)) and torch.equal(_bits(s.cpu().t().contiguous()), _bits(want_s))
    q, s = q.cpu(), s.cpu()
    assert s[:, 0].tolist() == [2.0 ** -3, 2.0 ** 5] and _u8(q)[0, 5].item() == 0x7E and _u8(q)[0, 128 + 9].item() == 0xFE
    assert q[0, 6].float().item() == -1.0 and q[0, 128 + 10].float().item() == 3.0
    assert _u8(q)[1, :3].tolist() == [0x7E, 0x7E, 0x7D] and q[1, 2].float().item() == 416.0
    assert s[0, 2].item() == 2.0 ** -126 and not _u8(q)[2, :128].any() and bool((_u8(q)[2, 128:] == 0x7E).all())


# ---- the layer ------------------------------------------------------------------------------------------------------------
E, TOP_K, H, I = 8, 2, 256, 128


@functools.lru_cache(maxsize=None)
def _layer_case(T, offset, G, routing="renormalize", logits_dtype=torch.float32):
    """Inputs on the device and the oracle's result.  Activations come from fp8_quantize_1x128; weights are quantised on
    the CPU per 128 x 128 block (scales amax / 448: no powers of two)."""
    from flashinfer.fp8_quantization import fp8_quantize_1x128

    g = torch.Generator().manual_seed(100 * T + 10 * offset + G)
    x = torch.randn(T, H, generator=g).to(torch.bfloat16)
    w1 = torch.randn(G, 2 * I, H, generator=g) / H ** 0.5
    w2 = 4 * torch.randn(G, H, I, generator=g) / I ** 0.5  # outputs of order 1: well above the atol
    routing_args = dict(routing_bias=None, n_group=None, topk_group=None, routed_scaling_factor=None)
    if routing == "deepseek":
        logits, bias, _ = S.sigmoid_case(T, E, 4, seed=T + offset)
        routing_args = dict(routing_bias=bias, n_group=4, topk_group=2, routed_scaling_factor=2.5)
        method = S.DEEPSEEK_V3
    else:
        logits = M.tie_free_logits(T, E, seed=T + offset, dtype=logits_dtype)
        method = M.RENORMALIZE
    x_q, x_scale = fp8_quantize_1x128(x.to(DEV))
    w1_q, w1_s = R8.quantize_weights_ref(w1)
    w2_q, w2_s = R8.quantize_weights_ref(w2)
    for s in (w1_s, w2_s):  # no power of two among the weight scales
        assert bool((torch.frexp(s)[0] != 0.5).all())
    want = R8.moe_fp8_ref(logits, x_q.cpu(), x_scale.cpu(), w1_q, w1_s, w2_q, w2_s, TOP_K, method, offset, G, **routing_args)
    args = dict(
        routing_logits=logits.to(DEV), hidden_states=x_q, hidden_states_scale=x_scale, gemm1_weights=w1_q.to(DEV),
        gemm1_weights_scale=w1_s.to(DEV), gemm2_weights=w2_q.to(DEV), gemm2_weights_scale=w2_s.to(DEV), num_experts=E,
        top_k=TOP_K, intermediate_size=I, local_expert_offset=offset, local_num_experts=G, routing_method_type=method,
        **{k: v.to(DEV) if isinstance(v, torch.Tensor) else v for k, v in routing_args.items()})
    return args, want


LAYER_CASES = [(1, 0, 8, "renormalize", torch.float32), (67, 0, 8, "renormalize", torch.float32),
               (67, 2, 3, "renormalize", torch.float32), (67, 0, 8, "deepseek", torch.float32),
               (67, 0, 8, "renormalize", torch.bfloat16)]
LAYER_IDS = ["T1", "T67", "T67_local_window", "T67_deepseek_v3", "T67_bf16_logits"]


@pytest.mark.parametrize("T,offset,G,routing,logits_dtype", LAYER_CASES, ids=LAYER_IDS)
def test_layer_is_its_stages_and_meets_the_reference_bar(T, offset, G, routing, logits_dtype):
    F = _fm()
    from flashinfer.gemm import _group_gemm_fp8_into

    args, want = _layer_case(T, offset, G, routing, logits_dtype)
    out = _layer()(**args)
    assert isinstance(out, torch.Tensor) and out.shape == (T, H) and out.dtype == torch.bfloat16
    # (a) the stages and the GEMM by hand: bit-identical
    ids, w = F.moe_route(args["routing_logits"], TOP_K, args["routing_method_type"], routing_bias=args["routing_bias"],
                         n_group=args["n_group"], topk_group=args["topk_group"],
                         routed_scaling_factor=args["routed_scaling_factor"])
    m_indptr, emap, x_perm, s_perm = F.moe_permute_fp8_block(ids, args["hidden_states"], args["hidden_states_scale"], offset, G)
    y1 = torch.empty(T * TOP_K, 2 * I, dtype=torch.bfloat16, device=DEV)
    _group_gemm_fp8_into(x_perm, args["gemm1_weights"], s_perm, args["gemm1_weights_scale"], y1, m_indptr)
    act, act_s = F.moe_gated_act_fp8_block(y1, m_indptr)
    y2 = torch.empty(T * TOP_K, H, dtype=torch.bfloat16, device=DEV)
    _group_gemm_fp8_into(act, args["gemm2_weights"], act_s, args["gemm2_weights_scale"], y2, m_indptr)
    by_hand = F.moe_finalize(y2, w, emap)
    assert torch.equal(_bits(out), _bits(by_hand))
    # the scales as the transposed view of a [T, H / 128] tensor: the same bits
    view = args["hidden_states_scale"].t().contiguous().t()
    assert view.stride() != args["hidden_states_scale"].stride() or T == 1
    assert torch.equal(_bits(_layer()(**{**args, "hidden_states_scale": view})), _bits(out))
    # (b) the oracle, at the reference's bar for this mode (tests/moe/test_trtllm_gen_fused_moe.py:806-808)
    torch.cuda.synchronize()
    assert want.abs().mean().item() > 0.2  # outputs of order 1: the atol does not carry the check
    check_accuracy(want, out.cpu().double(), atol=0.1, rtol=0.85, percent=0.8)
    # (c) tokens without a local expert are exactly zero
    no_local = (emap.cpu().view(T, TOP_K) < 0).all(dim=1)
    if G < E:
        assert no_local.any() and not no_local.all()
    else:
        assert not no_local.any()
    assert not out.cpu()[no_local].view(torch.int16).any()  # exact zeros, +0
    assert bool(out.cpu()[~no_local].view(torch.int16).any(dim=1).all())


# ---- graph capture --------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result():
    F = _fm()
    args_a, _ = _layer_case(67, 0, 8)
    args_b, _ = _layer_case(67, 2, 3)  # other logits and activations of the same shapes
    static = dict(args_a)
    for name in ("routing_logits", "hidden_states", "hidden_states_scale"):
        static[name] = args_a[name].clone()
    eager_a = _layer()(**static)  # the eager warm-up call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _layer()(**static)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(captured), _bits(eager_a))
    for name in ("routing_logits", "hidden_states", "hidden_states_scale"):
        static[name].view(torch.uint8).copy_(args_b[name].view(torch.uint8))
    graph.replay()
    torch.cuda.synchronize()
    replayed = captured.clone()
    eager_b = _layer()(**static)
    torch.cuda.synchronize()
    assert torch.equal(_bits(replayed), _bits(eager_b))
    assert not torch.equal(_bits(eager_a), _bits(eager_b))
