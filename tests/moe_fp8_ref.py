"""CPU oracle of the fp8 block-scale MoE layer (tests/test_fused_moe_fp8_cpu.py, tests/test_fused_moe_fp8_gpu.py): plain
torch, fp64, no kernel.  Routing, the permutation, the activation and finalize are tests/moe_ref.py's and
tests/moe_sigmoid_ref.py's; here is what the format adds:

  * the dequantisation of the reference's test (dequant_reference_dsfp8, tests/moe/test_trtllm_gen_fused_moe.py:1458-1481):
    a weight element times the scale of its 128 x 128 block, an activation element times the scale of its token and 128
    columns, the latter stored [H / 128, T];
  * the block rule of include/fi_mi355.h: per row and 128 columns s = max(amax / 448, 2^-126), q = e4m3(clamp(x / s, -448,
    448)) rounded to nearest even -- in fp64, or with the scale computed in f32 as the device does;
  * which quotients lie so close to a rounding boundary of e4m3 that an f32 device may round them the other way;
  * the whole layer as the device runs it, the bf16 rounding after GEMM1 included.
"""
import torch

import moe_ref as M
import moe_sigmoid_ref as S

BLOCK = 128
FLOOR = 2.0 ** -126


# ---- dequantisation ---------------------------------------------------------------------------------------------------
def dequant_activations(x_q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x_q float8_e4m3fn [T, H], scale [H / 128, T] (any strides) -> fp64 [T, H]."""
    T, H = x_q.shape
    assert tuple(scale.shape) == (H // BLOCK, T)
    return x_q.to(torch.float32).double() * scale.double().t().repeat_interleave(BLOCK, dim=1)


def dequant_rows(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """q float8_e4m3fn [m, k], scale [m, k / 128] row-major -> fp64 [m, k]."""
    return q.to(torch.float32).double() * scale.double().repeat_interleave(BLOCK, dim=1)


def dequant_weights(w_q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """w_q float8_e4m3fn [G, n, k], scale [G, n / 128, k / 128] -> fp64 [G, n, k]."""
    G, n, k = w_q.shape
    assert tuple(scale.shape) == (G, n // BLOCK, k // BLOCK)
    return w_q.to(torch.float32).double() * scale.double().repeat_interleave(BLOCK, dim=1).repeat_interleave(BLOCK, dim=2)


# ---- the block rule ---------------------------------------------------------------------------------------------------
def to_e4m3(y: torch.Tensor) -> torch.Tensor:
    """fp64 -> float8_e4m3fn, clamped to +-448 first (0x7F is NaN), round to nearest even.  The f32 step in between is
    harmless: an fp64 value that f32 rounds onto a tie of e4m3's 4-bit grid lies within 2^-25 of it."""
    return y.clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn)


def block_scale(amax: torch.Tensor) -> torch.Tensor:
    """max(amax / 448, 2^-126) in the dtype of amax: fp64 for the oracle, f32 for what the device computes bit for bit
    from an exact amax (IEEE division is correctly rounded)."""
    return torch.clamp(amax / 448.0, min=FLOOR)


def block_quantize_ref(x: torch.Tensor, scale_dtype=torch.float64):
    """x [m, k] (any float dtype) -> (q float8_e4m3fn [m, k], s [m, k / 128] of scale_dtype).  The quotient is always
    taken in fp64, of the exact x and the scale as stored."""
    m, k = x.shape
    assert k % BLOCK == 0
    blocks = x.double().view(m, k // BLOCK, BLOCK)
    s = block_scale(blocks.abs().amax(dim=-1).to(scale_dtype))
    y = blocks / s.double().unsqueeze(-1)
    return to_e4m3(y).view(m, k), s


def e4m3_step(v: torch.Tensor) -> torch.Tensor:
    """Spacing of e4m3 at |v| <= 448 (fp64): 2^(floor(log2 |v|) - 3), the subnormal spacing 2^-9 below 2^-6."""
    e = torch.frexp(v.abs().clamp(min=2.0 ** -6))[1] - 1
    return torch.exp2(e.double() - 3)


def near_rounding_boundary(y: torch.Tensor, rel: float = 2.0 ** -20) -> torch.Tensor:
    """Where the quotient y (fp64, |y| <= 448) lies within rel * |y| of a midpoint between two neighbouring e4m3 values: a
    device that computes y in f32 (relative error ~2^-24 of the division, 2^-22 with an f32 activation in front) may
    round such a value either way; any other value it must round as the oracle does."""
    step = e4m3_step(y)
    frac = torch.remainder(y.abs() / step, 1.0)
    return (frac - 0.5).abs() * step <= rel * y.abs()


def quantize_weights_ref(w: torch.Tensor):
    """w [G, n, k] -> (float8_e4m3fn [G, n, k], f32 scales [G, n / 128, k / 128]): amax / 448 per 128 x 128 block, which is
    no power of two for random weights (DeepSeek's checkpoints are made like this)."""
    G, n, k = w.shape
    blocks = w.double().view(G, n // BLOCK, BLOCK, k // BLOCK, BLOCK)
    scale = block_scale(blocks.abs().amax(dim=(2, 4)).float())
    q = to_e4m3(blocks / scale.double()[:, :, None, :, None]).view(G, n, k)
    return q, scale


# ---- inputs of the quantiser's tests ----------------------------------------------------------------------------------
QUANT_SHAPES = [(1, 128), (1, 4224), (67, 128), (67, 4224)]  # H = 4224: 528 chunks of 8 columns, three team passes


def quantiser_input(T: int, H: int) -> torch.Tensor:
    """bf16 [T, H]: normal values with a per-row magnitude of 2^-3 .. 2^3, one all-zero block when there are two."""
    g = torch.Generator().manual_seed(1000 * T + H)
    x = (torch.randn(T, H, generator=g) * torch.exp2(torch.randint(-3, 4, (T, 1), generator=g).float())).to(torch.bfloat16)
    if H > 128:
        x[0, 128:256] = 0
    return x


# ---- the layer --------------------------------------------------------------------------------------------------------
def moe_fp8_ref(logits, x_q, x_scale, w1_q, w1_scale, w2_q, w2_scale, top_k, method, offset, num_local, routing_bias=None,
                n_group=None, topk_group=None, routed_scaling_factor=None) -> torch.Tensor:
    """The layer as the device runs it: x_q [T, H] with x_scale [H / 128, T]; w1_q [G, 2 I, H], w2_q [G, H, I] with their
    128 x 128 scales.  Routing weights are rounded to bf16 and GEMM1's output is rounded to bf16 before the activation, as
    on the device.  Returns fp64 [T, H]."""
    if method == S.DEEPSEEK_V3:
        ids, w = S.route_sigmoid_ref(logits, routing_bias, n_group, topk_group, top_k, routed_scaling_factor, method)
    else:
        ids, w = M.route_ref(logits, top_k, method)
    w = w.to(torch.bfloat16)
    m_indptr, emap, inverse = M.permute_ref(ids, offset, num_local)
    ms = M.segments(m_indptr)
    tokens = torch.tensor([i // top_k for i in inverse], dtype=torch.long)
    a = dequant_activations(x_q, x_scale)[tokens]
    b1, b2 = dequant_weights(w1_q, w1_scale), dequant_weights(w2_q, w2_scale)
    y1 = torch.zeros(sum(ms), b1.shape[1], dtype=torch.float64)
    begin = 0
    for g, m in enumerate(ms):
        y1[begin:begin + m] = a[begin:begin + m] @ b1[g].T
        begin += m
    act = M.gated_act_ref(y1.to(torch.bfloat16), m_indptr)
    q, s = block_quantize_ref(act)
    a2 = dequant_rows(q, s)
    y2 = torch.zeros(sum(ms), b2.shape[1], dtype=torch.float64)
    begin = 0
    for g, m in enumerate(ms):
        y2[begin:begin + m] = a2[begin:begin + m] @ b2[g].T
        begin += m
    return M.finalize_ref(y2, w, emap, top_k)[0]
