"""CPU oracle of the MoE layer (tests/test_fused_moe_cpu.py, tests/test_fused_moe_gpu.py): plain torch, fp64, no kernel.

  * routing for the four methods provided (the reference's routing_reference_* functions, tests/moe/
    test_trtllm_gen_fused_moe.py:1209-1259, without their dense score matrix): ids by descending logit, ties to the
    lower expert, weights in fp64;
  * the permutation: the reference's routing_reference (:1083-1142) with padding 1, restricted to the local window;
  * the gated activation of compute_with_experts (tests/moe/test_trtllm_cutlass_fused_moe.py:195-203);
  * MXFP8 quantisation through mx_ref.mxfp8_quantize_ref;
  * finalize, and the whole layer as the device runs it, the bf16 rounding after GEMM1 included.
"""
import torch

import mx_ref as R

DEFAULT, RENORMALIZE, RENORMALIZE_NAIVE, TOPK = 0, 1, 4, 5
METHODS = (DEFAULT, RENORMALIZE, RENORMALIZE_NAIVE, TOPK)


def tie_free_logits(T: int, E: int, seed: int, dtype=torch.float32) -> torch.Tensor:
    """Every row a random permutation of (k - E / 2) / 8, k < E: exact in bf16 for E <= 512 and without ties, so the
    order of the experts does not depend on anybody's tie rule."""
    g = torch.Generator().manual_seed(seed)
    rows = [(torch.randperm(E, generator=g).double() - E // 2) / 8 for _ in range(T)]
    x = torch.stack(rows) if T else torch.zeros(0, E, dtype=torch.float64)
    assert torch.equal(x.to(torch.bfloat16).double(), x)
    return x.to(dtype)


def route_ref(logits: torch.Tensor, top_k: int, method: int):
    """logits [T, E] -> (ids int32 [T, top_k], weights fp64 [T, top_k]).  A stable descending sort: ties to the lower
    expert index."""
    x = logits.double()
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :top_k]
    chosen = torch.gather(x, 1, order)
    if method == TOPK:
        w = chosen
    elif method == RENORMALIZE:
        w = torch.softmax(chosen, dim=-1)
    else:
        w = torch.gather(torch.softmax(x, dim=-1), 1, order)
        if method == RENORMALIZE_NAIVE:
            w = w / w.sum(dim=-1, keepdim=True)
        else:
            assert method == DEFAULT
    return order.to(torch.int32), w


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 at |x| (fp64 in, fp64 out): 2^(floor(log2 |x|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    e = torch.frexp(x.abs().clamp(min=2.0 ** -126))[1] - 1
    return torch.exp2(e.double() - 7)


def pack_topk_ids(ids: torch.Tensor, weights_bf16: torch.Tensor) -> torch.Tensor:
    """The routed call's packing: low 16 bits the expert, high 16 bits the bf16 weight's bit pattern."""
    w = weights_bf16.view(torch.int16).to(torch.int32) & 0xFFFF
    packed = (w.to(torch.int64) << 16) | (ids.to(torch.int64) & 0xFFFF)
    return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)


def permute_ref(ids: torch.Tensor, offset: int, num_local: int):
    """ids [T, top_k] -> (m_indptr int32 [num_local + 1], expanded_idx_to_permuted_idx int32 [T * top_k],
    permuted_idx_to_expanded_idx list).  routing_reference with padding 1: expanded indices are walked in order and every
    expert's rows are handed out in that order; a slot on an expert outside [offset, offset + num_local) gets -1."""
    flat = ids.reshape(-1).tolist()
    counts = [0] * num_local
    in_expert = []
    for e in flat:
        le = e - offset
        if 0 <= le < num_local:
            in_expert.append(counts[le])
            counts[le] += 1
        else:
            in_expert.append(-1)
    indptr = [0]
    for c in counts:
        indptr.append(indptr[-1] + c)
    emap = [indptr[e - offset] + r if r >= 0 else -1 for e, r in zip(flat, in_expert)]
    inverse = [-1] * indptr[-1]
    for i, p in enumerate(emap):
        if p >= 0:
            inverse[p] = i
    return torch.tensor(indptr, dtype=torch.int32), torch.tensor(emap, dtype=torch.int32), inverse


def segments(m_indptr) -> tuple:
    m = [int(v) for v in m_indptr]
    return tuple(b - a for a, b in zip(m[:-1], m[1:]))


def gated_act_ref(x: torch.Tensor, m_indptr, bias=None, alpha=None, beta=None, limit=None) -> torch.Tensor:
    """x [cum_m, 2 I] (any float dtype) -> fp64 [m_indptr[-1], I]: columns [0, I) are the linear half, [I, 2 I) the gate."""
    ms = segments(m_indptr)
    I = x.shape[1] // 2
    out = torch.zeros(sum(ms), I, dtype=torch.float64)
    begin = 0
    for g, m in enumerate(ms):
        rows = x[begin:begin + m].double()
        x1, x2 = rows[:, :I], rows[:, I:]
        if bias is not None:
            x1 = x1 + bias[g, :I].double()
            x2 = x2 + bias[g, I:].double()
        lim = float("inf") if limit is None else float(limit[g])
        a = 1.0 if alpha is None else float(alpha[g])
        b = 0.0 if beta is None else float(beta[g])
        gate = x2.clamp(max=lim)
        lin = x1.clamp(min=-lim, max=lim) + b
        out[begin:begin + m] = gate * torch.sigmoid(a * gate) * lin
        begin += m
    return out


def quantize_act_ref(act: torch.Tensor):
    """fp64 [m, I] -> (q float8_e4m3fn [m, I], sf uint8 [m, I / 32]) by the rule of fi_mxfp8_quantize."""
    return R.mxfp8_quantize_ref(act)


def finalize_ref(y: torch.Tensor, weights: torch.Tensor, emap: torch.Tensor, top_k: int, bias=None, m_indptr=None):
    """y [rows, H], weights [T, top_k], emap [T * top_k] -> (fp64 [T, H], the sum of |terms| [T, H])."""
    T, H = weights.shape[0], y.shape[1]
    out = torch.zeros(T, H, dtype=torch.float64)
    mag = torch.zeros(T, H, dtype=torch.float64)
    bounds = None if m_indptr is None else [int(v) for v in m_indptr]
    for i, p in enumerate(emap.tolist()):
        if p < 0:
            continue
        row = y[p].double()
        if bias is not None:
            g = max(g for g in range(len(bounds) - 1) if bounds[g] <= p)
            row = row + bias[g].double()
        term = weights.reshape(-1)[i].double() * row
        out[i // top_k] += term
        mag[i // top_k] += term.abs()
    return out, mag


def moe_ref(logits, x_q, x_sf, w1, w1_sf, w2, w2_sf, top_k, method, offset, num_local, bias1=None, alpha=None, beta=None,
            limit=None, bias2=None) -> torch.Tensor:
    """The layer as the device runs it.  x_q float8_e4m3fn [T, H] with linear scales x_sf [T, H / 32]; w1 [G, 2 I, H / 2],
    w2 [G, H, I / 2] packed e2m1 with LINEAR scales w1_sf [G, 2 I, H / 32], w2_sf [G, H, I / 32].  Weights are rounded to
    bf16 and GEMM1's output is rounded to bf16 before the activation, as on the device.  Returns fp64 [T, H]."""
    ids, w = route_ref(logits, top_k, method)
    w = w.to(torch.bfloat16)
    m_indptr, emap, inverse = permute_ref(ids, offset, num_local)
    ms = segments(m_indptr)
    tokens = torch.tensor([i // top_k for i in inverse], dtype=torch.long)
    a = R.fp8_to_f64(x_q)[tokens]
    y1 = R.group_gemm_ref(a, x_sf[tokens], w1, w1_sf, ms).to(torch.bfloat16)
    act = gated_act_ref(y1, m_indptr, bias1, alpha, beta, limit)
    q, sf = quantize_act_ref(act)
    y2 = R.group_gemm_ref(R.fp8_to_f64(q), sf, w2, w2_sf, ms)
    return finalize_ref(y2, w, emap, top_k, bias2, m_indptr)[0]
