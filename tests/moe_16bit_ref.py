"""CPU oracle of the unquantised MoE layer (tests/test_cutlass_moe_gpu.py): plain torch, fp64, no kernel.  The per-expert
loop is compute_with_experts of the reference's tests/moe/test_trtllm_cutlass_fused_moe.py:171-210 restricted to a window of
local experts; group_gemm_ref restates one GEMM of it on sorted rows."""
import torch

import moe_ref as M

MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of `dtype` at |x| (fp64 in, fp64 out), the subnormal spacing below the smallest normal."""
    e = torch.frexp(x.abs().clamp(min=2.0 ** EMIN[dtype]))[1] - 1
    return torch.exp2(e.double() - MANT[dtype])


def swiglu_ref(x1, x2, alpha=None, beta=None, limit=None):
    """x1 the gate, x2 the linear half (fp64); the three scalars all given or all None (lines 195-207)."""
    if alpha is None:
        return x1 * torch.sigmoid(x1) * x2
    x1 = x1.clamp(max=limit)
    return x1 * torch.sigmoid(alpha * x1) * (x2.clamp(min=-limit, max=limit) + beta)


def group_gemm_ref(a, b, m_indptr, row_ids=None, swiglu=False, alpha=None, beta=None, limit=None) -> torch.Tensor:
    """a [*, k], b [G, n, k] -> fp64 [m_indptr[-1], n] (or [.., n / 2] with swiglu: rows [0, I) of b[g] are the linear half,
    [I, 2 I) the gate).  Row r of group g reads a[row_ids[r]] (a[r] without row_ids)."""
    a, b = a.double(), b.double()
    rows = []
    begin = 0
    for g, m in enumerate(M.segments(m_indptr)):
        src = torch.arange(begin, begin + m) if row_ids is None else row_ids[begin:begin + m].long()
        x = a[src] @ b[g].T
        if swiglu:
            x2, x1 = x.chunk(2, dim=1)
            x = swiglu_ref(x1, x2, *(None if t is None else float(t[g]) for t in (alpha, beta, limit)))
        rows.append(x)
        begin += m
    return torch.cat(rows)


def moe_16bit_ref(x, ids, scales, w31, w2, offset=0, alpha=None, beta=None, limit=None) -> torch.Tensor:
    """x [T, H], ids / scales [T, top_k] (global expert ids), w31 [G, 2 I, H] and w2 [G, H, I] of the experts [offset,
    offset + G) -> fp64 [T, H]; nothing is rounded on the way."""
    x = x.double()
    out = torch.zeros_like(x)
    for g in range(w31.shape[0]):
        batch_idx, nth = torch.where(ids == offset + g)
        if not len(batch_idx):
            continue
        w3, w1 = w31[g].double().chunk(2, dim=0)
        xe = x[batch_idx]
        inter = swiglu_ref(xe @ w1.T, xe @ w3.T, *(None if t is None else float(t[g]) for t in (alpha, beta, limit)))
        out.index_add_(0, batch_idx, scales[batch_idx, nth, None].double() * (inter @ w2[g].double().T))
    return out
