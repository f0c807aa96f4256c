#!/usr/bin/env python
"""cutlass_fused_moe (bf16) through flashinfer.fused_moe_16bit, timed with device events in one process: the layer, its two
grouped GEMMs on their own, and as comparator the same layer written as a per-expert loop of torch.matmul and torch
elementwise ops (its per-expert row lists are made outside the timed region, which favours it).  The variants of a shape
alternate round by round; every figure is a median over the rounds with its spread, (max - min) / median.  One JSON line
per shape.

Shapes: Mixtral (E = 8, top_k = 2, H = 4096, I = 14336) and a many-expert shape (E = 128, top_k = 8, H = 2048, I = 768),
each at T = 64 and T = 4096.

    python tools/bench_cutlass_moe.py [--rounds 7] [--shapes mixtral,many] [--tokens 64,4096]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flashinfer-ai_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from flashinfer import fused_moe as F  # noqa: E402
from flashinfer.fused_moe_16bit import cutlass_fused_moe  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
WINDOW_MS = 40.0  # device time one timed window should hold
SHAPES = {"mixtral": (8, 2, 4096, 14336), "many": (128, 8, 2048, 768)}


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(variants, rounds):
    """{name: (median ms, spread)} of the callables in ``variants``, timed in turn round after round."""
    inner = {}
    for name, fn in variants.items():
        fn(), fn()
        inner[name] = max(1, min(200, math.ceil(WINDOW_MS / max(event_ms(fn, 1), 1e-3))))
    series = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            series[name].append(event_ms(fn, inner[name]))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in series.items()}


def torch_loop(x, w31, w2, rows_of, scales_of):
    """compute_with_experts of the reference's test (tests/moe/test_trtllm_cutlass_fused_moe.py:171-210) in bf16."""
    out = torch.zeros_like(x)
    for e, rows in enumerate(rows_of):
        if rows.numel() == 0:
            continue
        xe = x[rows]
        w3, w1 = w31[e].chunk(2, dim=0)
        inter = torch.nn.functional.silu(xe @ w1.t()) * (xe @ w3.t())
        out.index_add_(0, rows, scales_of[e] * (inter @ w2[e].t()))
    return out


def bench(name, T, rounds):
    E, top_k, H, I = SHAPES[name]
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(T, H, device=DEV, dtype=BF16, generator=g) / 5
    w31 = torch.randn(E, 2 * I, H, device=DEV, dtype=BF16, generator=g) / 5
    w2 = torch.randn(E, H, I, device=DEV, dtype=BF16, generator=g) / 5
    scales, ids = torch.topk(torch.softmax(torch.randn(T, E, device=DEV, generator=g), dim=-1), top_k, dim=-1)
    ids, scales = ids.int(), scales.float().contiguous()
    where = [torch.where(ids == e) for e in range(E)]
    rows_of = [w[0] for w in where]
    scales_of = [scales[w[0], w[1], None].to(BF16) for w in where]
    out = torch.empty_like(x)
    m_indptr, emap, p2e = F.moe_sort(ids, 0, E)
    act = torch.empty(T * top_k, I, device=DEV, dtype=BF16)
    y = torch.empty(T * top_k, H, device=DEV, dtype=BF16)
    variants = {
        "layer": lambda: cutlass_fused_moe(x, ids, scales, w31, w2, BF16, None, output=out),
        "gemm1": lambda: F.moe_group_gemm_16bit(x, w31, m_indptr, a_row_ids=p2e, swiglu=True, out=act, a_row_ids_div=top_k),
        "gemm2": lambda: F.moe_group_gemm_16bit(act, w2, m_indptr, out=y),
        "torch_loop": lambda: torch_loop(x, w31, w2, rows_of, scales_of),
    }
    res = alternate(variants, rounds)
    diff = (variants["layer"]()[0].float() - variants["torch_loop"]().float()).abs().max().item()
    flops1, flops2 = 2.0 * T * top_k * 2 * I * H, 2.0 * T * top_k * H * I
    row = dict(shape=name, E=E, top_k=top_k, H=H, I=I, T=T, dtype="bf16", max_abs_diff_to_torch_loop=diff,
               layer_over_torch_loop=res["layer"][0] / res["torch_loop"][0],
               gemm1_tflops=flops1 / res["gemm1"][0] / 1e9, gemm2_tflops=flops2 / res["gemm2"][0] / 1e9)
    for v, (ms, spread) in res.items():
        row[v + "_ms"], row[v + "_spread"] = ms, spread
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="mixtral,many")
    ap.add_argument("--tokens", default="64,4096")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cutlass_moe.py needs the GPU: there is nothing to time without it")
    for name in a.shapes.split(","):
        for T in (int(t) for t in a.tokens.split(",")):
            bench(name, T, a.rounds)


if __name__ == "__main__":
    main()
