#!/usr/bin/env python
"""Block-sparse attention through flashinfer.sparse, timed with device events (run()) or a host clock around a
synchronised call (plan()).  Within a group the variants alternate round by round, so they see the same clocks and the
same neighbours; every figure is a median over the rounds with its spread, (max - min) / median.  One JSON line each.

(a) BlockSparseAttentionWrapper.run() at R = C in {64, 128}, M = N in {16384, 32768}, 8/8 and 32/8 heads, head_dim
    128, bf16, block density 1.0 / 0.5 / 0.25 / 0.1, against single_prefill_with_kv_cache on the same dense shape.
(b) R = 1, C = 16: 64 block rows, each selecting a quarter of the pages of its own 8192-token history, against
    BatchDecodeWithPagedKVCacheWrapper on the same page table.
(c) VariableBlockSparseAttentionWrapper, 8 kv heads, 16384 tokens, 128 x 128 blocks, density 0.3: plan() against a
    torch statement of the reference's expansion (index arithmetic on the device, then every index to the host),
    and run() with column sizes that are multiples of 16 (pages of 16 tokens) and with arbitrary sizes (pages of 1).

    python tools/bench_block_sparse.py [--parts abc] [--rounds 7] [--quick]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flashinfer-ai_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import flashinfer  # noqa: E402

DEV = "cuda:0"
BF16 = torch.bfloat16
WINDOW_MS = 40.0  # device time one timed window should hold


def workspace():
    return torch.zeros(256 << 20, dtype=torch.uint8, device=DEV)


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def host_ms(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / inner


def alternate(variants, rounds, timer=event_ms):
    """{name: (median ms, spread)} of the callables in ``variants``, timed in turn round after round."""
    inner = {}
    for name, fn in variants.items():
        fn(), fn()
        once = timer(fn, 1)
        inner[name] = max(1, min(50, math.ceil(WINDOW_MS / max(once, 1e-3))))
    series = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            series[name].append(timer(fn, inner[name]))
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in series.items()}


def emit(**row):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


def bsr_pattern(MB, NB, density, g):
    """(indptr, indices) on the device: rand < density, the diagonal kept so that no block row is empty."""
    keep = torch.rand(MB, NB, generator=g, device=DEV) < density
    keep |= torch.eye(MB, NB, dtype=torch.bool, device=DEV)
    indptr = torch.zeros(MB + 1, dtype=torch.int32, device=DEV)
    indptr[1:] = keep.sum(1).cumsum(0)
    return indptr, keep.nonzero()[:, 1].to(torch.int32), float(keep.float().mean())


def part_a(rounds, quick):
    g = torch.Generator(device=DEV).manual_seed(0)
    d = 128
    sizes = (16384,) if quick else (16384, 32768)
    for n in sizes:
        for hq, hkv in ((8, 8), (32, 8)):
            q = torch.randn(n, hq, d, device=DEV, dtype=BF16, generator=g)
            k = torch.randn(n, hkv, d, device=DEV, dtype=BF16, generator=g)
            v = torch.randn(n, hkv, d, device=DEV, dtype=BF16, generator=g)
            out = torch.empty_like(q)
            for blk in (64, 128):
                variants = {"dense": lambda: flashinfer.single_prefill_with_kv_cache(q, k, v)}
                kept = {}
                for density in (1.0, 0.5, 0.25, 0.1):
                    indptr, indices, kept[density] = bsr_pattern(n // blk, n // blk, density, g)
                    w = flashinfer.BlockSparseAttentionWrapper(workspace())
                    try:
                        w.plan(indptr, indices, n, n, blk, blk, hq, hkv, d, q_data_type=BF16, o_data_type=BF16)
                    except RuntimeError as e:  # the planner's refusal is the result for this shape
                        emit(part="a", R=blk, C=blk, M=n, N=n, heads=f"{hq}/{hkv}", density=density,
                             plan_refused=str(e))
                        continue
                    variants[density] = lambda w=w: w.run(q, k, v, out=out)
                res = alternate(variants, rounds)
                dense_ms = res["dense"][0]
                flops = 4.0 * n * n * d * hq
                emit(part="a", R=blk, C=blk, M=n, N=n, heads=f"{hq}/{hkv}", variant="single_prefill dense",
                     ms=dense_ms, spread=res["dense"][1], tflops=flops / dense_ms / 1e9)
                for density in (x for x in kept if x in res):
                    ms, spread = res[density]
                    emit(part="a", R=blk, C=blk, M=n, N=n, heads=f"{hq}/{hkv}", variant="block sparse run()",
                         density=density, blocks_kept=kept[density], ms=ms, spread=spread,
                         over_dense=ms / dense_ms, tflops_of_kept_blocks=flops * kept[density] / ms / 1e9)
            del q, k, v, out


def part_b(rounds):
    g = torch.Generator(device=DEV).manual_seed(1)
    rows, hist, page, hq, hkv, d = 64, 8192, 16, 32, 8, 128
    pages_per_row, n = hist // page, rows * hist
    k = torch.randn(n, hkv, d, device=DEV, dtype=BF16, generator=g)
    v = torch.randn(n, hkv, d, device=DEV, dtype=BF16, generator=g)
    q = torch.randn(rows, hq, d, device=DEV, dtype=BF16, generator=g)
    picked = torch.stack([torch.randperm(pages_per_row, device=DEV, generator=g)[: pages_per_row // 4].sort().values
                          + r * pages_per_row for r in range(rows)])
    indptr = (torch.arange(rows + 1, dtype=torch.int32) * (pages_per_row // 4)).to(DEV)
    indices = picked.flatten().to(torch.int32)
    w = flashinfer.BlockSparseAttentionWrapper(workspace())
    w.plan(indptr, indices, rows, n, 1, page, hq, hkv, d, q_data_type=BF16, o_data_type=BF16)
    plain = flashinfer.BatchDecodeWithPagedKVCacheWrapper(workspace(), "NHD")
    plain.plan(indptr, indices, torch.full((rows,), page, dtype=torch.int32, device=DEV), hq, hkv, d, page,
               q_data_type=BF16, kv_data_type=BF16)
    cache = (k.view(-1, page, hkv, d), v.view(-1, page, hkv, d))
    out = torch.empty_like(q)
    res = alternate({"sparse": lambda: w.run(q, k, v, out=out), "decode": lambda: plain.run(q, cache, out=out)},
                    rounds)
    kv_bytes = 2.0 * indices.numel() * page * hkv * d * 2
    for name, label in (("decode", "BatchDecodeWithPagedKVCacheWrapper.run()"), ("sparse", "block sparse run()")):
        emit(part="b", rows=rows, history=hist, C=page, selected_pages_per_row=pages_per_row // 4, heads=f"{hq}/{hkv}",
             variant=label, us=res[name][0] * 1e3, spread=res[name][1], kv_gb_per_s=kv_bytes / res[name][0] / 1e6)
    emit(part="b", sparse_over_decode=res["sparse"][0] / res["decode"][0], took_decode_path=not w._use_tensor_cores)


def reference_expansion(block_mask_map, block_col_sz):
    """The expansion the reference's plan() performs (flashinfer/sparse.py:929-980), stated in torch: one-token
    pages, index arithmetic on the device, then the prefix sums and every index copied to the host."""
    sizes = block_col_sz.long()
    heads, kv_len = sizes.shape[0], int(sizes[0].sum())
    first = sizes.cumsum(1) - sizes + torch.arange(heads, device=sizes.device)[:, None] * kv_len
    h, _, c = block_mask_map.nonzero(as_tuple=True)
    lens, base = sizes[h, c], first[h, c]
    ends = lens.cumsum(0)
    token = torch.arange(int(ends[-1]), device=sizes.device)
    indices = torch.repeat_interleave(base - (ends - lens), lens) + token
    indptr = torch.zeros(block_mask_map.shape[0] * block_mask_map.shape[1] + 1, dtype=torch.long, device=sizes.device)
    indptr[1:] = (block_mask_map * sizes[:, None, :]).sum(-1).flatten().cumsum(0)
    return indptr.to(torch.int32).cpu(), indices.to(torch.int32).cpu()


def partition(total, parts, step, g):
    """`parts` positive multiples of `step` summing to `total`, drawn at random."""
    cuts = (torch.randperm(total // step - 1, generator=g)[: parts - 1] + 1).sort().values
    edges = torch.cat([torch.zeros(1, dtype=torch.long), cuts, torch.tensor([total // step])])
    return ((edges[1:] - edges[:-1]) * step).to(torch.int32)


def part_c(rounds):
    g = torch.Generator().manual_seed(2)
    heads, n, blocks, d, density = 8, 16384, 128, 128, 0.3
    block_map = (torch.rand(heads, blocks, blocks, generator=g) < density).to(DEV)
    block_map |= torch.eye(blocks, dtype=torch.bool, device=DEV)[None]
    q = torch.randn(heads, n, d, dtype=BF16, generator=g).to(DEV)
    k, v = torch.randn(heads, n, d, dtype=BF16, generator=g).to(DEV), torch.randn(heads, n, d, dtype=BF16,
                                                                                generator=g).to(DEV)
    out = torch.empty_like(q)
    for step, label in ((16, "column sizes multiples of 16"), (1, "arbitrary column sizes")):
        row_sz = torch.stack([partition(n, blocks, step, g) for _ in range(heads)]).to(DEV)
        col_sz = torch.stack([partition(n, blocks, step, g) for _ in range(heads)]).to(DEV)
        w = flashinfer.VariableBlockSparseAttentionWrapper(workspace())
        plan = lambda: w.plan(block_map, row_sz, col_sz, heads, heads, d, q_data_type=BF16)
        res = alternate({"plan": plan, "reference": lambda: reference_expansion(block_map, col_sz)}, rounds, host_ms)
        plan()
        run_ms, run_spread = alternate({"run": lambda: w.run(q, k, v, out=out)}, rounds)["run"]
        selected = float((block_map * col_sz[:, None, :].float() * row_sz[:, :, None].float()).sum())
        emit(part="c", kv_heads=heads, tokens=n, blocks=f"{blocks}x{blocks}", density=density, sizes=label,
             page_size=w._page_size, page_indices=int(w._prefill._paged_kv_indices_buf.numel()),
             plan_ms=res["plan"][0], plan_spread=res["plan"][1], reference_expansion_ms=res["reference"][0],
             reference_expansion_spread=res["reference"][1], run_ms=run_ms, run_spread=run_spread,
             tflops_of_selected=4.0 * selected * d / run_ms / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="part (a) at 16384 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_block_sparse.py needs the GPU: there is nothing to time without it")
    if "a" in a.parts:
        part_a(a.rounds, a.quick)
    if "b" in a.parts:
        part_b(a.rounds)
    if "c" in a.parts:
        part_c(a.rounds)


if __name__ == "__main__":
    main()
