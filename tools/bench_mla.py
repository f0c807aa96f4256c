"""MLA paged decode benchmark: BatchMLAPagedAttentionWrapper over the grid of the reference's
benchmarks/bench_deepseek_mla.py (seq 1024 / 2048 / 8192 x batch 64 / 128 / 768 x heads 64 / 128, page size 1),
plus the TP8 shape (16 heads) and page size 64.

Per point: run() time from device events (median of --iters timed calls after warm-up), TB/s of KV read
(batch x seq x 576 x the cache's element size), TFLOP/s (2 x heads x batch x seq x (576 + 512)), the run() time of a graph plan
(fixed grid, merge always launched), and a naive torch gather + matmul baseline on the same GPU.  Prints one JSON
line per point; --out writes them all to a file.  --kv-dtype fp8 runs the float8_e4m3fn cache (q stays bfloat16);
--kv-dtype both runs the two caches of every point one after the other, so that they share the session and its clocks.
--rope-quantize adds one line per nnz for flashinfer.rope.mla_rope_quantize_fp8 at 128 heads (time, GB/s read + written).

    python tools/bench_mla.py [--quick] [--kv-dtype bf16|fp8|both] [--rope-quantize] [--no-naive] [--out profiles/mla_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import flashinfer  # noqa: E402

CKV, KPE = 512, 64


def event_time_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def naive(q_nope, q_pe, ckv, kpe, kv_indices, batch, seq, sm_scale):
    """torch baseline: gather every request's pages, then two batched matmuls and a softmax."""
    k_ckv = ckv[kv_indices.long()].view(batch, seq, CKV)
    k_pe = kpe[kv_indices.long()].view(batch, seq, KPE)
    s = (torch.bmm(q_nope, k_ckv.transpose(1, 2)) + torch.bmm(q_pe, k_pe.transpose(1, 2))).float() * sm_scale
    p = torch.softmax(s, -1).to(q_nope.dtype)
    return torch.bmm(p, k_ckv)


def bench_point(batch, seq, heads, page_size, iters, warmup, dtype=torch.bfloat16, with_naive=True, kv_dtype=None):
    dev = "cuda:0"
    torch.manual_seed(0)
    kv_dtype = kv_dtype or dtype
    pages_per = seq // page_size
    total_pages = batch * pages_per
    ckv = torch.randn(total_pages, page_size, CKV, dtype=dtype, device=dev).to(kv_dtype)
    kpe = torch.randn(total_pages, page_size, KPE, dtype=dtype, device=dev).to(kv_dtype)
    q_nope = torch.randn(batch, heads, CKV, dtype=dtype, device=dev)
    q_pe = torch.randn(batch, heads, KPE, dtype=dtype, device=dev)
    qo_indptr = torch.arange(batch + 1, dtype=torch.int32, device=dev)
    kv_indptr = torch.arange(batch + 1, dtype=torch.int32, device=dev) * pages_per
    kv_indices = torch.randperm(total_pages, device=dev).to(torch.int32)
    kv_lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
    sm_scale = 1.0 / ((128 + 64) ** 0.5)
    ws = torch.empty(128 << 20, dtype=torch.uint8, device=dev)
    w = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, backend="fa2")
    w.plan(qo_indptr, kv_indptr, kv_indices, kv_lens, heads, CKV, KPE, page_size, False, sm_scale, dtype, kv_dtype)
    out = torch.empty(batch, heads, CKV, dtype=dtype, device=dev)
    ms = event_time_ms(lambda: w.run(q_nope, q_pe, ckv, kpe, out=out), iters, warmup)
    kv_bytes = batch * seq * (CKV + KPE) * ckv.element_size()
    flops = 2 * heads * batch * seq * (CKV + KPE + CKV)
    rec = dict(batch=batch, seq=seq, heads=heads, page_size=page_size, dtype=str(dtype).split(".")[-1],
               kv_dtype=str(kv_dtype).split(".")[-1],
               us=round(ms * 1e3, 2), kv_tb_s=round(kv_bytes / ms / 1e9, 3), tflop_s=round(flops / ms / 1e9, 1),
               kv_chunk=int(w._plan_info[flashinfer._lib.FI_MLA_KV_CHUNK_SIZE]),
               split=int(w._plan_info[flashinfer._lib.FI_MLA_SPLIT_KV]))
    # a graph plan (use_cuda_graph=True) launches a fixed grid and always the merge, one workgroup per packed row
    # (rows of unsplit requests exit at once); run eagerly it launches what a replay launches
    bufs = [qo_indptr.clone(), kv_indptr.clone(), kv_indices.clone(), kv_lens.clone()]
    wg = flashinfer.mla.BatchMLAPagedAttentionWrapper(ws, True, *bufs, backend="fa2")
    wg.plan(qo_indptr, kv_indptr, kv_indices, kv_lens, heads, CKV, KPE, page_size, False, sm_scale, dtype, kv_dtype)
    gout = torch.empty_like(out)
    rec["graph_plan_us"] = round(event_time_ms(lambda: wg.run(q_nope, q_pe, ckv, kpe, out=gout), iters, warmup) * 1e3, 2)
    rec["graph_plan_split"] = int(wg._plan_info[flashinfer._lib.FI_MLA_SPLIT_KV])
    if with_naive and kv_dtype == dtype:
        try:
            nms = event_time_ms(lambda: naive(q_nope, q_pe, ckv, kpe, kv_indices, batch, seq, sm_scale), max(iters // 4, 3), 2)
            rec["naive_us"] = round(nms * 1e3, 2)
            rec["speedup_vs_naive"] = round(nms / ms, 2)
            ref = naive(q_nope, q_pe, ckv, kpe, kv_indices, batch, seq, sm_scale)
            rec["max_abs_diff_vs_naive"] = float((ref.float() - out.float()).abs().max())
        except torch.OutOfMemoryError:
            rec["naive_us"] = None
        torch.cuda.empty_cache()
    return rec


def bench_rope_quantize(nnz, heads, iters, warmup, dtype=torch.bfloat16):
    """mla_rope_quantize_fp8 on slices of 576-wide tensors, into 576-wide e4m3 tensors."""
    from flashinfer.rope import mla_rope_quantize_fp8

    dev = "cuda:0"
    torch.manual_seed(0)
    q = torch.randn(nnz, heads, CKV + KPE, dtype=dtype, device=dev)
    k = torch.randn(nnz, CKV + KPE, dtype=dtype, device=dev)
    q8 = torch.empty(nnz, heads, CKV + KPE, dtype=torch.float8_e4m3fn, device=dev)
    k8 = torch.empty(nnz, CKV + KPE, dtype=torch.float8_e4m3fn, device=dev)
    cache = torch.randn(8192, KPE, dtype=torch.float32, device=dev)
    pos = torch.randint(0, 8192, (nnz,), dtype=torch.int32, device=dev)
    ms = event_time_ms(lambda: mla_rope_quantize_fp8(
        q[..., CKV:], k[..., CKV:], q[..., :CKV], k[..., :CKV], cache, pos, q_rope_out=q8[..., CKV:],
        k_rope_out=k8[..., CKV:], q_nope_out=q8[..., :CKV], k_nope_out=k8[..., :CKV]), iters, warmup)
    moved = nnz * (heads + 1) * (CKV + KPE) * (q.element_size() + 1)
    return dict(op="mla_rope_quantize_fp8", nnz=nnz, heads=heads, dtype=str(dtype).split(".")[-1],
                us=round(ms * 1e3, 2), gb_s=round(moved / ms / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a few points only")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8", "both"), default="bf16",
                    help="the cache's dtype: bfloat16, float8_e4m3fn, or both in turn at every point")
    ap.add_argument("--no-naive", action="store_true", help="skip the torch baseline")
    ap.add_argument("--rope-quantize", action="store_true", help="add mla_rope_quantize_fp8 at nnz 1 / 256 / 8192")
    a = ap.parse_args()
    kv_dtypes = {"bf16": [torch.bfloat16], "fp8": [torch.float8_e4m3fn],
                 "both": [torch.bfloat16, torch.float8_e4m3fn]}[a.kv_dtype]
    if a.quick:
        points = [(64, 8192, 16, 64), (128, 8192, 128, 1), (768, 1024, 128, 1)]
    else:
        points = [(b, s, h, 1) for s in (1024, 2048, 8192) for b in (64, 128, 768) for h in (64, 128)]
        points += [(b, s, 16, ps) for s in (1024, 8192) for b in (64, 128, 768) for ps in (1, 64)]
        points += [(b, s, 128, 64) for s in (8192,) for b in (64, 128)]
    recs = []
    for b, s, h, ps in points:
        for kv_dtype in kv_dtypes:
            rec = bench_point(b, s, h, ps, a.iters, a.warmup, with_naive=not a.no_naive and b * s <= 128 * 8192,
                              kv_dtype=kv_dtype)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    if a.rope_quantize:
        for nnz in (1, 256, 8192):
            rec = bench_rope_quantize(nnz, 128, a.iters, a.warmup)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
