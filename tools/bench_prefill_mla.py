"""Prefill at head_dim_qk 192 / head_dim_vo 128 (DeepSeek-style MLA prefill, non-absorbed form) against two yardsticks,
timed alternately in one process with device events (warm-up, then the median of the repeats):
  new   BatchPrefillWithRaggedKVCacheWrapper planned with head_dim_qk=192, head_dim_vo=128
  pad   the workaround without it: zero-pad q / k / v to 256, run the head_dim 256 kernel with sm_scale = 1 / sqrt(192),
        slice the output (pad copies and slice included)
  d128  the head_dim 128 ragged kernel on the same (batch, seq, heads): a rate yardstick
Grid: the reference's routine (benchmarks/test_flashinfer_benchmark.py:31-40: ragged, 128 / 128 heads, causal, batch
{16, 32} x seq {1024, 2048}), one long request at 16 / 16 heads (seq 8192 / 16384), and the reference's single-prefill
point (tests/attention/test_deepseek_mla.py: qo 3928, kv 7563, 128 heads); bf16, plus one f16 row.
TFLOP/s = 2 x visible (q, k) pairs x heads x (head_dim_qk + head_dim_vo) / time: batch x s^2 x H x (192 + 128) for a
causal s x s request (causal counted as half, as tools/bench_ref_grids.py); the d128 row uses 128 + 128.
Usage: python tools/bench_prefill_mla.py [--out profiles/prefill_mla_bench.jsonl] [--iters 20]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import flashinfer  # noqa: E402

DEV = torch.device("cuda:0")

# (name, batch, qo_len, kv_len, heads, causal, dtype)
GRID = [
    ("ref_routine", 16, 1024, 1024, 128, True, torch.bfloat16),
    ("ref_routine", 16, 2048, 2048, 128, True, torch.bfloat16),
    ("ref_routine", 32, 1024, 1024, 128, True, torch.bfloat16),
    ("ref_routine", 32, 2048, 2048, 128, True, torch.bfloat16),
    ("long_tp8", 1, 8192, 8192, 16, True, torch.bfloat16),
    ("long_tp8", 1, 16384, 16384, 16, True, torch.bfloat16),
    ("ref_single", 1, 3928, 7563, 128, True, torch.bfloat16),
    ("ref_routine_f16", 16, 2048, 2048, 128, True, torch.float16),
]


def visible_pairs(qo, kv, causal):
    if not causal:
        return qo * kv
    return qo * (kv - qo) + qo * (qo + 1) // 2


def ragged(ws, batch, qo, kv, heads, causal, dtype, dqk, dvo, sm_scale=None):
    qi = (torch.arange(batch + 1, dtype=torch.int32) * qo).to(DEV)
    ki = (torch.arange(batch + 1, dtype=torch.int32) * kv).to(DEV)
    w = flashinfer.BatchPrefillWithRaggedKVCacheWrapper(ws, "NHD")
    w.plan(qi, ki, heads, heads, dqk, head_dim_vo=dvo, causal=causal, q_data_type=dtype, sm_scale=sm_scale)
    return w


def time_alternating(fns, iters, warm):
    """median ms of each fn, the fns run in turn every iteration"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
    for _ in range(iters):
        for i, f in enumerate(fns):
            ev[i][0].record()
            f()
            ev[i][1].record()
        torch.cuda.synchronize()
        for i in range(len(fns)):
            times[i].append(ev[i][0].elapsed_time(ev[i][1]))
    return [sorted(t)[len(t) // 2] for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_mla_bench.jsonl"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    ws = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    ws2 = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    ws3 = torch.empty(512 << 20, dtype=torch.uint8, device=DEV)
    print(f"{'point':16s} {'dtype':8s} {'b':>3s} {'qo':>6s} {'kv':>6s} {'H':>4s}   new ms  pad ms  d128 ms   "
          f"new TF/s  d128 TF/s  pad/new", flush=True)
    with open(args.out, "a") as fo:
        for name, b, qo, kv, h, causal, dtype in GRID:
            torch.manual_seed(0)
            q = torch.randn(b * qo, h, 192, dtype=dtype, device=DEV)
            k = torch.randn(b * kv, h, 192, dtype=dtype, device=DEV)
            v = torch.randn(b * kv, h, 128, dtype=dtype, device=DEV)
            w_new = ragged(ws, b, qo, kv, h, causal, dtype, 192, 128)
            w_pad = ragged(ws2, b, qo, kv, h, causal, dtype, 256, 256, sm_scale=1.0 / math.sqrt(192))
            w_128 = ragged(ws3, b, qo, kv, h, causal, dtype, 128, 128)
            q128, k128, v128 = q[..., :128].contiguous(), k[..., :128].contiguous(), v.clone()

            def run_pad():
                o = w_pad.run(F.pad(q, (0, 64)), F.pad(k, (0, 64)), F.pad(v, (0, 128)))
                return o[..., :128]

            fns = [lambda: w_new.run(q, k, v), run_pad, lambda: w_128.run(q128, k128, v128)]
            t_new, t_pad, t_128 = time_alternating(fns, args.iters, args.warm)
            pairs = b * visible_pairs(qo, kv, causal)
            tf_new = 2 * pairs * h * (192 + 128) / t_new / 1e9
            tf_128 = 2 * pairs * h * (128 + 128) / t_128 / 1e9
            rec = dict(point=name, dtype=str(dtype).replace("torch.", ""), batch=b, qo_len=qo, kv_len=kv, heads=h,
                       causal=causal, new_ms=t_new, pad256_ms=t_pad, d128_ms=t_128, new_tflops=tf_new,
                       d128_tflops=tf_128, pad_over_new=t_pad / t_new, split_kv=bool(w_new._plan_info[14]),
                       iters=args.iters)
            fo.write(json.dumps(rec) + "\n")
            print(f"{name:16s} {rec['dtype']:8s} {b:3d} {qo:6d} {kv:6d} {h:4d} {t_new:8.3f} {t_pad:7.3f} {t_128:8.3f} "
                  f"{tf_new:10.1f} {tf_128:10.1f} {t_pad / t_new:8.2f}", flush=True)
            del q, k, v, q128, k128, v128, w_new, w_pad, w_128
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
