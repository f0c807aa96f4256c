"""group_gemm_mxfp8_mxfp4_nt_groupwise at GPT-OSS-like MoE shapes against what a user has without it.

    python tools/bench_mxfp4_gemm.py [--out profiles/mxfp4_gemm_bench.jsonl] [--groups 32] [--k 2944] [--ns 5760,2880]
                                     [--rows 4,16,64,256,1024] [--warmup 10] [--runs 30]

Per (n, rows per expert) one JSON line with the device-event median and the run-to-run spread (quartiles, min, max) of
three candidates, timed alternately in one loop after --warmup rounds of all three:

  mxfp4   the new kernel on MXFP8 activations (quantised once, untimed) and MXFP4 weights;
  bf16    what users have today: the weights dequantised once to bf16 (untimed), then torch.matmul per group in a Python
          loop over the groups (the row ranges are known on the host);
  fp8     group_gemm_fp8_nt_groupwise, this project's tuned fp8 kernel, on the same weights re-quantised to e4m3 with
          128 x 128 block scales: twice the weight bytes of mxfp4.

and from them: the algorithmic bytes of each candidate (weights + activations + output), the new kernel's rate in
bytes/s and FLOP/s, its share of the 5 PFLOP/s fp8 figure, and the speed-ups.  A sample is the time between two events
around the Python call on an idle stream.  Weight sets rotate so that at least 512 MB pass between two uses of the
same bytes (the Infinity Cache holds 256 MB).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch

import flashinfer
from flashinfer import _mx, fp8_quantization

DEV = torch.device("cuda", 0)
FP8_PEAK = 5.0e15
ROTATE_BYTES = 512 << 20
E2M1 = [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]


def ceil_to(x, m):
    return (x + m - 1) // m * m


def swizzle_b_scale(sf):
    """[G, n, nkb] -> (G, ceil(n / 128) * 128, nkb) in the swizzled layout, on the device"""
    G, n, nkb = sf.shape
    n_pad = ceil_to(n, 128)
    r = torch.arange(n, device=sf.device).view(-1, 1).expand(n, nkb)
    kb = torch.arange(nkb, device=sf.device).view(1, -1).expand(n, nkb)
    off = _mx.sf_offset(r, kb, nkb).reshape(-1)
    out = torch.zeros(G, n_pad * nkb, dtype=torch.uint8, device=sf.device)
    out[:, off] = sf.reshape(G, -1)
    return out.view(G, n_pad, nkb)


def make_weights(G, n, k, seed):
    """one weight set in the three formats"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    packed = torch.randint(0, 256, (G, n, k // 2), dtype=torch.uint8, device=DEV, generator=g)
    sf = torch.randint(118, 124, (G, n, k // 32), dtype=torch.uint8, device=DEV, generator=g)
    table = torch.tensor(E2M1, dtype=torch.float32, device=DEV)
    w_bf16 = torch.empty(G, n, k, dtype=torch.bfloat16, device=DEV)
    n_pad, kb128 = ceil_to(n, 128), k // 128
    w_fp8 = torch.empty(G, n, k, dtype=torch.float8_e4m3fn, device=DEV)
    s_fp8 = torch.empty(G, kb128, n_pad // 128, dtype=torch.float32, device=DEV)  # "MN" major: (G, k / 128, n / 128)
    for i in range(G):
        codes = torch.stack([packed[i] & 15, packed[i] >> 4], dim=-1).flatten(-2).long()
        w = table[codes] * torch.exp2(sf[i].float() - 127).repeat_interleave(32, dim=1)
        w_bf16[i] = w.to(torch.bfloat16)  # exact: 2 mantissa bits times a power of two
        wp = torch.zeros(n_pad, k, device=DEV)
        wp[:n] = w
        blocks = wp.view(n_pad // 128, 128, kb128, 128)
        scale = (blocks.abs().amax(dim=(1, 3)) / 448.0).clamp(min=1e-30)
        w_fp8[i] = (blocks / scale[:, None, :, None]).view(n_pad, k)[:n].to(torch.float8_e4m3fn)
        s_fp8[i] = scale.T
    return {"packed": packed, "b_scale": swizzle_b_scale(sf), "bf16": w_bf16, "fp8": w_fp8, "fp8_scale": s_fp8}


def time_alternating(fns, warmup, runs):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            samples[name].append(start.elapsed_time(stop) * 1e-3)
    return samples


def summary(xs):
    t = torch.tensor(sorted(xs), dtype=torch.float64)
    q = torch.quantile(t, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)).tolist()
    return {"median_us": q[1] * 1e6, "q25_us": q[0] * 1e6, "q75_us": q[2] * 1e6, "min_us": t[0].item() * 1e6,
            "max_us": t[-1].item() * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--k", type=int, default=2944)
    ap.add_argument("--ns", default="5760,2880")
    ap.add_argument("--rows", default="4,16,64,256,1024")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    assert args.warmup >= 10 and args.runs >= 30, "at least 10 warm-ups and 30 timed runs"
    G, k = args.groups, args.k
    out_f = open(args.out, "w") if args.out else None
    for n in (int(x) for x in args.ns.split(",")):
        fp4_bytes = G * n * (k // 2 + k // 32)
        sets = [make_weights(G, n, k, 100 + i) for i in range(max(1, -(-ROTATE_BYTES // fp4_bytes)))]
        for rows in (int(x) for x in args.rows.split(",")):
            cum_m = G * rows
            bounds = [g * rows for g in range(G + 1)]
            indptr = torch.tensor(bounds, dtype=torch.int32, device=DEV)
            x = torch.randn(cum_m, k, device=DEV, dtype=torch.bfloat16)
            x_q, a_scale = fp8_quantization.mxfp8_quantize_grouped(x, indptr)
            ones = torch.ones(k // 128, cum_m, dtype=torch.float32, device=DEV)
            out = torch.empty(cum_m, n, dtype=torch.bfloat16, device=DEV)
            turn = {"mxfp4": 0, "bf16": 0, "fp8": 0}

            def pick(name):
                turn[name] += 1
                return sets[turn[name] % len(sets)]

            def run_mxfp4():
                w = pick("mxfp4")
                flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise(x_q, w["packed"], a_scale, w["b_scale"], indptr, out=out)

            def run_bf16():
                w = pick("bf16")["bf16"]
                for g in range(G):
                    torch.matmul(x[bounds[g]:bounds[g + 1]], w[g].T, out=out[bounds[g]:bounds[g + 1]])

            def run_fp8():
                w = pick("fp8")
                flashinfer.group_gemm_fp8_nt_groupwise(x_q, w["fp8"], ones, w["fp8_scale"], indptr, out=out)

            samples = time_alternating({"mxfp4": run_mxfp4, "bf16": run_bf16, "fp8": run_fp8}, args.warmup, args.runs)
            stats = {name: summary(xs) for name, xs in samples.items()}
            act_out = cum_m * k + cum_m * n * 2
            bytes_ = {"mxfp4": fp4_bytes + act_out + cum_m * k // 32, "bf16": G * n * k * 2 + cum_m * k + act_out,
                      "fp8": G * n * k + act_out}
            t = stats["mxfp4"]["median_us"] * 1e-6
            flops = 2.0 * cum_m * n * k
            spread = max(s["q75_us"] - s["q25_us"] for s in (stats["mxfp4"], stats["bf16"]))
            line = {
                "groups": G, "n": n, "k": k, "rows_per_group": rows, "weight_sets": len(sets), "runs": args.runs,
                "warmup": args.warmup, **{f"{name}_{key}": round(v, 2) for name, s in stats.items() for key, v in s.items()},
                **{f"{name}_bytes": b for name, b in bytes_.items()},
                "mxfp4_TBps": round(bytes_["mxfp4"] / t * 1e-12, 3), "mxfp4_PFLOPs": round(flops / t * 1e-15, 4),
                "mxfp4_share_of_5PF": round(flops / t / FP8_PEAK, 4),
                "speedup_vs_bf16": round(stats["bf16"]["median_us"] / stats["mxfp4"]["median_us"], 3),
                "speedup_vs_fp8": round(stats["fp8"]["median_us"] / stats["mxfp4"]["median_us"], 3),
                "faster_than_bf16_by_more_than_the_spread":
                    stats["bf16"]["median_us"] - stats["mxfp4"]["median_us"] > spread,
            }
            print(json.dumps(line), flush=True)
            if out_f:
                out_f.write(json.dumps(line) + "\n")
                out_f.flush()
        del sets
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
