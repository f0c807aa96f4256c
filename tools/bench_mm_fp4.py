"""mm_fp4 (MXFP4 x MXFP4) at the projections of a 70B-class dense layer against what a user has without it.

    python tools/bench_mm_fp4.py [--out profiles/mm_fp4_bench.jsonl] [--weights 10240x8192,8192x8192,57344x8192,8192x28672]
                                 [--rows 1,16,64,256,1024,4096,8192] [--rounds 7] [--warmup 2] [--window-ms 10] [--kernels]

Per (weight (n, k), rows m) one JSON line with the median over --rounds rounds and the run-to-run spread (max - min over
the rounds) of the per-call time of each candidate, bf16 output, alpha=None.  A round times, per candidate in turn, a
window of back-to-back calls between two device events on an idle stream (as many calls as fill --window-ms, at least
one) and divides by the calls; --warmup untimed rounds come first.

  fp4     flashinfer.mm_fp4, the entry point's own kernel choice;
  bf16    baseline (a): torch.matmul in bf16 on weights dequantised beforehand (untimed), the strongest thing a user
          has without this function;
  fp8     baseline (b): this library's gemm_fp8_nt_groupwise on the same (m, n, k) with power-of-two (unit) scales;
  fp4_streaming / fp4_tiled   with --kernels: each of the two kernels forced (FI_MM_FP4_KERNEL = 1 / 2), the sweep the
          entry point's switch row count comes from.

and from them: weight bytes per second against the 8 TB/s HBM peak (m <= 64), FLOP/s against the 10 PFLOP/s fp4 peak
(m >= 1024), the speed-ups, and whether fp4 beats bf16 by more than the larger of the two spreads.  Operands are random,
not zeros.  Weight sets rotate so that at least 512 MB pass between two uses of the same bytes (the Infinity Cache holds
256 MB).
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
from flashinfer import _lib, _mx

DEV = torch.device("cuda", 0)
HBM_PEAK = 8.0e12
FP4_PEAK = 10.0e15
ROTATE_BYTES = 512 << 20
E2M1 = [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]


def ceil_to(x, m):
    return (x + m - 1) // m * m


def swizzle_scale(sf):
    """[rows, nkb] -> the swizzled bytes (ceil(rows / 128) * 128, nkb), on the device"""
    rows, nkb = sf.shape
    r = torch.arange(rows, device=sf.device).view(-1, 1).expand(rows, nkb)
    kb = torch.arange(nkb, device=sf.device).view(1, -1).expand(rows, nkb)
    out = torch.zeros(ceil_to(rows, 128) * nkb, dtype=torch.uint8, device=sf.device)
    out[_mx.sf_offset(r, kb, nkb).reshape(-1)] = sf.reshape(-1)
    return out.view(-1, nkb)


def random_mxfp4(rows, k, lo, hi, gen):
    packed = torch.randint(0, 256, (rows, k // 2), dtype=torch.uint8, device=DEV, generator=gen)
    sf = torch.randint(lo, hi, (rows, k // 32), dtype=torch.uint8, device=DEV, generator=gen)
    return packed, sf


def dequantize_bf16(packed, sf):
    """exact: an e2m1 value times a power of two fits bf16"""
    table = torch.tensor(E2M1, dtype=torch.float32, device=DEV)
    out = torch.empty(packed.shape[0], packed.shape[1] * 2, dtype=torch.bfloat16, device=DEV)
    for r0 in range(0, packed.shape[0], 4096):
        p = packed[r0:r0 + 4096]
        codes = torch.stack([p & 15, p >> 4], dim=-1).flatten(-2).long()
        out[r0:r0 + 4096] = (table[codes] * torch.exp2(sf[r0:r0 + 4096].float() - 127).repeat_interleave(32, dim=1)).to(torch.bfloat16)
    return out


def random_fp8(rows, k, gen):
    raw = torch.randint(0, 256, (rows, k), dtype=torch.uint8, device=DEV, generator=gen)
    return torch.where((raw & 0x7F) == 0x7F, raw & 0xF0, raw).view(torch.float8_e4m3fn)  # no NaN codes


def make_weights(n, k, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    packed, sf = random_mxfp4(n, k, 118, 124, gen)
    return {"packed_t": packed.T, "sf_t": swizzle_scale(sf).T, "bf16_t": dequantize_bf16(packed, sf).T,
            "fp8": random_fp8(n, k, gen), "fp8_scale": torch.ones(k // 128, ceil_to(n, 128) // 128, dtype=torch.float32, device=DEV)}


def time_rounds(fns, rounds, warmup, window_s):
    """per candidate the per-call seconds of every round"""
    calls = {}
    for name, fn in fns.items():  # first calls load code and pick algorithms; the second is the estimate
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        calls[name] = max(1, min(1000, int(window_s / max(start.elapsed_time(stop) * 1e-3, 1e-7))))
    samples = {name: [] for name in fns}
    for rnd in range(warmup + rounds):
        for name, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(calls[name]):
                fn()
            stop.record()
            stop.synchronize()
            if rnd >= warmup:
                samples[name].append(start.elapsed_time(stop) * 1e-3 / calls[name])
    return samples, calls


def summary(xs):
    t = torch.tensor(sorted(xs), dtype=torch.float64)
    return {"median_us": t.median().item() * 1e6, "min_us": t[0].item() * 1e6, "max_us": t[-1].item() * 1e6,
            "spread_us": (t[-1] - t[0]).item() * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--weights", default="10240x8192,8192x8192,57344x8192,8192x28672")
    ap.add_argument("--rows", default="1,16,64,256,1024,4096,8192")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=10.0)
    ap.add_argument("--kernels", action="store_true", help="also time each of the two kernels forced")
    ap.add_argument("--no-baselines", action="store_true", help="with --kernels: skip bf16 and fp8")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    assert args.rounds >= 7 and args.warmup >= 1, "at least 7 timed rounds and one warm-up round"
    out_f = open(args.out, "a") if args.out else None
    for n, k in (tuple(int(v) for v in w.split("x")) for w in args.weights.split(",")):
        fp4_bytes = n * (k // 2 + k // 32)
        sets = [make_weights(n, k, 100 + i) for i in range(1 + -(-ROTATE_BYTES // fp4_bytes))]
        for m in (int(x) for x in args.rows.split(",")):
            gen = torch.Generator(device=DEV).manual_seed(m)
            a_q, a_sf = random_mxfp4(m, k, 125, 129, gen)
            a_sf = swizzle_scale(a_sf)
            x = torch.randn(m, k, device=DEV, dtype=torch.bfloat16, generator=gen)
            x_fp8 = random_fp8(m, k, gen)
            ones = torch.ones(k // 128, m, dtype=torch.float32, device=DEV)
            out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
            turn = {}

            def pick(name):
                turn[name] = turn.get(name, 0) + 1
                return sets[turn[name] % len(sets)]

            def run_fp4(name="fp4"):
                w = pick(name)
                flashinfer.mm_fp4(a_q, w["packed_t"], a_sf, w["sf_t"], None, torch.bfloat16, out, block_size=32,
                                  use_nvfp4=False)

            def run_bf16():
                torch.matmul(x, pick("bf16")["bf16_t"], out=out)

            def run_fp8():
                w = pick("fp8")
                flashinfer.gemm_fp8_nt_groupwise(x_fp8, w["fp8"], ones, w["fp8_scale"], "MN", out=out)

            def forced(value, name):
                def run():
                    _lib.set_option("FI_MM_FP4_KERNEL", value)
                    run_fp4(name)
                    _lib.set_option("FI_MM_FP4_KERNEL", None)
                return run

            fns = {"fp4": run_fp4}
            if not args.no_baselines:
                fns.update({"bf16": run_bf16, "fp8": run_fp8})
            if args.kernels:
                fns.update({"fp4_streaming": forced(1, "fp4_streaming"), "fp4_tiled": forced(2, "fp4_tiled")})
            samples, calls = time_rounds(fns, args.rounds, args.warmup, args.window_ms * 1e-3)
            stats = {name: summary(xs) for name, xs in samples.items()}
            t = stats["fp4"]["median_us"] * 1e-6
            flops = 2.0 * m * n * k
            line = {"n": n, "k": k, "m": m, "weight_sets": len(sets), "rounds": args.rounds, "warmup": args.warmup,
                    "calls_per_round": calls,
                    **{f"{name}_{key}": round(v, 2) for name, s in stats.items() for key, v in s.items()},
                    "fp4_weight_bytes": fp4_bytes, "fp4_weight_TBps": round(fp4_bytes / t * 1e-12, 3),
                    "fp4_share_of_8TBps": round(fp4_bytes / t / HBM_PEAK, 4), "fp4_PFLOPs": round(flops / t * 1e-15, 4),
                    "fp4_share_of_10PF": round(flops / t / FP4_PEAK, 4)}
            if "bf16" in stats:
                spread = max(stats["fp4"]["spread_us"], stats["bf16"]["spread_us"])
                line.update({
                    "speedup_vs_bf16": round(stats["bf16"]["median_us"] / stats["fp4"]["median_us"], 3),
                    "speedup_vs_fp8": round(stats["fp8"]["median_us"] / stats["fp4"]["median_us"], 3),
                    "faster_than_bf16_by_more_than_the_spread": stats["bf16"]["median_us"] - stats["fp4"]["median_us"] > spread})
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
