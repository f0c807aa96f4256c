"""bmm_fp8 (csrc/bmm_fp8.hip) at the shapes it is for, beside the path a user has without it.

    python tools/bench_bmm_fp8.py [--out profiles/bmm_fp8_bench.jsonl] [--rounds 7] [--warmup 2] [--window-ms 50]

(b, m, n, k) = (128, 16, 512, 128) and (128, 16, 128, 512), the absorbed MLA projections of DeepSeek decode at 16 tokens,
and (1, 16, 4096, 4096), a decode-time linear layer.  Per shape one JSON line with the median and spread (max - min) over
--rounds rounds of the per-call time of

  bmm_fp8      the call, into a preallocated bf16 out;
  dequant_bmm  both operands cast to bf16, torch.bmm, times A_scale * B_scale: what a user runs without the kernel.

A round times, per candidate in turn, a window of back-to-back calls between two device events (as many calls as fill
--window-ms) and divides by the calls; --warmup untimed rounds come first.  `fp8_bytes` is what the call must move (a and
b once, out once) and `share_of_stream_floor` is fp8_bytes / time over the streaming-read floor of this chip (6.5 TB/s,
DESIGN.md 3.1).  The operands of these shapes (2 .. 17 MB) stay in the 256 MB Infinity Cache between back-to-back calls,
so that share says how far the call is from a bandwidth-bound one, not what HBM delivered.  `waves` names the wave
arrangement the host's rule picks on this device.
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
from flashinfer import _lib

DEV = torch.device("cuda", 0)
STREAM_FLOOR = 6.5e12
SHAPES = [(128, 16, 512, 128), (128, 16, 128, 512), (1, 16, 4096, 4096)]


def waves_along_k(b, m, n, k, cus):
    """The host's choice rule (csrc/bmm_fp8.hip, bmm_waves_along_k)."""
    bm = 16 if m <= 16 else 32 if m <= 32 else 64 if m <= 64 else 128
    return bm <= 32 and -(-k // 128) >= 4 and b * -(-m // bm) * -(-n // 128) < cus


def time_rounds(fns, rounds, warmup, window_s):
    """per candidate the per-call seconds of every round"""
    calls = {}
    for name, fn in fns.items():  # the first call loads code; the second is the estimate
        fn()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        calls[name] = max(1, min(20000, int(window_s / max(start.elapsed_time(stop) * 1e-3, 1e-7))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=50.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    assert args.rounds >= 7 and args.warmup >= 1, "at least 7 timed rounds and one warm-up round"
    cus = _lib.lib().fi_num_compute_units()
    out_f = open(args.out, "a") if args.out else None
    for b, m, n, k in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(n + k)
        a = torch.randn(b, m, k, device=DEV, generator=gen).to(torch.float8_e4m3fn)
        w = (torch.randn(b, n, k, device=DEV, generator=gen) / k ** 0.5).to(torch.float8_e4m3fn).transpose(-2, -1)
        sa, sb = torch.tensor([0.5], device=DEV), torch.tensor([1.5], device=DEV)
        out = torch.empty(b, m, n, dtype=torch.bfloat16, device=DEV)

        def run_bmm_fp8():
            flashinfer.bmm_fp8(a, w, sa, sb, torch.bfloat16, out=out)

        def run_dequant_bmm():
            torch.mul(torch.bmm(a.to(torch.bfloat16), w.to(torch.bfloat16)), sa * sb, out=out)

        samples, calls = time_rounds({"bmm_fp8": run_bmm_fp8, "dequant_bmm": run_dequant_bmm}, args.rounds, args.warmup,
                                     args.window_ms * 1e-3)
        fp8_bytes = a.numel() + w.numel() + 2 * out.numel()
        line = {"b": b, "m": m, "n": n, "k": k, "compute_units": cus, "waves": "along k" if waves_along_k(b, m, n, k, cus) else "along n",
                "fp8_bytes": fp8_bytes, "rounds": args.rounds, "warmup": args.warmup, "calls_per_round": calls}
        for cand, xs in samples.items():
            t = torch.tensor(sorted(xs), dtype=torch.float64)
            line.update({f"{cand}_median_us": round(t.median().item() * 1e6, 2),
                         f"{cand}_spread_us": round((t[-1] - t[0]).item() * 1e6, 2)})
        line["share_of_stream_floor"] = round(fp8_bytes / (line["bmm_fp8_median_us"] * 1e-6) / STREAM_FLOOR, 3)
        print(json.dumps(line), flush=True)
        if out_f:
            out_f.write(json.dumps(line) + "\n")
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
