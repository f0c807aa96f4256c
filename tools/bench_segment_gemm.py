"""SegmentGEMMWrapper (csrc/segment_gemm.hip) at multi-LoRA shapes against what a user has without it.

    python tools/bench_segment_gemm.py [--out profiles/segment_gemm_bench.jsonl] [--rounds 7] [--warmup 2] [--window-ms 10]

bf16, column-major weights, d = 4096, rank 16 and 64, the shrink step (d -> rank) and the expand step (rank -> d); a
decode-like batch (256 segments of 1 row) and a prefill-like one (16 segments of 512 rows), 8 distinct adapters chosen
through weight_indices in both.  Per case one JSON line with the median and spread (max - min) over --rounds rounds of
the per-call time of

  segment     the new call, seg_indptr and weight_indices on the device;
  loop        torch.matmul per segment into its slice of the output; slices and weight views are made beforehand, untimed;
  group16     fused_moe.moe_group_gemm_16bit, rank-64 shrink only (its n % 64 == 0, k % 64 == 0 rule): it has no weight
              indirection, so it gets one gathered copy of the weight per segment, made beforehand, untimed.

A round times, per candidate in turn, a window of back-to-back calls between two device events (as many calls as fill
--window-ms) and divides by the calls; --warmup untimed rounds come first.  The floor of a case is the bytes it must
move -- x, the 8 distinct weights, y -- at the 6.5 TB/s streaming rate of this chip; `share_of_floor` is
floor / median of `segment`.  The outputs of the three candidates are compared before anything is timed.
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
from flashinfer import fused_moe

DEV = torch.device("cuda", 0)
STREAM_FLOOR = 6.5e12
D, ADAPTERS = 4096, 8
BATCHES = {"decode_256x1": (256, 1), "prefill_16x512": (16, 512)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window-ms", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    assert args.rounds >= 7 and args.warmup >= 1, "at least 7 timed rounds and one warm-up round"
    out_f = open(args.out, "a") if args.out else None
    wrapper = flashinfer.SegmentGEMMWrapper(torch.empty(1024, dtype=torch.int8, device=DEV))
    for rank in (16, 64):
        for step, (d_in, d_out) in (("shrink", (D, rank)), ("expand", (rank, D))):
            for batch_name, (segments, seg_rows) in BATCHES.items():
                gen = torch.Generator(device=DEV).manual_seed(rank + d_in)
                rows = segments * seg_rows
                x = torch.randn(rows, d_in, device=DEV, generator=gen).bfloat16()
                weights = (torch.randn(ADAPTERS, d_out, d_in, device=DEV, generator=gen) * d_in ** -0.5).bfloat16()
                ids = (torch.arange(segments) * 5 + 3) % ADAPTERS
                indptr = (torch.arange(segments + 1) * seg_rows).to(DEV)
                ids_dev = ids.to(DEV)
                y = {name: torch.zeros(rows, d_out, dtype=torch.bfloat16, device=DEV) for name in ("segment", "loop")}
                pieces = [(x[s * seg_rows:(s + 1) * seg_rows], weights[int(ids[s])].T, y["loop"][s * seg_rows:(s + 1) * seg_rows])
                          for s in range(segments)]

                def run_segment():
                    wrapper.run(x, weights, segments, True, out=y["segment"], seg_indptr=indptr, weight_indices=ids_dev)

                def run_loop():
                    for xs, wt, ys in pieces:
                        torch.matmul(xs, wt, out=ys)

                fns = {"segment": run_segment, "loop": run_loop}
                if step == "shrink" and rank % 64 == 0:
                    gathered = weights[ids_dev].contiguous()
                    indptr32 = indptr.int()
                    y["group16"] = torch.zeros(rows, d_out, dtype=torch.bfloat16, device=DEV)

                    def run_group16():
                        fused_moe.moe_group_gemm_16bit(x, gathered, indptr32, out=y["group16"])

                    fns["group16"] = run_group16
                for fn in fns.values():
                    fn()
                torch.cuda.synchronize()
                for name in fns:  # bf16 outputs of two f32 accumulation orders: an ulp or two apart
                    torch.testing.assert_close(y[name].float(), y["loop"].float(), rtol=2.0 ** -6, atol=2.0 ** -6)
                samples, calls = time_rounds(fns, args.rounds, args.warmup, args.window_ms * 1e-3)
                moved = 2 * (x.numel() + weights.numel() + rows * d_out)
                line = {"rank": rank, "step": step, "d_in": d_in, "d_out": d_out, "batch": batch_name, "rows": rows,
                        "bytes_moved": moved, "floor_us": round(moved / STREAM_FLOOR * 1e6, 3), "rounds": args.rounds,
                        "warmup": args.warmup, "calls_per_round": calls}
                for cand, xs in samples.items():
                    t = torch.tensor(sorted(xs), dtype=torch.float64)
                    line.update({f"{cand}_median_us": round(t.median().item() * 1e6, 2),
                                 f"{cand}_spread_us": round((t[-1] - t[0]).item() * 1e6, 2)})
                line["share_of_floor"] = round(line["floor_us"] / line["segment_median_us"], 4)
                for cand in fns:
                    if cand != "segment":
                        line[f"speedup_vs_{cand}"] = round(line[f"{cand}_median_us"] / line["segment_median_us"], 3)
                print(json.dumps(line), flush=True)
                if out_f:
                    out_f.write(json.dumps(line) + "\n")
                    out_f.flush()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
