"""batch_deepgemm_fp8_nt_groupwise (masked layout, csrc/gemm_masked.hip) at DeepSeek-V3 expert shapes at EP 8 against
the path a user has without it.

    python tools/bench_masked_gemm.py [--out profiles/masked_gemm_bench.jsonl] [--rounds 7] [--warmup 2] [--window-ms 10]

E = 32 local experts, (n, k) = (4096, 7168) and (7168, 2048), a buffer of m = 1024 rows per expert; masked_m uniform at 1,
8, 32, 64, 128 and one skewed draw (a quarter of the experts hold 48 .. 64 rows, the rest 0 .. 8).  Per case one JSON line
with the median and spread (max - min) over --rounds rounds of the per-call time of

  masked         the new call, expected_m = the mean of masked_m rounded up;
  grouped        group_gemm_fp8_nt_groupwise ("K" scales) on rows already packed expert after expert: the GEMM alone;
  grouped_gather the same plus what the masked layout costs in front of it on every decode step: m_indptr from masked_m
                 (entries rounded up to 4, a cumsum on the device) and the gather of a and a_scale into packed rows.  The
                 gather's row index is built beforehand, untimed (building it needs a host read of masked_m).

A round times, per candidate in turn, a window of back-to-back calls between two device events (as many calls as fill
--window-ms) and divides by the calls; --warmup untimed rounds come first.  The weights are 940 MB resp. 470 MB per call,
more than the 256 MB Infinity Cache, so every call streams them from HBM: bytes(b) / time is reported in TB/s, beside
its share of the streaming-read floor of this chip (6.3 .. 6.8 TB/s; 6.5 is used).  Operands are random
bytes (no NaN codes) and random scales in [0.5, 1.5): not powers of two, the general path of the grouped kernels.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch

import flashinfer.gemm

DEV = torch.device("cuda", 0)
STREAM_FLOOR = 6.5e12
E, M = 32, 1024


def random_fp8(shape, gen):
    raw = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=gen)
    return torch.where((raw & 0x7F) == 0x7F, raw & 0xF0, raw).view(torch.float8_e4m3fn)  # no NaN codes


def random_scale(shape, gen):
    return torch.rand(shape, device=DEV, generator=gen) + 0.5


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


def masked_draws():
    g = torch.Generator().manual_seed(7)
    skew = torch.where(torch.arange(E) % 4 == 0, torch.randint(48, 65, (E,), generator=g), torch.randint(0, 9, (E,), generator=g))
    return [(f"uniform_{r}", torch.full((E,), r)) for r in (1, 8, 32, 64, 128)] + [("skewed", skew)]


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
    for n, k in ((4096, 7168), (7168, 2048)):
        gen = torch.Generator(device=DEV).manual_seed(n)
        a, a_scale = random_fp8((E, M, k), gen), random_scale((E, M, k // 128), gen)
        b, b_scale = random_fp8((E, n, k), gen), random_scale((E, n // 128, k // 128), gen)
        out = torch.empty(E, M, n, dtype=torch.bfloat16, device=DEV)
        for name, draw in masked_draws():
            masked_m = draw.to(torch.int32).to(DEV)
            expected_m = max(1, -(-int(draw.sum()) // E))
            padded = (draw + 3) // 4 * 4
            cum_m = int(padded.sum())
            # packed row p of expert e is row p - m_indptr[e] of a[e]; padding rows re-read the expert's row 0
            starts = torch.cumsum(padded, 0) - padded
            rows = torch.cat([e * M + torch.where(torch.arange(int(padded[e])) < draw[e], torch.arange(int(padded[e])), 0)
                              for e in range(E)]).to(DEV)
            a_packed = torch.empty(cum_m, k, dtype=torch.float8_e4m3fn, device=DEV)
            sa_packed = torch.empty(cum_m, k // 128, dtype=torch.float32, device=DEV)
            out_packed = torch.empty(cum_m, n, dtype=torch.bfloat16, device=DEV)
            m_indptr = torch.zeros(E + 1, dtype=torch.int32, device=DEV)
            a_bytes, a_flat, sa_flat = a_packed.view(torch.uint8), a.view(torch.uint8).view(E * M, k), a_scale.view(E * M, k // 128)

            def run_masked():
                flashinfer.gemm.batch_deepgemm_fp8_nt_groupwise(a, b, a_scale, b_scale, masked_m, expected_m, out=out)

            def run_grouped():
                flashinfer.gemm.group_gemm_fp8_nt_groupwise(a_packed, b, sa_packed, b_scale, m_indptr, scale_major_mode="K",
                                                            out=out_packed)

            def run_grouped_gather():
                m_indptr[1:] = torch.cumsum((masked_m + 3) // 4 * 4, 0)
                torch.index_select(a_flat, 0, rows, out=a_bytes)
                torch.index_select(sa_flat, 0, rows, out=sa_packed)
                run_grouped()

            run_grouped_gather()  # fills the packed operands and m_indptr for run_grouped
            assert int(m_indptr[-1]) == cum_m and int(starts[-1] + padded[-1]) == cum_m
            fns = {"masked": run_masked, "grouped": run_grouped, "grouped_gather": run_grouped_gather}
            samples, calls = time_rounds(fns, args.rounds, args.warmup, args.window_ms * 1e-3)
            line = {"E": E, "m": M, "n": n, "k": k, "masked_m": name, "live_rows": int(draw.sum()), "expected_m": expected_m,
                    "b_bytes": b.numel(), "rounds": args.rounds, "warmup": args.warmup, "calls_per_round": calls}
            for cand, xs in samples.items():
                t = torch.tensor(sorted(xs), dtype=torch.float64)
                med = t.median().item()
                line.update({f"{cand}_median_us": round(med * 1e6, 2), f"{cand}_spread_us": round((t[-1] - t[0]).item() * 1e6, 2),
                             f"{cand}_b_TBps": round(b.numel() / med * 1e-12, 3)})
            line["masked_share_of_stream_floor"] = round(line["masked_b_TBps"] * 1e12 / STREAM_FLOOR, 3)
            line["speedup_vs_grouped"] = round(line["grouped_median_us"] / line["masked_median_us"], 3)
            line["speedup_vs_grouped_gather"] = round(line["grouped_gather_median_us"] / line["masked_median_us"], 3)
            print(json.dumps(line), flush=True)
            if out_f:
                out_f.write(json.dumps(line) + "\n")
                out_f.flush()
        del a, b, out
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
