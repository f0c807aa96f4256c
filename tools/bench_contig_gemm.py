"""group_deepgemm_fp8_nt_groupwise (contiguous layout, csrc/gemm_contig.hip) against group_gemm_fp8_nt_groupwise ("K"
major scales, the m_indptr path) on sorted, padding-free layouts, where both calls apply.

    python tools/bench_contig_gemm.py [--out profiles/contig_gemm_bench.jsonl] [--samples 21]

Cases at n = 4096, k = 7168: 8 experts x 1024 rows and 64 experts x 128 rows, each with random scales in [0.5, 1.5)
(the general fold path of the m_indptr kernels) and with power-of-two scales (what the reference's quantiser produces:
the m_indptr path may then take its hardware-scale 256 x 256 kernel, which the contiguous kernel has no form of).
A sample is ONE call between two device events, behind a write of a 512 MB buffer that evicts L2 and the Infinity
Cache.  First the baseline alone, twice (--samples each): the distance of the two medians is the spread a difference
must exceed.  Then the two calls alternately, --samples rounds.  Medians in microseconds and PFLOP/s (2 m n k) per JSON
line, and the largest difference of the two outputs.  `half_dead` is the 8 x 1024 layout with a dead 128-row block
behind every live one (twice the rows) against its live half alone: what dead blocks cost."""
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
N, K = 4096, 7168


def random_fp8(shape, gen):
    raw = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=gen)
    return torch.where((raw & 0x7F) == 0x7F, raw & 0xF0, raw).view(torch.float8_e4m3fn)  # no NaN codes


def scales(shape, gen, pow2):
    if pow2:
        return torch.exp2(torch.randint(-3, 1, shape, device=DEV, generator=gen).float())
    return torch.rand(shape, device=DEV, generator=gen) + 0.5


def sample(fn, flush, count):
    """per-call seconds of `count` single calls, each behind a cache flush"""
    out = []
    for _ in range(count):
        flush.add_(1)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop) * 1e-3)
    return out


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=21)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    flush = torch.zeros(512 << 20, dtype=torch.uint8, device=DEV)
    out_f = open(args.out, "a") if args.out else None

    def emit(line):
        print(json.dumps(line), flush=True)
        if out_f:
            out_f.write(json.dumps(line) + "\n")
            out_f.flush()

    for G, rows in ((8, 1024), (64, 128)):
        m = G * rows
        gen = torch.Generator(device=DEV).manual_seed(G)
        a, b = random_fp8((m, K), gen), random_fp8((G, N, K), gen)
        idx = torch.arange(m, device=DEV, dtype=torch.int32) // rows
        indptr = torch.arange(G + 1, device=DEV, dtype=torch.int32) * rows
        out_c = torch.empty(m, N, dtype=torch.bfloat16, device=DEV)
        out_i = torch.empty(m, N, dtype=torch.bfloat16, device=DEV)
        for pow2 in (False, True):
            sa, sb = scales((m, K // 128), gen, pow2), scales((G, N // 128, K // 128), gen, pow2)

            def contig():
                flashinfer.gemm.group_deepgemm_fp8_nt_groupwise(a, b, sa, sb, idx, out=out_c)

            def by_indptr():
                flashinfer.gemm.group_gemm_fp8_nt_groupwise(a, b, sa, sb, indptr, scale_major_mode="K", out=out_i)

            for fn in (contig, by_indptr, contig, by_indptr):  # code objects, flag slots
                fn()
            torch.cuda.synchronize()
            diff = (out_c.float() - out_i.float()).abs().max().item()
            base1, base2 = sample(by_indptr, flush, args.samples), sample(by_indptr, flush, args.samples)
            ts = {"contig": [], "indptr": []}
            for _ in range(args.samples):
                ts["contig"] += sample(contig, flush, 1)
                ts["indptr"] += sample(by_indptr, flush, 1)
            flop = 2.0 * m * N * K
            mc, mi = median(ts["contig"]), median(ts["indptr"])
            emit({"case": f"{G}x{rows}", "n": N, "k": K, "scales": "pow2" if pow2 else "random", "samples": args.samples,
                  "baseline_alone_median_us": [round(median(base1) * 1e6, 1), round(median(base2) * 1e6, 1)],
                  "baseline_spread_us": round(abs(median(base1) - median(base2)) * 1e6, 1),
                  "contig_median_us": round(mc * 1e6, 1), "indptr_median_us": round(mi * 1e6, 1),
                  "contig_min_max_us": [round(min(ts["contig"]) * 1e6, 1), round(max(ts["contig"]) * 1e6, 1)],
                  "indptr_min_max_us": [round(min(ts["indptr"]) * 1e6, 1), round(max(ts["indptr"]) * 1e6, 1)],
                  "contig_PFLOPs": round(flop / mc * 1e-15, 3), "indptr_PFLOPs": round(flop / mi * 1e-15, 3),
                  "contig_over_indptr": round(mc / mi, 3), "max_abs_output_difference": diff})
            if G == 8 and not pow2:
                # a dead block behind every live one: block j of the live layout is block 2 j here
                m2 = 2 * m
                a2 = torch.zeros(m2, K, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)
                sa2 = torch.ones(m2, K // 128, device=DEV)
                idx2 = torch.full((m2,), -1, dtype=torch.int32, device=DEV)
                live = (torch.arange(m2, device=DEV) // 128) % 2 == 0
                a2.view(torch.uint8)[live], sa2[live], idx2[live] = a.view(torch.uint8), sa, idx
                out2 = torch.empty(m2, N, dtype=torch.bfloat16, device=DEV)

                def half_dead():
                    flashinfer.gemm.group_deepgemm_fp8_nt_groupwise(a2, b, sa2, sb, idx2, out=out2)

                half_dead()
                torch.cuda.synchronize()
                assert torch.equal(out2[live], out_c)
                td, tl = [], []
                for _ in range(args.samples):
                    td += sample(half_dead, flush, 1)
                    tl += sample(contig, flush, 1)
                emit({"case": "half_dead_8x1024", "n": N, "k": K, "scales": "random", "samples": args.samples,
                      "half_dead_median_us": round(median(td) * 1e6, 1), "live_half_median_us": round(median(tl) * 1e6, 1),
                      "half_dead_over_live_half": round(median(td) / median(tl), 3)})
                del a2, sa2, out2
        del a, b, out_c, out_i
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
