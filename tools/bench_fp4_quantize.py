"""mxfp4_quantize and block_scale_interleave at a weight-sized shape, with mxfp8_quantize on the same input as the
yardstick (the quantiser the MXFP4 one is modelled on).

    python tools/bench_fp4_quantize.py [--experts 32] [--n 2880] [--k 2880] [--dtype bf16] [--rounds 30] [--calls 10]
                                       [--out file.jsonl]

Per operator one JSON line: the median over --rounds of the time per call (the three operators alternate inside every
round, all warmed up first), the bytes the operator must move -- every input byte read once, every output byte
written once, scale padding included -- and the resulting GB/s.  The default input is 531 MB, past the 256 MB
Infinity Cache, so the quantisers' figures are HBM rates; the 17 MB of the interleave stay in the cache.  A sample
is the time between two device events around --calls back-to-back Python calls, divided by their number: the host path
of a call (allocating the outputs, the ctypes call) runs while the kernel before it does, so from the second call on
the stream is never idle; --calls 1 gives the time of a single call on an idle stream, host path included.  There is
no gate.
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

DEV = torch.device("cuda", 0)
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def once(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experts", type=int, default=32)
    ap.add_argument("--n", type=int, default=2880)
    ap.add_argument("--k", type=int, default=2880)
    ap.add_argument("--dtype", default="bf16", choices=sorted(DTYPES))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m, k, nkb = args.experts * args.n, args.k, args.k // 32
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(m, k, device=DEV, generator=g).to(DTYPES[args.dtype])
    sf_linear = torch.randint(0, 255, (args.experts, args.n, nkb), dtype=torch.uint8, device=DEV, generator=g)
    pad = lambda v, a: (v + a - 1) // a * a
    sf_swizzled = pad(m, 128) * pad(nkb, 4)
    ops = {
        "mxfp4_quantize": (lambda: flashinfer.mxfp4_quantize(x), m * k * 2 + m * k // 2 + sf_swizzled),
        "mxfp8_quantize": (lambda: flashinfer.mxfp8_quantize(x), m * k * 2 + m * k + sf_swizzled),
        "block_scale_interleave": (lambda: flashinfer.block_scale_interleave(sf_linear),
                                   sf_linear.numel() + args.experts * pad(args.n, 128) * pad(nkb, 4)),
    }
    for fn, _ in ops.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in ops}
    for _ in range(args.rounds):
        for name, (fn, _) in ops.items():
            times[name].append(once(fn, args.calls))
    out = open(args.out, "w") if args.out else None
    for name, (_, nbytes) in ops.items():
        t = sorted(times[name])
        med = t[len(t) // 2]
        line = {"op": name, "shape": [args.experts, args.n, args.k], "dtype": args.dtype, "time_us": round(med * 1e6, 1),
                "min_us": round(t[0] * 1e6, 1), "max_us": round(t[-1] * 1e6, 1), "rounds": len(t),
                "calls_per_sample": args.calls, "bytes": nbytes, "GBps": round(nbytes / med / 1e9, 1)}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            out.write(text + "\n")
    if out:
        out.close()


if __name__ == "__main__":
    main()
