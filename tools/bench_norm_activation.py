"""flashinfer.norm and flashinfer.activation, operator by operator, against the torch-composed equivalent on the
same GPU.

    python tools/bench_norm_activation.py [--out profiles/norm_activation_bench.jsonl] [--rows 1,16,64,256,989,8192]
                                          [--hiddens 1024,4096,8192,16384] [--ds 11008,14336] [--dtypes bf16,f16]
                                          [--ops rmsnorm,fused_add_rmsnorm,...] [--fill 0.1]

Per (operator, rows, hidden, dtype) one JSON line: the device-event median of this library's call and of the torch
composition (alternating in one loop, enough repeats to fill --fill seconds each, every shape warmed up), the median
of torch.nn.functional.rms_norm as a second comparison where torch has it (the plain row and head forms), the
algorithmic bytes (norm: one read and one write of the rows; fused add: two reads and two writes; activation:
3 * d * itemsize per token), the resulting rate and its share of the 6.3 TB/s streaming figure.  From 4 MB per set
of inputs (what L2 no longer holds and the 256 MB Infinity Cache would serve) the inputs rotate over more than 256 MB.

A sample is the time between two events recorded around the Python call on an idle stream, so at small shapes it is
the host path of the call, not the kernel: points below 64 rows are launch-bound and reported only.  Kernel times come
from `rocprofv3 --kernel-trace --stats -- python tools/bench_norm_activation.py ...`.

torch compositions (what a serving stack runs when these operators are missing; f32 arithmetic like the kernels):
  rmsnorm            x.float() -> pow(2).mean(-1) -> rsqrt(+eps) -> * -> * w.float() -> .to(dtype)
  fused_add_rmsnorm  the same after s = x.float() + r.float(); r.copy_(s); x.copy_(result)
  act_and_mul        F.silu / F.gelu(gate.float()) * up.float() -> .to(dtype)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch
import torch.nn.functional as F

import flashinfer

DEV = torch.device("cuda", 0)
EPS = 1e-6
HBM_STREAM = 6.3e12  # bytes / s
ROTATE_BYTES = 256 << 20
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def torch_norm(x, w, bias):
    x32 = x.float()
    x32 = x32 * torch.rsqrt(x32.pow(2).mean(dim=-1, keepdim=True) + EPS)
    return (x32 * (w.float() + bias if bias else w.float())).to(x.dtype)


def torch_fused(x, r, w, bias):
    s = x.float() + r.float()
    r.copy_(s)
    out = s * torch.rsqrt(s.pow(2).mean(dim=-1, keepdim=True) + EPS)
    x.copy_(out * (w.float() + bias if bias else w.float()))


def torch_act(x, fn):
    d = x.shape[-1] // 2
    return (fn(x[..., :d].float()) * x[..., d:].float()).to(x.dtype)


HAS_F_RMS_NORM = hasattr(F, "rms_norm")
# name -> (kind, ours(bufs, w), torch composition(bufs, w), F.rms_norm variant or None)
OPS = {
    "rmsnorm": ("norm", lambda b, w: flashinfer.rmsnorm(b[0], w, EPS), lambda b, w: torch_norm(b[0], w, 0.0),
                lambda b, w: F.rms_norm(b[0], (b[0].shape[-1],), w, EPS)),
    "gemma_rmsnorm": ("norm", lambda b, w: flashinfer.gemma_rmsnorm(b[0], w, EPS),
                      lambda b, w: torch_norm(b[0], w, 1.0), None),
    "fused_add_rmsnorm": ("fused", lambda b, w: flashinfer.fused_add_rmsnorm(b[0], b[1], w, EPS),
                          lambda b, w: torch_fused(b[0], b[1], w, 0.0), None),
    "gemma_fused_add_rmsnorm": ("fused", lambda b, w: flashinfer.gemma_fused_add_rmsnorm(b[0], b[1], w, EPS),
                                lambda b, w: torch_fused(b[0], b[1], w, 1.0), None),
    "rmsnorm[heads=8]": ("head", lambda b, w: flashinfer.rmsnorm(b[0], w, EPS), lambda b, w: torch_norm(b[0], w, 0.0),
                         lambda b, w: F.rms_norm(b[0], (b[0].shape[-1],), w, EPS)),
    "rmsnorm[heads=32]": ("head", lambda b, w: flashinfer.rmsnorm(b[0], w, EPS), lambda b, w: torch_norm(b[0], w, 0.0),
                          lambda b, w: F.rms_norm(b[0], (b[0].shape[-1],), w, EPS)),
    "silu_and_mul": ("act", lambda b, w: flashinfer.silu_and_mul(b[0]), lambda b, w: torch_act(b[0], F.silu), None),
    "gelu_and_mul": ("act", lambda b, w: flashinfer.gelu_and_mul(b[0]), lambda b, w: torch_act(b[0], F.gelu), None),
    "gelu_tanh_and_mul": ("act", lambda b, w: flashinfer.gelu_tanh_and_mul(b[0]),
                          lambda b, w: torch_act(b[0], lambda t: F.gelu(t, approximate="tanh")), None),
}


def once(fn, bufs, w):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(bufs, w)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(fns, sets, w, fill_s):
    """fns[0] is ours; the others run every few rounds of it so that all alternate over the same window"""
    for s in sets[:2]:
        for fn in fns:
            fn(s, w)
    torch.cuda.synchronize()
    first = [once(fn, sets[0], w) for fn in fns]
    n = [min(max(math.ceil(fill_s / max(t, 1e-6)), 7), 4000) for t in first]
    every = [max(n[0] // min(k, n[0]), 1) for k in n]
    times = [[] for _ in fns]
    for i in range(n[0]):
        s = sets[i % len(sets)]
        for j, fn in enumerate(fns):
            if i % every[j] == 0:
                times[j].append(once(fn, s, w))
    return [(median(t), len(t)) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", default="1,16,64,256,989,8192")
    ap.add_argument("--hiddens", default="1024,4096,8192,16384")
    ap.add_argument("--ds", default="11008,14336")
    ap.add_argument("--head-dim", type=int, default=128)
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--fill", type=float, default=0.1)
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None
    g = torch.Generator(device=DEV).manual_seed(0)
    for name in args.ops.split(","):
        kind, ours, theirs, f_rms = OPS[name]
        widths = {"act": args.ds, "head": str(args.head_dim)}.get(kind, args.hiddens)
        for dtype_name in args.dtypes.split(","):
            dtype = DTYPES[dtype_name]
            for width in map(int, widths.split(",")):
                for rows in map(int, args.rows.split(",")):
                    heads = int(name.split("=")[1][:-1]) if kind == "head" else 1
                    shape = {"act": (rows, 2 * width), "head": (rows, heads, width)}.get(kind, (rows, width))
                    tensors = 2 if kind == "fused" else 1
                    elems = rows * heads * width
                    algo = {"norm": 2, "head": 2, "fused": 4, "act": 3}[kind] * elems * 2
                    set_bytes = tensors * math.prod(shape) * 2
                    nsets = 1 if set_bytes < (4 << 20) else ROTATE_BYTES // set_bytes + 2
                    sets = [[(torch.randn(shape, device=DEV, generator=g) * (3.0 if kind == "act" else 1.0)).to(dtype)
                             for _ in range(tensors)] for _ in range(nsets)]
                    w = (1.0 + 0.1 * torch.randn(width, device=DEV, generator=g)).to(dtype)
                    fns = [ours, theirs] + ([f_rms] if f_rms is not None and HAS_F_RMS_NORM else [])
                    res = measure(fns, sets, w, args.fill)
                    (t, n), (t_torch, n_torch) = res[0], res[1]
                    line = {
                        "op": name, "rows": rows, "hidden": width, "dtype": dtype_name, "time_us": round(t * 1e6, 2),
                        "repeats": n, "algorithmic_bytes": algo, "rate_TBps": round(algo / t / 1e12, 3),
                        "share_of_6.3TBps": round(algo / t / HBM_STREAM, 3), "torch_time_us": round(t_torch * 1e6, 2),
                        "torch_repeats": n_torch, "speedup_vs_torch": round(t_torch / t, 2),
                        "rotating_sets": nsets,
                    }
                    if len(res) > 2:
                        line["torch_F_rms_norm_time_us"] = round(res[2][0] * 1e6, 2)
                        line["speedup_vs_F_rms_norm"] = round(res[2][0] / t, 2)
                    text = json.dumps(line)
                    print(text, flush=True)
                    if out:
                        out.write(text + "\n")
                        out.flush()
                    del sets
    if out:
        out.close()


if __name__ == "__main__":
    main()
