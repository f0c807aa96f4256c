"""flashinfer.sampling, operator by operator, against the torch-composed equivalent on the same GPU.

    python tools/bench_sampling.py [--out profiles/sampling_bench.jsonl] [--batches 1,16,64,256,989]
                                   [--vocabs 32000,128256] [--ops softmax,top_k_sampling_from_probs,...]

Per (operator, batch, vocab, distribution) one JSON line: the device-event median of this library's call and of the
torch composition (alternating in one loop, enough repeats to fill 0.2 s each, every shape warmed up), the algorithmic
bytes (one read of the rows, plus one write where the operator writes rows), the resulting rate, and "equivalent
passes" = time x 6.3 TB/s / row bytes.  Inputs are f32; probabilities come from softmax(normal(1)) and from the peaky
gumbel(0.1) of the reference's tests; k = 50, p = 0.9, min_p = 0.1.  From batch 256 on the inputs rotate over more
than 256 MB so that the Infinity Cache does not serve them.

A sample is the time between two events recorded around the Python call on an idle stream, so it holds the host path
of the call as well (dtype / contiguity checks, the output allocation, reading and advancing the generator, ctypes)
wherever that is longer than the kernel: at batch 1-16 most of a sample is that host path, at batch 989 x 128256
about a tenth.  Kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_sampling.py ...`.

torch equivalents: torch.softmax; torch.multinomial; for top-k / top-p / joint samplers and the two renorms a
descending sort + cumsum + mask + renormalise (+ multinomial and a gather, or a scatter back); min-p needs no sort in
torch either (max, mask, renormalise, multinomial); top_k_mask_logits is torch.topk + masked_fill.
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

import flashinfer

DEV = torch.device("cuda", 0)
K, P, MIN_P = 50, 0.9, 0.1
HBM_STREAM = 6.3e12  # bytes / s, the streaming rate the pass count is expressed in
ROTATE_BYTES = 256 << 20
FILL_S = 0.2


def make_logits(dist, rows, vocab, g):
    if dist == "normal(1)":
        return torch.randn(rows, vocab, device=DEV, generator=g)
    u = torch.rand(rows, vocab, device=DEV, generator=g)
    return torch.log(-torch.log(u + 1e-20) + 1e-20) / 0.1


def sorted_filter(probs, k=None, p=None):
    sp, idx = torch.sort(probs, dim=-1, descending=True)
    keep = torch.ones_like(sp, dtype=torch.bool)
    if k is not None:
        keep[:, k:] = False
    if p is not None:
        keep &= (torch.cumsum(sp, dim=-1) - sp) < p
    sp = sp * keep
    return sp / sp.sum(dim=-1, keepdim=True), idx


def sorted_sample(probs, k=None, p=None):
    sp, idx = sorted_filter(probs, k, p)
    return idx.gather(1, torch.multinomial(sp, 1))


def sorted_renorm(probs, k=None, p=None):
    sp, idx = sorted_filter(probs, k, p)
    return torch.empty_like(probs).scatter_(1, idx, sp)


def top_k_first_torch(probs):
    sp, idx = sorted_filter(probs, k=K)
    keep = (torch.cumsum(sp, dim=-1) - sp) < P
    sp = sp * keep
    return idx.gather(1, torch.multinomial(sp / sp.sum(dim=-1, keepdim=True), 1))


def min_p_torch(probs):
    kept = probs * (probs >= MIN_P * probs.max(dim=-1, keepdim=True).values)
    return torch.multinomial(kept / kept.sum(dim=-1, keepdim=True), 1)


def mask_logits_torch(logits):
    kth = torch.topk(logits, K, dim=-1).values[:, -1:]
    return logits.masked_fill(logits < kth, float("-inf"))


S = flashinfer.sampling
# name -> (input kind, writes rows, ours, torch)
OPS = {
    "softmax": ("logits", True, lambda x: S.softmax(x), lambda x: torch.softmax(x, dim=-1)),
    "sampling_from_probs": ("probs", False, lambda x: S.sampling_from_probs(x), lambda x: torch.multinomial(x, 1)),
    "sampling_from_logits": ("logits", False, lambda x: S.sampling_from_logits(x),
                             lambda x: torch.multinomial(torch.softmax(x, dim=-1), 1)),
    "top_k_sampling_from_probs": ("probs", False, lambda x: S.top_k_sampling_from_probs(x, K),
                                  lambda x: sorted_sample(x, k=K)),
    "top_p_sampling_from_probs": ("probs", False, lambda x: S.top_p_sampling_from_probs(x, P),
                                  lambda x: sorted_sample(x, p=P)),
    "min_p_sampling_from_probs": ("probs", False, lambda x: S.min_p_sampling_from_probs(x, MIN_P), min_p_torch),
    "top_k_top_p_sampling_from_probs[joint]": (
        "probs", False, lambda x: S.top_k_top_p_sampling_from_probs(x, K, P, filter_apply_order="joint"),
        lambda x: sorted_sample(x, k=K, p=P)),
    "top_k_top_p_sampling_from_probs[top_k_first]": (
        "probs", False, lambda x: S.top_k_top_p_sampling_from_probs(x, K, P), top_k_first_torch),
    "top_k_top_p_sampling_from_logits[top_k_first]": (
        "logits", False, lambda x: S.top_k_top_p_sampling_from_logits(x, K, P),
        lambda x: top_k_first_torch(torch.softmax(x, dim=-1))),
    "top_p_renorm_probs": ("probs", True, lambda x: S.top_p_renorm_probs(x, P), lambda x: sorted_renorm(x, p=P)),
    "top_k_renorm_probs": ("probs", True, lambda x: S.top_k_renorm_probs(x, K), lambda x: sorted_renorm(x, k=K)),
    "top_k_mask_logits": ("logits", True, lambda x: S.top_k_mask_logits(x, K), mask_logits_torch),
}


def once(fn, x):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(ours, theirs, bufs):
    for x in bufs[:2]:  # warm-up on this shape
        ours(x)
        theirs(x)
    torch.cuda.synchronize()
    t_o, t_t = once(ours, bufs[0]), once(theirs, bufs[0])
    n_o = min(max(math.ceil(FILL_S / max(t_o, 1e-6)), 7), 4000)
    n_t = min(max(math.ceil(FILL_S / max(t_t, 1e-6)), 5), n_o)
    every = max(n_o // n_t, 1)  # the torch call runs every `every`-th round, so the two alternate over the window
    to, tt = [], []
    for i in range(n_o):
        x = bufs[i % len(bufs)]
        to.append(once(ours, x))
        if i % every == 0:
            tt.append(once(theirs, x))
    return median(to), len(to), median(tt), len(tt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default="1,16,64,256,989")
    ap.add_argument("--vocabs", default="32000,128256")
    ap.add_argument("--ops", default=",".join(OPS))
    args = ap.parse_args()
    out = open(args.out, "w") if args.out else None
    torch.manual_seed(0)
    g = torch.Generator(device=DEV).manual_seed(0)
    for vocab in map(int, args.vocabs.split(",")):
        for batch in map(int, args.batches.split(",")):
            row_bytes = batch * vocab * 4
            nbuf = 1 if batch < 256 else ROTATE_BYTES // row_bytes + 2
            for dist in ("normal(1)", "gumbel(0.1)"):
                logits = make_logits(dist, nbuf * batch, vocab, g)
                inputs = {"logits": logits, "probs": torch.softmax(logits, dim=-1)}
                for name in args.ops.split(","):
                    kind, writes, ours, theirs = OPS[name]
                    bufs = list(inputs[kind].split(batch))
                    t, n, t_torch, n_torch = measure(ours, theirs, bufs)
                    algo = row_bytes * (2 if writes else 1)
                    line = {
                        "op": name, "batch": batch, "vocab": vocab, "dist": dist, "k": K, "p": P, "min_p": MIN_P,
                        "time_us": round(t * 1e6, 2), "repeats": n, "algorithmic_bytes": algo,
                        "rate_TBps": round(algo / t / 1e12, 3),
                        "equivalent_passes": round(t * HBM_STREAM / row_bytes, 2),
                        "torch_time_us": round(t_torch * 1e6, 2), "torch_repeats": n_torch,
                        "speedup_vs_torch": round(t_torch / t, 2), "rotating_buffers": nbuf,
                    }
                    text = json.dumps(line)
                    print(text, flush=True)
                    if out:
                        out.write(text + "\n")
                        out.flush()
                del logits, inputs
    if out:
        out.close()


if __name__ == "__main__":
    main()
