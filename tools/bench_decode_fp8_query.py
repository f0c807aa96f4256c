"""A decode step over an fp8 (e4m3) paged KV cache timed two ways on one cache:

  fp8q    an e4m3 query on the fp8-native kernel (decode_fp8_kernel.h: fp8 MFMAs, K straight from the cache, bf16 out)
  upcast  what a caller without it does: the query upcast to bf16 (timed with the step) and the 16-bit-query kernel,
          which converts every K / V byte to bf16 on the vector ALU while staging

Shapes: C2 (64 requests x 8192 keys) and 8 x 1024; 32 / 8 heads, head_dim 128, page 16, shuffled pages.  Times are medians
of device-event-timed STEPS, not kernel times: a step is every launch of one run() (decode and merge of a split plan;
the upcast route's conversion launch too), so at the small shape it is largely launch and enqueue cost.  The two routes
alternate inside every round so that drift hits them alike; TB/s is on
the algorithmic bytes of DESIGN.md section 3.1 with the cache's element size, 2 L Hkv D + 2 Hq D bytes per request.  The
routes are compared on their outputs first.  One JSON line per shape.

    python tools/bench_decode_fp8_query.py [--rounds 50]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))

import torch

import flashinfer
from flashinfer import _lib

DEV = torch.device("cuda:0")
E4M3 = torch.float8_e4m3fn


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_fp8_query: no GPU; nothing is measured without one")
    hq, hkv, d, ps = 32, 8, 128, 16
    for b, L in ((64, 8192), (8, 1024)):
        g = torch.Generator(device=DEV).manual_seed(0)
        npages = b * L // ps
        cache = torch.randn(npages, 2, ps, hkv, d, device=DEV, dtype=torch.bfloat16, generator=g).to(E4M3)
        indptr = (torch.arange(b + 1, dtype=torch.int32) * (L // ps)).to(DEV)
        indices = torch.randperm(npages, device=DEV, generator=g).to(torch.int32)
        last = torch.full((b,), ps, dtype=torch.int32, device=DEV)
        q8 = torch.randn(b, hq, d, device=DEV, generator=g).to(E4M3)
        wrappers = {}
        for name, q_dt in (("fp8q", E4M3), ("upcast", torch.bfloat16)):
            w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "NHD")
            w.plan(indptr, indices, last, hq, hkv, d, ps, q_data_type=q_dt, kv_data_type=E4M3)
            wrappers[name] = w
        o8 = torch.empty(b, hq, d, device=DEV, dtype=torch.bfloat16)
        o16 = torch.empty_like(o8)
        routes = {"fp8q": lambda: wrappers["fp8q"].run(q8, cache, out=o8),
                  "upcast": lambda: wrappers["upcast"].run(q8.to(torch.bfloat16), cache, out=o16)}
        for fn in routes.values():  # warm-up: code objects, the wrappers' cached argument blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        max_diff = (o8.float() - o16.float()).abs().max().item()
        events = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                events[k].append(timed(fn))
        torch.cuda.synchronize()
        nbytes = b * (2 * L * hkv * d + 2 * hq * d)
        res = {"batch": b, "kv_len": L, "heads": f"{hq}/{hkv}", "head_dim": d, "page": ps, "kv_dtype": "e4m3",
               "rounds": a.rounds, "algorithmic_bytes": nbytes, "max_abs_diff_fp8q_vs_upcast": max_diff,
               "split_kv": {k: int(w._plan_info[_lib.FI_DP_SPLIT_KV]) for k, w in wrappers.items()}}
        for k, ev in events.items():
            ts = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
            res[k + "_us_median"] = round(ts[len(ts) // 2], 1)
            res[k + "_us_min"] = round(ts[0], 1)
            res[k + "_tbps"] = round(nbytes / ts[len(ts) // 2] / 1e6, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
