"""A speculative-verify step (T query tokens per request against a long paged KV cache) timed three ways on one cache:

  multi    BatchDecodeWithPagedKVCacheWrapper.run(q, cache, q_len_per_req=T)   (decode_mfma16_kernel, MULTI form)
  prefill  BatchPrefillWithPagedKVCacheWrapper, causal, qo_len = T             (the only route before q_len_per_req)
  decode1  the one-token decode step on the same cache                         (the floor: the KV stream alone)

bf16, 32 / 8 heads, head_dim 128, page 16, batch 64, 8192 keys per request; T in 2, 4, 8.  Times are medians of
device-event-timed calls, the three routes alternating inside every round so that drift hits them alike; the two
multi-token routes are compared on their outputs first.  One JSON line per T.

    python tools/bench_decode_multi_token.py [--rounds 30] [--batch 64] [--kv-len 8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))

import torch

import flashinfer

DEV = torch.device("cuda:0")


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--kv-len", type=int, default=8192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode_multi_token: no GPU; nothing is measured without one")
    b, L, hq, hkv, d, ps, dt = a.batch, a.kv_len, 32, 8, 128, 16, torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(0)
    npages = b * L // ps
    cache = torch.randn(npages, 2, ps, hkv, d, device=DEV, dtype=dt, generator=g)
    indptr = (torch.arange(b + 1, dtype=torch.int32) * (L // ps)).to(DEV)
    indices = torch.randperm(npages, device=DEV, generator=g).to(torch.int32)
    last = torch.full((b,), ps, dtype=torch.int32, device=DEV)
    dec = flashinfer.BatchDecodeWithPagedKVCacheWrapper(torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "NHD")
    dec.plan(indptr, indices, last, hq, hkv, d, ps, q_data_type=dt, kv_data_type=dt)
    q1 = torch.randn(b, hq, d, device=DEV, dtype=dt, generator=g)
    o1 = torch.empty_like(q1)
    for T in (2, 4, 8):
        q = torch.randn(b * T, hq, d, device=DEV, dtype=dt, generator=g)
        pre = flashinfer.BatchPrefillWithPagedKVCacheWrapper(
            torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "NHD")
        pre.plan((torch.arange(b + 1, dtype=torch.int32) * T).to(DEV), indptr, indices, last, hq, hkv, d, ps,
                 causal=True, q_data_type=dt, kv_data_type=dt)
        om, op = torch.empty_like(q), torch.empty_like(q)
        routes = {"multi": lambda: dec.run(q, cache, out=om, q_len_per_req=T),
                  "prefill": lambda: pre.run(q, cache, out=op),
                  "decode1": lambda: dec.run(q1, cache, out=o1)}
        for fn in routes.values():  # warm-up: code objects, the wrappers' cached argument blocks
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        max_diff = (om.float() - op.float()).abs().max().item()
        events = {k: [] for k in routes}
        for _ in range(a.rounds):
            for k, fn in routes.items():
                events[k].append(timed(fn))
        torch.cuda.synchronize()
        res = {"T": T, "batch": b, "kv_len": L, "heads": f"{hq}/{hkv}", "head_dim": d, "page": ps, "dtype": "bf16",
               "rounds": a.rounds, "max_abs_diff_multi_vs_prefill": max_diff}
        for k, ev in events.items():
            ts = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
            res[k + "_us_median"] = round(ts[len(ts) // 2], 1)
            res[k + "_us_min"] = round(ts[0], 1)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
