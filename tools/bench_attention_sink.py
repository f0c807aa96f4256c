#!/usr/bin/env python
"""Attention sinks on against off, through the wrappers: the call time of run() with ``sinks=`` and without it on the
same plan and tensors, measured with device events and alternating in one process (off, on, off, on ...: both see
the same clocks and the same neighbours).  Prints one JSON line per shape.

Shapes: the C2 decode shape of bench.py (bf16, 32 / 8 heads, head_dim 128, page 16, batch 64 x kv 8192) and GPT-OSS
like shapes (64 / 8 heads, head_dim 64, page 16, window_left 128 and -1, batch 1 / 16 / 64, kv 1024 / 8192) through
the decode wrapper, the window ones also as one-token requests through BatchAttentionWithAttentionSinkWrapper.

    python tools/bench_attention_sink.py [--rounds 20] [--inner 20] [--quick]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "flashinfer-ai_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import flashinfer  # noqa: E402

DEV = "cuda:0"


def page_table(batch, kv_len, page, g):
    per = -(-kv_len // page)
    indptr = (torch.arange(batch + 1, dtype=torch.int32) * per).to(DEV)
    indices = torch.randperm(batch * per, device=DEV, generator=g).to(torch.int32)
    last = torch.full((batch,), (kv_len - 1) % page + 1, dtype=torch.int32, device=DEV)
    return indptr, indices, last, batch * per


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner  # us per call


def compare(name, off, on, rounds, inner):
    for _ in range(3):
        off(), on()
    torch.cuda.synchronize()
    t_off, t_on = [], []
    for _ in range(rounds):
        t_off.append(timed(off, inner))
        t_on.append(timed(on, inner))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    print(json.dumps({
        "shape": name, "call_us_sinks_off": round(m_off, 2), "call_us_sinks_on": round(m_on, 2),
        "on_over_off": round(m_on / m_off, 4),
        # spread of the off series against itself: (max - min) / median over the rounds
        "off_spread": round((max(t_off) - min(t_off)) / m_off, 4),
        "on_spread": round((max(t_on) - min(t_on)) / m_on, 4), "rounds": rounds, "calls_per_round": inner}), flush=True)


def decode_shape(name, batch, kv_len, hq, hkv, d, page, window_left, rounds, inner):
    g = torch.Generator(device=DEV).manual_seed(0)
    indptr, indices, last, npages = page_table(batch, kv_len, page, g)
    cache = torch.randn(npages, 2, page, hkv, d, device=DEV, dtype=torch.bfloat16, generator=g)
    q = torch.randn(batch, hq, d, device=DEV, dtype=torch.bfloat16, generator=g)
    sinks = torch.linspace(-4.0, 6.0, hq, device=DEV)
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "NHD")
    w.plan(indptr, indices, last, hq, hkv, d, page, window_left=window_left, q_data_type=torch.bfloat16,
           kv_data_type=torch.bfloat16)
    out = torch.empty_like(q)
    compare(name, lambda: w.run(q, cache, out=out), lambda: w.run(q, cache, out=out, sinks=sinks), rounds, inner)


def sink_wrapper_shape(name, batch, kv_len, hq, hkv, d, page, window_left, rounds, inner):
    """One new token per request through BatchAttentionWithAttentionSinkWrapper (sinks on) against the plain paged
    prefill wrapper on the same plan arguments (sinks off)."""
    g = torch.Generator(device=DEV).manual_seed(0)
    indptr, indices, last, npages = page_table(batch, kv_len, page, g)
    cache = torch.randn(npages, 2, page, hkv, d, device=DEV, dtype=torch.bfloat16, generator=g)
    q = torch.randn(batch, hq, d, device=DEV, dtype=torch.bfloat16, generator=g)
    sinks = torch.linspace(-4.0, 6.0, hq, device=DEV)
    qo_indptr = torch.arange(batch + 1, dtype=torch.int32, device=DEV)
    sm_scale = 1.0 / math.sqrt(d)
    ws = lambda: torch.zeros(256 << 20, dtype=torch.uint8, device=DEV)
    w_on = flashinfer.BatchAttentionWithAttentionSinkWrapper(ws(), "NHD", head_dim_qk=d, head_dim_vo=d,
                                                             window_left=window_left)
    w_off = flashinfer.BatchPrefillWithPagedKVCacheWrapper(ws(), "NHD")
    for w in (w_on, w_off):
        w.plan(qo_indptr, indptr, indices, last, hq, hkv, d, page, causal=True, window_left=window_left,
               sm_scale=sm_scale, q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16)
    out = torch.empty_like(q)
    compare(name, lambda: w_off.run(q, cache, out=out), lambda: w_on.run(q, cache, sinks, sm_scale, out=out), rounds,
            inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the C2 shape and one GPT-OSS shape only")
    a = ap.parse_args()
    decode_shape("C2 decode bf16 32/8 d128 page16 bs64 kv8192", 64, 8192, 32, 8, 128, 16, -1, a.rounds, a.inner)
    grid = [(16, 8192, 128)] if a.quick else [(b, kv, wl) for wl in (128, -1) for b in (1, 16, 64)
                                              for kv in (1024, 8192)]
    for batch, kv_len, wl in grid:
        tag = f"64/8 d64 page16 bs{batch} kv{kv_len} window{wl}"
        decode_shape("decode " + tag, batch, kv_len, 64, 8, 64, 16, wl, a.rounds, a.inner)
    for batch, kv_len, wl in ([(16, 8192, 128)] if a.quick else [(b, kv, 128) for b in (1, 16, 64)
                                                                  for kv in (1024, 8192)]):
        tag = f"64/8 d64 page16 bs{batch} kv{kv_len} window{wl}"
        sink_wrapper_shape("sink wrapper, 1 token / request " + tag, batch, kv_len, 64, 8, 64, 16, wl, a.rounds,
                           a.inner)


if __name__ == "__main__":
    main()
