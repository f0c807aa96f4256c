"""Plan-free decode (flashinfer.decode.trtllm_batch_decode_with_kv_cache) against "host plan() + replayed run()".

Prints one JSON line per measurement (profiles/decode_device_plan_bench.jsonl keeps a run):
  planner   the two planner launches alone (fi_batch_decode_plan_device), B = 8 / 64 / 512 x 8192 tokens, page 16:
            event-timed back-to-back calls, and with max_grid_hint = 1 (the unsplit branch: no chunk search), so the
            difference is what the search costs
  step      per shape (C2 = 64 x 8192 and 8 x 1024, 32 / 8 heads, bf16, HND cache):
            device_plan   the whole call captured once and replayed
            host_plan     CUDA-graph wrapper: plan() on the host every step, then the captured run() replayed
            host_plan_eager  the plain wrapper: plan() then run() every step (what bench.py times at C2 is its run())
            gpu_us: events around the replays / run() calls alone, queue kept full; wall_us: host clock around the
            Python step (plan included where there is one), device synchronised at the end of the loop; host_us: the
            same loop without waiting for the device.
Kernel-level times (scan / fill / decode / merge) come from a separate rocprofv3 --kernel-trace --stats run of this
script with --profile, which runs each path a few times and nothing else
(tools/summarize_decode_device_plan_trace.py reads the trace)."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch

import flashinfer
from flashinfer import _lib
from flashinfer.decode import trtllm_batch_decode_with_kv_cache

DEV = torch.device("cuda:0")
HQ, HKV, D, PS = 32, 8, 128, 16


def event_us(fn, n, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def wall_us(fn, n, warmup=20):
    """(host clock per call with the device drained at the end, host clock per call until the calls return)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) / n * 1e6, (t1 - t0) / n * 1e6


def planner_only(B, kv_len, hint, n):
    max_blocks = -(-kv_len // PS)
    table = torch.randint(0, 1 << 16, (B, max_blocks), dtype=torch.int32, device=DEV)
    lens = torch.full((B,), kv_len, dtype=torch.int32, device=DEV)
    p = _lib.fi_batch_decode_plan_device_params_t(
        block_tables=table.data_ptr(), seq_lens=lens.data_ptr(), block_tables_stride=max_blocks, batch_size=B,
        max_blocks=max_blocks, page_size=PS, num_qo_heads=HQ, num_kv_heads=HKV, head_dim=D,
        q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16, max_grid_hint=hint)
    ib, fb = C.c_size_t(), C.c_size_t()
    lib = _lib.lib()
    _lib.check(lib.fi_batch_decode_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)), "workspace")
    iws = torch.empty(ib.value, dtype=torch.uint8, device=DEV)
    fws = torch.empty(max(fb.value, 16), dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes, p.float_ws, p.float_ws_bytes = iws.data_ptr(), ib.value, fws.data_ptr(), fb.value
    info, csr = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)(), (C.c_int64 * 3)()

    def call():  # on the current stream: the capture below has its own
        _lib.check(lib.fi_batch_decode_plan_device(C.byref(p), info, csr, torch.cuda.current_stream().cuda_stream),
                   "plan_device")

    eager = event_us(call, n)
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return dict(kind="planner", batch=B, kv_len=kv_len, max_grid_hint=hint, split_kv=int(info[_lib.FI_DP_SPLIT_KV]),
                padded=int(info[_lib.FI_DP_PADDED_BATCH_SIZE]), eager_gpu_us=round(eager, 2),
                graph_gpu_us=round(event_us(g.replay, n), 2))


def problem(B, kv_len):
    pages = -(-kv_len // PS)
    total = B * pages
    g = torch.Generator().manual_seed(B)
    perm = torch.randperm(total, generator=g).to(torch.int32)
    cache = torch.randn(total, 2, HKV, PS, D, device=DEV, dtype=torch.bfloat16)
    q = torch.randn(B, HQ, D, device=DEV, dtype=torch.bfloat16)
    indptr = torch.arange(B + 1, dtype=torch.int32) * pages
    last = torch.full((B,), (kv_len - 1) % PS + 1, dtype=torch.int32)
    return dict(B=B, kv_len=kv_len, pages=pages, cache=cache, q=q, indptr=indptr, indices=perm, last=last,
                table=perm.reshape(B, pages).to(DEV), lens=torch.full((B,), kv_len, dtype=torch.int32, device=DEV))


def paths(pr):
    """{name: (step with its plan, the GPU part alone)} of the three ways to run one decode step, and their outputs."""
    B = pr["B"]
    out_dev = torch.empty_like(pr["q"])
    ws_dev = torch.empty(128 << 20, dtype=torch.uint8, device=DEV)

    def device_call():
        trtllm_batch_decode_with_kv_cache(pr["q"], pr["cache"], ws_dev, pr["table"], pr["lens"], pr["kv_len"],
                                          1.0 / math.sqrt(D), 1.0, out=out_dev)

    device_call()
    torch.cuda.synchronize()
    g_dev = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_dev):
        device_call()

    gw = flashinfer.BatchDecodeWithPagedKVCacheWrapper(
        torch.zeros(128 << 20, dtype=torch.uint8, device=DEV), "HND", use_cuda_graph=True,
        paged_kv_indptr_buffer=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buffer=torch.zeros(B * pr["pages"], dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buffer=torch.zeros(B, dtype=torch.int32, device=DEV))
    out_host = torch.empty_like(pr["q"])
    indptr_d, indices_d, last_d = pr["indptr"].to(DEV), pr["indices"].to(DEV), pr["last"].to(DEV)

    def graph_plan():
        # as examples/serving_loop.py: the page table is on the device, plan() reads the indptr back
        gw.plan(indptr_d, indices_d, last_d, HQ, HKV, D, PS, q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16)

    graph_plan()
    gw.run(pr["q"], pr["cache"], out=out_host)
    torch.cuda.synchronize()
    g_host = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_host):
        gw.run(pr["q"], pr["cache"], out=out_host)

    ew = flashinfer.BatchDecodeWithPagedKVCacheWrapper(torch.zeros(128 << 20, dtype=torch.uint8, device=DEV), "HND")
    out_eager = torch.empty_like(pr["q"])

    def eager_plan():
        ew.plan(indptr_d, indices_d, last_d, HQ, HKV, D, PS, q_data_type=torch.bfloat16, kv_data_type=torch.bfloat16)

    def eager_run():
        ew.run(pr["q"], pr["cache"], out=out_eager)

    eager_plan()

    def host_step():
        graph_plan()
        g_host.replay()

    def eager_step():
        eager_plan()
        eager_run()

    return (dict(device_plan=(g_dev.replay, g_dev.replay), host_plan=(host_step, g_host.replay),
                 host_plan_eager=(eager_step, eager_run)),
            dict(device_plan=out_dev, host_plan=out_host, host_plan_eager=out_eager))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--profile", action="store_true", help="a few calls of each path only, for a kernel trace")
    args = ap.parse_args()
    n = 5 if args.profile else args.steps
    for B in (8, 64, 512):
        for hint in (0, 1):
            print(json.dumps(planner_only(B, 8192, hint, n)), flush=True)
    for B, kv_len in ((64, 8192), (8, 1024)):
        pr = problem(B, kv_len)
        steps, outs = paths(pr)
        # three rounds, the paths alternating, so that drift hits all of them alike
        gpu = {name: [] for name in steps}
        for _ in range(3):
            for name, (_, gpu_part) in steps.items():
                gpu[name].append(round(event_us(gpu_part, n), 2))
        for name, (step, _) in steps.items():
            wall, host = wall_us(step, n)
            print(json.dumps(dict(kind="step", path=name, batch=B, kv_len=kv_len, gpu_us=gpu[name],
                                  wall_us=round(wall, 2), host_us=round(host, 2))), flush=True)
        torch.cuda.synchronize()
        same = torch.equal(outs["device_plan"], outs["host_plan"])
        err = (outs["device_plan"].float() - outs["host_plan_eager"].float()).abs().max().item()
        print(json.dumps(dict(kind="check", batch=B, kv_len=kv_len, device_equals_graph_host_plan=same,
                              max_abs_diff_to_eager_host_plan=err)), flush=True)


if __name__ == "__main__":
    main()
