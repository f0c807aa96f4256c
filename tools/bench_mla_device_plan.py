"""Plan-free MLA decode (flashinfer.decode.trtllm_batch_decode_with_kv_cache_mla) against "host plan() + replayed
run()" of BatchMLAPagedAttentionWrapper.

Prints one JSON line per measurement (profiles/mla_device_plan_bench.jsonl keeps a run):
  planner   the two planner launches alone (fi_batch_mla_plan_device), B = 8 / 64 / 512 x 8192 tokens, page 64, 16 and
            128 heads, one query token: event-timed back-to-back calls, eager and as a replayed graph
  step      per shape (64 x 8192 and 8 x 1024 tokens; 16 and 128 heads; q_len 1 and 2; bf16, page 64):
            device_plan   the whole call captured once and replayed
            host_plan     the graph wrapper: plan() on the host every step, then the captured run() replayed
            gpu_us: events around the replays alone, queue kept full, three rounds with the paths alternating;
            wall_us: host clock around the Python step (plan included where there is one), device synchronised at the
            end of the loop; host_us: the same loop without waiting for the device.
  check     the two paths' outputs compared bit for bit (the same work list through the same kernel)
Kernel-level times (scan / fill / attention / merge) are not taken here: they need a kernel trace of a --profile run,
which runs each path a few times and nothing else."""
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

from flashinfer import _lib
from flashinfer.decode import trtllm_batch_decode_with_kv_cache_mla
from flashinfer.mla import BatchMLAPagedAttentionWrapper

DEV = torch.device("cuda:0")
CKV, KPE, PS = 512, 64, 64
SM = 1.0 / math.sqrt(128 + 64)
DTYPE = torch.bfloat16
WS_BYTES = 128 << 20


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


def planner_only(B, kv_len, H, n):
    max_blocks = -(-kv_len // PS)
    table = torch.randint(0, 1 << 16, (B, max_blocks), dtype=torch.int32, device=DEV)
    lens = torch.full((B,), kv_len, dtype=torch.int32, device=DEV)
    p = _lib.fi_batch_mla_plan_device_params_t(
        block_tables=table.data_ptr(), seq_lens=lens.data_ptr(), block_tables_stride=max_blocks, batch_size=B,
        max_blocks=max_blocks, page_size=PS, num_heads=H, q_len_per_request=1, head_dim_ckv=CKV, head_dim_kpe=KPE,
        q_dtype=_lib.FI_DTYPE_BF16, kv_dtype=_lib.FI_DTYPE_BF16, max_items_hint=0)
    ib, fb = C.c_size_t(), C.c_size_t()
    lib = _lib.lib()
    _lib.check(lib.fi_batch_mla_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)), "workspace")
    iws = torch.empty(ib.value, dtype=torch.uint8, device=DEV)
    fws = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes, p.float_ws, p.float_ws_bytes = iws.data_ptr(), ib.value, fws.data_ptr(), WS_BYTES
    info = (C.c_int64 * _lib.FI_MLA_PLAN_INFO_LEN)()

    def call():  # on the current stream: the capture below has its own
        _lib.check(lib.fi_batch_mla_plan_device(C.byref(p), info, torch.cuda.current_stream().cuda_stream),
                   "plan_device")

    eager = event_us(call, n)
    call()
    torch.cuda.synchronize()
    header = iws[:16].view(torch.int32).tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return dict(kind="planner", batch=B, kv_len=kv_len, num_heads=H, num_work=header[1], split_kv=header[3],
                eager_gpu_us=round(eager, 2), graph_gpu_us=round(event_us(g.replay, n), 2))


def problem(B, kv_len, H, q_len):
    pages = -(-kv_len // PS)
    total = B * pages
    perm = torch.randperm(total, generator=torch.Generator().manual_seed(B)).to(torch.int32)
    cache = torch.randn(total, 1, PS, CKV + KPE, device=DEV, dtype=DTYPE) * 0.5
    q = torch.randn(B, q_len, H, CKV + KPE, device=DEV, dtype=DTYPE)
    return dict(B=B, kv_len=kv_len, H=H, q_len=q_len, pages=pages, cache=cache, q=q, indices=perm.to(DEV),
                kv_indptr=(torch.arange(B + 1, dtype=torch.int32) * pages).to(DEV),
                qo_indptr=(torch.arange(B + 1, dtype=torch.int32) * q_len).to(DEV),
                table=perm.reshape(B, pages).to(DEV), lens=torch.full((B,), kv_len, dtype=torch.int32, device=DEV))


def paths(pr):
    """{name: (step with its plan, the GPU part alone)} of the two ways to run one MLA decode step, and their outputs."""
    B, H, q_len = pr["B"], pr["H"], pr["q_len"]
    out_dev = torch.empty(B, q_len, H, CKV, dtype=DTYPE, device=DEV)
    ws_dev = torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV)

    def device_call():
        trtllm_batch_decode_with_kv_cache_mla(pr["q"], pr["cache"], ws_dev, 128, CKV, KPE, pr["table"], pr["lens"],
                                              pr["kv_len"], out=out_dev, bmm1_scale=SM)

    device_call()
    torch.cuda.synchronize()
    g_dev = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_dev):
        device_call()

    gw = BatchMLAPagedAttentionWrapper(
        torch.empty(WS_BYTES, dtype=torch.uint8, device=DEV), True, torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        torch.zeros(B + 1, dtype=torch.int32, device=DEV), torch.zeros(B * pr["pages"], dtype=torch.int32, device=DEV),
        torch.zeros(B, dtype=torch.int32, device=DEV))
    out_host = torch.empty(B * q_len, H, CKV, dtype=DTYPE, device=DEV)
    q = pr["q"].view(B * q_len, H, CKV + KPE)
    q_nope, q_pe = q[..., :CKV], q[..., CKV:]
    cache = pr["cache"].squeeze(1)
    ckv, kpe = cache[..., :CKV], cache[..., CKV:]

    def graph_plan():  # the page table is on the device, plan() reads the indptrs and the lengths back
        gw.plan(pr["qo_indptr"], pr["kv_indptr"], pr["indices"], pr["lens"], H, CKV, KPE, PS, True, SM, DTYPE, DTYPE)

    graph_plan()
    gw.run(q_nope, q_pe, ckv, kpe, out=out_host)
    torch.cuda.synchronize()
    g_host = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_host):
        gw.run(q_nope, q_pe, ckv, kpe, out=out_host)

    def host_step():
        graph_plan()
        g_host.replay()

    return (dict(device_plan=(g_dev.replay, g_dev.replay), host_plan=(host_step, g_host.replay)),
            dict(device_plan=out_dev.view(B * q_len, H, CKV), host_plan=out_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--profile", action="store_true", help="a few calls of each path only, for a kernel trace")
    args = ap.parse_args()
    n = 5 if args.profile else args.steps
    for B in (8, 64, 512):
        for H in (16, 128):
            # ~10 us a call: many more calls than a step gets, for a window the clock can resolve
            print(json.dumps(planner_only(B, 8192, H, 20 * n)), flush=True)
    for B, kv_len in ((64, 8192), (8, 1024)):
        for H in (16, 128):
            for q_len in (1, 2):
                pr = problem(B, kv_len, H, q_len)
                steps, outs = paths(pr)
                # three rounds, the paths alternating, so that drift hits both alike
                gpu = {name: [] for name in steps}
                for _ in range(3):
                    for name, (_, gpu_part) in steps.items():
                        gpu[name].append(round(event_us(gpu_part, n), 2))
                shape = dict(batch=B, kv_len=kv_len, num_heads=H, q_len=q_len)
                for name, (step, _) in steps.items():
                    wall, host = wall_us(step, n)
                    print(json.dumps(dict(kind="step", path=name, **shape, gpu_us=gpu[name], wall_us=round(wall, 2),
                                          host_us=round(host, 2))), flush=True)
                torch.cuda.synchronize()
                print(json.dumps(dict(kind="check", **shape, device_equals_graph_host_plan=torch.equal(
                    outs["device_plan"], outs["host_plan"]))), flush=True)
                del pr, steps, outs


if __name__ == "__main__":
    main()
