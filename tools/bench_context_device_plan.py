"""Plan-free prefill (flashinfer.prefill.trtllm_batch_context_with_kv_cache) against "host plan() + run()".

Prints one JSON line per measurement and appends it to --out (profiles/context_device_plan_bench.jsonl keeps a run):
  planner   the two planner launches alone (fi_batch_prefill_plan_device) for each shape: event-timed back-to-back
            calls, and the same captured in a graph
  step      per shape (32 / 8 heads, bf16, page 16, HND cache):
              chunked      8 requests x 512 new tokens on 4096 tokens of context
              mixed        120 x 1 row + 8 x 256 rows, kv 2k-8k
              mixed_split  56 x 1 row + 4 x 256 rows, kv 2k-8k: few enough q tiles for the split branch, where the
                           work list's order (request order here, sorted and interleaved on the host) is all that
                           differs from the host's graph plan
              small        4 x 16 rows on 1024 tokens of context
            device_plan      the whole call captured once and replayed
            host_plan        CUDA-graph wrapper: plan() on the host every step, then the captured run() replayed
            host_plan_eager  the plain wrapper: plan() then run() every step
            gpu_us: events around the replays / run() calls alone, queue kept full, three rounds with the paths
            alternating; wall_us: host clock around the Python step (plan included where there is one), device
            synchronised at the end of the loop; host_us: the same loop without waiting for the device."""
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
from flashinfer.prefill import trtllm_batch_context_with_kv_cache

DEV = torch.device("cuda:0")
HQ, HKV, D, PS = 32, 8, 128, 16
DT = torch.bfloat16


def _spread(lo, hi, n):
    return [lo + (hi - lo) * i // max(n - 1, 1) for i in range(n)]


SHAPES = {
    "chunked": ([512] * 8, [4096 + 512] * 8),
    "mixed": ([1] * 120 + [256] * 8, _spread(2048, 8192, 120) + _spread(2048, 8192, 8)),
    "mixed_split": ([1] * 56 + [256] * 4, _spread(2048, 8192, 56) + _spread(2048, 8192, 4)),
    "small": ([16] * 4, [1024 + 16] * 4),
}


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


def problem(qo_lens, kv_lens):
    B = len(qo_lens)
    pages = [-(-l // PS) for l in kv_lens]
    total, max_blocks = sum(pages), max(pages)
    perm = torch.randperm(total, generator=torch.Generator().manual_seed(B)).to(torch.int32)
    indptr = torch.tensor([0] + pages, dtype=torch.int64).cumsum(0).to(torch.int32)
    table = torch.zeros(B, max_blocks, dtype=torch.int32)
    for b in range(B):
        table[b, : pages[b]] = perm[int(indptr[b]): int(indptr[b + 1])]
    qo_indptr = torch.tensor([0] + qo_lens, dtype=torch.int64).cumsum(0).to(torch.int32)
    return dict(B=B, rows=sum(qo_lens), max_blocks=max_blocks, indptr=indptr.to(DEV), indices=perm.to(DEV),
                last=torch.tensor([(l - 1) % PS + 1 for l in kv_lens], dtype=torch.int32, device=DEV),
                qo_indptr=qo_indptr.to(DEV), table=table.to(DEV),
                lens=torch.tensor(kv_lens, dtype=torch.int32, device=DEV),
                cache=torch.randn(total, 2, HKV, PS, D, device=DEV, dtype=DT),
                q=torch.randn(sum(qo_lens), HQ, D, device=DEV, dtype=DT))


def planner_only(name, pr, n):
    p = _lib.fi_batch_prefill_plan_device_params_t(
        block_tables=pr["table"].data_ptr(), seq_lens=pr["lens"].data_ptr(), cum_seq_lens_q=pr["qo_indptr"].data_ptr(),
        block_tables_stride=pr["max_blocks"], batch_size=pr["B"], max_blocks=pr["max_blocks"], page_size=PS,
        total_num_rows=pr["rows"], num_qo_heads=HQ, num_kv_heads=HKV, head_dim=D, q_dtype=_lib.FI_DTYPE_BF16,
        kv_dtype=_lib.FI_DTYPE_BF16, window_left=-1, max_items_hint=0)
    ib, fb = C.c_size_t(), C.c_size_t()
    lib = _lib.lib()
    _lib.check(lib.fi_batch_prefill_plan_device_workspace(C.byref(p), C.byref(ib), C.byref(fb)), "workspace")
    iws = torch.empty(ib.value, dtype=torch.uint8, device=DEV)
    fws = torch.empty(max(fb.value, 16), dtype=torch.uint8, device=DEV)
    p.int_ws, p.int_ws_bytes, p.float_ws, p.float_ws_bytes = iws.data_ptr(), ib.value, fws.data_ptr(), fb.value
    info, csr = (C.c_int64 * _lib.FI_PREFILL_PLAN_INFO_LEN)(), (C.c_int64 * 4)()

    def call():  # on the current stream: the capture below has its own
        _lib.check(lib.fi_batch_prefill_plan_device(C.byref(p), info, csr, torch.cuda.current_stream().cuda_stream),
                   "plan_device")

    eager = event_us(call, n)
    call()
    torch.cuda.synchronize()
    chunk, items = iws[info[_lib.FI_PP_KV_CHUNK_SIZE_PTR_OFFSET]:][:8].view(torch.int32).tolist()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return dict(kind="planner", shape=name, batch=pr["B"], rows=pr["rows"], split_kv=int(info[_lib.FI_PP_SPLIT_KV]),
                capacity=int(info[_lib.FI_PP_PADDED_BATCH_SIZE]), kv_chunk=chunk, items=items,
                float_ws_bytes=fb.value, eager_gpu_us=round(eager, 2), graph_gpu_us=round(event_us(g.replay, n), 2))


def paths(pr):
    """{name: (step with its plan, the GPU part alone)} of the three ways to run one prefill step, and their outputs."""
    B = pr["B"]
    out_dev = torch.empty_like(pr["q"])
    ws_dev = torch.empty(256 << 20, dtype=torch.uint8, device=DEV)

    def device_call():
        trtllm_batch_context_with_kv_cache(pr["q"], pr["cache"], ws_dev, pr["table"], pr["lens"], pr["rows"],
                                           pr["max_blocks"] * PS, 1.0 / math.sqrt(D), 1.0, B, pr["qo_indptr"], None,
                                           out=out_dev)

    device_call()
    torch.cuda.synchronize()
    g_dev = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_dev):
        device_call()

    gw = flashinfer.BatchPrefillWithPagedKVCacheWrapper(
        torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "HND", use_cuda_graph=True,
        qo_indptr_buf=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indptr_buf=torch.zeros(B + 1, dtype=torch.int32, device=DEV),
        paged_kv_indices_buf=torch.zeros(len(pr["indices"]), dtype=torch.int32, device=DEV),
        paged_kv_last_page_len_buf=torch.zeros(B, dtype=torch.int32, device=DEV))
    out_host = torch.empty_like(pr["q"])
    plan_args = (pr["qo_indptr"], pr["indptr"], pr["indices"], pr["last"], HQ, HKV, D, PS)
    plan_kw = dict(causal=True, q_data_type=DT, kv_data_type=DT)

    def graph_plan():  # the page table is on the device, plan() reads the indptrs back
        gw.plan(*plan_args, **plan_kw)

    graph_plan()
    gw.run(pr["q"], pr["cache"], out=out_host)
    torch.cuda.synchronize()
    g_host = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_host):
        gw.run(pr["q"], pr["cache"], out=out_host)

    ew = flashinfer.BatchPrefillWithPagedKVCacheWrapper(torch.zeros(256 << 20, dtype=torch.uint8, device=DEV), "HND")
    out_eager = torch.empty_like(pr["q"])

    def eager_plan():
        ew.plan(*plan_args, **plan_kw)

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
            dict(device_plan=out_dev, host_plan=out_host, host_plan_eager=out_eager),
            dict(host_plan=int(gw._plan_info[_lib.FI_PP_SPLIT_KV]), host_plan_eager=int(ew._plan_info[_lib.FI_PP_SPLIT_KV])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_device_plan_bench.jsonl"))
    args = ap.parse_args()
    n = args.steps
    sink = open(args.out, "a")

    def emit(**rec):
        line = json.dumps(rec)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    for name in args.shapes.split(","):
        pr = problem(*SHAPES[name])
        emit(**planner_only(name, pr, n))
        steps, outs, host_split = paths(pr)
        # three rounds, the paths alternating, so that drift hits all of them alike
        gpu = {path: [] for path in steps}
        for _ in range(3):
            for path, (_, gpu_part) in steps.items():
                gpu[path].append(round(event_us(gpu_part, n), 2))
        for path, (step, _) in steps.items():
            wall, host = wall_us(step, n)
            split = {"split_kv": host_split[path]} if path in host_split else {}  # the device plan's: its planner line
            emit(kind="step", shape=name, path=path, batch=pr["B"], rows=pr["rows"], gpu_us=gpu[path],
                 wall_us=round(wall, 2), host_us=round(host, 2), **split)
        torch.cuda.synchronize()
        same = torch.equal(outs["device_plan"], outs["host_plan"])
        err = (outs["device_plan"].float() - outs["host_plan_eager"].float()).abs().max().item()
        emit(kind="check", shape=name, device_equals_graph_host_plan=same, max_abs_diff_to_eager_host_plan=err)
        del pr, steps, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
