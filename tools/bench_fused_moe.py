"""trtllm_fp4_block_scale_moe at a GPT-OSS-like shape, stage by stage, against the same layer written with torch ops;
with --mode fp8, trtllm_fp8_block_scale_moe at the DeepSeek-V3 shape, stage by stage (see main_fp8).

    python tools/bench_fused_moe.py [--out profiles/fused_moe_bench.jsonl] [--experts 32] [--top-k 4] [--hidden 2944]
                                    [--inter 2944] [--tokens 1,32,128,2048,8192] [--warmup 10] [--runs 30]
    python tools/bench_fused_moe.py --mode fp8 [--out profiles/fused_moe_fp8_bench.jsonl] [--experts 256] [--top-k 8]
                                    [--hidden 7168] [--inter 2048] [--tokens 1,64,1024,8192]

Per token count one JSON line with the device-event median and the run-to-run spread (quartiles, min, max) of these
candidates, timed alternately in one loop after --warmup rounds of all of them:

  quantize   mxfp8_quantize(x, False) of the bf16 activations: what the caller runs in front of the layer;
  route, permute, gemm1, act, gemm2, finalize
             the six steps of the layer, each on the outputs of the one before it (made once, untimed);
  layer      trtllm_fp4_block_scale_moe, Renormalize routing, SwiGlu with alpha and a clamp limit, no biases;
  baseline   the same layer as a user writes it without the module: torch.topk, softmax, argsort (stable), bincount and
             cumsum for the segments, index_select of the bf16 rows, mxfp8_quantize_grouped, the same two GEMM calls, the
             activation in torch (f32), mxfp8_quantize_grouped again, index_add_ of the weighted rows.

and from them: what the steps around the GEMMs cost as a share of the layer, and the speed-up of quantize + layer over
the baseline (the baseline starts from bf16 activations, so the layer is charged with its quantiser).  A sample is the
time between two events around the Python call on an idle stream.  The weights are one set of 32 experts (416 MB of
codes, more than the 256 MB Infinity Cache); the inputs rotate over 8 sets whose logits are rolled by 4 experts each,
so that at small token counts successive runs read other experts' weights.
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
from flashinfer import fp8_quantization, fused_moe, fused_moe_fp8
from flashinfer.gemm import _group_gemm_fp8_into, _group_gemm_mxfp4_into

DEV = torch.device("cuda", 0)
INPUT_SETS = 8
ALPHA, LIMIT = 1.702, 7.0


def make_weights(G, n, k, seed):
    """random MXFP4 codes and scale bytes; n is a multiple of 128 here, so the swizzled scale tensor has no padding"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    packed = torch.randint(0, 256, (G, n, k // 2), dtype=torch.uint8, device=DEV, generator=g)
    n_pad = (n + 127) // 128 * 128
    sf = torch.randint(118, 124, (G, n_pad, k // 32), dtype=torch.uint8, device=DEV, generator=g)
    return packed, sf


def make_inputs(T, E, H, seed):
    """tie-free logits (a random permutation of (j - E / 2) / 8 per row), rolled by 4 experts per set"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.stack([torch.randperm(E, device=DEV, generator=g) for _ in range(T)]).float()
    x = torch.randn(T, H, device=DEV, dtype=torch.bfloat16, generator=g)
    sets = []
    for s in range(INPUT_SETS):
        logits = ((torch.roll(base, 4 * s, dims=1) - E // 2) / 8).contiguous()
        x_s = torch.roll(x, s, dims=0).contiguous()
        q, sf = flashinfer.mxfp8_quantize(x_s, False)
        sets.append({"logits": logits, "x": x_s, "q": q, "sf": sf.view(T, H // 32)})
    return sets


def time_alternating(fns, warmup, runs):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name in fns}
    for _ in range(runs):
        for name, fn in fns.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            samples[name].append(start.elapsed_time(stop) * 1e-3)
    return samples


def summary(xs):
    t = torch.tensor(sorted(xs), dtype=torch.float64)
    q = torch.quantile(t, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)).tolist()
    return {"median_us": q[1] * 1e6, "q25_us": q[0] * 1e6, "q75_us": q[2] * 1e6, "min_us": t[0].item() * 1e6,
            "max_us": t[-1].item() * 1e6}


def make_fp8_weights(G, n, k, seed):
    """random e4m3 bytes (magnitudes up to 240, no NaN byte) and f32 scales per 128 x 128 block that are no powers of two,
    sized so that a product with unit-variance activations over k comes out of order 1"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randint(0, 0x78, (G, n, k), dtype=torch.uint8, device=DEV, generator=g)
    w |= torch.randint(0, 2, (G, n, k), dtype=torch.uint8, device=DEV, generator=g) << 7
    scale = (0.75 + 0.5 * torch.rand(G, n // 128, k // 128, device=DEV, generator=g)) / (60.0 * k ** 0.5)
    return w.view(torch.float8_e4m3fn), scale


def main_fp8(args):
    """trtllm_fp8_block_scale_moe at the DeepSeek-V3 shape (256 experts, top-8, H 7168, I 2048, DeepSeekV3 routing with 8
    groups of which 4 are kept), all experts local.  Per token count one JSON line with the device-event median and spread of

      quantize   fp8_quantize_1x128 of the bf16 activations: what the caller runs in front of the layer;
      route, permute, gemm1, act, gemm2, finalize
                 the six steps, each on the outputs of the one before it (made once, untimed); gemm1 and gemm2 are the two
                 grouped-GEMM calls alone, on the layer's own m_indptr;
      layer      the whole call;

    the share of the layer that is not the two GEMMs, and for the three kernels of this format (quantize, the permute
    call with its three sorting launches, act) the bytes they must move over their time."""
    E, K, H, I = args.experts, args.top_k, args.hidden, args.inter
    n_group, topk_group, factor = 8, 4, 2.5
    w1, w1_s = make_fp8_weights(E, 2 * I, H, 1)
    w2, w2_s = make_fp8_weights(E, H, I, 2)
    method = fused_moe.RoutingMethodType.DeepSeekV3
    out_f = open(args.out, "w") if args.out else None
    for T in (int(x) for x in args.tokens.split(",")):
        g = torch.Generator(device=DEV).manual_seed(10 + T)
        n = T * K
        bias = 0.1 * torch.randn(E, device=DEV, generator=g)
        sets = []
        for s_i in range(INPUT_SETS):
            s = {"logits": torch.randn(T, E, device=DEV, generator=g),
                 "x": torch.randn(T, H, device=DEV, dtype=torch.bfloat16, generator=g)}
            s["q"], s["scale"] = fp8_quantization.fp8_quantize_1x128(s["x"])
            s["ids"], s["w"] = fused_moe.moe_route(s["logits"], K, method, bias, n_group, topk_group, factor)
            s["m_indptr"], s["emap"], s["xp"], s["xp_s"] = fused_moe.moe_permute_fp8_block(s["ids"], s["q"], s["scale"], 0, E)
            s["y1"] = torch.empty(n, 2 * I, dtype=torch.bfloat16, device=DEV)
            _group_gemm_fp8_into(s["xp"], w1, s["xp_s"], w1_s, s["y1"], s["m_indptr"])
            s["act"], s["act_s"] = fused_moe.moe_gated_act_fp8_block(s["y1"], s["m_indptr"])
            s["y2"] = torch.empty(n, H, dtype=torch.bfloat16, device=DEV)
            _group_gemm_fp8_into(s["act"], w2, s["act_s"], w2_s, s["y2"], s["m_indptr"])
            sets.append(s)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(sets[0]["y2"].float()).all())
        turn = {}

        def pick(name):
            turn[name] = turn.get(name, 0) + 1
            return sets[turn[name] % INPUT_SETS]

        def layer():
            s = pick("layer")
            return fused_moe_fp8.trtllm_fp8_block_scale_moe(s["logits"], bias, s["q"], s["scale"], w1, w1_s, w2, w2_s, E, K, n_group,
                                                        topk_group, I, 0, E, factor, routing_method_type=method)

        fns = {
            "quantize": lambda: fp8_quantization.fp8_quantize_1x128(pick("quantize")["x"]),
            "route": lambda: fused_moe.moe_route(pick("route")["logits"], K, method, bias, n_group, topk_group, factor),
            "permute": lambda: (lambda s: fused_moe.moe_permute_fp8_block(s["ids"], s["q"], s["scale"], 0, E))(pick("permute")),
            "gemm1": lambda: (lambda s: _group_gemm_fp8_into(s["xp"], w1, s["xp_s"], w1_s, s["y1"], s["m_indptr"]))(pick("gemm1")),
            "act": lambda: (lambda s: fused_moe.moe_gated_act_fp8_block(s["y1"], s["m_indptr"]))(pick("act")),
            "gemm2": lambda: (lambda s: _group_gemm_fp8_into(s["act"], w2, s["act_s"], w2_s, s["y2"], s["m_indptr"]))(pick("gemm2")),
            "finalize": lambda: (lambda s: fused_moe.moe_finalize(s["y2"], s["w"], s["emap"]))(pick("finalize")),
            "layer": layer,
        }
        # the layer is its stages before it is timed
        turn["layer"] = 0
        s1 = sets[1]
        assert torch.equal(layer().view(torch.int16), fused_moe.moe_finalize(s1["y2"], s1["w"], s1["emap"]).view(torch.int16))
        samples = time_alternating(fns, args.warmup, args.runs)
        stats = {name: summary(xs) for name, xs in samples.items()}
        med = {name: s["median_us"] for name, s in stats.items()}
        around = med["route"] + med["permute"] + med["act"] + med["finalize"]
        steps = around + med["gemm1"] + med["gemm2"]
        # bytes each kernel of this format must move: every input read once, every output written once
        moved = {
            "quantize": T * H * 3 + T * (H // 128) * 4,
            "permute": n * H * 2 + n * (H // 128) * 8 + n * 12 + (E + 1) * 4,
            "act": n * I * 5 + n * (I // 128) * 4,
        }
        flops = {"gemm1": 2.0 * n * 2 * I * H, "gemm2": 2.0 * n * H * I}
        line = {
            "mode": "fp8", "experts": E, "top_k": K, "hidden": H, "inter": I, "tokens": T, "runs": args.runs,
            "warmup": args.warmup, "input_sets": INPUT_SETS,
            **{f"{name}_{key}": round(v, 2) for name, s in stats.items() for key, v in s.items()},
            "sum_of_steps_us": round(steps, 2),
            "gemms_alone_us": round(med["gemm1"] + med["gemm2"], 2),
            "non_gemm_share_of_steps": round(around / steps, 4),
            "non_gemm_share_of_layer": round((med["layer"] - med["gemm1"] - med["gemm2"]) / med["layer"], 4),
            **{f"{name}_gbytes_per_s": round(b / med[name] * 1e-3, 1) for name, b in moved.items()},
            **{f"{name}_tflops": round(f / med[name] * 1e-6, 1) for name, f in flops.items()},
        }
        print(json.dumps(line), flush=True)
        if out_f:
            out_f.write(json.dumps(line) + "\n")
            out_f.flush()
        del sets
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["fp4", "fp8"], default="fp4")
    ap.add_argument("--out", default=None)
    ap.add_argument("--experts", type=int, default=None)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--hidden", type=int, default=None)
    ap.add_argument("--inter", type=int, default=None)
    ap.add_argument("--tokens", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=30)
    args = ap.parse_args()
    defaults = {"fp4": (32, 4, 2944, 2944, "1,32,128,2048,8192"), "fp8": (256, 8, 7168, 2048, "1,64,1024,8192")}[args.mode]
    for name, value in zip(("experts", "top_k", "hidden", "inter", "tokens"), defaults):
        if getattr(args, name) is None:
            setattr(args, name, value)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures nothing without one")
    assert args.warmup >= 10 and args.runs >= 30, "at least 10 warm-ups and 30 timed runs"
    if args.mode == "fp8":
        return main_fp8(args)
    E, K, H, I = args.experts, args.top_k, args.hidden, args.inter
    w1, w1_sf = make_weights(E, 2 * I, H, 1)
    w2, w2_sf = make_weights(E, H, I, 2)
    alpha = torch.full((E,), ALPHA, device=DEV)
    limit = torch.full((E,), LIMIT, device=DEV)
    out_f = open(args.out, "w") if args.out else None
    for T in (int(x) for x in args.tokens.split(",")):
        sets = make_inputs(T, E, H, 10 + T)
        n = T * K
        # the inputs of every step, made once from the step before it
        for s in sets:
            s["ids"], s["w"] = fused_moe.moe_route(s["logits"], K, fused_moe.RoutingMethodType.Renormalize)
            s["m_indptr"], s["emap"], s["xp"], s["xp_sf"] = fused_moe.moe_permute_mxfp8(s["ids"], s["q"], s["sf"], 0, E)
            s["y1"] = torch.empty(n, 2 * I, dtype=torch.bfloat16, device=DEV)
            _group_gemm_mxfp4_into(s["xp"], w1, s["xp_sf"], w1_sf, s["y1"], s["m_indptr"], 2 * I, H)
            s["act"], s["act_sf"] = fused_moe.moe_gated_act_mxfp8(s["y1"], s["m_indptr"], None, alpha, None, limit)
            s["y2"] = torch.empty(n, H, dtype=torch.bfloat16, device=DEV)
            _group_gemm_mxfp4_into(s["act"], w2, s["act_sf"], w2_sf, s["y2"], s["m_indptr"], H, I)
        torch.cuda.synchronize()
        turn = {}

        def pick(name):
            turn[name] = turn.get(name, 0) + 1
            return sets[turn[name] % INPUT_SETS]

        def layer():
            s = pick("layer")
            return fused_moe.trtllm_fp4_block_scale_moe(
                s["logits"], None, s["q"], s["sf"], w1, w1_sf, None, alpha, None, limit, w2, w2_sf, None, None, None, None,
                E, K, None, None, I, 0, E, None, routing_method_type=fused_moe.RoutingMethodType.Renormalize)[0]

        def baseline():
            s = pick("baseline")
            vals, ids = torch.topk(s["logits"], K, dim=-1)
            w = torch.softmax(vals, dim=-1)
            flat = ids.reshape(-1)
            order = torch.argsort(flat, stable=True)
            m_indptr = torch.zeros(E + 1, dtype=torch.int32, device=DEV)
            m_indptr[1:] = torch.bincount(flat, minlength=E).cumsum(0)
            tok = order // K
            q, sf = fp8_quantization.mxfp8_quantize_grouped(s["x"].index_select(0, tok), m_indptr)
            y1 = torch.empty(n, 2 * I, dtype=torch.bfloat16, device=DEV)
            _group_gemm_mxfp4_into(q, w1, sf, w1_sf, y1, m_indptr, 2 * I, H)
            gate = y1[:, I:].float().clamp(max=LIMIT)
            lin = y1[:, :I].float().clamp(min=-LIMIT, max=LIMIT)
            act = (gate * torch.sigmoid(ALPHA * gate) * lin).to(torch.bfloat16)
            q2, sf2 = fp8_quantization.mxfp8_quantize_grouped(act, m_indptr)
            y2 = torch.empty(n, H, dtype=torch.bfloat16, device=DEV)
            _group_gemm_mxfp4_into(q2, w2, sf2, w2_sf, y2, m_indptr, H, I)
            out = torch.zeros(T, H, dtype=torch.float32, device=DEV)
            out.index_add_(0, tok, y2.float() * w.reshape(-1)[order].unsqueeze(1))
            return out.to(torch.bfloat16)

        def gemm1():
            s = pick("gemm1")
            _group_gemm_mxfp4_into(s["xp"], w1, s["xp_sf"], w1_sf, s["y1"], s["m_indptr"], 2 * I, H)

        def gemm2():
            s = pick("gemm2")
            _group_gemm_mxfp4_into(s["act"], w2, s["act_sf"], w2_sf, s["y2"], s["m_indptr"], H, I)

        fns = {
            "quantize": lambda: flashinfer.mxfp8_quantize(pick("quantize")["x"], False),
            "route": lambda: fused_moe.moe_route(pick("route")["logits"], K, fused_moe.RoutingMethodType.Renormalize),
            "permute": lambda: (lambda s: fused_moe.moe_permute_mxfp8(s["ids"], s["q"], s["sf"], 0, E))(pick("permute")),
            "gemm1": gemm1,
            "act": lambda: (lambda s: fused_moe.moe_gated_act_mxfp8(s["y1"], s["m_indptr"], None, alpha, None, limit))(
                pick("act")),
            "gemm2": gemm2,
            "finalize": lambda: (lambda s: fused_moe.moe_finalize(s["y2"], s["w"], s["emap"]))(pick("finalize")),
            "layer": layer,
            "baseline": baseline,
        }
        # the two ways agree before they are timed (the baseline rounds its activation to bf16 once more)
        turn["layer"] = turn["baseline"] = 0
        a, b = layer().float(), baseline().float()
        rel = ((a - b).norm() / b.norm()).item()
        assert rel < 0.05, f"layer and baseline differ: relative error {rel}"
        samples = time_alternating(fns, args.warmup, args.runs)
        stats = {name: summary(xs) for name, xs in samples.items()}
        med = {name: s["median_us"] for name, s in stats.items()}
        around = med["route"] + med["permute"] + med["act"] + med["finalize"]
        steps = around + med["gemm1"] + med["gemm2"]
        line = {
            "experts": E, "top_k": K, "hidden": H, "inter": I, "tokens": T, "runs": args.runs, "warmup": args.warmup,
            "input_sets": INPUT_SETS, "layer_vs_baseline_rel_err": round(rel, 5),
            **{f"{name}_{key}": round(v, 2) for name, s in stats.items() for key, v in s.items()},
            "sum_of_steps_us": round(steps, 2),
            "non_gemm_share_of_steps": round(around / steps, 4),
            "non_gemm_share_of_layer": round((med["layer"] - med["gemm1"] - med["gemm2"]) / med["layer"], 4),
            "permute_over_gemm1": round(med["permute"] / med["gemm1"], 4),
            "act_over_gemm2": round(med["act"] / med["gemm2"], 4),
            "speedup_layer_plus_quantize_vs_baseline": round(med["baseline"] / (med["layer"] + med["quantize"]), 3),
            "faster_than_baseline_by_more_than_the_spread":
                med["baseline"] - med["layer"] - med["quantize"] >
                max(s["q75_us"] - s["q25_us"] for s in (stats["layer"], stats["baseline"])),
        }
        print(json.dumps(line), flush=True)
        if out_f:
            out_f.write(json.dumps(line) + "\n")
            out_f.flush()
        del sets
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
