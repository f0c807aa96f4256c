#!/usr/bin/env python3
"""One decode step of a pre-norm transformer layer (Qwen3 style: QK-norm, gated SiLU MLP) on a paged KV cache,
written with the public flashinfer API only:

    fused_add_rmsnorm -> q/k/v projection -> head-form rmsnorm on q and k -> RoPE + cache append -> batch decode
    -> output projection -> fused_add_rmsnorm -> gate/up projection -> silu_and_mul -> down projection

    PYTHONPATH=flashinfer-ai_amd python examples/decoder_layer.py

The projections are plain torch matmuls; everything between them is one flashinfer call.  Weights are random: the
point is the data flow, and which tensor each call reads and writes in place.
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))

import torch  # noqa: E402

import flashinfer  # noqa: E402

EPS = 1e-6


def make_weights(hidden, hq, hkv, d, inter, dtype, dev):
    def mat(k, n):
        return (torch.randn(k, n, device=dev) / k ** 0.5).to(dtype)

    def gain(n):
        return (1.0 + 0.1 * torch.randn(n, device=dev)).to(dtype)

    return SimpleNamespace(
        input_norm=gain(hidden), post_norm=gain(hidden), q_norm=gain(d), k_norm=gain(d),
        wqkv=mat(hidden, (hq + 2 * hkv) * d), wo=mat(hq * d, hidden), w_gate_up=mat(hidden, 2 * inter),
        w_down=mat(inter, hidden), hq=hq, hkv=hkv, d=d)


def decoder_layer(x, residual, w, cache, indptr, indices, last, batch_indices, positions, decode, record=None):
    """One layer step for one new token per request.  ``x`` [batch, hidden] is the previous layer's output and
    ``residual`` the running residual stream; both are updated in place by the two fused norms.  ``decode`` is a
    planned BatchDecodeWithPagedKVCacheWrapper.  Returns (the MLP output, the residual): the next layer's inputs.
    ``record``, if given, is a list that receives (stage, inputs, outputs) with copies of every stage's tensors."""
    def note(stage, inputs, outputs):
        if record is not None:
            record.append((stage, [t.clone() for t in inputs], [t.clone() for t in outputs]))

    hq, hkv, d = w.hq, w.hkv, w.d
    b = x.shape[0]

    before = (x.clone(), residual.clone()) if record is not None else ()
    flashinfer.fused_add_rmsnorm(x, residual, w.input_norm, EPS)  # residual += x; x = norm(residual)
    note("input_norm", before, (x, residual))

    qkv = (x @ w.wqkv).view(b, hq + 2 * hkv, d)
    q, k, v = qkv[:, :hq], qkv[:, hq:hq + hkv], qkv[:, hq + hkv:]  # strided views: nothing is copied
    qn = flashinfer.rmsnorm(q, w.q_norm, EPS)  # 3-D input: one norm per (token, head)
    kn = flashinfer.rmsnorm(k, w.k_norm, EPS)
    note("q_norm", (q,), (qn,))
    note("k_norm", (k,), (kn,))

    # rotate q and k at the token's position; k and v go straight into their page
    qr = flashinfer.apply_rope_append_paged_kv_cache(qn, kn, v, batch_indices, positions, cache, indices, indptr, last)
    o = decode.run(qr, cache)
    note("attention", (qr,), (o,))

    x = o.view(b, hq * d) @ w.wo
    before = (x.clone(), residual.clone()) if record is not None else ()
    flashinfer.fused_add_rmsnorm(x, residual, w.post_norm, EPS)
    note("post_norm", before, (x, residual))

    gate_up = x @ w.w_gate_up
    h = flashinfer.silu_and_mul(gate_up)
    note("silu_and_mul", (gate_up,), (h,))
    return h @ w.w_down, residual


def main(batch=8, context=333, hidden=512, hq=8, hkv=2, d=128, inter=1024, page_size=16, dtype=torch.bfloat16,
         record=None):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    # every request has `context` tokens in the cache and appends one more
    lens = [context + 1 + i for i in range(batch)]
    n_pages = [(l + page_size - 1) // page_size for l in lens]
    indptr = torch.tensor([0] + list(torch.tensor(n_pages).cumsum(0)), dtype=torch.int32, device=dev)
    indices = torch.randperm(sum(n_pages), device=dev).to(torch.int32)
    last = torch.tensor([(l - 1) % page_size + 1 for l in lens], dtype=torch.int32, device=dev)
    cache = torch.randn(sum(n_pages), 2, page_size, hkv, d, device=dev).to(dtype)
    one_each = torch.arange(batch + 1, dtype=torch.int32, device=dev)
    batch_indices, positions = flashinfer.get_batch_indices_positions(
        one_each, flashinfer.get_seq_lens(indptr, last, page_size), batch)

    ws = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
    decode = flashinfer.BatchDecodeWithPagedKVCacheWrapper(ws, "NHD")
    decode.plan(indptr, indices, last, hq, hkv, d, page_size, q_data_type=dtype, kv_data_type=dtype)

    w = make_weights(hidden, hq, hkv, d, inter, dtype, dev)
    x = torch.randn(batch, hidden, device=dev).to(dtype)
    residual = torch.randn(batch, hidden, device=dev).to(dtype)
    out, residual = decoder_layer(x, residual, w, cache, indptr, indices, last, batch_indices, positions, decode,
                                  record)
    torch.cuda.synchronize()
    print("layer  :", tuple(out.shape), "finite:", bool(torch.isfinite(out.float()).all()),
          "residual finite:", bool(torch.isfinite(residual.float()).all()))
    return SimpleNamespace(out=out, residual=residual, weights=w, cache=cache, indptr=indptr, indices=indices,
                           last=last)


if __name__ == "__main__":
    main()
