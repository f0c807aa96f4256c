#!/usr/bin/env python
"""Writes tests/golden/attention_sink_golden.npz: inputs and outputs of the reference's pure-torch statement of
attention with sinks, ``sink_attention_unified`` (tests/test_helpers/sink_attention_reference.py of a FlashInfer
checkout), in float32 on the CPU.

    python tools/make_attention_sink_golden.py /path/to/flashinfer-checkout

The helper is loaded from the checkout by path (it needs torch and einops, nothing compiled) and is run here, at
generation time, only: the tests read the arrays.  Cases: the helper's four modes (incremental, prefill, chunk,
varlen) x causal on / off x window_left -1 / 16, at 8 / 2 heads with head_dim 64 and 4 / 4 heads with head_dim 128;
sinks per head are linspace(-4, 6).  Inputs are drawn once per shape, rounded to float16 values and stored as float16
(the helper sees them as float32), and every mode reads its rows from them, which keeps the file small:
  <shape>_q [18, Hq, D], <shape>_k / _v [2, 20, Hkv, D] (two requests of 20 keys), <shape>_sink [Hq]
  incremental  q rows 0..1, one per request, over all 20 keys of each
  prefill      the 18 q rows over the first 18 keys of request 0
  chunk        q rows 0..1 over the 20 keys of request 0
  varlen       q rows 0 | 1..3 over the first 18 keys of request 0 | the 20 keys of request 1
The outputs are the helper's float32 for each (causal, window_left), <mode>_<shape>_o_c<causal>_w<window>; of prefill
mode the rows PREFILL_ROWS only (the first, the middle, and the last two, where window_left = 16 masks keys).  The file
holds arrays only.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "attention_sink_golden.npz")

SHAPES = {"h8x2d64": (8, 2, 64), "h4x4d128": (4, 4, 128)}
Q_ROWS, KV_REQUESTS, KV_LEN = 18, 2, 20  # kv_len > 17 so that window_left = 16 masks something
PREFILL_LEN = 18
PREFILL_ROWS = (0, 1, 9, 16, 17)
VARLEN_QO, VARLEN_KV = (1, 3), (18, 20)
CAUSAL = (False, True)
WINDOWS = (-1, 16)


def load_helper(checkout: str):
    path = os.path.join(checkout, "tests", "test_helpers", "sink_attention_reference.py")
    spec = importlib.util.spec_from_file_location("sink_attention_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.sink_attention_unified


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    unified = load_helper(sys.argv[1])
    g = torch.Generator().manual_seed(20250)
    rnd = lambda *shape: torch.randn(*shape, generator=g).half().float()
    arrays = {}
    for sname, (hq, hkv, d) in SHAPES.items():
        sink = torch.linspace(-4.0, 6.0, hq)
        sm_scale = 1.0 / d ** 0.5
        q, k, v = rnd(Q_ROWS, hq, d), rnd(KV_REQUESTS, KV_LEN, hkv, d), rnd(KV_REQUESTS, KV_LEN, hkv, d)
        arrays[sname + "_q"], arrays[sname + "_k"], arrays[sname + "_v"] = (t.half().numpy() for t in (q, k, v))
        arrays[sname + "_sink"] = sink.numpy()
        varlen_kv = lambda x: torch.cat([x[0, :VARLEN_KV[0]], x[1, :VARLEN_KV[1]]])
        indptr = lambda lens: torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
        # per mode: (q, k, v, keywords of the helper, output rows kept)
        cases = {
            "incremental": (q[:KV_REQUESTS], k, v, {}, None),
            "prefill": (q[:PREFILL_LEN], k[0, :PREFILL_LEN], v[0, :PREFILL_LEN], dict(batch_size=1),
                        list(PREFILL_ROWS)),
            "chunk": (q[:2], k[0], v[0], dict(batch_size=1), None),
            "varlen": (q[:sum(VARLEN_QO)], varlen_kv(k), varlen_kv(v),
                       dict(qo_indptr=indptr(VARLEN_QO), kv_indptr=indptr(VARLEN_KV)), None),
        }
        for mode, (mq, mk, mv, kw, rows) in cases.items():
            for causal in CAUSAL:
                for window in WINDOWS:
                    o = unified(mq.contiguous(), mk.contiguous(), mv.contiguous(), sink, window, causal, sm_scale,
                                mode=mode, **kw)
                    assert o.dtype == torch.float32 and bool(torch.isfinite(o).all())
                    arrays[f"{mode}_{sname}_o_c{int(causal)}_w{window}"] = (o if rows is None else o[rows]).numpy()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
