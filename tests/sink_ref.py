"""Oracle for attention sinks: the repository's attention oracle, then one merge.

A sink (ref: AttentionSink, flashinfer/jit/attention/variants.py:17-53) is a per-head logit in natural-log units that
joins the softmax denominator and has no value vector, i.e. the attention state (o, lse) merged with the state
(0, sink * log2(e)).  An empty row (o = 0, lse = -5e4) merges to (0, sink * log2(e)); sink = -inf leaves the state
as it is.  tests/test_attention_sink_cpu.py holds this to the reference's own pure-torch statement
(tests/golden/attention_sink_golden.npz)."""
import math

import torch

from oracle import attention_ref as R

LOG2E = math.log2(math.e)


def fold_sink(o: torch.Tensor, lse: torch.Tensor, sinks: torch.Tensor):
    """(o [rows, H, D], lse [rows, H]) of plain attention and sinks [H] -> the state with the sink folded in (f64)."""
    o, lse = o.double(), lse.double()
    s = (sinks.double() * LOG2E).expand_as(lse)
    off = torch.isinf(s) & (s < 0)  # a sink of -inf: merge_state_ref would form -inf - -inf on an empty row
    o2, lse2 = R.merge_state_ref(o, lse, torch.zeros_like(o), torch.where(off, lse, s))
    return torch.where(off[..., None], o, o2), torch.where(off, lse, lse2)


def attention_sink_ref(q, k, v, sinks, **kw):
    """One request: R.attention_ref(q, k, v, **kw) with the sinks folded."""
    return fold_sink(*R.attention_ref(q, k, v, **kw), sinks)


def batch_decode_sink_ref(q, cache, layout, indptr, indices, last, sinks, **kw):
    return fold_sink(*R.batch_decode_ref(q, cache, layout, indptr, indices, last, **kw), sinks)


def batch_prefill_sink_ref(q, qo_indptr, cache, layout, indptr, indices, last, sinks, **kw):
    return fold_sink(*R.batch_prefill_ref(q, qo_indptr, cache, layout, indptr, indices, last, **kw), sinks)
