"""CPU: what flashinfer.SegmentGEMMWrapper.run refuses, each before it asks for a GPU tensor."""
import pytest
import torch

import flashinfer

F16, BF16 = torch.float16, torch.bfloat16


def _call(x=(10, 16), w=(4, 24, 16), column_major=True, dtype=F16, w_dtype=None, out=None, batch=4, workspace=1 << 20,
          workspace_device="cpu", **kw):
    """A valid call on CPU tensors (10 rows, d_in 16, d_out 24, 4 segments) with the named pieces replaced."""
    wrapper = flashinfer.SegmentGEMMWrapper(torch.empty(16, dtype=torch.int8))
    wrapper.reset_workspace_buffer(torch.empty(16, dtype=torch.int8),
                                   torch.empty(workspace, dtype=torch.int8, device=workspace_device))
    weights = torch.zeros(w).to(w_dtype or dtype) if isinstance(w, tuple) else w
    if not any(k in kw for k in ("seg_lens", "seg_indptr")):
        kw["seg_lens"] = torch.tensor([1, 2, 3, 4])
    return wrapper.run(torch.zeros(x).to(dtype), weights, batch, column_major, out=out, **kw)


REFUSALS = {
    "no_cpu_fallback": (RuntimeError, {}),
    "no_segments": (ValueError, dict(seg_lens=None, seg_indptr=None)),
    "out_shape": (ValueError, dict(out=torch.zeros(10, 16, dtype=F16))),
    "out_shape_row_major": (ValueError, dict(w=(4, 16, 24), column_major=False, out=torch.zeros(10, 16, dtype=F16))),
    "weights_dtype": (ValueError, dict(w_dtype=BF16)),
    "out_dtype": (ValueError, dict(out=torch.zeros(10, 24, dtype=BF16))),
    "d_in_not_8": (ValueError, dict(x=(10, 12), w=(4, 24, 12))),
    "d_out_not_8": (ValueError, dict(w=(4, 20, 16))),
    "weights_not_contiguous": (ValueError, dict(w=torch.zeros(4, 16, 24, dtype=F16).transpose(1, 2))),
    "seg_lens_length": (ValueError, dict(seg_lens=torch.tensor([1, 2, 3, 4, 0]))),
    "seg_indptr_length": (ValueError, dict(seg_indptr=torch.tensor([0, 1, 3, 6]))),
    "weight_indices_length": (ValueError, dict(weight_indices=torch.tensor([0, 1, 2]))),
    "workspace_too_small": (ValueError, dict(workspace=16 + 16 * 4 - 1)),
    "workspace_on_another_device": (ValueError, dict(workspace_device="meta")),
    "fp8": (NotImplementedError, dict(dtype=torch.float8_e4m3fn)),
    "f32": (NotImplementedError, dict(dtype=torch.float32)),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_run_refuses(case):
    """The first entry is the unchanged call: it gets as far as the GPU requirement, so every other refusal is the work
    of the one piece its case replaces."""
    error, changes = REFUSALS[case]
    with pytest.raises(error):
        _call(**changes)


def test_wrapper_is_exported():
    assert flashinfer.SegmentGEMMWrapper is flashinfer.gemm.SegmentGEMMWrapper
    assert flashinfer.SegmentGEMMWrapper.forward is flashinfer.SegmentGEMMWrapper.run
