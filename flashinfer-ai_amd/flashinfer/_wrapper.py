"""What the batch attention wrappers (decode, paged prefill, ragged prefill, MLA) share: the workspaces, the binding
of a plan's index tensors (CUDA-graph buffers or fresh device copies), and the per-run options."""
from __future__ import annotations

import functools
from typing import Any, List, Optional, Sequence

import torch

from . import _lib


def is_attention_sink_variant(jit_args: Optional[Sequence[Any]]) -> bool:
    """True for the reference's jit_args list of the attention-sink variant (entry 11, the variant name, is
    ``"AttentionSink"``: flashinfer/attention.py:241-255); the CUDA declaration in entry 12 is ignored, the kernels
    here being built ahead of time."""
    return jit_args is not None and len(jit_args) > 11 and jit_args[11] == "AttentionSink"


def refuses_sinks(run):
    """For the run() of a wrapper whose kernels have no attention-sink term (MLA): ``sinks=`` is answered with a
    ValueError that says so.  The method keeps the reference's signature, which has no such parameter."""
    @functools.wraps(run)
    def run_without_sinks(self, *args, **kwargs):
        if kwargs.pop("sinks", None) is not None:
            raise ValueError(f"{type(self).__name__} does not support attention sinks")
        return run(self, *args, **kwargs)
    return run_without_sinks


class BatchAttentionWrapper:
    """Base of the plan() / run() wrappers.  ``_plan_info`` is the ctypes array the C plan call filled (None before
    the first plan()); the index tensors of a plan live in attributes named ``_<name>_buf``."""

    def __init__(self, float_workspace_buffer: torch.Tensor, use_cuda_graph: bool, backend: str,
                 backends: Sequence[str], jit_args: Optional[List[Any]] = None,
                 int_workspace_bytes: int = 8 * 1024 * 1024, sink_variant: bool = False) -> None:
        # sink_variant: the wrapper takes the reference's "AttentionSink" jit_args (the prefill wrappers); its run()
        # is then run(q, <kv>, sink, sm_scale), as the reference's generated module is called
        self._sink_variant = sink_variant and is_attention_sink_variant(jit_args)
        if jit_args is not None and not self._sink_variant:
            raise ValueError("jit_args is not supported: kernels are built ahead of time")
        if backend not in backends:
            raise ValueError(f"backend {backend!r} is not available on MI355X (use 'auto')")
        _lib.require_gpu_tensor(float_workspace_buffer, "float_workspace_buffer")
        self.device = float_workspace_buffer.device
        self.reset_workspace_buffer(
            float_workspace_buffer, torch.empty((int_workspace_bytes,), dtype=torch.uint8, device=self.device))
        self._use_cuda_graph = use_cuda_graph
        self._fixed_batch_size = 0  # set by the subclass in CUDA-graph mode
        self._backend = backend
        self._plan_info = None

    @property
    def is_cuda_graph_enabled(self) -> bool:
        return self._use_cuda_graph

    def reset_workspace_buffer(
        self, float_workspace_buffer: torch.Tensor, int_workspace_buffer: torch.Tensor
    ) -> None:
        r"""Swap the workspaces; a new pinned mirror of the int workspace is allocated."""
        self._float_workspace_buffer = float_workspace_buffer
        self._int_workspace_buffer = int_workspace_buffer
        self._pin_memory_int_workspace_buffer = torch.empty(
            int_workspace_buffer.shape, dtype=int_workspace_buffer.dtype, device="cpu", pin_memory=True
        )
        # (pointer, bytes) of the float and of the int workspace: the leading arguments of the C run calls
        self._workspace_args = (float_workspace_buffer.data_ptr(), _lib.nbytes(float_workspace_buffer),
                                int_workspace_buffer.data_ptr(), _lib.nbytes(int_workspace_buffer))

    def _bind_index_tensors(self, batch_size: int, non_blocking: bool, prefix: Sequence[str] = (),
                            adopt: bool = False, **tensors: torch.Tensor) -> None:
        """Bind the int32 index tensors of a plan, given as ``name=tensor`` for the attribute ``_<name>_buf``.
        In CUDA-graph mode the batch size is the constructor's and each tensor is copied into the user's buffer: whole,
        or as a prefix for the names in ``prefix``, which must fit.  Otherwise each is moved to the wrapper's device.
        ``adopt`` (fast_decode_plan) skips the graph copies, the caller having written the buffers in place, and
        outside graph mode takes the given tensors as they are."""
        for name, t in tensors.items():
            if t.dtype != torch.int32:
                raise ValueError(f"{name} must have dtype torch.int32, got {t.dtype}")
        if not self._use_cuda_graph:
            for name, t in tensors.items():
                setattr(self, f"_{name}_buf", t if adopt else t.to(self.device, non_blocking=non_blocking))
            return
        if batch_size != self._fixed_batch_size:
            raise ValueError(
                "The batch size should be fixed in cudagraph mode, the runtime batch size {} "
                " mismatches the batch size set during initialization {}".format(batch_size, self._fixed_batch_size)
            )
        for name in prefix:
            if len(tensors[name]) > len(getattr(self, f"_{name}_buf")):
                raise ValueError(f"The size of {name} should be less than or equal to the allocated buffer")
        if adopt:
            return
        for name, t in tensors.items():
            buf = getattr(self, f"_{name}_buf")
            if name in prefix:
                buf[: len(t)].copy_(t, non_blocking=(t.device == self.device) and non_blocking)
            else:
                buf.copy_(t, non_blocking=non_blocking)

    def _set_run_options(self, pos_encoding_mode, window_left, logits_soft_cap, sm_scale, rope_scale,
                         rope_theta) -> None:
        """The attention variant run() computes: set by plan(), and again by the deprecated forward() calls."""
        self._pos_encoding_mode = pos_encoding_mode
        self._window_left = window_left
        self._logits_soft_cap = logits_soft_cap
        self._sm_scale = sm_scale
        self._rope_scale = rope_scale
        self._rope_theta = rope_theta

    def _check_run_args(self, args=()) -> None:
        if self._plan_info is None:
            raise RuntimeError("plan() must be called before run()")
        if args:
            raise ValueError("additional kernel arguments require jit_args, which is not supported")

    def _sink_variant_args(self, args, sinks):
        """(args, sinks, sm_scale) of a run(): a wrapper built with the "AttentionSink" jit_args takes the sink tensor
        and the softmax scale as its two additional positional arguments (ref: additional_tensor_names ``sink``,
        additional_scalar_names ``sm_scale``); any other wrapper passes its arguments through, sm_scale None."""
        if not self._sink_variant:
            return args, sinks, None
        if len(args) != 2 or sinks is not None:
            raise ValueError("a wrapper built with the AttentionSink jit_args is run as run(q, <kv>, sink, sm_scale)")
        return (), args[0], float(args[1])

    def _sinks_ptr(self, sinks: Optional[torch.Tensor], q: torch.Tensor) -> int:
        """Device pointer of the per-head attention sinks (0 for None) once they are float32, contiguous,
        ``[num_qo_heads]`` and on the wrapper's device.  No tensor is created: run() stays capturable."""
        if sinks is None:
            return 0
        if (not torch.is_tensor(sinks) or sinks.dtype != torch.float32 or sinks.dim() != 1
                or sinks.shape[0] != self._num_qo_heads or not sinks.is_contiguous() or sinks.device != self.device):
            raise ValueError(
                f"sinks must be a contiguous float32 tensor of shape [{self._num_qo_heads}] (num_qo_heads) on "
                f"{self.device}; got {getattr(sinks, 'dtype', type(sinks))} {tuple(getattr(sinks, 'shape', ()))} on "
                f"{getattr(sinks, 'device', None)}")
        if q.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"attention sinks need float16 or bfloat16 queries (got {q.dtype})")
        return sinks.data_ptr()
