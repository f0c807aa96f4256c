"""Logits to token: softmax, categorical draws with top-k / top-p / min-p filters, renormalisation and chain
speculative sampling.  Mirrors flashinfer/sampling.py (v0.3.1) name by name and argument by argument; the kernels
are csrc/sampling.hip behind the C ABI (include/fi_mi355.h, "Sampling").

Differences from the reference (also in INTEGRATION.md):
  * ``generator=None`` means the device's default generator (``torch.cuda.default_generators``), so
    ``torch.manual_seed`` governs the stream and consecutive calls differ.  The reference builds a fresh generator
    per call (sampling.py:36-38), i.e. the same seed and offset 0 every time.
  * ``deterministic`` and ``enable_pdl`` are accepted and ignored: every kernel is bit-reproducible for the same
    (inputs, seed, offset), and there is no programmatic dependent launch on this hardware.
  * ``top_k_top_p_sampling_from_logits`` uses this module's ``softmax`` where the reference calls torch.softmax.
  * a per-request parameter tensor (top_k, top_p, min_p) used together with ``indices`` is read at the row drawn from,
    ``param[indices[i]]``, which is what its required length ``probs.shape[0]`` means; the reference reads top_k and
    min_p at the output row ``param[i]``.  Without ``indices`` the two are the same.
  * top-p works on rows that sum to about 1 (an entry counts as at most 2.0); vocabularies go up to 2^22 entries.
  * the random stream is Philox4x32-10 keyed by (seed, offset, output row); it is not the reference's stream.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace
from typing import Any, Optional, Tuple, Union

import torch

from . import _lib

_GENERATOR_STATE_BYTES = 16  # (seed, offset) as two int64: the state of a device generator


def _default_generator(device: Optional[torch.device]) -> torch.Generator:
    if not torch.cuda.is_available():
        raise RuntimeError("sampling needs a GPU generator and no GPU is visible; there is no CPU fallback")
    index = torch.cuda.current_device() if device is None or device.index is None else device.index
    torch.cuda.init()
    return torch.cuda.default_generators[index]


def _seed_and_offset(increment: int, generator: Optional[torch.Generator], device: Optional[torch.device]):
    if generator is None:
        generator = _default_generator(device)
    state = generator.get_state()
    if state.numel() != _GENERATOR_STATE_BYTES:
        raise ValueError(
            f"generator on {generator.device} has a {state.numel()}-byte state; sampling needs a GPU generator, whose "
            f"state is the {_GENERATOR_STATE_BYTES} bytes (seed, offset)"
        )
    seed, offset = state.view(torch.int64).tolist()
    offset += (increment + 3) // 4 * 4
    generator.set_state(torch.tensor([seed, offset], dtype=torch.int64).view(torch.uint8))
    return int(seed), int(offset)


def get_seed_and_offset(increment: int, generator: Optional[torch.Generator] = None) -> Tuple[int, int]:
    """Advance ``generator`` by ``increment`` rounded up to a multiple of 4 and return ``(seed, offset)``
    (ref: sampling.py:33-46).  ``generator=None`` is the current device's default generator."""
    return _seed_and_offset(increment, generator, None)


def _u64(x: int) -> int:
    return x & 0xFFFFFFFFFFFFFFFF


def _rows(t: torch.Tensor, name: str) -> torch.Tensor:
    _lib.require_gpu_tensor(t, name)
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2D (batch_size, num_classes), got shape {tuple(t.shape)}")
    return t.float().contiguous()


def _arr(t: Optional[torch.Tensor], dtype: torch.dtype, device: torch.device) -> Optional[torch.Tensor]:
    return None if t is None else t.to(device=device, dtype=dtype).contiguous()


def _draw(symbol: str, probs: torch.Tensor, indices: Optional[torch.Tensor], increment_per_row: int,
          generator: Optional[torch.Generator], top_k_arr=None, top_k_val: int = 0, top_p_arr=None,
          top_p_val: float = 1.0, name: str = "probs") -> torch.Tensor:
    probs = _rows(probs, name)
    dev = probs.device
    idx = _arr(indices, torch.int32, dev)
    batch = idx.numel() if idx is not None else probs.shape[0]
    k_arr, p_arr = _arr(top_k_arr, torch.int32, dev), _arr(top_p_arr, torch.float32, dev)
    param_len = max([a.numel() for a in (k_arr, p_arr) if a is not None], default=0)
    samples = torch.empty(batch, dtype=torch.int32, device=dev)
    seed, offset = _seed_and_offset(batch * increment_per_row, generator, dev)
    p = _lib.fi_sampling_params_t(
        probs=probs.data_ptr(), samples=samples.data_ptr(), indices=_lib.ptr(idx), top_k_arr=_lib.ptr(k_arr),
        top_p_arr=_lib.ptr(p_arr), top_k_val=int(top_k_val), top_p_val=float(top_p_val), batch=batch,
        num_rows=probs.shape[0], vocab=probs.shape[1], param_len=param_len, philox_seed=_u64(seed),
        philox_offset=_u64(offset))
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), symbol)(C.byref(p), _lib.current_stream(dev)), symbol[3:])
    return samples


def _transform(symbol: str, x: torch.Tensor, name: str, top_k_arr=None, top_k_val: int = 0, scalar_arr=None,
               scalar_val: float = 1.0) -> torch.Tensor:
    x = _rows(x, name)
    dev = x.device
    out = torch.empty_like(x)
    k_arr, s_arr = _arr(top_k_arr, torch.int32, dev), _arr(scalar_arr, torch.float32, dev)
    param_len = max([a.numel() for a in (k_arr, s_arr) if a is not None], default=0)
    p = _lib.fi_row_transform_params_t(
        in_=x.data_ptr(), out=out.data_ptr(), top_k_arr=_lib.ptr(k_arr), scalar_arr=_lib.ptr(s_arr),
        top_k_val=int(top_k_val), scalar_val=float(scalar_val), batch=x.shape[0], vocab=x.shape[1],
        param_len=param_len)
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.lib(), symbol)(C.byref(p), _lib.current_stream(dev)), symbol[3:])
    return out


@functools.cache
def get_sampling_module():
    """The reference's module getter (sampling.py:60-487): functions with the positional signatures of its custom
    ops, forwarding to the C ABI.  The random-number increments per operator are the reference's."""

    def softmax(workspace_buffer, logits, maybe_temperature_arr, temperature_val, enable_pdl) -> torch.Tensor:
        """ref: sampling.py:64-85 (the workspace is unused: one workgroup owns a row)."""
        return _transform("fi_softmax", logits, "logits", scalar_arr=maybe_temperature_arr, scalar_val=temperature_val)

    def sampling_from_logits(logits, indices, deterministic, generator) -> torch.Tensor:
        """ref: sampling.py:98-120."""
        return _draw("fi_sampling_from_logits", logits, indices, logits.shape[-1], generator, name="logits")

    def sampling_from_probs(probs, indices, deterministic, generator) -> torch.Tensor:
        """ref: sampling.py:134-154."""
        return _draw("fi_sampling_from_probs", probs, indices, 1, generator)

    def top_p_sampling_from_probs(probs, indices, maybe_top_p_arr, top_p_val, deterministic, generator):
        """ref: sampling.py:170-197."""
        return _draw("fi_top_p_sampling_from_probs", probs, indices, 32, generator, top_p_arr=maybe_top_p_arr,
                     top_p_val=top_p_val)

    def top_k_sampling_from_probs(probs, indices, maybe_top_k_arr, top_k_val, deterministic, generator):
        """ref: sampling.py:213-238."""
        return _draw("fi_top_k_sampling_from_probs", probs, indices, 32, generator, top_k_arr=maybe_top_k_arr,
                     top_k_val=top_k_val)

    def min_p_sampling_from_probs(probs, indices, maybe_min_p_arr, min_p_val, deterministic, generator):
        """ref: sampling.py:255-282."""
        return _draw("fi_min_p_sampling_from_probs", probs, indices, 1, generator, top_p_arr=maybe_min_p_arr,
                     top_p_val=min_p_val)

    def top_k_top_p_sampling_from_probs(probs, indices, maybe_top_k_arr, top_k_val, maybe_top_p_arr, top_p_val,
                                        deterministic, generator):
        """ref: sampling.py:286-318 (the joint filter)."""
        return _draw("fi_top_k_top_p_sampling_from_probs", probs, indices, 32, generator, top_k_arr=maybe_top_k_arr,
                     top_k_val=top_k_val, top_p_arr=maybe_top_p_arr, top_p_val=top_p_val)

    def top_p_renorm_probs(probs, maybe_top_p_arr, top_p_val) -> torch.Tensor:
        """ref: sampling.py:337-354."""
        return _transform("fi_top_p_renorm_probs", probs, "probs", scalar_arr=maybe_top_p_arr, scalar_val=top_p_val)

    def top_k_renorm_probs(probs, maybe_top_k_arr, top_k_val) -> torch.Tensor:
        """ref: sampling.py:366-381."""
        return _transform("fi_top_k_renorm_probs", probs, "probs", top_k_arr=maybe_top_k_arr, top_k_val=top_k_val)

    def top_k_mask_logits(logits, maybe_top_k_arr, top_k_val) -> torch.Tensor:
        """ref: sampling.py:393-408."""
        return _transform("fi_top_k_mask_logits", logits, "logits", top_k_arr=maybe_top_k_arr, top_k_val=top_k_val)

    def chain_speculative_sampling(draft_probs, draft_token_ids, target_probs, output_accepted_token_num,
                                   output_emitted_draft_token_num, deterministic, generator) -> torch.Tensor:
        """ref: sampling.py:420-458.  The two counters are accumulated in place."""
        for t, name in ((draft_probs, "draft_probs"), (draft_token_ids, "draft_token_ids"),
                        (target_probs, "target_probs"), (output_accepted_token_num, "output_accepted_token_num"),
                        (output_emitted_draft_token_num, "output_emitted_draft_token_num")):
            _lib.require_gpu_tensor(t, name)
        dev = draft_probs.device
        b, n = draft_token_ids.shape
        d = target_probs.shape[-1]
        if tuple(draft_probs.shape) != (b, n, d) or tuple(target_probs.shape) != (b, n + 1, d):
            raise ValueError(
                f"chain_speculative_sampling: draft_probs {tuple(draft_probs.shape)} / target_probs "
                f"{tuple(target_probs.shape)} do not match draft_token_ids {tuple(draft_token_ids.shape)}")
        if output_accepted_token_num.numel() != b or output_emitted_draft_token_num.numel() != b:
            raise ValueError("chain_speculative_sampling: the counters must have batch_size entries")
        draft = draft_probs.float().contiguous()
        target = target_probs.float().contiguous()
        ids = draft_token_ids.int().contiguous()
        # counters of another dtype or layout are accumulated in an int32 copy and written back
        acc = output_accepted_token_num.int().contiguous()
        emi = output_emitted_draft_token_num.int().contiguous()
        out = torch.empty((b, n + 1), dtype=torch.int32, device=dev)
        seed, offset = _seed_and_offset(b * (n + 1), generator, dev)
        p = _lib.fi_chain_speculative_params_t(
            draft_probs=draft.data_ptr(), draft_token_ids=ids.data_ptr(), target_probs=target.data_ptr(),
            output_token_ids=out.data_ptr(), output_accepted_token_num=acc.data_ptr(),
            output_emitted_draft_token_num=emi.data_ptr(), batch=b, num_speculative_tokens=n, vocab=d,
            philox_seed=_u64(seed), philox_offset=_u64(offset))
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().fi_chain_speculative_sampling(C.byref(p), _lib.current_stream(dev)),
                       "chain_speculative_sampling")
        if acc.data_ptr() != output_accepted_token_num.data_ptr():
            output_accepted_token_num.copy_(acc.view_as(output_accepted_token_num))
        if emi.data_ptr() != output_emitted_draft_token_num.data_ptr():
            output_emitted_draft_token_num.copy_(emi.view_as(output_emitted_draft_token_num))
        return out

    return SimpleNamespace(
        softmax=softmax,
        sampling_from_probs=sampling_from_probs,
        sampling_from_logits=sampling_from_logits,
        top_p_sampling_from_probs=top_p_sampling_from_probs,
        top_k_sampling_from_probs=top_k_sampling_from_probs,
        min_p_sampling_from_probs=min_p_sampling_from_probs,
        top_k_top_p_sampling_from_probs=top_k_top_p_sampling_from_probs,
        top_p_renorm_probs=top_p_renorm_probs,
        top_k_renorm_probs=top_k_renorm_probs,
        top_k_mask_logits=top_k_mask_logits,
        chain_speculative_sampling=chain_speculative_sampling,
    )


def _to_tensor_scalar_tuple(x):
    return (x, 0) if isinstance(x, torch.Tensor) else (None, x)


def _check_tensor_param(param: Any, tensor: torch.Tensor) -> None:
    """A per-request parameter is a scalar or a 1D tensor of batch_size entries (ref: sampling.py:497-515)."""
    if isinstance(param, torch.Tensor):
        if param.dim() == 0:
            raise ValueError(
                "Expected a 1D tensor of shape (batch_size,) or scalar for the sampling parameter, "
                f"but got a 0-dimensional tensor with shape {param.shape}. ")
        elif param.dim() > 1:
            raise ValueError(
                "Expected a 1D tensor or scalar for the sampling parameter, "
                f"but got a {param.dim()}D tensor with shape {param.shape}.")
        elif param.shape[0] != tensor.shape[0]:
            raise ValueError(
                "Sampling parameter tensor batch size mismatch: "
                f"expected length {tensor.shape[0]} to match the reference tensor batch size, "
                f"but got length {param.shape[0]} with shape {param.shape}.")


def _check_nan(t: torch.Tensor, what: str) -> None:
    if torch.any(torch.isnan(t)):
        raise ValueError(f"Input {what} contains NaN.")


def _check_order(filter_apply_order: str) -> None:
    if filter_apply_order not in ("top_k_first", "joint"):
        raise ValueError(f"Invalid filter_apply_order: {filter_apply_order}")


def softmax(
    logits: torch.Tensor,
    temperature: Optional[Union[torch.Tensor, float]] = None,
    enable_pdl: Optional[bool] = None,
) -> torch.Tensor:
    r"""``softmax(logits / temperature)`` in float32; rows may contain ``-inf`` (ref: sampling.py:518-572).

    ``temperature`` is a scalar or a ``(batch_size,)`` tensor, ``None`` means 1.0; ``enable_pdl`` is ignored.

    >>> logits = torch.tensor([[0.8823, 0.9150, 0.3829, 0.9593, 0.3904]], device="cuda")
    >>> flashinfer.sampling.softmax(logits, temperature=1.0)
    tensor([[0.2309, 0.2385, 0.1401, 0.2493, 0.1412]], device='cuda:0')
    """
    if temperature is None:
        temperature = 1.0
    _check_tensor_param(temperature, logits)
    return get_sampling_module().softmax(None, logits, *_to_tensor_scalar_tuple(temperature), bool(enable_pdl))


def sampling_from_logits(
    logits: torch.Tensor,
    indices: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Draw one category per output row from ``softmax(logits)`` without materialising it
    (ref: sampling.py:575-630).  ``indices[i] = j`` makes output ``i`` a draw from row ``j``; int32 ``(batch_size,)``
    is returned.  A category with logit ``-inf`` is never returned."""
    if check_nan:
        _check_nan(logits, "logits")
    return get_sampling_module().sampling_from_logits(logits, indices, deterministic, generator)


def sampling_from_probs(
    probs: torch.Tensor,
    indices: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Draw one category per output row from ``probs`` by inverse CDF (ref: sampling.py:633-694).  A category of
    probability 0 is never returned."""
    if check_nan:
        _check_nan(probs, "probs")
    return get_sampling_module().sampling_from_probs(probs, indices, deterministic, generator)


def top_p_sampling_from_probs(
    probs: torch.Tensor,
    top_p: Union[torch.Tensor, float],
    indices: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Nucleus sampling (ref: sampling.py:697-777): a draw from ``probs`` restricted to the smallest set of
    highest-probability categories whose mass reaches ``top_p`` and renormalised.  Sort-free: the threshold is found
    by a radix select over the float bit pattern."""
    if check_nan:
        _check_nan(probs, "probs")
    _check_tensor_param(top_p, probs)
    return get_sampling_module().top_p_sampling_from_probs(
        probs, indices, *_to_tensor_scalar_tuple(top_p), deterministic, generator)


def top_k_sampling_from_probs(
    probs: torch.Tensor,
    top_k: Union[torch.Tensor, int],
    indices: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Top-k sampling (ref: sampling.py:780-860): a draw from ``probs`` restricted to the categories not smaller
    than the k-th largest (ties at the pivot included) and renormalised.  ``top_k = 0`` or ``>= num_classes`` keeps
    every category."""
    if check_nan:
        _check_nan(probs, "probs")
    _check_tensor_param(top_k, probs)
    return get_sampling_module().top_k_sampling_from_probs(
        probs, indices, *_to_tensor_scalar_tuple(top_k), deterministic, generator)


def min_p_sampling_from_probs(
    probs: torch.Tensor,
    min_p: Union[torch.Tensor, float],
    indices: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Min-p sampling (ref: sampling.py:863-939): a draw from ``probs`` restricted to the categories with
    ``p >= min_p * max(p)`` and renormalised."""
    if check_nan:
        _check_nan(probs, "probs")
    _check_tensor_param(min_p, probs)
    return get_sampling_module().min_p_sampling_from_probs(
        probs, indices, *_to_tensor_scalar_tuple(min_p), deterministic, generator)


def top_k_top_p_sampling_from_logits(
    logits: torch.Tensor,
    top_k: Union[torch.Tensor, int],
    top_p: Union[torch.Tensor, float],
    indices: Optional[torch.Tensor] = None,
    filter_apply_order: str = "top_k_first",
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Top-k and top-p sampling from pre-softmax logits (ref: sampling.py:942-1061).  ``"top_k_first"`` is
    ``top_k_mask_logits`` -> ``softmax`` -> ``top_p_sampling_from_probs``; ``"joint"`` is ``softmax`` -> the joint
    filter (both sets taken on the unfiltered probabilities)."""
    _check_order(filter_apply_order)
    _check_tensor_param(top_k, logits)
    _check_tensor_param(top_p, logits)
    if filter_apply_order == "top_k_first":
        probs = softmax(top_k_mask_logits(logits, top_k))
        return top_p_sampling_from_probs(probs, top_p, indices, deterministic, check_nan=check_nan, generator=generator)
    probs = softmax(logits)
    if check_nan:
        _check_nan(probs, "probs")
    return get_sampling_module().top_k_top_p_sampling_from_probs(
        probs, indices, *_to_tensor_scalar_tuple(top_k), *_to_tensor_scalar_tuple(top_p), deterministic, generator)


def top_k_top_p_sampling_from_probs(
    probs: torch.Tensor,
    top_k: Union[torch.Tensor, int],
    top_p: Union[torch.Tensor, float],
    indices: Optional[torch.Tensor] = None,
    filter_apply_order: str = "top_k_first",
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
    check_nan: bool = False,
) -> torch.Tensor:
    r"""Top-k and top-p sampling from probabilities (ref: sampling.py:1064-1176).  ``"top_k_first"`` is
    ``top_k_renorm_probs`` -> ``top_p_sampling_from_probs``; ``"joint"`` draws from the intersection of the top-k and
    the top-p set of the given probabilities."""
    _check_order(filter_apply_order)
    _check_tensor_param(top_k, probs)
    _check_tensor_param(top_p, probs)
    if filter_apply_order == "top_k_first":
        renorm_probs = top_k_renorm_probs(probs, top_k)
        return top_p_sampling_from_probs(
            renorm_probs, top_p, indices, deterministic, check_nan=check_nan, generator=generator)
    if check_nan:
        _check_nan(probs, "probs")
    return get_sampling_module().top_k_top_p_sampling_from_probs(
        probs, indices, *_to_tensor_scalar_tuple(top_k), *_to_tensor_scalar_tuple(top_p), deterministic, generator)


def top_p_renorm_probs(
    probs: torch.Tensor,
    top_p: Union[torch.Tensor, float],
) -> torch.Tensor:
    r"""Zero everything outside the top-p set and divide by the kept mass (ref: sampling.py:1179-1239).

    >>> prob = torch.tensor([[0.2499, 0.2592, 0.1085, 0.2718, 0.1106]], device="cuda")
    >>> flashinfer.sampling.top_p_renorm_probs(prob, 0.3)
    tensor([[0.0000, 0.4882, 0.0000, 0.5118, 0.0000]], device='cuda:0')
    """
    _check_tensor_param(top_p, probs)
    return get_sampling_module().top_p_renorm_probs(probs, *_to_tensor_scalar_tuple(top_p))


top_p_renorm_prob = top_p_renorm_probs


def top_k_renorm_probs(
    probs: torch.Tensor,
    top_k: Union[torch.Tensor, int],
) -> torch.Tensor:
    r"""Keep the categories not smaller than the k-th largest, zero the rest, renormalise
    (ref: sampling.py:1245-1304).

    >>> prob = torch.tensor([[0.2499, 0.2592, 0.1085, 0.2718, 0.1106]], device="cuda")
    >>> flashinfer.sampling.top_k_renorm_probs(prob, 3)
    tensor([[0.3201, 0.3319, 0.0000, 0.3480, 0.0000]], device='cuda:0')
    """
    _check_tensor_param(top_k, probs)
    return get_sampling_module().top_k_renorm_probs(probs, *_to_tensor_scalar_tuple(top_k))


top_k_renorm_prob = top_k_renorm_probs


def top_k_mask_logits(
    logits: torch.Tensor, top_k: Union[torch.Tensor, int]
) -> torch.Tensor:
    r"""Keep the logits not smaller than the k-th largest and set the rest to ``-inf``
    (ref: sampling.py:1310-1364); ``softmax`` of the result equals ``top_k_renorm_probs`` of the softmax."""
    _check_tensor_param(top_k, logits)
    return get_sampling_module().top_k_mask_logits(logits, *_to_tensor_scalar_tuple(top_k))


def chain_speculative_sampling(
    draft_probs,
    draft_token_ids,
    target_probs,
    maybe_output_accepted_token_num: Optional[torch.Tensor] = None,
    maybe_output_emitted_draft_token_num: Optional[torch.Tensor] = None,
    deterministic: bool = True,
    generator: Optional[torch.Generator] = None,
) -> torch.Tensor:
    r"""Speculative sampling over a chain of draft tokens (ref: sampling.py:1367-1477, https://arxiv.org/abs/2302.01318).

    ``draft_probs`` ``(batch, n, vocab)``, ``draft_token_ids`` ``(batch, n)``, ``target_probs`` ``(batch, n + 1, vocab)``.
    Returns ``(output_token_ids (batch, n + 1), output_accepted_token_num, output_emitted_draft_token_num)``: draft
    tokens are accepted while ``u * p_draft < p_target``, the first rejected position is redrawn from
    ``relu(target - draft)`` (the bonus position from the target alone) and later positions are ``-1``.  The two
    counters are added to the given tensors in place, or returned fresh when ``None``."""
    b = draft_probs.size(0)
    dev = draft_probs.device
    if maybe_output_accepted_token_num is None:
        output_accepted_token_num = torch.zeros(b, dtype=torch.int32, device=dev)
    else:
        output_accepted_token_num = maybe_output_accepted_token_num
    if maybe_output_emitted_draft_token_num is None:
        output_emitted_draft_token_num = torch.zeros(b, dtype=torch.int32, device=dev)
    else:
        output_emitted_draft_token_num = maybe_output_emitted_draft_token_num
    output_token_ids = get_sampling_module().chain_speculative_sampling(
        draft_probs, draft_token_ids, target_probs, output_accepted_token_num, output_emitted_draft_token_num,
        deterministic, generator)
    return output_token_ids, output_accepted_token_num, output_emitted_draft_token_num
