"""fp64 oracle of flashinfer.norm and flashinfer.activation for the CPU and GPU tests.  Everything works from the
16-bit inputs as given and returns float64 (the fused form also returns the residual in the input's dtype)."""
import math

import torch

ACTIVATIONS = ("silu", "gelu", "gelu_tanh")


def half_ulp(dtype: torch.dtype) -> float:
    """Half a unit in the last place of a 16-bit output, relative: what the final rounding may cost."""
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]


def tolerances(dtype: torch.dtype) -> dict:
    """The project's bar: 1e-3 relative and absolute, plus the output rounding of the 16-bit type."""
    return {"rtol": 1e-3 + half_ulp(dtype), "atol": 1e-3}


def assert_close(got, want, dtype, what=""):
    assert got.dtype == dtype, what
    torch.testing.assert_close(got.double(), want, **tolerances(dtype), msg=lambda m: f"{what}: {m}")


def rmsnorm_ref(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6, weight_bias: float = 0.0) -> torch.Tensor:
    """x * rsqrt(mean(x^2) + eps) * (weight_bias + w) over the last dim, in fp64."""
    x = x.double()
    scale = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    return x * scale * (weight_bias + w.double())


def fused_add_rmsnorm_ref(x: torch.Tensor, residual: torch.Tensor, w: torch.Tensor, eps: float = 1e-6,
                          weight_bias: float = 0.0):
    """(norm in fp64 of the f32 sum, the sum rounded to the input dtype).  The f32 add of two 16-bit values and the
    round-to-nearest-even conversion have one answer each, so the residual is exact."""
    s = x.float() + residual.float()
    return rmsnorm_ref(s, w, eps, weight_bias), s.to(x.dtype)


def act_ref(x: torch.Tensor, act: str) -> torch.Tensor:
    x = x.double()
    if act == "silu":
        return x / (1.0 + torch.exp(-x))
    if act == "gelu":
        return x * 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))
    if act == "gelu_tanh":
        return x * 0.5 * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    raise ValueError(act)


def act_and_mul_ref(x: torch.Tensor, act: str) -> torch.Tensor:
    """act(x[..., :d]) * x[..., d:] in fp64."""
    d = x.shape[-1] // 2
    return act_ref(x[..., :d], act) * x[..., d:].double()
