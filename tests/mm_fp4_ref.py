"""CPU oracle of flashinfer.mm_fp4 (tests/test_mm_fp4_cpu.py, tests/test_mm_fp4_gpu.py): plain torch, fp64, no kernel.

    mm_fp4_ref(a_q, sa, b_q, sb, alpha) = (e2m1(a) * 2^(sa - 127)) @ (e2m1(b) * 2^(sb - 127)).T * alpha

a_q [m, k / 2] and b_q [n, k / 2] packed e2m1 bytes, sa [m, k / 32] and sb [n, k / 32] LINEAR scale bytes.  Every product of
two dequantised elements is exact in fp64, and so is every sum the tests ask to be exact.
"""
import torch

import mx_ref as R


def mm_fp4_ref(a_q: torch.Tensor, sa: torch.Tensor, b_q: torch.Tensor, sb: torch.Tensor, alpha=None) -> torch.Tensor:
    a = R.dequantize(R.e2m1_to_f64(a_q), sa)
    b = R.dequantize(R.e2m1_to_f64(b_q), sb)
    out = a @ b.T
    return out if alpha is None else out * float(alpha)


def abs_product_ref(a_q: torch.Tensor, sa: torch.Tensor, b_q: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """|A| @ |B|.T of the dequantised operands: what an f32 accumulation bound is relative to."""
    return R.dequantize(R.e2m1_to_f64(a_q), sa).abs() @ R.dequantize(R.e2m1_to_f64(b_q), sb).abs().T


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """[..., k] e2m1 codes (0..15) -> [..., k / 2] bytes, element 2 i in the low nibble of byte i."""
    codes = codes.to(torch.uint8)
    return codes[..., 0::2] | (codes[..., 1::2] << 4)


def round_once(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """fp64 -> the 16-bit dtype with ONE rounding.  torch converts through f32, so the value must be exact in f32 (the
    bit-exact tests' sums are: multiples of 2^-6 below 2^20); that is asserted here."""
    assert torch.equal(x.to(torch.float32).double(), x), "the value is not exact in f32: two roundings"
    return x.to(dtype)


def ulp(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of `dtype` at |x| (fp64 in, fp64 out), the subnormal spacing below the smallest normal."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** emin)))
    return torch.exp2(e - mant)
