"""CPU oracle of the MXFP4 quantiser (tests/test_fp4_cpu.py, tests/test_fp4_gpu.py): plain torch, fp64, no kernel.
Layouts and e2m1 decoding are mx_ref's.

The rule of fi_mxfp4_quantize: per block of 32, e = the smallest integer in [-127, 127] with 6 * 2^e >= amax (an
all-zero block: e = -127), scale byte e + 127, code = e2m1(x * 2^-e) rounded to nearest with ties to even, two codes
per byte with element 2 i in the low nibble of byte i.
"""
import torch

import mx_ref as R

BLOCK = R.BLOCK


def f64_to_e2m1_rne(x: torch.Tensor) -> torch.Tensor:
    """[..., k] fp64, |x| <= 6 -> [..., k / 2] packed codes, nearest with ties to the code whose mantissa bit is 0.
    The magnitudes are 0, .5, 1, 1.5, 2, 3, 4, 6 for codes 0 .. 7, so of two neighbours the even CODE is the even
    value: the midpoints .25, 1.25, 2.5, 5 go down (to codes 0, 2, 4, 6) and .75, 1.75, 3.5 go up (to codes 2, 4, 6).
    (mx_ref.f64_to_e2m1 breaks every tie toward zero: it is a generator of weights, not this.)"""
    a = x.abs()
    assert a.numel() == 0 or a.max().item() <= 6.0
    code = ((a > 0.25).long() + (a >= 0.75).long() + (a > 1.25).long() + (a >= 1.75).long() + (a > 2.5).long()
            + (a >= 3.5).long() + (a > 5.0).long())
    code = (code + 8 * (x < 0).long()).to(torch.uint8)
    return code[..., 0::2] | (code[..., 1::2] << 4)


def mxfp4_quantize_ref(x: torch.Tensor):
    """x [..., k] f16 / bf16 -> (packed uint8 [..., k / 2], sf uint8 [..., k / 32])."""
    k = x.shape[-1]
    assert k % BLOCK == 0
    blocks = x.double().unflatten(-1, (k // BLOCK, BLOCK))
    amax = blocks.abs().amax(dim=-1)
    # smallest e with 6 * 2^e >= amax, found in exact arithmetic: frexp gives amax = f * 2^E with 0.5 <= f < 1, and
    # 6 = 0.75 * 2^3
    f, E = torch.frexp(amax)
    e = torch.where(f <= 0.75, E - 3, E - 2).clamp(-127, 127)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)
    scaled = blocks * torch.exp2(-e.double()).unsqueeze(-1)  # exact in fp64
    return f64_to_e2m1_rne(scaled.flatten(-2)), (e + 127).to(torch.uint8)


def block_inputs(m: int, k: int, dtype, seed: int) -> torch.Tensor:
    """randn times one magnitude per block of 32, spread over 2^-12 .. 2^12."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp2(torch.randint(-12, 13, (m, k // BLOCK, 1), generator=g).double())
    return (torch.randn(m, k // BLOCK, BLOCK, generator=g).double() * mag).view(m, k).to(dtype)


TIE_VALUES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
TIE_DECODED = (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)


def tie_block(dtype) -> torch.Tensor:
    """One block with amax = 6 (e = 0, byte 127) that holds every midpoint of two neighbouring e2m1 values, both signs:
    +-{.25, .75, 1.25, 1.75, 2.5, 3.5, 5} must decode to +-{0, 1, 1, 2, 2, 4, 4}."""
    x = torch.zeros(1, BLOCK, dtype=torch.float64)
    x[0, 0] = 6.0
    for i, v in enumerate(TIE_VALUES):
        x[0, 2 + 2 * i] = v
        x[0, 3 + 2 * i] = -v
    return x.to(dtype)


def tie_block_decoded() -> torch.Tensor:
    want = torch.zeros(1, BLOCK, dtype=torch.float64)
    want[0, 0] = 6.0
    for i, v in enumerate(TIE_DECODED):
        want[0, 2 + 2 * i] = v
        want[0, 3 + 2 * i] = -v
    return want


def next_up(x: float, dtype) -> float:
    """The next value of `dtype` above the positive, representable x."""
    bits = torch.tensor([x], dtype=dtype).view(torch.int16)
    return float((bits + 1).view(dtype).item())


def boundary_rows(dtype, exps=(-10, 0, 7)):
    """Rows of one block each: amax = 6 * 2^e exactly (wants e) and the next value of the dtype above it (wants e + 1).
    Returns (x [2 len(exps), 32], wanted scale bytes [2 len(exps)])."""
    rows, want = [], []
    for e in exps:
        top = 6.0 * 2.0 ** e
        for amax, we in ((top, e), (next_up(top, dtype), e + 1)):
            row = torch.full((BLOCK,), top / 4, dtype=torch.float64)
            row[5] = -amax
            rows.append(row)
            want.append(we + 127)
    return torch.stack(rows).to(dtype), torch.tensor(want, dtype=torch.uint8)
