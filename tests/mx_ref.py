"""CPU oracle of the MX operators (tests/test_mx_cpu.py, tests/test_mx_gpu.py): plain torch, fp64, no kernel.

  * where a scale byte lives: the swizzled "128x4" layout and the grouped placement of the row operand's scales;
  * e2m1 (fp4) decoding, two codes per byte, element k = 2i in the low nibble of byte i;
  * the quantiser rule of fi_mxfp8_quantize: per block of 32, e = the smallest integer in [-127, 127] with
    448 * 2^e >= amax, scale byte e + 127, q = e4m3(x * 2^-e) rounded to nearest even;
  * the MX "floor" quantiser of the reference's GEMM test (scale exponent floor(log2 amax) - floor(log2 qmax), values
    clamped to the format's range) as a generator of MXFP8 / MXFP4 inputs;
  * the grouped GEMM: dequantise both operands to fp64 and multiply.
"""
import math

import torch

BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
FP8_MAX = {torch.float8_e4m3fn: 448.0, torch.float8_e5m2: 57344.0}


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ---- scale layouts ------------------------------------------------------------------------------------------------
def sf_offset(r, kb, nkb: int):
    """Byte of (row r, k block kb) in a swizzled scale tensor with nkb blocks per row; ints or int64 tensors."""
    k_tiles = (nkb + 3) // 4
    return (r // 128) * k_tiles * 512 + (kb // 4) * 512 + (r % 32) * 16 + ((r % 128) // 32) * 4 + kb % 4


def sf_row_offsets(ms):
    """First scale row of every group, and of the end: sf_off(g) = (m_indptr[g] + 127 g) / 128 * 128."""
    indptr = [0]
    for m in ms:
        indptr.append(indptr[-1] + m)
    return [(indptr[g] + 127 * g) // 128 * 128 for g in range(len(ms) + 1)]


def swizzle(sf: torch.Tensor, fill: int = 0) -> torch.Tensor:
    """[rows, nkb] uint8 -> flat swizzled bytes (rows padded to 128, blocks to 4, padding = fill)."""
    rows, nkb = sf.shape
    out = torch.full((ceil_to(rows, 128) * ceil_to(nkb, 4),), fill, dtype=torch.uint8)
    if rows and nkb:
        r = torch.arange(rows).view(-1, 1).expand(rows, nkb)
        kb = torch.arange(nkb).view(1, -1).expand(rows, nkb)
        out[sf_offset(r, kb, nkb).reshape(-1)] = sf.reshape(-1)
    return out


def unswizzle(flat: torch.Tensor, rows: int, nkb: int) -> torch.Tensor:
    r = torch.arange(rows).view(-1, 1).expand(rows, nkb)
    kb = torch.arange(nkb).view(1, -1).expand(rows, nkb)
    return flat.reshape(-1)[sf_offset(r, kb, nkb).reshape(-1)].view(rows, nkb)


def group_swizzle_a(sf: torch.Tensor, ms, fill: int = 0) -> torch.Tensor:
    """[cum_m, nkb] row scales -> (sf_off(G), nkb): every group swizzled on its own from its first scale row."""
    nkb = sf.shape[1]
    assert nkb % 4 == 0
    off = sf_row_offsets(ms)
    out = torch.full((off[-1] * nkb,), fill, dtype=torch.uint8)
    begin = 0
    for g, m in enumerate(ms):
        piece = swizzle(sf[begin:begin + m], fill)
        out[off[g] * nkb: off[g] * nkb + piece.numel()] = piece
        begin += m
    return out.view(off[-1], nkb)


def swizzle_b(sf: torch.Tensor, fill: int = 0) -> torch.Tensor:
    """[G, n, nkb] -> (G, ceil(n / 128) * 128, nkb), every group swizzled on its own."""
    G, n, nkb = sf.shape
    assert nkb % 4 == 0
    return torch.stack([swizzle(sf[g], fill) for g in range(G)]).view(G, ceil_to(n, 128), nkb)


# ---- number formats -----------------------------------------------------------------------------------------------
def e2m1_to_f64(packed: torch.Tensor) -> torch.Tensor:
    """[..., k / 2] bytes -> [..., k] fp64; the low nibble of byte i is element 2 i, bit 3 of a code is the sign."""
    codes = torch.stack([packed & 15, packed >> 4], dim=-1).flatten(-2).long()
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float64)[codes & 7]
    return torch.where((codes & 8) != 0, -mag, mag)


def f64_to_e2m1(x: torch.Tensor) -> torch.Tensor:
    """Nearest e2m1 code of every element (|x| <= 6), packed two per byte: a generator of weights, not a kernel's spec."""
    grid = torch.tensor(E2M1_VALUES, dtype=torch.float64)
    codes = (x.abs().unsqueeze(-1) - grid).abs().argmin(dim=-1) + 8 * (x < 0)
    codes = codes.to(torch.uint8)
    return codes[..., 0::2] | (codes[..., 1::2] << 4)


def fp8_to_f64(q: torch.Tensor) -> torch.Tensor:
    return q.to(torch.float32).double()


def scale_f64(sf: torch.Tensor) -> torch.Tensor:
    return torch.exp2(sf.double() - 127.0)


def dequantize(q_f64: torch.Tensor, sf: torch.Tensor) -> torch.Tensor:
    """[..., k] values and [..., k / 32] scale bytes -> fp64 (exact: fp64 holds every product)."""
    return (q_f64.unflatten(-1, (-1, BLOCK)) * scale_f64(sf).unsqueeze(-1)).flatten(-2)


# ---- the quantiser rule -------------------------------------------------------------------------------------------
def mxfp8_quantize_ref(x: torch.Tensor, alignment: int = 32):
    """x [m, k] f16 / bf16 -> (q float8_e4m3fn [m, k_pad], sf uint8 [m, k_pad / 32]); padded columns and blocks are 0."""
    m, k = x.shape
    assert k % BLOCK == 0
    k_pad = ceil_to(k, alignment)
    xd = torch.zeros(m, k_pad, dtype=torch.float64)
    xd[:, :k] = x.double()
    blocks = xd.view(m, k_pad // BLOCK, BLOCK)
    amax = blocks.abs().amax(dim=-1)
    # smallest e with 448 * 2^e >= amax, found in exact arithmetic: frexp gives amax = f * 2^E with 0.5 <= f < 1
    f, E = torch.frexp(amax)
    e = torch.where(f * 2 <= 1.75, E - 1 - 8, E - 1 - 7).clamp(-127, 127)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)
    scaled = blocks * torch.exp2(-e.double()).unsqueeze(-1)  # exact in fp64
    assert scaled.abs().max().item() <= 448.0 if scaled.numel() else True
    q = scaled.view(m, k_pad).to(torch.float32).to(torch.float8_e4m3fn)
    return q, (e + 127).to(torch.uint8)


def mx_floor_quantize(x: torch.Tensor, fmt):
    """The recipe of the reference's GEMM test: scale exponent floor(log2 amax) - floor(log2 qmax) per block of 32,
    values divided by the scale and clamped to the format's range.  fmt: a torch fp8 dtype, or "fp4" (returns packed
    bytes).  Returns (values, scale bytes [..., k / 32])."""
    qmax = 6.0 if fmt == "fp4" else FP8_MAX[fmt]
    blocks = x.double().unflatten(-1, (-1, BLOCK))
    amax = blocks.abs().amax(dim=-1)
    e = (torch.floor(torch.log2(amax)) - math.floor(math.log2(qmax))).clamp(-127, 127)
    scaled = (blocks / torch.exp2(e).unsqueeze(-1)).clamp(-qmax, qmax).flatten(-2)
    sf = (e + 127).to(torch.uint8)
    if fmt == "fp4":
        return f64_to_e2m1(scaled), sf
    return scaled.to(torch.float32).to(fmt), sf


# ---- the grouped GEMM ---------------------------------------------------------------------------------------------
def group_gemm_ref(a_f64: torch.Tensor, sa: torch.Tensor, b_packed: torch.Tensor, sb: torch.Tensor, ms) -> torch.Tensor:
    """a_f64 [cum_m, k] (the fp8 values as fp64), sa [cum_m, k / 32], b_packed [G, n, k / 2], sb [G, n, k / 32] ->
    fp64 [sum(ms), n]."""
    a = dequantize(a_f64, sa)
    b = dequantize(e2m1_to_f64(b_packed), sb)
    out = torch.zeros(sum(ms), b.shape[1], dtype=torch.float64)
    begin = 0
    for g, m in enumerate(ms):
        out[begin:begin + m] = a[begin:begin + m] @ b[g].T
        begin += m
    return out
