"""CPU: the MX operators (mxfp8_quantize, group_gemm_mxfp8_mxfp4_nt_groupwise) have the reference's public surface, their
host-side validation reports without a launch, and the fp64 oracle of the GPU tests (tests/mx_ref.py) agrees with
hand-worked examples and with a plain f32 restatement of the reference test's dequantise-then-matmul."""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

import mx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mx_signatures.json")
MS = [4, 132, 0, 260]


def _params(fn):
    return [
        {"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
        for p in inspect.signature(fn).parameters.values()
    ]


def test_signatures_match_the_reference():
    import flashinfer

    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == ["fp8_quantization", "gemm"]
    assert sorted(g["fp8_quantization"]["functions"]) == ["mxfp8_dequantize_host", "mxfp8_quantize"]
    assert sorted(g["gemm"]["functions"]) == ["group_gemm_mxfp8_mxfp4_nt_groupwise"]
    for module_name, entry in g.items():
        module = getattr(flashinfer, module_name)
        assert module.__name__ == f"flashinfer.{module_name}"
        for name, params in entry["functions"].items():
            assert _params(getattr(module, name)) == params, name
        for new, old in entry["aliases"].items():
            assert getattr(module, new) is getattr(module, old), new
        for name in entry["top_level"]:
            assert getattr(flashinfer, name) is getattr(module, name), name
    assert g["fp8_quantization"]["top_level"] == ["mxfp8_dequantize_host", "mxfp8_quantize"]
    assert g["gemm"]["aliases"] == {"group_gemm_mxfp4_nt_groupwise": "group_gemm_mxfp8_mxfp4_nt_groupwise"}
    # the table of the change, spelled out
    assert _params(flashinfer.mxfp8_quantize) == [
        {"name": "input"}, {"name": "is_sf_swizzled_layout", "default": True}, {"name": "alignment", "default": 32},
        {"name": "enable_pdl", "default": None}]
    assert _params(flashinfer.mxfp8_dequantize_host) == [
        {"name": "input"}, {"name": "scale_tensor"}, {"name": "is_sf_swizzled_layout", "default": True}]
    assert _params(flashinfer.gemm.group_gemm_mxfp4_nt_groupwise) == [
        {"name": "a"}, {"name": "b"}, {"name": "a_scale"}, {"name": "b_scale"}, {"name": "m_indptr"},
        {"name": "mma_sm", "default": 1}, {"name": "tile_m", "default": 128}, {"name": "tile_n", "default": 128},
        {"name": "tile_k", "default": 128}, {"name": "swap_ab", "default": True}, {"name": "out", "default": None},
        {"name": "out_dtype", "default": None}]
    assert list(inspect.signature(flashinfer.fp8_quantization.mxfp8_quantize_grouped).parameters) == ["input", "m_indptr"]


def test_compat_getter_has_the_reference_op():
    from flashinfer import compat

    # get_gemm_sm100_module() loads the library; the op itself is only looked at
    m = compat.get_gemm_sm100_module()
    assert list(inspect.signature(m.group_gemm_mxfp4_nt_groupwise).parameters) == [
        "int_workspace_buffer", "float_workspace_buffer", "a", "b", "a_scale", "b_scale", "out", "m_indptr", "n", "k",
        "mma_sm", "tile_m", "tile_n", "tile_k", "swap_ab"]


def test_swizzled_offsets():
    # hand-worked at nkb = 8 (two 512-byte k tiles per 128 rows): row 1 is 16 bytes on, row 32 is the second dword of
    # row 0's 16 bytes, (33, 5) = k tile 1 (512) + row 33 % 32 = 1 (16) + row block 1 (4) + block 5 % 4 (1)
    assert R.sf_offset(0, 0, 8) == 0
    assert R.sf_offset(1, 0, 8) == 16
    assert R.sf_offset(32, 0, 8) == 4
    assert R.sf_offset(33, 5, 8) == 533
    assert R.sf_offset(128, 0, 8) == 1024
    # the four scales of a row over 128 k elements are one aligned dword
    for r in (0, 5, 77, 200):
        first = R.sf_offset(r, 4, 8)
        assert first % 4 == 0 and [R.sf_offset(r, 4 + i, 8) for i in range(4)] == [first + i for i in range(4)]
    # a bijection on the padded 256 x 8 region, also when nkb itself is padded (6 -> 8)
    r = torch.arange(256).view(-1, 1).expand(256, 8)
    kb = torch.arange(8).view(1, -1).expand(256, 8)
    for nkb in (8, 6, 5):
        assert sorted(R.sf_offset(r, kb, nkb).reshape(-1).tolist()) == list(range(256 * 8))
    sf = torch.randint(0, 255, (200, 6), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    flat = R.swizzle(sf, fill=7)
    assert flat.numel() == 256 * 8 and torch.equal(R.unswizzle(flat, 200, 6), sf)
    assert int((flat == 7).sum()) >= 256 * 8 - 200 * 6
    # the package's own copy of the function (mxfp8_dequantize_host) is the same function
    from flashinfer import _mx

    assert torch.equal(_mx.sf_offset(r, kb, 6), R.sf_offset(r, kb, 6))


def test_grouped_scale_row_offsets():
    """sf_off(g) = (m_indptr[g] + 127 g) / 128 * 128, the formula of the reference
    (group_gemm_mxfp4_groupwise_sm100.cuh:66-68) and of include/fi_mi355.h.  For ms = [4, 132, 0, 260], m_indptr =
    [0, 4, 136, 136, 396], it gives [0, 128, 384, 512, 896].  (The running sum of the groups' sizes padded to 128,
    [0, 128, 384, 384, 768], is a lower bound of it, not the placement: the formula cannot see which earlier groups were
    empty or already aligned.)"""
    from flashinfer import fp8_quantization as Q

    off = R.sf_row_offsets(MS)
    assert off == [0, 128, 384, 512, 896]
    indptr = [0, 4, 136, 136, 396]
    assert off == [(indptr[g] + 127 * g) // 128 * 128 for g in range(5)]
    assert off == [Q.sf_row_offset(indptr[g], g) for g in range(5)]
    padded_sum = [0, 128, 384, 384, 768]
    for g in range(4):
        assert off[g] % 128 == 0 and off[g] >= padded_sum[g]
        assert off[g + 1] - off[g] >= R.ceil_to(MS[g], 128)  # every group's padded rows fit in front of the next group
    sf = torch.arange(396 * 12, dtype=torch.int64).remainder(251).to(torch.uint8).view(396, 12)
    grouped = R.group_swizzle_a(sf, MS, fill=254)
    assert grouped.shape == (896, 12)
    begin = 0
    for g, m in enumerate(MS):
        assert torch.equal(R.unswizzle(grouped.reshape(-1)[off[g] * 12:], m, 12), sf[begin:begin + m])
        begin += m
    assert int((grouped == 254).sum()) >= 896 * 12 - 396 * 12


def test_scale_tensor_sizes():
    """flashinfer._mx.sf_shape sizes every scale tensor the package allocates or checks: it gives the byte counts of
    the oracle's swizzle and group_swizzle_a, padding in both dimensions included, and it is the one function the
    modules that size a scale tensor call."""
    from flashinfer import _mx, fp4_quantization, fp8_quantization, fused_moe

    for rows, nkb in ((1, 1), (127, 4), (128, 5), (129, 6), (200, 6), (300, 129)):
        sf = torch.zeros(rows, nkb, dtype=torch.uint8)
        assert _mx.sf_shape(rows, nkb, False) == (rows, nkb)  # linear
        swz = _mx.sf_shape(rows, nkb, True)  # swizzled
        assert swz[0] * swz[1] == R.swizzle(sf).numel() and swz[0] % 128 == 0 and swz[1] % 4 == 0
    for ms in (MS, (130,), (0, 0, 5), (3, 0, 1, 2, 0, 5, 1, 1)):  # grouped
        grouped = R.group_swizzle_a(torch.zeros(sum(ms), 12, dtype=torch.uint8), ms)
        assert _mx.sf_shape(sum(ms), 12, groups=len(ms)) == tuple(grouped.shape)
        assert _mx.sf_shape(sum(ms), 12, groups=len(ms))[0] == _mx.sf_row_offset(sum(ms), len(ms))
    for module in (fp8_quantization, fp4_quantization, fused_moe):
        assert module.sf_shape is _mx.sf_shape
    assert fp8_quantization.sf_row_offset is _mx.sf_row_offset  # the public name


def test_e2m1_decoding():
    codes = torch.arange(16, dtype=torch.uint8)
    packed = codes[0::2] | (codes[1::2] << 4)  # byte i holds element 2 i in its low nibble
    assert R.e2m1_to_f64(packed).tolist() == [0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6]
    assert R.e2m1_to_f64(torch.tensor([0x2F], dtype=torch.uint8)).tolist() == [-6.0, 1.0]
    x = torch.tensor([0.0, 0.5, -1.5, 6.0, -4.0, 3.0, 2.0, -0.5], dtype=torch.float64)
    assert torch.equal(R.e2m1_to_f64(R.f64_to_e2m1(x)), x)


def test_quantiser_oracle_hand_worked_examples():
    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    x[0, :32] = 1.0
    x[0, 3] = 448.0       # 448 * 2^0 >= 448: e = 0
    x[0, 32:] = -2.0
    x[0, 40] = 450.0      # the next bf16 above 448: e = 1
    x[1, 5] = 0.4375      # 448 * 2^-10: e = -10
    x[2, 9] = -0.439453125  # the next bf16 above 0.4375 in magnitude: e = -9
    q, sf = R.mxfp8_quantize_ref(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == (4, 64) and sf.shape == (4, 2)
    assert sf[0].tolist() == [127, 128]
    assert sf[1].tolist() == [117, 0] and sf[2].tolist() == [118, 0]
    assert sf[3].tolist() == [0, 0] and not q[3].view(torch.uint8).any()  # all-zero blocks: byte 0, q = 0
    assert q[0, 3].item() == 448.0 and q[0, 0].item() == 1.0
    assert q[0, 40].item() == 224.0 and q[0, 33].item() == -1.0  # 450 / 2 = 225 rounds to 224 (e4m3 step 16 there)
    assert q[1, 5].item() == 448.0
    # f16: 448.25 is the next value above 448
    h = torch.zeros(1, 32, dtype=torch.float16)
    h[0, 0] = 448.25
    assert R.mxfp8_quantize_ref(h)[1].item() == 128
    # padded columns and their blocks are zero
    q, sf = R.mxfp8_quantize_ref(torch.ones(2, 96, dtype=torch.float16), alignment=128)
    assert q.shape == (2, 128) and sf.shape == (2, 4) and sf[:, 3].tolist() == [0, 0]
    assert not q[:, 96:].view(torch.uint8).any()
    # random rows with magnitudes 2^-20 .. 2^20: every scaled value fits e4m3, and the scale is the smallest that does
    g = torch.Generator().manual_seed(2)
    for dtype in (torch.float16, torch.bfloat16):
        mag = torch.exp2(torch.randint(-20, 21, (64, 1), generator=g).double())
        if dtype == torch.float16:
            mag = mag.clamp(max=2.0 ** 12)
        xr = (torch.randn(64, 256, generator=g).double() * mag).to(dtype)
        q, sf = R.mxfp8_quantize_ref(xr)
        assert R.fp8_to_f64(q).abs().max().item() <= 448.0
        amax = xr.double().view(64, 8, 32).abs().amax(-1)
        e = sf.double() - 127
        assert bool((448.0 * torch.exp2(e) >= amax).all())
        assert bool(((448.0 * torch.exp2(e - 1) < amax) | (amax == 0)).all())


def test_gemm_oracle_agrees_with_dequantise_then_matmul():
    """The reference's test dequantises both operands to f32 (values times 2^(scale - 127), one scale per 32) and
    multiplies; restated here with plain f32 torch ops."""
    g = torch.Generator().manual_seed(3)
    ms, n, k = [4, 36, 0, 24], 40, 256
    for fp8 in (torch.float8_e4m3fn, torch.float8_e5m2):
        a, sa = R.mx_floor_quantize(torch.randn(sum(ms), k, generator=g), fp8)
        b, sb = R.mx_floor_quantize(torch.randn(len(ms), n, k, generator=g) / k ** 0.5, "fp4")
        assert a.dtype == fp8 and b.shape == (len(ms), n, k // 2) and sa.shape == (sum(ms), k // 32)
        want = R.group_gemm_ref(R.fp8_to_f64(a), sa, b, sb, ms)
        a32 = a.float() * torch.exp2(sa.float() - 127).repeat_interleave(32, dim=1)
        lo, hi = (b & 15).long(), (b >> 4).long()
        nib = torch.stack([lo, hi], dim=-1).flatten(-2)
        table = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
        b32 = table[nib] * torch.exp2(sb.float() - 127).repeat_interleave(32, dim=2)
        begin = 0
        for gi, m in enumerate(ms):
            got = a32[begin:begin + m] @ b32[gi].T
            torch.testing.assert_close(got.double(), want[begin:begin + m], rtol=1e-4, atol=1e-4)
            begin += m
        # the generator is a faithful quantiser: the dequantised operands are near the inputs' scale
        assert want.abs().max().item() > 0.1


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error

    def gemm_params(**kw):
        base = dict(a=a, b=a, a_scale=a, b_scale=a, d=a, m_indptr=a, a_scale_bytes=1 << 20, b_scale_bytes=1 << 20,
                    num_groups=2, cum_m=8, n=16, k=128, a_dtype=_lib.FI_DTYPE_FP8_E4M3, d_dtype=_lib.FI_DTYPE_BF16)
        base.update(kw)
        return _lib.fi_group_gemm_mxfp4_params_t(**base)

    fn = fi_lib.fi_group_gemm_mxfp8_mxfp4_nt_groupwise
    assert fn(None, None) != 0 and b"null" in err()
    for field in ("a", "b", "a_scale", "b_scale", "d", "m_indptr"):
        assert fn(C.byref(gemm_params(**{field: None})), None) != 0 and b"null" in err(), field
    for k in (64, 130, 0):
        assert fn(C.byref(gemm_params(k=k)), None) != 0 and b"multiple of 128" in err(), k
    for n in (4, 17):
        assert fn(C.byref(gemm_params(n=n)), None) != 0 and b"multiple of 8" in err(), n
    for dtype in (_lib.FI_DTYPE_F16, _lib.FI_DTYPE_F32, 17):
        assert fn(C.byref(gemm_params(a_dtype=dtype)), None) != 0 and b"dtype" in err(), dtype
    for dtype in (_lib.FI_DTYPE_FP8_E4M3, _lib.FI_DTYPE_F32):
        assert fn(C.byref(gemm_params(d_dtype=dtype)), None) != 0 and b"dtype" in err(), dtype
    for field in ("num_groups", "cum_m", "n", "k"):
        assert fn(C.byref(gemm_params(**{field: -1})), None) != 0 and b"negative" in err(), field
    # a_scale: (cum_m + 127 G) / 128 * 128 = 256 rows of k / 32 = 4 bytes
    assert fn(C.byref(gemm_params(a_scale_bytes=256 * 4 - 1)), None) != 0 and b"a_scale" in err()
    # b_scale: G * 128 rows
    assert fn(C.byref(gemm_params(b_scale_bytes=2 * 128 * 4 - 1)), None) != 0 and b"b_scale" in err()
    assert fn(C.byref(gemm_params(a=a + 1)), None) != 0 and b"aligned" in err()
    empty = dict(a=None, b=None, a_scale=None, b_scale=None, d=None, m_indptr=None)
    assert fn(C.byref(gemm_params(num_groups=0, **empty)), None) == 0
    assert fn(C.byref(gemm_params(cum_m=0, **empty)), None) == 0

    def quant_params(**kw):
        base = dict(input=a, q=a, sf=a, m_indptr=None, input_stride=64, sf_bytes=1 << 20, m=4, k=64, alignment=32,
                    num_groups=0, sf_layout=_lib.FI_MX_SF_SWIZZLED_128X4, dtype=_lib.FI_DTYPE_F16)
        base.update(kw)
        return _lib.fi_mxfp8_quantize_params_t(**base)

    fn = fi_lib.fi_mxfp8_quantize
    assert fn(None, None) != 0 and b"null" in err()
    for field in ("input", "q", "sf"):
        assert fn(C.byref(quant_params(**{field: None})), None) != 0 and b"null" in err(), field
    for k in (31, 48):
        assert fn(C.byref(quant_params(k=k)), None) != 0 and b"multiple of 32" in err(), k
    for alignment in (0, 16, 48, -32):
        assert fn(C.byref(quant_params(alignment=alignment)), None) != 0 and b"alignment" in err(), alignment
    for dtype in (_lib.FI_DTYPE_F32, _lib.FI_DTYPE_FP8_E4M3, 17):
        assert fn(C.byref(quant_params(dtype=dtype)), None) != 0 and b"dtype" in err(), dtype
    for field in ("m", "k", "num_groups"):
        assert fn(C.byref(quant_params(**{field: -1})), None) != 0 and b"negative" in err(), field
    assert fn(C.byref(quant_params(sf_layout=2)), None) != 0 and b"layout" in err()
    assert fn(C.byref(quant_params(input_stride=32)), None) != 0 and b"stride" in err()
    assert fn(C.byref(quant_params(input_stride=68)), None) != 0 and b"aligned" in err()
    # swizzled: 128 rows x 4 blocks; linear: 4 rows x 2 blocks
    assert fn(C.byref(quant_params(sf_bytes=511)), None) != 0 and b"sf holds" in err()
    assert fn(C.byref(quant_params(sf_bytes=7, sf_layout=_lib.FI_MX_SF_LINEAR)), None) != 0 and b"sf holds" in err()
    # the grouped layout is swizzled and needs its group count
    assert fn(C.byref(quant_params(m_indptr=a, num_groups=2, sf_layout=_lib.FI_MX_SF_LINEAR)), None) != 0 \
        and b"grouped" in err()
    assert fn(C.byref(quant_params(m_indptr=a, num_groups=0)), None) != 0 and b"grouped" in err()
    assert fn(C.byref(quant_params(m=0, input=None, q=None, sf=None)), None) == 0


def test_python_side_errors():
    import flashinfer

    x = torch.zeros(4, 128, dtype=torch.float16)
    a = torch.zeros(4, 128, dtype=torch.float8_e4m3fn)
    b = torch.zeros(1, 8, 64, dtype=torch.uint8)
    s = torch.zeros(128, 4, dtype=torch.uint8)
    indptr = torch.tensor([0, 4], dtype=torch.int32)
    calls = [
        lambda: flashinfer.mxfp8_quantize(x),
        lambda: flashinfer.mxfp8_quantize(x, False, 64),
        lambda: flashinfer.fp8_quantization.mxfp8_quantize_grouped(x, indptr),
        lambda: flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise(a, b, s, s, indptr),
        lambda: flashinfer.gemm.group_gemm_mxfp4_nt_groupwise(a, b, s, s, indptr),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_python_side_checks_run_before_any_launch(monkeypatch):
    """The argument checks sit behind the device check; let CPU tensors through to reach them (nothing is launched:
    every case must raise first)."""
    import flashinfer
    from flashinfer import _lib
    from flashinfer import fp8_quantization as Q

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    with pytest.raises(AssertionError, match="^$"):
        flashinfer.mxfp8_quantize(torch.zeros(4, 48, dtype=torch.float16))
    with pytest.raises(ValueError, match="dtype"):
        flashinfer.mxfp8_quantize(torch.zeros(4, 64, dtype=torch.float32))
    for alignment in (0, 16, 48):
        with pytest.raises(ValueError, match="alignment"):
            flashinfer.mxfp8_quantize(torch.zeros(4, 64, dtype=torch.float16), True, alignment)
    x = torch.zeros(8, 128, dtype=torch.bfloat16)
    indptr = torch.tensor([0, 4, 8], dtype=torch.int32)
    with pytest.raises(ValueError, match="2D"):
        Q.mxfp8_quantize_grouped(x.view(2, 4, 128), indptr)
    with pytest.raises(ValueError, match="multiple of 128"):
        Q.mxfp8_quantize_grouped(torch.zeros(8, 64, dtype=torch.bfloat16), indptr)
    with pytest.raises(ValueError, match="int32"):
        Q.mxfp8_quantize_grouped(x, indptr.long())

    gemm = flashinfer.gemm.group_gemm_mxfp8_mxfp4_nt_groupwise
    a = torch.zeros(8, 128, dtype=torch.float8_e4m3fn)
    b = torch.zeros(2, 16, 64, dtype=torch.uint8)
    sa = torch.zeros(256, 4, dtype=torch.uint8)
    sb = torch.zeros(2, 128, 4, dtype=torch.uint8)
    bad = [
        dict(a=a.view(torch.uint8)), dict(b=b.view(torch.int8)), dict(a_scale=sa.float()), dict(b_scale=sb.float()),
        dict(m_indptr=indptr.long()), dict(mma_sm=3), dict(tile_m=64), dict(tile_n=96), dict(tile_k=64),
        dict(swap_ab=None), dict(out_dtype=torch.float32), dict(m_indptr=indptr[:2]),
        dict(a=torch.zeros(8, 256, dtype=torch.float8_e4m3fn)),                      # k of a and b differ
        dict(b=torch.zeros(2, 12, 64, dtype=torch.uint8)),                           # n % 8
        dict(a=torch.zeros(8, 64, dtype=torch.float8_e4m3fn), b=torch.zeros(2, 16, 32, dtype=torch.uint8)),  # k % 128
        dict(out=torch.zeros(8, 8, dtype=torch.bfloat16)),
        dict(out=torch.zeros(8, 16, dtype=torch.bfloat16), out_dtype=torch.float16),
    ]
    for kw in bad:
        args = dict(a=a, b=b, a_scale=sa, b_scale=sb, m_indptr=indptr)
        args.update(kw)
        with pytest.raises(AssertionError, match="^$"):
            gemm(**args)


@pytest.mark.parametrize("swizzled", [True, False])
def test_dequantize_host_inverts_the_oracle_quantiser(swizzled):
    import flashinfer

    g = torch.Generator().manual_seed(5)
    x = (torch.randn(130, 96, generator=g) * torch.exp2(torch.randint(-12, 12, (130, 1), generator=g).float())).half()
    x[7, 32:64] = 0
    q, sf = R.mxfp8_quantize_ref(x)
    want = R.dequantize(R.fp8_to_f64(q), sf)
    flat = R.swizzle(sf) if swizzled else sf.reshape(-1)
    got = flashinfer.mxfp8_dequantize_host(q, flat, swizzled)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got.double(), want)
    assert torch.equal(flashinfer.mxfp8_dequantize_host(q.view(torch.uint8), flat, swizzled), got)
    # and the quantiser is accurate: the scaled amax is at least 224, where half an e4m3 step is 16 (8 below 256)
    amax = x.double().view(130, 3, 32).abs().amax(-1, keepdim=True)
    assert bool(((got.double() - x.double()).view(130, 3, 32).abs() <= amax * 2.0 ** -3 + 1e-30).all())
    with pytest.raises(ValueError, match="bytes"):
        flashinfer.mxfp8_dequantize_host(q, flat[:-1], swizzled)
