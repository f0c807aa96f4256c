"""CPU: flashinfer.fp4_quantization has the reference's public surface for its MX half and refuses the nvfp4 half, both
entry points validate on the host without a launch, and the fp64 oracle of the GPU tests (tests/fp4_ref.py) agrees with
hand-worked examples and with the package's host dequantisers."""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

import fp4_ref as F
import mx_ref as R
from flashinfer import fp4_quantization as Q  # the module under test: without it nothing here is collected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fp4_signatures.json")
REFERENCE_NAMES = ["block_scale_interleave", "e2m1_and_ufp8sf_scale_to_float", "fp4_quantize", "mxfp4_dequantize",
                   "mxfp4_dequantize_host", "mxfp4_quantize", "nvfp4_block_scale_interleave"]


def _params(fn):
    return [
        {"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
        for p in inspect.signature(fn).parameters.values()
    ]


def test_signatures_match_the_reference():
    import flashinfer

    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == ["fp4_quantization"]
    entry = g["fp4_quantization"]
    module = flashinfer.fp4_quantization
    assert module is Q and module.__name__ == "flashinfer.fp4_quantization"
    assert sorted(list(entry["functions"]) + list(entry["aliases"])) == REFERENCE_NAMES
    assert entry["top_level"] == REFERENCE_NAMES  # the reference's top level exports every one of them
    for name, params in entry["functions"].items():
        assert _params(getattr(module, name)) == params, name
    assert entry["aliases"] == {"nvfp4_block_scale_interleave": "block_scale_interleave"}
    assert module.nvfp4_block_scale_interleave is module.block_scale_interleave
    for name in REFERENCE_NAMES + ["mxfp4_quantize_grouped"]:
        assert getattr(flashinfer, name) is getattr(module, name), name
    # the table of the change, spelled out
    assert _params(flashinfer.fp4_quantize) == [
        {"name": "input"}, {"name": "global_scale", "default": None}, {"name": "sf_vec_size", "default": 16},
        {"name": "sf_use_ue8m0", "default": False}, {"name": "is_sf_swizzled_layout", "default": True},
        {"name": "is_sf_8x4_layout", "default": False}, {"name": "enable_pdl", "default": None}]
    assert _params(flashinfer.mxfp4_quantize) == [{"name": "a"}]
    assert _params(flashinfer.mxfp4_dequantize) == [{"name": "a_fp4"}, {"name": "a_sf"}]
    assert _params(flashinfer.mxfp4_dequantize_host) == [
        {"name": "weight"}, {"name": "scale"}, {"name": "group_size", "default": 32}]
    assert _params(flashinfer.mxfp4_quantize_grouped) == [{"name": "input"}]


def test_nvfp4_and_the_8x4_layout_are_refused():
    """Refused before the device check: CPU tensors reach the refusal."""
    import flashinfer

    x = torch.zeros(4, 64, dtype=torch.bfloat16)
    gs = torch.ones(1)
    calls = [
        lambda: flashinfer.fp4_quantize(x),                               # the defaults select nvfp4
        lambda: flashinfer.fp4_quantize(x, gs),
        lambda: flashinfer.fp4_quantize(x, gs, 16, False, True, False),
        lambda: flashinfer.fp4_quantize(x, gs, 16, True),                 # sf_vec_size 16
        lambda: flashinfer.fp4_quantize(x, gs, 32, False),                # e4m3 scales
        lambda: flashinfer.fp4_quantize(x, None, 32, True, True, True),   # the 8x4 layout
        lambda: flashinfer.fp4_quantize(x, gs, 16, False, True, True),
        lambda: flashinfer.fp4_quantize(x, None, 64, True),
    ]
    q = torch.zeros(4, 32, dtype=torch.uint8)
    sf = torch.zeros(512, dtype=torch.uint8)
    calls += [
        lambda: flashinfer.e2m1_and_ufp8sf_scale_to_float(q, sf),          # the defaults: 16, ufp8_type 1
        lambda: flashinfer.e2m1_and_ufp8sf_scale_to_float(q, sf, None, 32, 1),
        lambda: flashinfer.e2m1_and_ufp8sf_scale_to_float(q, sf, None, 16, 0),
        lambda: flashinfer.e2m1_and_ufp8sf_scale_to_float(q, sf, gs, 16, 1, False),
        lambda: flashinfer.mxfp4_dequantize_host(q, sf[:8].view(4, 2), 16),
    ]
    for call in calls:
        with pytest.raises(NotImplementedError, match="nvfp4|8x4|sf_vec_size|group_size"):
            call()
    for i in (0, 5):
        with pytest.raises(NotImplementedError, match="not provided"):
            calls[i]()
    for name in ("nvfp4_quantize", "nvfp4_batched_quantize", "shuffle_matrix_a", "shuffle_matrix_sf_a", "SfLayout"):
        assert not hasattr(flashinfer, name) and not hasattr(flashinfer.fp4_quantization, name), name


def test_device_ops_fail_loudly_on_cpu_tensors():
    import flashinfer

    x = torch.zeros(4, 128, dtype=torch.float16)
    calls = [
        lambda: flashinfer.fp4_quantize(x, None, 32, True),
        lambda: flashinfer.mxfp4_quantize(x),
        lambda: flashinfer.mxfp4_quantize_grouped(x.view(1, 4, 128)),
        lambda: flashinfer.block_scale_interleave(torch.zeros(4, 4, dtype=torch.uint8)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(AssertionError, match="uint8"):
        flashinfer.block_scale_interleave(torch.zeros(4, 4, dtype=torch.int8))


def test_python_side_checks_run_before_any_launch(monkeypatch):
    import flashinfer
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    with pytest.raises(AssertionError, match="^$"):
        flashinfer.mxfp4_quantize(torch.zeros(4, 48, dtype=torch.float16))
    with pytest.raises(ValueError, match="dtype"):
        flashinfer.mxfp4_quantize(torch.zeros(4, 64, dtype=torch.float32))
    with pytest.raises(ValueError, match="reshape"):
        flashinfer.mxfp4_quantize(torch.zeros(4, 96, dtype=torch.float16))  # 128 x 4 bytes are no rows of 3
    with pytest.raises(ValueError, match="3D"):
        flashinfer.mxfp4_quantize_grouped(torch.zeros(4, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 128"):
        flashinfer.mxfp4_quantize_grouped(torch.zeros(2, 4, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="2D or 3D"):
        flashinfer.block_scale_interleave(torch.zeros(8, dtype=torch.uint8))


def test_symbols_are_declared_bound_and_exported(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    for name in ("fi_mxfp4_quantize", "fi_mx_sf_interleave"):
        assert f"FI_API int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, name), name
        assert getattr(fi_lib, name).argtypes[0] is C.POINTER(getattr(_lib, name + "_params_t"))
    assert fi_lib.fi_abi_version() == 2  # the change is additive


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error

    def quant_params(**kw):
        base = dict(input=a, q=a, sf=a, input_stride=64, sf_bytes=1 << 20, num_groups=1, rows=4, k=64,
                    sf_layout=_lib.FI_MX_SF_SWIZZLED_128X4, dtype=_lib.FI_DTYPE_F16)
        base.update(kw)
        return _lib.fi_mxfp4_quantize_params_t(**base)

    fn = fi_lib.fi_mxfp4_quantize
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("input", "q", "sf"):
        assert fn(C.byref(quant_params(**{field: None})), None) != 0 and b"null" in err(), field
    for k in (31, 48):
        assert fn(C.byref(quant_params(k=k)), None) != 0 and b"multiple of 32" in err(), k
    for dtype in (_lib.FI_DTYPE_F32, _lib.FI_DTYPE_FP8_E4M3, 17):
        assert fn(C.byref(quant_params(dtype=dtype)), None) != 0 and b"dtype" in err(), dtype
    for field in ("num_groups", "rows", "k"):
        assert fn(C.byref(quant_params(**{field: -1})), None) != 0 and b"negative" in err(), field
    assert fn(C.byref(quant_params(sf_layout=2)), None) != 0 and b"layout" in err()
    assert fn(C.byref(quant_params(input_stride=32)), None) != 0 and b"stride" in err()
    assert fn(C.byref(quant_params(input_stride=68)), None) != 0 and b"aligned" in err()
    assert fn(C.byref(quant_params(input=a + 8)), None) != 0 and b"aligned" in err()
    assert fn(C.byref(quant_params(q=a + 2)), None) != 0 and b"aligned" in err()
    # swizzled: 128 rows x 4 blocks per group; linear: 4 rows x 2 blocks per group
    assert fn(C.byref(quant_params(sf_bytes=511)), None) != 0 and b"sf holds 511 bytes, 512 needed" in err()
    assert fn(C.byref(quant_params(sf_bytes=3 * 512 - 1, num_groups=3)), None) != 0 and b"1536 needed" in err()
    assert fn(C.byref(quant_params(sf_bytes=7, sf_layout=_lib.FI_MX_SF_LINEAR)), None) != 0 and b"8 needed" in err()
    empty = dict(input=None, q=None, sf=None)
    assert fn(C.byref(quant_params(rows=0, **empty)), None) == 0
    assert fn(C.byref(quant_params(num_groups=0, **empty)), None) == 0
    assert fn(C.byref(quant_params(k=0, **empty)), None) == 0

    def il_params(**kw):
        base = dict(input=a, output=a, output_bytes=1 << 20, num_groups=1, rows=4, cols=6)
        base.update(kw)
        return _lib.fi_mx_sf_interleave_params_t(**base)

    fn = fi_lib.fi_mx_sf_interleave
    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("input", "output"):
        assert fn(C.byref(il_params(**{field: None})), None) != 0 and b"null" in err(), field
    for field in ("num_groups", "rows", "cols"):
        assert fn(C.byref(il_params(**{field: -1})), None) != 0 and b"negative" in err(), field
    assert fn(C.byref(il_params(output=a + 1)), None) != 0 and b"aligned" in err()
    assert fn(C.byref(il_params(output_bytes=128 * 8 - 1)), None) != 0 and b"1024 needed" in err()
    assert fn(C.byref(il_params(output_bytes=2 * 128 * 8 - 1, num_groups=2)), None) != 0 and b"2048 needed" in err()
    for field in ("num_groups", "rows", "cols"):
        assert fn(C.byref(il_params(input=None, output=None, **{field: 0})), None) == 0, field


def test_e2m1_encoder_rounds_ties_to_even():
    grid = torch.tensor(R.E2M1_VALUES, dtype=torch.float64)
    both = torch.cat([grid, -grid])
    assert torch.equal(R.e2m1_to_f64(F.f64_to_e2m1_rne(both)), both)  # every e2m1 value encodes to itself
    # between two neighbours: below, at and above the midpoint
    for lo, hi, tie_goes in zip(R.E2M1_VALUES[:-1], R.E2M1_VALUES[1:], (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)):
        mid = (lo + hi) / 2
        x = torch.tensor([mid - 2.0 ** -20, mid, mid + 2.0 ** -20, -(mid - 2.0 ** -20), -mid, -(mid + 2.0 ** -20)],
                         dtype=torch.float64)
        assert R.e2m1_to_f64(F.f64_to_e2m1_rne(x)).tolist() == [lo, tie_goes, hi, -lo, -tie_goes, -hi], mid
    # packing: element 2 i is the low nibble of byte i
    assert F.f64_to_e2m1_rne(torch.tensor([1.0, -6.0], dtype=torch.float64)).tolist() == [0xF2]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_oracle_ties_hand_worked(dtype):
    x = F.tie_block(dtype)
    assert x.double().abs().max().item() == 6.0
    for v in F.TIE_VALUES:
        assert v in x.double()[0].tolist() and -v in x.double()[0].tolist()
    packed, sf = F.mxfp4_quantize_ref(x)
    assert packed.shape == (1, 16) and sf.tolist() == [[127]]
    got = R.e2m1_to_f64(packed)
    assert torch.equal(got, F.tie_block_decoded())
    assert got[0, 2:16].tolist() == [0, -0.0, 1, -1, 1, -1, 2, -2, 2, -2, 4, -4, 4, -4]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_oracle_scale_boundary(dtype):
    x, want = F.boundary_rows(dtype)
    assert want.tolist() == [117, 118, 127, 128, 134, 135]
    # the rows are what they claim: 6 * 2^e, then one ulp of the dtype above it
    amax = x.double().abs().amax(-1)
    ulp = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}[dtype]
    for i, e in enumerate((-10, 0, 7)):
        assert amax[2 * i].item() == 6.0 * 2.0 ** e
        assert amax[2 * i + 1].item() == 6.0 * 2.0 ** e + ulp * 2.0 ** (e + 2)
    packed, sf = F.mxfp4_quantize_ref(x)
    assert torch.equal(sf.view(-1), want)
    dec = R.e2m1_to_f64(packed)
    assert dec[0::2, 5].tolist() == [-6.0] * 3   # amax itself is the code 6 ...
    assert dec[1::2, 5].tolist() == [-3.0] * 3   # ... and just above it, half of it rounds to 3 at the next scale
    assert dec[0::2, 0].tolist() == [1.5] * 3 and dec[1::2, 0].tolist() == [1.0] * 3  # amax / 4 -> 1.5; 0.75 ties up to 1


def test_oracle_zero_block_and_minimality():
    x = torch.zeros(2, 64, dtype=torch.bfloat16)
    x[0, 40] = 3.0
    packed, sf = F.mxfp4_quantize_ref(x)
    assert sf.tolist() == [[0, 126], [0, 0]]
    assert not packed[1].any() and not packed[0, :16].any()
    assert R.e2m1_to_f64(packed)[0, 40].item() == 6.0  # 3 = 6 * 2^-1
    for dtype in (torch.float16, torch.bfloat16):
        xr = F.block_inputs(64, 256, dtype, seed=2)
        packed, sf = F.mxfp4_quantize_ref(xr)
        amax = xr.double().view(64, 8, 32).abs().amax(-1)
        e = sf.double() - 127
        assert bool((6.0 * torch.exp2(e) >= amax).all())
        assert bool(((6.0 * torch.exp2(e - 1) < amax) | (amax == 0)).all())


def test_host_dequantisers_invert_the_oracle():
    import flashinfer

    m, k = 200, 160
    x = F.block_inputs(m, k, torch.float16, seed=5)
    x[7, 32:64] = 0
    packed, sf = F.mxfp4_quantize_ref(x)
    want = R.dequantize(R.e2m1_to_f64(packed), sf)
    got = flashinfer.mxfp4_dequantize_host(packed, sf)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got.double(), want)
    assert torch.equal(flashinfer.mxfp4_dequantize_host(packed, sf.reshape(-1), 32), got)
    swizzled = R.swizzle(sf, fill=0xAA)  # padding is never read
    got = flashinfer.e2m1_and_ufp8sf_scale_to_float(packed, swizzled, None, 32, 0, True)
    assert got.dtype == torch.float32 and torch.equal(got.double(), want)
    assert torch.equal(flashinfer.e2m1_and_ufp8sf_scale_to_float(packed, sf, torch.ones(1), 32, 0, False), got)
    assert torch.equal(flashinfer.mxfp4_dequantize(packed, swizzled), got)
    # the error of a block is at most 2^e: the widest gap between e2m1 neighbours is 2 (between 4 and 6), half of it 1
    e = (sf.double() - 127).unsqueeze(-1)
    assert bool(((want - x.double()).view(m, k // 32, 32).abs() <= torch.exp2(e)).all())
    with pytest.raises(ValueError, match="bytes"):
        flashinfer.e2m1_and_ufp8sf_scale_to_float(packed, swizzled[:-1], None, 32, 0, True)
    with pytest.raises(ValueError, match="bytes"):
        flashinfer.mxfp4_dequantize_host(packed, sf[:-1])
