"""CPU: flashinfer.mm_fp4 has the reference's signature and refuses everything but its MXFP4 mode before any launch,
fi_mm_mxfp4 validates on the host without a launch, and the fp64 oracle of the GPU tests (tests/mm_fp4_ref.py) agrees
with a hand-worked case and with mxfp4_dequantize_host followed by a matmul."""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

import mm_fp4_ref as M
import mx_ref as R
from flashinfer import mm_fp4  # the function under test: without it nothing here is collected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mm_fp4_signatures.json")


def test_signature_and_export_match_the_reference():
    import flashinfer

    with open(GOLDEN) as f:
        g = json.load(f)
    assert sorted(g) == ["gemm"] and sorted(g["gemm"]["functions"]) == ["mm_fp4"]
    assert g["gemm"]["top_level"] == ["mm_fp4"]
    assert flashinfer.mm_fp4 is flashinfer.gemm.mm_fp4 is mm_fp4
    ours = []
    for p in inspect.signature(mm_fp4).parameters.values():
        entry = {"name": p.name}
        if p.default is not inspect.Parameter.empty:
            entry["default"] = str(p.default) if isinstance(p.default, torch.dtype) else p.default
        ours.append(entry)
    assert ours == g["gemm"]["functions"]["mm_fp4"]
    assert [p["name"] for p in ours] == ["a", "b", "a_descale", "b_descale", "alpha", "out_dtype", "out", "block_size",
                                         "use_8x4_sf_layout", "backend", "use_nvfp4"]


def _no_library(monkeypatch):
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)


def _args(m=3, n=8, k=128, **over):
    """Arguments of a valid MXFP4 call on CPU tensors, passed as the reference's test passes them."""
    w_q = torch.zeros(n, k // 2, dtype=torch.uint8)
    w_sf = torch.zeros((n + 127) // 128 * 128, k // 32, dtype=torch.uint8)
    a = dict(a=torch.zeros(m, k // 2, dtype=torch.uint8), b=w_q.T,
             a_descale=torch.zeros((m + 127) // 128 * 128, k // 32, dtype=torch.uint8), b_descale=w_sf.T, alpha=None,
             out_dtype=torch.bfloat16, out=None, block_size=32, use_8x4_sf_layout=False, backend="cudnn", use_nvfp4=False)
    a.update(over)
    return a


def test_the_bare_call_names_nvfp4(monkeypatch):
    _no_library(monkeypatch)
    v = _args()
    with pytest.raises(NotImplementedError, match="nvfp4"):
        mm_fp4(v["a"], v["b"], v["a_descale"], v["b_descale"])
    with pytest.raises(NotImplementedError, match="nvfp4"):
        mm_fp4(**_args(use_nvfp4=True, block_size=16, use_8x4_sf_layout=True, backend="trtllm"))


REFUSALS = [
    (NotImplementedError, "8x4", dict(use_8x4_sf_layout=True)),
    (ValueError, "mxfp4 supports block_size = 32", dict(block_size=16)),
    (ValueError, "nvfp4 only supports block_size = 16", dict(use_nvfp4=True, block_size=32)),
    (ValueError, "backend", dict(backend="cublas")),
    (ValueError, "a and b must have float4_e2m1fn_x2", dict(a=torch.zeros(3, 64, dtype=torch.int8))),
    (ValueError, "a and b must have float4_e2m1fn_x2", dict(b=torch.zeros(8, 64, dtype=torch.float16).T)),
    (ValueError, "a_descale and b_descale", dict(a_descale=torch.zeros(128, 4, dtype=torch.float32))),
    (ValueError, "a_descale and b_descale", dict(b_descale=torch.zeros(128, 4, dtype=torch.int8).T)),
    (ValueError, "alpha must be a float tensor", dict(alpha=torch.ones(1, dtype=torch.float64))),
    (ValueError, "alpha must be a scalar", dict(alpha=torch.ones(2))),
    (ValueError, "Unsupported output dtype", dict(out_dtype=torch.float32)),
    (ValueError, "2d tensors", dict(a=torch.zeros(1, 3, 64, dtype=torch.uint8))),
    (ValueError, "K dimension mismatch", dict(a=torch.zeros(3, 128, dtype=torch.uint8))),
    (ValueError, "column-major", dict(b=torch.zeros(64, 8, dtype=torch.uint8))),
    (ValueError, "b_descale must be", dict(b_descale=torch.zeros(128, 4, dtype=torch.uint8))),
    (ValueError, "b_descale must be", dict(b_descale=torch.zeros(2, 64, 4, dtype=torch.uint8))),
    (ValueError, "a_descale must be contiguous", dict(a_descale=torch.zeros(4, 128, dtype=torch.uint8).T)),
    (ValueError, "Output shape mismatch", dict(out=torch.zeros(3, 16, dtype=torch.bfloat16))),
    (ValueError, "Output dtype mismatch", dict(out=torch.zeros(3, 8, dtype=torch.float16))),
    (ValueError, "out must be contiguous", dict(out=torch.zeros(8, 3, dtype=torch.bfloat16).T)),
]


@pytest.mark.parametrize("exc,match,over", REFUSALS, ids=[f"{i}-{m.split()[0]}" for i, (_, m, _) in enumerate(REFUSALS)])
def test_refusals_before_any_launch(exc, match, over, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(exc, match=match):
        mm_fp4(**_args(**over))


def test_unpadded_k_and_n_are_refused_by_name(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(NotImplementedError, match=r"k = 96.*pad"):
        mm_fp4(**_args(k=96))
    with pytest.raises(NotImplementedError, match=r"n = 12.*pad"):
        mm_fp4(**_args(n=12))


def test_accepted_spellings_reach_the_library(monkeypatch):
    """float8_e4m3fn scale bytes, a flat b_descale, every backend name, an out tensor, a one-element alpha: all pass the
    Python checks; an empty batch returns without the library."""
    _no_library(monkeypatch)
    flat = torch.zeros(128 * 4, dtype=torch.uint8)
    for over in (dict(), dict(a_descale=flat.view(torch.float8_e4m3fn)), dict(b_descale=flat), dict(backend="trtllm"),
                 dict(backend="cutlass"), dict(out=torch.zeros(3, 8, dtype=torch.bfloat16)),
                 dict(out_dtype=torch.float16, alpha=torch.ones(1, 1))):
        with pytest.raises(AssertionError, match="the library was reached"):
            mm_fp4(**_args(**over))
    empty = mm_fp4(**_args(m=0))
    assert empty.shape == (0, 8) and empty.dtype == torch.bfloat16
    given = torch.zeros(0, 8, dtype=torch.float16)
    assert mm_fp4(**_args(m=0, out=given, out_dtype=torch.float16)) is given


def test_device_op_fails_loudly_on_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU"):
        mm_fp4(**_args())


def test_symbol_is_declared_bound_and_exported(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    assert "FI_API int fi_mm_mxfp4(" in header
    assert "fi_mm_mxfp4" in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, "fi_mm_mxfp4")
    assert fi_lib.fi_mm_mxfp4.argtypes[0] is C.POINTER(_lib.fi_mm_mxfp4_params_t)
    assert [f[0] for f in _lib.fi_mm_mxfp4_params_t._fields_] == [
        "a", "b", "a_scale", "b_scale", "alpha", "d", "a_scale_bytes", "b_scale_bytes", "m", "n", "k", "d_dtype"]
    assert fi_lib.fi_abi_version() == 2  # the change is additive
    makefile = open(os.path.join(ROOT, "flashinfer-ai_amd", "csrc", "Makefile")).read()
    assert " mm_fp4" in [l for l in makefile.splitlines() if l.startswith("PLAIN_SRCS")][0]
    # the kernel switch is in the option table
    assert fi_lib.fi_set_option(b"FI_MM_FP4_KERNEL", b"2") == 0
    assert fi_lib.fi_set_option(b"FI_MM_FP4_KERNEL", None) == 0


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint8 * 4096)()
    a = (C.addressof(buf) + 63) // 64 * 64
    err = fi_lib.fi_last_error
    fn = fi_lib.fi_mm_mxfp4

    # m 130 -> 256 scale rows, n 136 -> 256 scale rows, k 256 -> 8 blocks per row
    def params(**kw):
        base = dict(a=a, b=a, a_scale=a, b_scale=a, alpha=None, d=a, a_scale_bytes=256 * 8, b_scale_bytes=256 * 8, m=130,
                    n=136, k=256, d_dtype=_lib.FI_DTYPE_BF16)
        base.update(kw)
        return _lib.fi_mm_mxfp4_params_t(**base)

    def refused(p, message):
        assert fn(C.byref(p), None) != 0 and message in err(), (message, err())

    assert fn(None, None) != 0 and b"null params" in err()
    for field in ("a", "b", "a_scale", "b_scale", "d"):
        refused(params(**{field: None}), b"null tensor")
    for field in ("m", "n", "k"):
        refused(params(**{field: -1}), b"negative")
    for k in (0, 96, 192):
        refused(params(k=k), b"multiple of 128")
    refused(params(n=12), b"n 12 must be a multiple of 8")
    for dt in (_lib.FI_DTYPE_F32, _lib.FI_DTYPE_FP8_E4M3):
        refused(params(d_dtype=dt), b"output dtype")
    for field, off in (("a", 8), ("a", 1), ("b", 8), ("b", 1), ("d", 4), ("d", 1), ("a_scale", 2), ("a_scale", 1),
                       ("b_scale", 2), ("b_scale", 1), ("alpha", 2), ("alpha", 1)):
        refused(params(**{field: a + off}), b"aligned")
    refused(params(a_scale_bytes=256 * 8 - 1), b"a_scale holds 2047 bytes, 2048 needed")
    refused(params(b_scale_bytes=256 * 8 - 1), b"b_scale holds 2047 bytes, 2048 needed")
    refused(params(m=128, a_scale_bytes=128 * 8 - 1), b"a_scale holds 1023 bytes, 1024 needed")
    refused(params(k=1 << 24, a_scale_bytes=1 << 40, b_scale_bytes=1 << 40), b"too large")
    none = dict(a=None, b=None, a_scale=None, b_scale=None, d=None)
    assert fn(C.byref(params(m=0, **none)), None) == 0
    assert fn(C.byref(params(n=0, **none)), None) == 0


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_oracle_hand_worked_2x8x128():
    m, n, k = 2, 8, 128
    a_codes = torch.zeros(m, k, dtype=torch.uint8)
    b_codes = torch.zeros(n, k, dtype=torch.uint8)
    # row 0 of a: 1.5 at k = 0 (block 0), -6 at k = 33 (block 1); row 1: 0.5 at k = 127 (block 3)
    a_codes[0, 0], a_codes[0, 33], a_codes[1, 127] = 3, 15, 1
    # row j of b: (j + 1 as a code) at k = 0, code 2 (1.0) at k = 33, code 12 (-2.0) at k = 127
    b_codes[:, 0] = torch.arange(1, 9, dtype=torch.uint8)
    b_codes[:, 33], b_codes[:, 127] = 2, 12
    sa = torch.tensor([[128, 126, 127, 127], [127, 127, 127, 130]], dtype=torch.uint8)  # 2, 1/2, 1, 1 | 1, 1, 1, 8
    sb = torch.full((n, 4), 127, dtype=torch.uint8)
    sb[:, 1] = 129  # 4
    sb[3, 3] = 125  # 1/4
    a_q, b_q = M.pack_codes(a_codes), M.pack_codes(b_codes)
    assert a_q.shape == (m, k // 2) and a_q[0, 0].item() == 3 and a_q[0, 16].item() == 15 << 4 and a_q[1, 63].item() == 1 << 4
    got = M.mm_fp4_ref(a_q, sa, b_q, sb)
    values = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0]  # codes 1..8
    want = torch.zeros(m, n, dtype=torch.float64)
    for j in range(n):
        want[0, j] = (1.5 * 2) * values[j] + (-6 * 0.5) * (1.0 * 4)
        want[1, j] = (0.5 * 8) * (-2.0 * (0.25 if j == 3 else 1.0))
    assert torch.equal(got, want)
    assert torch.equal(M.mm_fp4_ref(a_q, sa, b_q, sb, 0.25), want * 0.25)
    assert torch.equal(M.mm_fp4_ref(a_q, sa, b_q, sb, torch.tensor([0.5])), want * 0.5)
    assert torch.equal(M.abs_product_ref(a_q, sa, b_q, sb)[1], want[1].abs())


def test_oracle_agrees_with_the_host_dequantiser():
    from flashinfer import mxfp4_dequantize_host

    g = torch.Generator().manual_seed(5)
    m, n, k = 5, 16, 256
    a_q = torch.randint(0, 256, (m, k // 2), dtype=torch.uint8, generator=g)
    b_q = torch.randint(0, 256, (n, k // 2), dtype=torch.uint8, generator=g)
    sa = torch.randint(120, 135, (m, k // 32), dtype=torch.uint8, generator=g)
    sb = torch.randint(120, 135, (n, k // 32), dtype=torch.uint8, generator=g)
    want = mxfp4_dequantize_host(a_q, sa).double() @ mxfp4_dequantize_host(b_q, sb).double().T
    assert torch.equal(M.mm_fp4_ref(a_q, sa, b_q, sb), want)
    assert torch.equal(M.mm_fp4_ref(a_q, sa, b_q, sb, 0.5), want * 0.5)


def test_oracle_rounding_helpers():
    x = torch.tensor([1.0, 1.5, 3.0, 2.0 ** -20, 300.0], dtype=torch.float64)
    assert M.ulp(x, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -27, 2.0]
    assert M.ulp(x, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -24, 0.25]
    assert M.round_once(torch.tensor([1.0 + 2.0 ** -8]), torch.bfloat16).item() == 1.0  # tie to even
    with pytest.raises(AssertionError, match="two roundings"):
        M.round_once(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.bfloat16)
    assert R.BLOCK == 32
