"""CPU: flashinfer.norm and flashinfer.activation have the reference's public surface, their host-side validation
reports without a launch, and the fp64 oracle of the GPU tests (tests/norm_ref.py) agrees with hand-worked examples
and with the f32 torch formulations the reference's own tests use."""
import ctypes as C
import inspect
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import norm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "norm_activation_signatures.json")
NORMS = ("rmsnorm", "gemma_rmsnorm")
FUSED = ("fused_add_rmsnorm", "gemma_fused_add_rmsnorm")
ACTS = ("silu_and_mul", "gelu_and_mul", "gelu_tanh_and_mul")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _params(fn):
    return [
        {"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
        for p in inspect.signature(fn).parameters.values()
    ]


def test_signatures_match_the_reference():
    import flashinfer

    g = _golden()
    assert sorted(g["norm"]["functions"]) == sorted(NORMS + FUSED)
    assert sorted(g["activation"]["functions"]) == sorted(ACTS)
    for module_name, entry in g.items():
        module = getattr(flashinfer, module_name)
        assert module.__name__ == f"flashinfer.{module_name}"
        for name, params in entry["functions"].items():
            assert _params(getattr(module, name)) == params, name
        assert sorted(entry["top_level"]) == sorted(entry["functions"])
        for name in entry["top_level"]:
            assert getattr(flashinfer, name) is getattr(module, name), name
    # the table of the change, spelled out
    for name in NORMS:
        assert _params(getattr(flashinfer, name)) == [
            {"name": "input"}, {"name": "weight"}, {"name": "eps", "default": 1e-06}, {"name": "out", "default": None},
            {"name": "enable_pdl", "default": None}]
    for name in FUSED:
        assert _params(getattr(flashinfer, name)) == [
            {"name": "input"}, {"name": "residual"}, {"name": "weight"}, {"name": "eps", "default": 1e-06},
            {"name": "enable_pdl", "default": None}]
    for name in ACTS:
        assert _params(getattr(flashinfer, name)) == [
            {"name": "input"}, {"name": "out", "default": None}, {"name": "enable_pdl", "default": None}]


def test_compat_getters_have_the_reference_ops():
    from flashinfer import activation, compat, norm

    m = compat.get_norm_module()
    assert m is norm.get_norm_module()
    for name in NORMS + FUSED:
        assert len(inspect.signature(getattr(m, name)).parameters) == 5, name
    assert list(inspect.signature(m.rmsnorm).parameters)[:3] == ["out", "input", "weight"]
    assert list(inspect.signature(m.fused_add_rmsnorm).parameters)[:3] == ["input", "residual", "weight"]
    for act in R.ACTIVATIONS:
        ns = compat.get_act_and_mul_module(act)
        assert ns is activation.get_act_and_mul_module(act)
        assert list(inspect.signature(getattr(ns, f"{act}_and_mul")).parameters) == ["out", "input", "enable_pdl"]
    with pytest.raises(ValueError, match="activation"):
        compat.get_act_and_mul_module("relu")


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_uint16 * 64)()
    a = C.addressof(buf)
    err = fi_lib.fi_last_error

    def norm_params(**kw):
        base = dict(in_=a, weight=a, out=a, batch=1, num_heads=1, hidden=8, in_stride_n=8, in_stride_h=8,
                    out_stride_n=8, out_stride_h=8, eps=1e-6, weight_bias=0.0, dtype=_lib.FI_DTYPE_F16)
        base.update(kw)
        return _lib.fi_rmsnorm_params_t(**base)

    fn = fi_lib.fi_rmsnorm
    assert fn(None, None) != 0 and b"null" in err()
    for field in ("in_", "weight", "out"):
        assert fn(C.byref(norm_params(**{field: None})), None) != 0 and b"null" in err(), field
    for hidden in (0, -3, _lib.FI_NORM_MAX_HIDDEN + 1):
        assert fn(C.byref(norm_params(hidden=hidden)), None) != 0 and b"hidden" in err(), hidden
    assert fn(C.byref(norm_params(batch=-1)), None) != 0 and b"negative" in err()
    assert fn(C.byref(norm_params(in_stride_n=7)), None) != 0 and b"stride" in err()
    assert fn(C.byref(norm_params(out_stride_n=7)), None) != 0 and b"stride" in err()
    assert fn(C.byref(norm_params(num_heads=2, in_stride_h=4)), None) != 0 and b"stride" in err()
    assert fn(C.byref(norm_params(num_heads=2, out_stride_h=4)), None) != 0 and b"stride" in err()
    for dtype in (_lib.FI_DTYPE_F32, _lib.FI_DTYPE_FP8_E4M3, 17):
        assert fn(C.byref(norm_params(dtype=dtype)), None) != 0 and b"dtype" in err(), dtype
    assert fn(C.byref(norm_params(batch=0, in_=None, weight=None, out=None)), None) == 0

    def fused_params(**kw):
        base = dict(input=a, residual=a, weight=a, batch=1, hidden=8, input_stride=8, residual_stride=8, eps=1e-6,
                    weight_bias=0.0, dtype=_lib.FI_DTYPE_BF16)
        base.update(kw)
        return _lib.fi_fused_add_rmsnorm_params_t(**base)

    fn = fi_lib.fi_fused_add_rmsnorm
    assert fn(None, None) != 0 and b"null" in err()
    for field in ("input", "residual", "weight"):
        assert fn(C.byref(fused_params(**{field: None})), None) != 0 and b"null" in err(), field
    for hidden in (0, _lib.FI_NORM_MAX_HIDDEN + 1):
        assert fn(C.byref(fused_params(hidden=hidden)), None) != 0 and b"hidden" in err(), hidden
    assert fn(C.byref(fused_params(batch=-1)), None) != 0 and b"negative" in err()
    assert fn(C.byref(fused_params(input_stride=7)), None) != 0 and b"stride" in err()
    assert fn(C.byref(fused_params(residual_stride=0)), None) != 0 and b"stride" in err()
    assert fn(C.byref(fused_params(dtype=_lib.FI_DTYPE_F32)), None) != 0 and b"dtype" in err()
    assert fn(C.byref(fused_params(batch=0, input=None, residual=None, weight=None)), None) == 0

    def act_params(**kw):
        base = dict(in_=a, out=a, tokens=1, d=8, act=_lib.FI_ACT_SILU, dtype=_lib.FI_DTYPE_F16)
        base.update(kw)
        return _lib.fi_act_and_mul_params_t(**base)

    fn = fi_lib.fi_act_and_mul
    assert fn(None, None) != 0 and b"null" in err()
    for field in ("in_", "out"):
        assert fn(C.byref(act_params(**{field: None})), None) != 0 and b"null" in err(), field
    for d in (0, -1, _lib.FI_NORM_MAX_HIDDEN + 1):
        assert fn(C.byref(act_params(d=d)), None) != 0 and b"hidden" in err(), d
    assert fn(C.byref(act_params(tokens=-1)), None) != 0 and b"negative" in err()
    assert fn(C.byref(act_params(dtype=_lib.FI_DTYPE_F32)), None) != 0 and b"dtype" in err()
    for act in (-1, 3):
        assert fn(C.byref(act_params(act=act)), None) != 0 and b"activation" in err(), act
    assert fn(C.byref(act_params(tokens=0, in_=None, out=None)), None) == 0


def test_python_side_errors():
    import flashinfer

    x = torch.zeros(3, 16, dtype=torch.float16)
    w = torch.ones(16, dtype=torch.float16)
    g = torch.zeros(3, 32, dtype=torch.float16)
    calls = [
        lambda: flashinfer.rmsnorm(x, w), lambda: flashinfer.gemma_rmsnorm(x, w),
        lambda: flashinfer.fused_add_rmsnorm(x, x.clone(), w),
        lambda: flashinfer.gemma_fused_add_rmsnorm(x, x.clone(), w),
        lambda: flashinfer.silu_and_mul(g), lambda: flashinfer.gelu_and_mul(g), lambda: flashinfer.gelu_tanh_and_mul(g),
        lambda: flashinfer.rmsnorm(x, w, out=torch.empty_like(x)),
        lambda: flashinfer.silu_and_mul(g, out=torch.empty_like(x)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()


def test_python_side_checks_run_before_any_launch(monkeypatch):
    """The argument checks sit behind the device check; let CPU tensors through to reach them (nothing is launched:
    every case must raise first)."""
    import flashinfer
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "require_gpu_tensor", lambda t, name: None)

    def no_launch():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_launch)
    x = torch.zeros(3, 16, dtype=torch.float16)
    w = torch.ones(16, dtype=torch.float16)
    for fn in (flashinfer.rmsnorm, flashinfer.gemma_rmsnorm):
        with pytest.raises(ValueError, match="weight"):
            fn(x, torch.ones(15, dtype=torch.float16))
        with pytest.raises(ValueError, match="weight"):
            fn(x, torch.ones(1, 16, dtype=torch.float16))
        with pytest.raises(ValueError, match="dtype"):
            fn(x, w.bfloat16())
        with pytest.raises(ValueError, match="dtype"):
            fn(x, w, out=torch.empty(3, 16, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="shape"):
            fn(x, w, out=torch.empty(3, 8, dtype=torch.float16))
        with pytest.raises(ValueError, match="2D"):
            fn(torch.zeros(2, 2, 2, 16, dtype=torch.float16), w)
        with pytest.raises(ValueError, match="2D"):
            fn(torch.zeros(16, dtype=torch.float16), w)
        with pytest.raises(ValueError, match="contiguous"):
            fn(torch.zeros(3, 32, dtype=torch.float16)[:, ::2], w)
    for fn in (flashinfer.fused_add_rmsnorm, flashinfer.gemma_fused_add_rmsnorm):
        with pytest.raises(ValueError, match="weight"):
            fn(x, x.clone(), torch.ones(15, dtype=torch.float16))
        with pytest.raises(ValueError, match="dtype"):
            fn(x, x.clone().bfloat16(), w)
        with pytest.raises(ValueError, match="dtype"):
            fn(x, x.clone(), w.bfloat16())
        with pytest.raises(ValueError, match="shape"):
            fn(x, torch.zeros(2, 16, dtype=torch.float16), w)
        with pytest.raises(ValueError, match="2D"):
            fn(torch.zeros(2, 3, 16, dtype=torch.float16), torch.zeros(2, 3, 16, dtype=torch.float16), w)
    for fn in (flashinfer.silu_and_mul, flashinfer.gelu_and_mul, flashinfer.gelu_tanh_and_mul):
        with pytest.raises(ValueError, match="multiple of 16 bytes"):
            fn(torch.zeros(3, 12, dtype=torch.float16))
        with pytest.raises(AssertionError):
            fn(torch.zeros(3, 32, dtype=torch.float16), out=torch.empty(3, 8, dtype=torch.float16))
        with pytest.raises(AssertionError):
            fn(torch.zeros(3, 32, dtype=torch.float16), out=torch.empty(16, dtype=torch.float16))
        with pytest.raises(AssertionError):
            fn(torch.zeros(3, 32, dtype=torch.float16), out=torch.empty(2, 16, dtype=torch.float16))
        with pytest.raises(ValueError, match="dtype"):
            fn(torch.zeros(3, 32, dtype=torch.float16), out=torch.empty(3, 16, dtype=torch.bfloat16))


def test_oracle_hand_worked_examples():
    x = torch.tensor([[3.0, 4.0]], dtype=torch.float16)
    one = torch.ones(2, dtype=torch.float16)
    # mean square 12.5 -> [3, 4] / sqrt(12.5) = [0.6, 0.8] * sqrt(2)
    want = torch.tensor([[0.6, 0.8]], dtype=torch.float64) * math.sqrt(2.0)
    assert torch.allclose(R.rmsnorm_ref(x, one, 0.0), want, rtol=1e-14, atol=0)
    assert torch.allclose(R.rmsnorm_ref(x, one, 1e-6), want, rtol=1e-7, atol=0)
    assert torch.equal(R.rmsnorm_ref(torch.zeros(2, 5, dtype=torch.bfloat16), torch.ones(5, dtype=torch.bfloat16)),
                       torch.zeros(2, 5, dtype=torch.float64))
    xr = torch.randn(4, 33, generator=torch.Generator().manual_seed(1)).half()
    assert torch.equal(R.rmsnorm_ref(xr, torch.zeros(33).half(), 1e-6, 1.0), R.rmsnorm_ref(xr, torch.ones(33).half()))
    # the fused form: [1, 2] + [2, 2] = [3, 4]; the residual is the rounded sum
    out, res = R.fused_add_rmsnorm_ref(torch.tensor([[1.0, 2.0]]).half(), torch.tensor([[2.0, 2.0]]).half(), one, 0.0)
    assert torch.allclose(out, want, rtol=1e-14, atol=0) and res.tolist() == [[3.0, 4.0]] and res.dtype == torch.float16
    # ... and the norm uses the unrounded sum: 2048 + 1 is not an f16 number (it rounds to 2048)
    out, res = R.fused_add_rmsnorm_ref(torch.tensor([[2048.0]]).half(), torch.tensor([[1.0]]).half(),
                                       torch.ones(1).half(), 0.0)
    assert res.item() == 2048.0 and out.item() == 1.0
    out, _ = R.fused_add_rmsnorm_ref(torch.tensor([[2048.0, 0.0]]).half(), torch.tensor([[1.0, 0.0]]).half(), one, 0.0)
    assert out[0, 0].item() == pytest.approx(math.sqrt(2.0), rel=1e-15)
    # activations
    gate_up = torch.tensor([[0.0, 0.0, 5.0, -7.0]], dtype=torch.float16)
    for act in R.ACTIVATIONS:
        assert R.act_and_mul_ref(gate_up, act).tolist() == [[0.0, 0.0]]  # act(0) * b = 0
        big = torch.tensor([[12.0, 40.0, 1.0, 1.0]], dtype=torch.float16)
        assert torch.allclose(R.act_and_mul_ref(big, act), torch.tensor([[12.0, 40.0]], dtype=torch.float64), rtol=1e-5)
        assert R.act_and_mul_ref(-big, act).abs().max() < 1e-3  # act(x) -> 0 for very negative x
    assert R.act_ref(torch.tensor([1.0]), "silu").item() == pytest.approx(1 / (1 + math.exp(-1)), rel=1e-15)
    assert R.act_ref(torch.tensor([1.0]), "gelu").item() == pytest.approx(0.5 * (1 + math.erf(math.sqrt(0.5))), rel=1e-15)
    assert R.act_ref(torch.tensor([1.0]), "gelu_tanh").item() == pytest.approx(
        0.5 * (1 + math.tanh(0.7978845608028654 * 1.044715)), rel=1e-15)
    assert R.half_ulp(torch.float16) == 2.0 ** -11 and R.half_ulp(torch.bfloat16) == 2.0 ** -8


def _f32_norm(x, w, eps, weight_bias):
    """The f32 formulation of the reference's tests (tests/utils/test_norm.py:24-41)."""
    x32 = x.float()
    x32 = x32 * torch.rsqrt(x32.pow(2).mean(dim=-1, keepdim=True) + eps)
    return (x32 * (weight_bias + w.float())).to(x.dtype)


def _f32_fused(x, r, w, eps, weight_bias):
    """tests/utils/test_norm.py:56-65 (the Gemma form with the same f32 add)."""
    s = x.float() + r.float()
    out = s * torch.rsqrt(s.pow(2).mean(dim=-1, keepdim=True) + eps)
    return (out * (weight_bias + w.float())).to(x.dtype), s.to(x.dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("hidden", [1, 7, 111, 500, 1024, 4096, 16384, 65536])
def test_oracle_agrees_with_the_f32_formulations(hidden, dtype):
    g = torch.Generator().manual_seed(hidden)
    x = torch.randn(5, hidden, generator=g).to(dtype)
    r = torch.randn(5, hidden, generator=g).to(dtype)
    w = torch.randn(hidden, generator=g).to(dtype)
    tol = R.tolerances(dtype)
    for weight_bias in (0.0, 1.0):
        torch.testing.assert_close(_f32_norm(x, w, 1e-6, weight_bias).double(), R.rmsnorm_ref(x, w, 1e-6, weight_bias),
                                   **tol)
        got, got_res = _f32_fused(x, r, w, 1e-6, weight_bias)
        want, want_res = R.fused_add_rmsnorm_ref(x, r, w, 1e-6, weight_bias)
        torch.testing.assert_close(got.double(), want, **tol)
        assert torch.equal(got_res, want_res)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_activation_oracle_agrees_with_torch(dtype):
    x = (torch.randn(7, 512, generator=torch.Generator().manual_seed(3)) * 3).to(dtype)
    d = x.shape[-1] // 2
    tol = R.tolerances(dtype)
    for act, fn in (("silu", F.silu), ("gelu", lambda t: F.gelu(t, approximate="none")),
                    ("gelu_tanh", lambda t: F.gelu(t, approximate="tanh"))):
        got = (fn(x[..., :d].float()) * x[..., d:].float()).to(dtype)
        torch.testing.assert_close(got.double(), R.act_and_mul_ref(x, act), **tol)
