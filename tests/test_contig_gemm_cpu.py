"""Host side of flashinfer.gemm.group_deepgemm_fp8_nt_groupwise: the reference's signature, the refusals that must come
before any launch, and the empty problem."""
import inspect

import pytest
import torch

E5M2, E4M3 = torch.float8_e5m2, torch.float8_e4m3fn


def valid_call():
    return dict(a=torch.zeros(8, 256).to(E4M3), b=torch.zeros(2, 128, 256).to(E4M3), a_scale=torch.ones(8, 2),
                b_scale=torch.ones(2, 1, 2), m_indices=torch.zeros(8, dtype=torch.int32))


def test_signature_is_the_reference_one():
    import flashinfer.gemm

    params = inspect.signature(flashinfer.gemm.group_deepgemm_fp8_nt_groupwise).parameters
    assert [(n, p.default) for n, p in params.items()] == [
        ("a", inspect.Parameter.empty), ("b", inspect.Parameter.empty), ("a_scale", inspect.Parameter.empty),
        ("b_scale", inspect.Parameter.empty), ("m_indices", inspect.Parameter.empty),
        ("scale_granularity_mnk", (1, 128, 128)), ("out", None), ("out_dtype", None)]


REFUSALS = {  # name: (changes to the arguments of a valid (m 8, G 2, n 128, k 256) call, exception)
    "rank": (dict(a=torch.zeros(2, 8, 256).to(E4M3)), ValueError),
    "k_mismatch": (dict(b=torch.zeros(2, 128, 128).to(E4M3)), ValueError),
    "n_not_128": (dict(b=torch.zeros(2, 64, 256).to(E4M3), b_scale=torch.ones(2, 1, 2)), ValueError),
    "k_not_128": (dict(a=torch.zeros(8, 192).to(E4M3), b=torch.zeros(2, 128, 192).to(E4M3)), ValueError),
    "a_scale_shape": (dict(a_scale=torch.ones(2, 8)), ValueError),
    "operand_dtype": (dict(a=torch.zeros(8, 256, dtype=torch.float16)), ValueError),
    "scale_dtype": (dict(a_scale=torch.ones(8, 2, dtype=torch.float16)), ValueError),
    "out_dtype": (dict(out_dtype=torch.float32), ValueError),
    "out_non_contiguous": (dict(out=torch.zeros(128, 8, dtype=torch.bfloat16).t()), ValueError),
    "m_indices_dtype": (dict(m_indices=torch.zeros(8, dtype=torch.int64)), ValueError),
    "scale_granularity_mnk": (dict(scale_granularity_mnk=(128, 128, 128)), NotImplementedError),
    "cpu_tensors": (dict(), RuntimeError),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(name, monkeypatch):
    import flashinfer.gemm
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    change, exc = REFUSALS[name]
    match = "scale_granularity_mnk|float8_e5m2" if exc is NotImplementedError else "GPU" if exc is RuntimeError else None
    with pytest.raises(exc, match=match):
        flashinfer.gemm.group_deepgemm_fp8_nt_groupwise(**{**valid_call(), **change})


def test_no_rows_is_an_empty_result(monkeypatch):
    import flashinfer.gemm
    from flashinfer import _lib

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    kw = valid_call()
    kw.update(a=kw["a"][:0], a_scale=kw["a_scale"][:0], m_indices=kw["m_indices"][:0])
    out = flashinfer.gemm.group_deepgemm_fp8_nt_groupwise(**kw, out_dtype=torch.float16)
    assert out.shape == (0, 128) and out.dtype == torch.float16
