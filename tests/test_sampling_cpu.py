"""CPU: flashinfer.sampling has the reference's public surface, its host-side validation reports without a launch,
and the fp64 oracle of the GPU tests (tests/sampling_ref.py) agrees with hand-worked examples."""
import ctypes as C
import inspect
import json
import os

import pytest
import torch

import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampling_signatures.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_signatures_match_the_reference():
    import flashinfer
    from flashinfer import sampling

    g = _golden()
    assert len(g["functions"]) == 13
    for name, params in g["functions"].items():
        sig = inspect.signature(getattr(sampling, name))
        got = [
            {"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
            for p in sig.parameters.values()
        ]
        assert got == params, f"{name}: {got} != {params}"
    for alias, target in g["aliases"].items():
        assert getattr(sampling, alias) is getattr(sampling, target)
    for name in g["top_level"]:
        assert getattr(flashinfer, name) is getattr(sampling, name), name
    assert flashinfer.sampling is sampling


def test_compat_getter_has_the_reference_ops():
    from flashinfer import compat

    m = compat.get_sampling_module()
    expected = {
        "softmax": 5, "sampling_from_logits": 4, "sampling_from_probs": 4, "top_p_sampling_from_probs": 6,
        "top_k_sampling_from_probs": 6, "min_p_sampling_from_probs": 6, "top_k_top_p_sampling_from_probs": 8,
        "top_p_renorm_probs": 3, "top_k_renorm_probs": 3, "top_k_mask_logits": 3, "chain_speculative_sampling": 7,
    }
    for name, nargs in expected.items():
        assert len(inspect.signature(getattr(m, name)).parameters) == nargs, name


def test_host_validation_without_a_launch(fi_lib):
    from flashinfer import _lib

    buf = (C.c_float * 16)()
    out = (C.c_int32 * 4)()
    addr, oaddr = C.addressof(buf), C.addressof(out)
    for name in _lib.SAMPLING_SYMBOLS:
        fn = getattr(fi_lib, name)
        assert fn(None, None) != 0 and b"null" in fi_lib.fi_last_error()
        p = _lib.fi_sampling_params_t(probs=None, samples=oaddr, batch=1, num_rows=1, vocab=4)
        assert fn(C.byref(p), None) != 0 and b"null" in fi_lib.fi_last_error(), name
        p = _lib.fi_sampling_params_t(probs=addr, samples=oaddr, batch=1, num_rows=1, vocab=0)
        assert fn(C.byref(p), None) != 0 and b"vocab" in fi_lib.fi_last_error(), name
        p = _lib.fi_sampling_params_t(probs=addr, samples=oaddr, batch=1, num_rows=1, vocab=(1 << 22) + 1)
        assert fn(C.byref(p), None) != 0 and b"vocab" in fi_lib.fi_last_error(), name
        p = _lib.fi_sampling_params_t(probs=addr, samples=oaddr, batch=-1, num_rows=1, vocab=4)
        assert fn(C.byref(p), None) != 0 and b"negative" in fi_lib.fi_last_error(), name
        p = _lib.fi_sampling_params_t(probs=addr, samples=oaddr, batch=2, num_rows=1, vocab=4)
        assert fn(C.byref(p), None) != 0 and b"indices" in fi_lib.fi_last_error(), name
        # an empty batch is a no-op, not a launch
        p = _lib.fi_sampling_params_t(probs=None, samples=None, batch=0, num_rows=0, vocab=4)
        assert fn(C.byref(p), None) == 0, name
    for name in _lib.ROW_TRANSFORM_SYMBOLS:
        fn = getattr(fi_lib, name)
        assert fn(None, None) != 0 and b"null" in fi_lib.fi_last_error()
        p = _lib.fi_row_transform_params_t(in_=addr, out=None, batch=1, vocab=4)
        assert fn(C.byref(p), None) != 0 and b"null" in fi_lib.fi_last_error(), name
        p = _lib.fi_row_transform_params_t(in_=addr, out=addr, batch=1, vocab=0)
        assert fn(C.byref(p), None) != 0 and b"vocab" in fi_lib.fi_last_error(), name
        p = _lib.fi_row_transform_params_t(in_=None, out=None, batch=0, vocab=4)
        assert fn(C.byref(p), None) == 0, name
    fn = fi_lib.fi_chain_speculative_sampling
    assert fn(None, None) != 0 and b"null" in fi_lib.fi_last_error()
    p = _lib.fi_chain_speculative_params_t(draft_probs=addr, draft_token_ids=oaddr, target_probs=addr, output_token_ids=oaddr,
                                    output_accepted_token_num=None, output_emitted_draft_token_num=oaddr, batch=1,
                                    num_speculative_tokens=1, vocab=4)
    assert fn(C.byref(p), None) != 0 and b"null" in fi_lib.fi_last_error()
    p.output_accepted_token_num = oaddr
    p.vocab = 0
    assert fn(C.byref(p), None) != 0 and b"vocab" in fi_lib.fi_last_error()


def test_parameter_tensors_and_devices_are_checked():
    import flashinfer

    probs = torch.full((3, 8), 1 / 8)
    # the reference's three cases (flashinfer/sampling.py:497-515): 0-dim, more than 1-dim, wrong length
    for bad in (torch.tensor(0.5), torch.full((3, 1), 0.5), torch.full((4,), 0.5)):
        with pytest.raises(ValueError, match="sampling parameter|batch size mismatch"):
            flashinfer.sampling.top_p_sampling_from_probs(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.min_p_sampling_from_probs(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.top_p_renorm_probs(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.softmax(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.top_k_top_p_sampling_from_probs(probs, 2, bad)
    for bad in (torch.tensor(2), torch.full((3, 1), 2), torch.full((4,), 2)):
        with pytest.raises(ValueError):
            flashinfer.sampling.top_k_sampling_from_probs(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.top_k_renorm_probs(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.top_k_mask_logits(probs, bad)
        with pytest.raises(ValueError):
            flashinfer.sampling.top_k_top_p_sampling_from_logits(probs, bad, 0.5)
    for fn in (flashinfer.sampling.top_k_top_p_sampling_from_probs, flashinfer.sampling.top_k_top_p_sampling_from_logits):
        with pytest.raises(ValueError, match="filter_apply_order"):
            fn(probs, 2, 0.5, filter_apply_order="top_p_first")
    # CPU tensors are refused like everywhere else in the package
    s = flashinfer.sampling
    calls = [
        lambda: s.softmax(probs), lambda: s.sampling_from_probs(probs), lambda: s.sampling_from_logits(probs),
        lambda: s.top_p_sampling_from_probs(probs, 0.5), lambda: s.top_k_sampling_from_probs(probs, 2),
        lambda: s.min_p_sampling_from_probs(probs, 0.1), lambda: s.top_k_top_p_sampling_from_probs(probs, 2, 0.5),
        lambda: s.top_k_top_p_sampling_from_probs(probs, 2, 0.5, filter_apply_order="joint"),
        lambda: s.top_k_top_p_sampling_from_logits(probs, 2, 0.5), lambda: s.top_p_renorm_probs(probs, 0.5),
        lambda: s.top_k_renorm_probs(probs, 2), lambda: s.top_k_mask_logits(probs, 2),
        lambda: s.chain_speculative_sampling(torch.zeros(1, 1, 8), torch.zeros(1, 1, dtype=torch.int32),
                                             torch.zeros(1, 2, 8)),
    ]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(ValueError, match="NaN"):
        s.sampling_from_probs(torch.tensor([[float("nan"), 1.0]]), check_nan=True)
    # a CPU generator cannot drive the kernels' counter-based stream
    with pytest.raises(ValueError, match="GPU generator"):
        s.get_seed_and_offset(4, torch.Generator())


P5 = torch.tensor([[0.4, 0.3, 0.15, 0.1, 0.05]])


def test_oracle_top_k_with_a_tie_at_the_pivot():
    p = torch.tensor([[0.4, 0.2, 0.2, 0.1, 0.1]])
    assert R.top_k_mask(p, 2).tolist() == [[True, True, True, False, False]]  # the 2nd largest is 0.2, twice
    assert R.top_k_mask(p, 1).tolist() == [[True, False, False, False, False]]
    assert torch.allclose(R.renorm(p, R.top_k_mask(p, 2)), torch.tensor([[0.5, 0.25, 0.25, 0, 0]], dtype=torch.float64))
    assert R.top_k_mask(torch.cat([p, p]), torch.tensor([1, 4])).sum(dim=1).tolist() == [1, 5]


def test_oracle_top_p_cut_in_the_middle():
    # mass strictly above each entry: 0, .4, .7, .85, .95 -> 0.6 keeps the first two
    assert R.top_p_mask(P5, 0.6).tolist() == [[True, True, False, False, False]]
    assert torch.allclose(R.renorm(P5, R.top_p_mask(P5, 0.6)),
                          torch.tensor([[4 / 7, 3 / 7, 0, 0, 0]], dtype=torch.float64))
    assert R.top_p_mask(P5, 0.75).tolist() == [[True, True, True, False, False]]
    assert R.top_p_mask(P5, 1.0).all()
    # the slack widens the set only at the boundary
    assert R.top_p_mask(P5, 0.7 - 5e-5, eps=1e-4).tolist() == [[True, True, True, False, False]]


def test_oracle_min_p():
    assert R.min_p_mask(P5, 0.3).tolist() == [[True, True, True, False, False]]  # threshold 0.12
    assert R.min_p_mask(P5, 1.0).tolist() == [[True, False, False, False, False]]


def test_oracle_joint_and_top_k_first_differ():
    # top-3 is {0, 1, 2}.  joint: top-p 0.45 on the original keeps {0, 1} (mass above 1 is .4).  top_k_first:
    # renormalised top-3 is (.4706, .3529, .1765), mass above 1 is .4706 >= .45 -> {0}
    assert R.top_k_top_p_mask(P5, 3, 0.45, "joint").tolist() == [[True, True, False, False, False]]
    assert R.top_k_top_p_mask(P5, 3, 0.45, "top_k_first").tolist() == [[True, False, False, False, False]]


def test_oracle_softmax_and_statistics():
    x = torch.tensor([[0.0, float("-inf"), 0.6931471805599453]])
    assert torch.allclose(R.softmax_ref(x), torch.tensor([[1 / 3, 0.0, 2 / 3]], dtype=torch.float64))
    assert torch.allclose(R.softmax_ref(x, 0.5), torch.tensor([[0.2, 0.0, 0.8]], dtype=torch.float64))
    uniform = torch.full((1000,), 1e-3)
    assert R.draws_needed(uniform) == 200_000 and R.draws_needed(uniform, floor=0) == 98_901
    assert abs(R.cosine(torch.tensor([2, 1, 1]), torch.tensor([0.5, 0.25, 0.25])) - 1) < 1e-12
    n = 10_000
    assert R.binomial_outliers(torch.tensor([5000, 5000]), torch.tensor([0.5, 0.5]), n) == []
    assert [b[0] for b in R.binomial_outliers(torch.tensor([5400, 4600]), torch.tensor([0.5, 0.5]), n)] == [0, 1]


def test_oracle_philox_known_answers():
    # Random123's known-answer vectors for philox4x32_10 (counter, key) -> output
    assert R.philox4x32_10(0, 0, 0, 0) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert R.philox4x32_10(0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == [
        0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_oracle_chain_structure():
    draft = torch.tensor([[3, 4, 5]])
    ok = torch.tensor([[3, 9, -1, -1]])
    assert R.chain_structure_errors(ok, draft, torch.tensor([1]), 16) == []
    assert R.chain_structure_errors(torch.tensor([[3, 9, 5, 2]]), draft, torch.tensor([3]), 16)  # token after a resample
    assert R.chain_structure_errors(ok, draft, torch.tensor([2]), 16)  # wrong counter
