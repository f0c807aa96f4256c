"""The case tables of tests/variant_cases.py, checked with the oracle alone (no GPU).

A case that moves a scalar or switches a feature on proves nothing if the answer does not depend on it: a window wider
than every request, a cap the logits never reach, a theta that only turns dimensions the softmax ignores.  So for every
case and every item of it (each scalar away from its default but v_scale / bmm2_scale, which scale the output
trivially, and each enabled feature) the oracle with that one item returned to its default or switched off must move
the answer by at least 20x the bar the GPU test holds the kernels to: 20x (atol + rtol max|o|) in o, or the same with
the lse bar in the lse.  Then the tables are checked to cover what they claim, and to have no query row without a
visible key but the declared ones."""
import itertools

import pytest
import torch

import variant_cases as V

GUARD = 20.0


def _alive(lse):
    return lse > -4e4  # rows without a visible key carry the -5e4 sentinel


@pytest.mark.parametrize("case", V.ALL_CASES, ids=str)
def test_every_item_of_the_case_moves_the_oracle(case):
    o, lse = V.oracle(case)
    o_bar, lse_bar = V.bars(case)
    alive = _alive(lse)
    assert bool(alive.any())
    o_unit, lse_unit = V.bar_of(o_bar, o), V.bar_of(lse_bar, lse[alive])
    assert V.guard_items(case) or any(k in V.TRIVIAL_SCALARS for k in case.scalar), "a case that tests nothing"
    for item in V.guard_items(case):
        o2, lse2 = V.oracle(case, drop=item)
        both = alive & _alive(lse2)
        do = float((o - o2).abs().max()) / o_unit
        dl = float((lse - lse2)[both].abs().max()) / lse_unit
        print(f"{case.name}: without {item} o moves {do:.0f}x its bar, lse {dl:.0f}x")
        assert max(do, dl) >= GUARD, (case.name, item, do, dl)


@pytest.mark.parametrize("case", [c for c in V.ALL_CASES if "window" in c.features], ids=str)
def test_the_window_is_shorter_than_a_request(case):
    assert V.feature_kw(case)["window_left"] + 1 < max(case.kv_lens)
    assert any(bool((a != b).any()) for a, b in zip(V.visible(case), V.visible(case, drop="window")))


@pytest.mark.parametrize("case", [c for c in V.ALL_CASES if "mask" in c.features], ids=str)
def test_the_mask_hides_a_key_that_causal_shows_in_every_request(case):
    assert all(q > 0 for q in case.qo_lens)
    for b, (m, ql, kl) in enumerate(zip(V.visible(case, drop="window"), case.qo_lens, case.kv_lens)):
        causal = V.R.visible_mask(ql, kl, True)
        assert bool((causal & ~m).any()), (case.name, b)


@pytest.mark.parametrize("case", V.ALL_CASES, ids=str)
def test_no_dead_rows_but_the_declared(case):
    dead = sum(int((~m.any(dim=1)).sum()) for m in V.visible(case))
    assert dead == case.dead_rows
    _, lse = V.oracle(case)
    if "sinks" not in case.features:
        assert int((~_alive(lse)).any(dim=1).sum()) == dead


# ---- coverage of the tables ----------------------------------------------------------------------------------------
PAIRABLE = ("rope", "alibi", "cap", "window", "mask")


def _accepted_pairs(decode):
    feats = [f for f in PAIRABLE if not (decode and f == "mask")]
    return [p for p in itertools.combinations(feats, 2) if p != ("rope", "alibi")]  # one pos_encoding_mode


def _combos(cases):
    return [c for c in cases if len([f for f in c.features if f in PAIRABLE]) >= 2]


@pytest.mark.parametrize("decode", [True, False], ids=["decode", "prefill"])
def test_every_accepted_pair_of_features_appears_twice(decode):
    cases = _combos(V.DECODE_COMBO_CASES if decode else V.PREFILL_COMBO_CASES)
    assert all(c.is_decode == decode for c in cases)
    for a, b in _accepted_pairs(decode):
        n = sum(1 for c in cases if a in c.features and b in c.features)
        assert n >= 2, (a, b, n)


@pytest.mark.parametrize("decode", [True, False], ids=["decode", "prefill"])
def test_head_dims_dtypes_caches_and_splits_appear_with_a_combination_twice(decode):
    cases = _combos(V.DECODE_COMBO_CASES if decode else V.PREFILL_COMBO_CASES)
    counts = {}
    for c in cases:
        fp8_cache = c.kv_dtype == V.E4M3 and c.entry != "fp8_prefill"
        # decode: a plan is split when the planner is free to (the GPU test asserts it for the cases it counts here)
        split = decode_splits(c) if decode else c.split
        for key in (("d", c.d), ("dtype", c.dtype), ("e4m3 cache", fp8_cache), ("split", split)):
            counts[key] = counts.get(key, 0) + 1
    for key in [("d", d) for d in (64, 128, 256)] + [("dtype", t) for t in (V.F16, V.BF16)] + \
            [("e4m3 cache", x) for x in (False, True)] + [("split", x) for x in (False, True)]:
        assert counts.get(key, 0) >= 2, (key, counts)


def decode_splits(case):
    """True / False where the test knows the plan: disabled, or free with the whole 2049-token request to cut (a
    window shortens what the planner cuts, so those stay None)."""
    if case.split is False:
        return False
    return True if "window" not in case.features and max(case.kv_lens) >= 2049 else None


def test_the_tables_span_what_they_claim():
    dec, pre = _combos(V.DECODE_COMBO_CASES), _combos(V.PREFILL_COMBO_CASES)
    assert {c.group for c in dec} >= {1, 4, 7, 16, 20}
    assert {c.page_size for c in dec} >= {1, 5, 16} and {c.page_size for c in pre} >= {1, 5, 16}
    assert {c.layout for c in dec} == {c.layout for c in pre} == {"NHD", "HND"}
    assert any(c.hi_lo for c in pre) and any(c.split and max(c.kv_lens) >= 600 for c in pre)
    # groups above 16 with ALiBi or a cap, and head_dim 256, run the VALU kernel with a feature under both choices
    wide = [c for c in dec if c.group > 16 and {"alibi", "cap"} & set(c.features)]
    assert len(wide) >= 2 and all(V.decode_kernel(c, v) == "valu" for c in wide for v in ("default", "r1"))
    assert sum(1 for c in dec if c.d == 256) >= 2
    # every decode kernel meets a moved scalar, under the default choice or under r1
    kernels = {(V.decode_kernel(c, v), k) for c in V.SCALAR_CASES if c.entry == "batch_decode"
               for v in ("default", "r1") for k in c.scalar}
    for kern in ("valu", "mfma16", "mfma32"):
        for k in ("sm_scale", "rope_theta", "rope_scale", "q_scale", "k_scale", "v_scale"):
            assert (kern, k) in kernels, (kern, k)
    entries = {c.entry for c in V.SCALAR_CASES}
    assert entries >= {"batch_decode", "single_decode", "trtllm_decode", "paged_prefill", "ragged_prefill",
                       "single_prefill", "trtllm_context"}
    assert sum(1 for c in V.PREFILL_COMBO_CASES if c.entry == "fp8_prefill") == 3
    assert 30 <= len(V.DECODE_COMBO_CASES) <= 45 and 30 <= len(V.PREFILL_COMBO_CASES) <= 55
    for c in V.ALL_CASES:
        assert max(c.kv_lens) <= 2100 and len(c.kv_lens) <= 8


def test_oracle_cap_and_mask_helpers_restate_attention_ref():
    """fp8_attention_ref takes window_left / logits_soft_cap / custom_mask through the helpers attention_ref uses: on
    fp8 inputs with unit scales, and P left unrounded by comparing the lse only, the two agree."""
    g = torch.Generator().manual_seed(3)
    q = torch.randn(9, 4, 64, generator=g).to(V.E4M3)
    k, v = torch.randn(40, 2, 64, generator=g).to(V.E4M3), torch.randn(40, 2, 64, generator=g).to(V.E4M3)
    mask = V.make_mask((9,), (40,), seed=1).reshape(9, 40)
    one_q, one_kv = torch.ones(4), torch.ones(2)
    for kw in (dict(causal=True, window_left=5), dict(logits_soft_cap=3.0), dict(custom_mask=mask, window_left=5,
                                                                                 logits_soft_cap=3.0)):
        o8, lse8 = V.R.fp8_attention_ref(q, k, v, one_q, one_kv, one_kv, **kw)
        o, lse = V.R.attention_ref(q.float(), k.float(), v.float(), **kw)
        torch.testing.assert_close(lse8, lse, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(o8, o, rtol=5e-2, atol=5e-2)
