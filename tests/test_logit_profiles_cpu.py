"""CPU: the prescribed-logit inputs of tests/logit_profiles.py are what they claim to be, the oracle is finite on every
one of them, and the fp8 list holds only profiles the fp8 oracle can vouch for."""
import math

import pytest
import torch

import logit_profiles as LP
from oracle import attention_ref as R

D, HQ, HKV = 128, 8, 2
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}  # half an ulp, relative


def _logits(q, k):
    """fp64 logits [hq, qo, kv] in nats of the rounded tensors at sm_scale = 1 / sqrt(d)."""
    kd = k.double().repeat_interleave(q.shape[1] // k.shape[1], dim=1)
    return torch.einsum("qhd,khd->hqk", q.double(), kd) / math.sqrt(q.shape[-1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("name", LP.PROFILES_16)
def test_logits_are_the_prescription(name, d, dtype):
    """logit = a[i] g[j] + offset within: the rounding of q and of k (half an ulp each, and coherent over the dims, as
    every dim holds the same magnitude), 6 sigma of the row noise (noise d^-1/4 |g[j]|), and for the offset one common
    shift of all logits (every query and every key holds the same second half)."""
    g, a, offset, noise, _ = LP.spec(name)
    q, k, _, _ = LP.inputs(name, d, HQ, HKV, dtype)
    lg = _logits(q, k)
    j0 = int(g.abs().argmin())  # where the structured part is smallest: the offset as the rounded tensors hold it
    slack0 = (2.5 * EPS[dtype] * abs(a[0]) + 6 * noise * d ** -0.25) * abs(g[j0])
    shift = lg[0, 0, j0] - a[0] * g[j0]
    assert abs(shift - offset) <= 2.5 * EPS[dtype] * abs(offset) + slack0 + 1e-9
    want = a[None, :, None] * g[None, None, :]
    bound = 2.5 * EPS[dtype] * want.abs() + 6 * noise * d ** -0.25 * g.abs()[None, None, :] + 1e-6 * max(1.0, abs(offset))
    assert ((lg - shift - want).abs() <= bound + slack0).all()


def _row_max_after_tiles(lg):
    """[hq, qo, tiles]: the running row maximum in log2 units after each 64-key tile."""
    kv = lg.shape[-1]
    pad = torch.full((*lg.shape[:-1], -kv % LP.TILE), float("-inf"), dtype=lg.dtype)
    t = torch.cat([lg, pad], -1).reshape(*lg.shape[:-1], -1, LP.TILE).amax(-1) * LP.LOG2E
    return torch.cummax(t, dim=-1).values


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_profiles_keep_the_property_they_are_named_for(d, dtype):
    def run_max(name):
        q, k, _, _ = LP.inputs(name, d, HQ, HKV, dtype)
        return _row_max_after_tiles(_logits(q, k))

    # the rise of the row maximum from tile to tile, on the intended side of 6 (16-bit prefill) or 3 (fp8 prefill)
    for step, thr in ((5, 6), (2, 3)):
        rise = run_max(f"tile_up({step})").diff(dim=-1)
        assert (rise > 0).all() and (rise < thr).all() and (rise > thr - 1.5).all()
        assert (rise[..., :2].sum(-1) > thr).all()  # ... and two tiles together cross it: a jump every other tile
    for step, thr in ((7, 6), (4, 3)):
        assert (run_max(f"tile_up({step})").diff(dim=-1) > thr).all()
    for step, thr in ((5.9, 6), (2.5, 3)):  # the stale exponent is kept for the whole rest of the row
        m = run_max(f"step_then_flat({step})")
        assert ((m[..., 1:] - m[..., :1]) < thr).all() and ((m[..., 1:] - m[..., :1]) > thr - 0.7).all()
    for step, thr in ((6.1, 6), (3.5, 3)):  # one jump, at the second tile
        m = run_max(f"step_then_flat({step})")
        assert ((m[..., 1] - m[..., 0]) > thr).all() and (m[..., 1:].diff(dim=-1) == 0).all()
    for step in (4, 7):  # the first tile holds the maximum, later tiles fall by `step` each
        q, k, _, _ = LP.inputs(f"tile_down({step})", d, HQ, HKV, dtype)
        lg = _logits(q, k) * LP.LOG2E
        assert (run_max(f"tile_down({step})").diff(dim=-1) == 0).all()
        fall = lg[..., 0:1] - lg[..., LP.TILE::LP.TILE]
        want = step * torch.arange(1, fall.shape[-1] + 1).double()
        assert ((fall - want).abs() < 0.1 * want).all()
    # the maximum moves inside every tile of every tile size: no key is below its predecessor, every fourth key is a
    # new row maximum (bf16 holds g = 83 to 0.25, so neighbouring keys may tie; f16 ties nowhere), 0.25 nats per key
    q, k, _, _ = LP.inputs("key_ramp(0.25)", d, HQ, HKV, dtype)
    lg = _logits(q, k)
    step = lg.diff(dim=-1)
    assert (step >= 0).all() and ((lg[..., 4:] - lg[..., :-4]) > 0).all()
    assert dtype == torch.bfloat16 or (step > 0).all()
    assert (step.mean(-1) - 0.25).abs().max() < 0.25 * 0.15
    # mixed_rows: neighbouring rows ascend, descend and stay (nearly) flat
    q, k, _, _ = LP.inputs("mixed_rows", d, HQ, HKV, dtype)
    slope = _logits(q, k).diff(dim=-1).mean(-1)  # [hq, qo]
    assert (slope[:, 0::4] > 0.2).all() and (slope[:, 1::4] < -0.2).all()
    assert (slope[:, 2::4].abs() < 0.03).all() and (slope[:, 3::4].abs() < 0.03).all()
    # spikes: the spike is the row maximum, by the prescribed height, for every row (causal included)
    spikes = [("late_spike(8)", None, 8.0), ("late_spike(40)", None, 40.0), ("spike_at(63)", 63, 8.0),
              ("spike_at(64)", 64, 8.0), ("spike_at(0)", 0, 8.0), ("spike_at(chunk_end-1)", LP.CHUNK - 1, 8.0),
              ("spike_at(chunk_end)", LP.CHUNK, 8.0)]
    for name, at, height in spikes:
        for causal in (False, True):
            vis = LP.KV - LP.QO + 1 if causal else LP.KV
            at_ = vis - 1 if at is None else at
            assert at_ < vis
            q, k, _, _ = LP.inputs(name, d, HQ, HKV, dtype, causal)
            lg = _logits(q, k)
            assert (lg.argmax(-1) == at_).all()
            rest = torch.cat([lg[..., :at_], lg[..., at_ + 1:]], -1).amax(-1)
            assert ((lg[..., at_] - rest - height).abs() < 0.1 * height).all()
    # the soft cap saturates at both ends: |logit| / cap > 10, tanh = +-1 to 1e-8
    q, k, _, kw = LP.inputs("cap_saturated", d, HQ, HKV, dtype)
    lg = _logits(q, k)
    assert kw == dict(logits_soft_cap=30.0) and (lg.abs() > 300).all()
    assert (lg[..., 0::2] > 0).all() and (lg[..., 1::2] < 0).all()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_oracle_is_finite_and_every_state_is_live(dtype, causal):
    """No row's lse is at or below the "saw no key" sentinel -5e4; offset(-30000) comes closest, at about -43 281."""
    lowest = 0.0
    for name in LP.PROFILES_16:
        for d in (64, 128, 256):
            q, k, v, kw = LP.inputs(name, d, HQ, HKV, dtype, causal)
            o, lse = R.attention_ref(q.float(), k.float(), v.float(), causal=causal, **kw)
            assert torch.isfinite(o).all() and torch.isfinite(lse).all(), name
            assert (lse > R.NEG_INF_SENTINEL).all(), name
            lowest = min(lowest, lse.min().item())
        if "cap" in name:
            continue
        for heads, qo in ((16, 1), (16, 5)):
            q_nope, q_pe, ckv, kpe = LP.mla_inputs(name, heads, dtype, causal, qo=qo)
            kk = torch.cat([ckv, kpe], -1)[:, None].float()
            o, lse = R.attention_ref(torch.cat([q_nope, q_pe], -1).float(), kk, ckv[:, None].float(), causal, LP.MLA_SM)
            assert torch.isfinite(o).all() and torch.isfinite(lse).all() and (lse > R.NEG_INF_SENTINEL).all(), name
    assert -45000 < lowest < -42000


@pytest.mark.parametrize("f8", [torch.float8_e4m3fn, torch.float8_e5m2], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_fp8_list_is_within_a_quarter_of_the_fp8_bar(f8, d):
    for name, causal in LP.PROFILES_FP8:
        q8, k8, v8, sq, sk, sv = LP.fp8_inputs(name, d, f8, causal)
        o8, _ = R.fp8_attention_ref(q8, k8, v8, sq, sk, sv, causal=causal)
        deq = lambda x, s: x.float() * s.view(1, -1, 1)
        o_x, _ = R.attention_ref(deq(q8, sq), deq(k8, sk), deq(v8, sv), causal=causal)
        err = (o8 - o_x).abs().max().item()
        print(f"{name} causal={causal} d={d} {f8}: fp8 oracle vs exact {err:.2e}")
        assert err <= LP.FP8_BAR[f8] / 4, (name, causal, err)
