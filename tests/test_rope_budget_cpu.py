"""CPU study behind the angle budget of oracle/rope_ref.py (ANGLE_BUDGET_A, ANGLE_BUDGET_B).

The long-position RoPE test allows the kernel, per element, hypot(x0, x1) * delta_theta on top of the usual
tolerance, delta_theta(p, m) = p f_m (A |log2 b_m| + B) 2^-23.  A and B are not fitted to the kernel: they bound the
relative frequency error of an f32 restatement of the reference's formula (include/flashinfer/pos_enc.cuh:481-493)

    freq_m = exp2(log2(1 / theta) * (2 m / rot)),  smooth = clamp(freq a + b, 0, 1),
    freq_m <- (1 - smooth) (freq_m / scale) + smooth freq_m

with every step in numpy float32, and the results of log2 and exp2 each pushed by n ulp (random sign per element)
to stand for hardware transcendentals that are good to n ulp.  The f64 oracle is the truth.

Asserted: the worst error / budget is <= 0.65 with 1 ulp pushes (the margin the budget keeps over 1-ulp hardware) and
<= 1.0 with 2 ulp pushes (the hardware quality the budget is sized for).
"""
import numpy as np
import pytest
import torch

from oracle import rope_ref as RR

ROTS = [32, 64, 128, 256]
# (name, theta, scale, llama-3.1 blend)
FORMS = [("plain-1e4", 1e4, 1.0, False), ("llama31-5e5", 5e5, 8.0, True), ("plain-1e6", 1e6, 1.0, False)]
DRAWS = 50


def _push(x, n, rng):
    """x moved by n ulp, sign drawn per element (float32 in, float32 out)."""
    if n == 0:
        return x
    up = rng.integers(0, 2, size=x.shape).astype(bool)
    for _ in range(n):
        x = np.where(up, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))).astype(np.float32)
    return x


def f32_freqs(rot, theta, scale, smooth_a, smooth_b, n, rng):
    """The f32 pipeline, per pair m [rot // 2]."""
    m = np.arange(rot // 2)
    rcp_theta = np.full(m.shape, 1.0 / theta, dtype=np.float32)
    lg = _push(np.log2(rcp_theta).astype(np.float32), n, rng)
    y = (2 * m).astype(np.float32) / np.float32(rot)
    freq = _push(np.exp2((y * lg).astype(np.float32)).astype(np.float32), n, rng)
    smooth = np.clip(freq * np.float32(smooth_a) + np.float32(smooth_b), np.float32(0), np.float32(1)).astype(np.float32)
    rcp_scale = np.float32(1.0 / scale)
    return ((np.float32(1) - smooth) * (freq * rcp_scale) + smooth * freq).astype(np.float32)


def worst_ratio(rot, theta, scale, llama31, n, seed):
    rng = np.random.default_rng(seed)
    a, b = RR.llama31_smooth() if llama31 else (0.0, 0.0)
    want = RR.rope_freqs(rot, True, scale, theta, a, b)[0::2].numpy()  # one value per pair, f64
    budget = RR.freq_rel_budget(rot, theta).numpy()
    worst = 0.0
    for _ in range(DRAWS if n else 1):
        got = f32_freqs(rot, theta, scale, a, b, n, rng).astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / want / budget).max()))
    return worst


@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_budget_covers_f32_pipeline_with_perturbed_transcendentals(form, rot):
    _, theta, scale, llama31 = form
    seed = rot * 7 + int(theta) % 1000
    r0, r1, r2 = (worst_ratio(rot, theta, scale, llama31, n, seed + n) for n in (0, 1, 2))
    print(f"{form[0]} rot={rot}: worst relative frequency error / budget = {r0:.3f} (exact f32), {r1:.3f} (1 ulp), "
          f"{r2:.3f} (2 ulp)")
    assert r1 <= 0.65, f"1-ulp envelope uses {r1:.3f} of the budget, more than 0.65"
    assert r2 <= 1.0, f"2-ulp envelope uses {r2:.3f} of the budget"


def test_budget_layout_matches_the_oracle_pairing():
    """angle_budget puts delta_theta(p, m) at the elements of pair m for either pairing."""
    rot, theta = 64, 1e4
    pos = torch.tensor([1, 1000, 131071])
    a, b = RR.llama31_smooth()
    for interleave in (False, True):
        got = RR.angle_budget(pos, rot, interleave, 8.0, theta, a, b)
        assert got.shape == (3, rot) and got.dtype == torch.float64
        m = RR.pair_index(rot, interleave)
        f = RR.rope_freqs(rot, interleave, 8.0, theta, a, b)
        log2_b = (2.0 * m.double() / rot) * np.log2(theta)
        want = pos.double()[:, None] * f[None] * ((RR.ANGLE_BUDGET_A * log2_b + RR.ANGLE_BUDGET_B) * 2.0 ** -23)[None]
        torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
        # partners share one allowance
        x = torch.arange(rot, dtype=torch.float64)[None]
        h = RR.pair_hypot(x, rot, interleave)
        p0 = torch.nonzero(m == 5).flatten()
        assert len(p0) == 2 and h[0, p0[0]] == h[0, p0[1]] == torch.hypot(x[0, p0[0]], x[0, p0[1]])
        assert got[2, p0[0]] == got[2, p0[1]]
