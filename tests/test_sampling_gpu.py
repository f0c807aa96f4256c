"""GPU: flashinfer.sampling against the fp64 CPU oracle of tests/sampling_ref.py.

Grid as the reference's tests (ref: tests/utils/test_sampling.py): batch {1, 99, 989} x vocab {111, 32000, 128256}.
Many draws come from ONE launch through ``indices`` (every row repeated), never from a loop of launches.  What is
claimed is the distribution, the support and reproducibility -- not the reference's random stream.
"""
import pytest
import torch

import sampling_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = [1, 99, 989]
VOCABS = [111, 32000, 128256]
KS = [10, 100, 500]
DRAWS_PER_LAUNCH = 16384  # support tests: every row is drawn from about DRAWS_PER_LAUNCH / batch times


def normal(std):
    def f(shape, g):
        return torch.randn(shape, generator=g) * std
    f.__name__ = f"normal({std})"
    return f


def gumbel(beta):
    # the reference's "gumbel_distribution" (tests/utils/test_sampling.py:31-38)
    def f(shape, g):
        u = torch.rand(shape, generator=g)
        return torch.log(-torch.log(u + 1e-20) + 1e-20) / beta
    f.__name__ = f"gumbel({beta})"
    return f


DISTS = [normal(1), normal(5), gumbel(0.1)]


def _gen(seed=42):
    return torch.Generator().manual_seed(seed)


def rand_probs(batch, vocab, seed=42):
    p = torch.rand(batch, vocab, generator=_gen(seed))
    return p / p.sum(dim=-1, keepdim=True)


def repeat_rows(batch, total=DRAWS_PER_LAUNCH):
    t = max(4, total // batch)
    return torch.arange(batch, dtype=torch.int32).repeat_interleave(t).to(DEV)


def assert_rows_close(got, want):
    """rtol = atol = 1e-3, the reference's bar (tests/utils/test_sampling.py:430-489); compared on the device"""
    torch.testing.assert_close(got.double(), want.to(DEV), rtol=1e-3, atol=1e-3)


def assert_in_mask(samples, indices, mask, vocab, what):
    s = samples.cpu().long()
    assert s.dtype == torch.int64 and bool(torch.all((s >= 0) & (s < vocab))), what
    rows = indices.cpu().long()
    ok = mask[rows, s]
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {len(s)} samples outside the filtered set"


def sampling():
    import flashinfer
    return flashinfer.sampling


# ---------------------------------------------------------------- 0. the generator and the random stream
def test_device_generator_state_is_seed_and_offset():
    g = torch.Generator(DEV)
    g.manual_seed(1234)
    st = g.get_state()
    assert st.numel() == 16 and st.view(torch.int64).tolist() == [1234, 0]
    seed, offset = sampling().get_seed_and_offset(5, g)
    assert (seed, offset) == (1234, 8) and g.get_state().view(torch.int64).tolist() == [1234, 8]
    torch.manual_seed(77)
    assert sampling().get_seed_and_offset(4)[0] == 77


def test_philox_stream_known_answers():
    # 4096 equal probabilities: the cumulative sums are exact, so the sample is floor(u * 4096), the top 12 bits of
    # word 0 of the Philox block keyed by (seed, offset, output row)
    probs = torch.full((1, 4096), 1.0 / 4096, device=DEV)
    g = torch.Generator(DEV)
    g.manual_seed(0x123456789ABCDEF)
    n = 257
    got = sampling().sampling_from_probs(probs, indices=torch.zeros(n, dtype=torch.int32, device=DEV), generator=g)
    offset = (n + 3) // 4 * 4
    want = [R.philox4x32_10(0x123456789ABCDEF, offset, row)[0] >> 20 for row in range(n)]
    assert got.cpu().tolist() == want


# ---------------------------------------------------------------- 1. softmax
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
def test_softmax(batch, vocab):
    s = sampling()
    for dist in DISTS:
        for neg_inf in (False, True):
            g = _gen()
            logits = dist((batch, vocab), g)
            if neg_inf:
                num_inf = int(torch.randint(0, logits.numel() - 1, (), generator=g))
                idx = torch.randperm(logits.numel(), generator=g)[:num_inf]
                logits.view(-1)[idx] = float("-inf")
            x = logits.to(DEV)
            for t in (1.0, 0.5, 0.1):
                ref_d = R.softmax_ref(logits, t).to(DEV)
                for as_tensor in (False, True):
                    temp = torch.full((batch,), t, device=DEV) if as_tensor else t
                    got = s.softmax(x, temperature=temp).double()
                    # the comparison itself runs on the device (the oracle is the CPU's); a NaN must meet a NaN
                    err = torch.where(torch.isnan(ref_d) & torch.isnan(got), torch.zeros_like(got), (got - ref_d).abs())
                    worst = float(err.max())
                    print(f"softmax b={batch} v={vocab} {dist.__name__} -inf={neg_inf} T={t} arr={as_tensor}: {worst:.3g}")
                    assert worst <= 1e-5, (dist.__name__, neg_inf, t, as_tensor, worst)
    if batch == 1:
        assert torch.equal(s.softmax(x), s.softmax(x, temperature=1.0))


# ---------------------------------------------------------------- 2. renormalisation and masking
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
def test_renorm_and_mask(batch, vocab):
    s = sampling()
    probs = rand_probs(batch, vocab)
    o = R.RowOracle(probs)
    x = probs.to(DEV)
    for p in (0.1, 0.5, 0.9, 1.0):
        assert_rows_close(s.top_p_renorm_probs(x, p), R.renorm(probs, o.top_p_mask(p)))
    assert_rows_close(s.top_p_renorm_prob(x, torch.full((batch,), 0.5, device=DEV)), R.renorm(probs, o.top_p_mask(0.5)))
    for k in [k for k in KS if k <= vocab]:
        assert_rows_close(s.top_k_renorm_probs(x, k), R.renorm(probs, o.top_k_mask(k)))
    kt = torch.randint(1, min(500, vocab) + 1, (batch,), generator=_gen(7))
    assert_rows_close(s.top_k_renorm_prob(x, kt.to(DEV)), R.renorm(probs, o.top_k_mask(kt)))
    for neg_inf in (False, True):
        g = _gen(3)
        logits = torch.randn(batch, vocab, generator=g) * 5
        if neg_inf:
            num = int(torch.randint(1, vocab * batch, (1,), generator=g))
            idx = torch.randperm(batch * vocab, generator=g)[:num]
            logits.view(-1)[idx] = float("-inf")
            logits[:, 0] = 0.0  # no row is left without a finite entry
        sm = R.softmax_ref(logits)
        osm = R.RowOracle(logits)  # the k largest logits are the k largest probabilities
        for k in [k for k in KS if k <= vocab]:
            masked = s.top_k_mask_logits(logits.to(DEV), k)
            want_mask = osm.top_k_mask(k)
            assert torch.equal(torch.isfinite(masked).cpu(), want_mask & torch.isfinite(logits)), (k, neg_inf)
            assert_rows_close(s.softmax(masked), R.renorm(sm, want_mask))


@pytest.mark.parametrize("vocab", VOCABS)
def test_top_k_renorm_keeps_ties_at_the_pivot(vocab):
    s = sampling()
    batch = 33
    # values on a grid of 64 levels: every pivot is tied many times over
    q = torch.randint(1, 65, (batch, vocab), generator=_gen(5)).float()
    probs = q / q.sum(dim=-1, keepdim=True)
    o = R.RowOracle(probs)
    for k in [1] + [k for k in KS if k <= vocab]:
        got = s.top_k_renorm_probs(probs.to(DEV), k).cpu()
        want = o.top_k_mask(k)
        assert int(want.sum()) > batch * k  # the sets really are larger than k
        assert torch.equal(got != 0, want), k


# ---------------------------------------------------------------- 3. support
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
def test_filtered_samplers_stay_in_the_filtered_set(batch, vocab):
    s = sampling()
    torch.manual_seed(42)
    probs = rand_probs(batch, vocab)
    o = R.RowOracle(probs)
    x = probs.to(DEV)
    idx = repeat_rows(batch)
    eps = 1e-4  # the reference's slack at the top-p boundary (tests/utils/test_sampling.py:231-237)
    for p in (0.1, 0.5, 0.9):
        mask = o.top_p_mask(p, eps)
        assert_in_mask(s.top_p_sampling_from_probs(x, p, indices=idx), idx, mask, vocab, f"top_p {p}")
        pt = torch.full((batch,), p, device=DEV)
        assert_in_mask(s.top_p_sampling_from_probs(x, pt, indices=idx), idx, mask, vocab, f"top_p tensor {p}")
    for k in [k for k in KS if k <= vocab]:
        mask = o.top_k_mask(k)
        assert_in_mask(s.top_k_sampling_from_probs(x, k, indices=idx), idx, mask, vocab, f"top_k {k}")
        kt = torch.randint(1, k + 1, (batch,), generator=_gen(k))  # a different k per row
        assert_in_mask(s.top_k_sampling_from_probs(x, kt.to(DEV), indices=idx), idx, o.top_k_mask(kt), vocab,
                       f"top_k variable <= {k}")
    for p in (0.05, 0.1, 0.2, 0.7, 1.0):
        mask = R.min_p_mask(probs, p)
        assert_in_mask(s.min_p_sampling_from_probs(x, p, indices=idx), idx, mask, vocab, f"min_p {p}")
        pt = torch.full((batch,), p, device=DEV)
        assert_in_mask(s.min_p_sampling_from_probs(x, pt, indices=idx), idx, mask, vocab, f"min_p tensor {p}")
    for k, p in ((int(vocab * 0.5), 0.1), (int(vocab * 0.1), 0.5)):
        mk = o.top_k_mask(k)
        masks = {"joint": mk & o.top_p_mask(p, eps), "top_k_first": mk & R.top_p_mask(R.renorm(probs, mk), p, eps)}
        for order, mask in masks.items():
            got = s.top_k_top_p_sampling_from_probs(x, k, p, indices=idx, filter_apply_order=order)
            assert_in_mask(got, idx, mask, vocab, f"{order} k={k} p={p}")
            kt, pt = torch.full((batch,), k, device=DEV), torch.full((batch,), p, device=DEV)
            got = s.top_k_top_p_sampling_from_probs(x, kt, pt, indices=idx, filter_apply_order=order)
            assert_in_mask(got, idx, mask, vocab, f"{order} tensors k={k} p={p}")


@pytest.mark.parametrize("vocab", VOCABS)
def test_per_row_parameters_follow_the_row_drawn_from(vocab):
    """Per-request tensors that differ from row to row, with `indices` that permute and repeat the rows: every
    parameter is read at the row drawn from (indices[i]).  Reading any other element leaves the filtered set of some
    row or, for the temperature, misses the oracle."""
    s = sampling()
    torch.manual_seed(42)
    batch = 37
    probs = rand_probs(batch, vocab)
    o = R.RowOracle(probs)
    x = probs.to(DEV)
    g = _gen(9)
    idx = torch.randperm(batch, generator=g).to(torch.int32).repeat_interleave(300)
    idx = idx[torch.randperm(idx.numel(), generator=g)].to(DEV)
    assert not torch.equal(idx[:batch].cpu(), torch.arange(batch, dtype=torch.int32))
    # thresholds far apart between neighbouring rows: a set read off the wrong row is much too wide or too narrow
    top_p = torch.tensor([0.02, 0.9, 0.3, 0.6])[torch.arange(batch) % 4]
    min_p = torch.tensor([1.0, 0.05, 0.7, 0.2])[torch.arange(batch) % 4]
    top_k = torch.tensor([1, min(400, vocab), 7, 60])[torch.arange(batch) % 4]
    narrow_p, narrow_k = o.top_p_mask(top_p), o.top_k_mask(top_k)
    assert int(narrow_p.sum(dim=1).max()) > 4 * int(narrow_p.sum(dim=1).min())
    assert_in_mask(s.top_p_sampling_from_probs(x, top_p.to(DEV), indices=idx), idx, o.top_p_mask(top_p, 1e-4), vocab, "top_p")
    assert_in_mask(s.min_p_sampling_from_probs(x, min_p.to(DEV), indices=idx), idx, R.min_p_mask(probs, min_p), vocab, "min_p")
    assert_in_mask(s.top_k_sampling_from_probs(x, top_k.to(DEV), indices=idx), idx, narrow_k, vocab, "top_k")
    for order in ("joint", "top_k_first"):
        mask = narrow_k & (o.top_p_mask(top_p, 1e-4) if order == "joint" else
                           R.top_p_mask(R.renorm(probs, narrow_k), top_p, 1e-4))
        got = s.top_k_top_p_sampling_from_probs(x, top_k.to(DEV), top_p.to(DEV), indices=idx, filter_apply_order=order)
        assert_in_mask(got, idx, mask, vocab, order)
    # the wide rows are really used as wide: some draw of a wide row lies outside what a narrow neighbour would allow
    wide = s.top_k_sampling_from_probs(x, top_k.to(DEV), indices=idx).cpu().long()
    rows = idx.cpu().long()
    assert bool((~o.top_k_mask(7)[rows, wide])[top_k[rows] >= 60].any())
    # renorms, the mask and softmax take no indices: row i reads element i
    assert_rows_close(s.top_p_renorm_probs(x, top_p.to(DEV)), R.renorm(probs, narrow_p))
    assert_rows_close(s.top_k_renorm_probs(x, top_k.to(DEV)), R.renorm(probs, narrow_k))
    logits = torch.randn(batch, vocab, generator=g) * 3
    temp = torch.tensor([1.0, 0.5, 0.1, 2.0])[torch.arange(batch) % 4]
    got = s.softmax(logits.to(DEV), temperature=temp.to(DEV)).double()
    assert float((got - R.softmax_ref(logits, temp).to(DEV)).abs().max()) <= 1e-5
    masked = s.top_k_mask_logits(logits.to(DEV), top_k.to(DEV))
    assert torch.equal(torch.isfinite(masked).cpu(), R.top_k_mask(logits, top_k))


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("zero_ratio", [0.5, 0.9])
def test_plain_samplers_never_return_an_impossible_token(batch, vocab, zero_ratio):
    s = sampling()
    torch.manual_seed(42)
    g = _gen()
    logits = torch.randn(batch, vocab, generator=g)
    for r in range(batch):
        logits[r, torch.randperm(vocab, generator=g)[: int(vocab * zero_ratio)]] = float("-inf")
    probs = torch.softmax(logits, dim=-1)
    idx = repeat_rows(batch)
    assert_in_mask(s.sampling_from_probs(probs.to(DEV), indices=idx), idx, probs > 0, vocab, "from_probs")
    assert_in_mask(s.sampling_from_logits(logits.to(DEV), indices=idx), idx, torch.isfinite(logits), vocab, "from_logits")


# ---------------------------------------------------------------- 4. known answers
@pytest.mark.parametrize("vocab", VOCABS)
def test_one_hot_rows_and_argmax_limits(vocab):
    s = sampling()
    torch.manual_seed(42)
    batch = 99
    hot = torch.randint(0, vocab, (batch,), generator=_gen())
    onehot = torch.zeros(batch, vocab)
    onehot[torch.arange(batch), hot] = 1.0
    x = onehot.to(DEV)
    logits = torch.full((batch, vocab), float("-inf"))
    logits[torch.arange(batch), hot] = 3.0
    want = hot.int()
    outs = {
        "from_probs": s.sampling_from_probs(x), "from_logits": s.sampling_from_logits(logits.to(DEV)),
        "top_p": s.top_p_sampling_from_probs(x, 0.9), "top_k": s.top_k_sampling_from_probs(x, 10),
        "min_p": s.min_p_sampling_from_probs(x, 0.1),
        "joint": s.top_k_top_p_sampling_from_probs(x, 10, 0.9, filter_apply_order="joint"),
        "top_k_first": s.top_k_top_p_sampling_from_probs(x, 10, 0.9),
        "logits_top_k_first": s.top_k_top_p_sampling_from_logits(logits.to(DEV), 10, 0.9),
        "logits_joint": s.top_k_top_p_sampling_from_logits(logits.to(DEV), 10, 0.9, filter_apply_order="joint"),
    }
    for name, got in outs.items():
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), name
    # argmax limits: rows without a tie at the maximum and with a maximum above 1e-6
    probs = rand_probs(batch, vocab)
    top = probs.argmax(dim=-1)
    probs[torch.arange(batch), top] *= 1.5
    probs = probs / probs.sum(dim=-1, keepdim=True)
    assert float(probs.max(dim=-1).values.min()) > 1e-6
    x = probs.to(DEV)
    want = top.int()
    assert torch.equal(s.top_k_sampling_from_probs(x, 1).cpu(), want)
    assert torch.equal(s.min_p_sampling_from_probs(x, 1.0).cpu(), want)
    assert torch.equal(s.top_p_sampling_from_probs(x, 1e-6).cpu(), want)


def test_docstring_examples_of_the_reference():
    """The worked examples of flashinfer/sampling.py that involve no random draw, to the 4 digits printed there
    (softmax :551-560, top_p_renorm_probs :1214-1223, top_k_renorm_probs :1279-1288, top_k_mask_logits :1342-1351)."""
    s = sampling()
    inf = float("inf")
    logits = torch.tensor([[0.8823, 0.9150, 0.3829, 0.9593, 0.3904], [0.6009, 0.2566, 0.7936, 0.9408, 0.1332],
                           [0.9346, 0.5936, 0.8694, 0.5677, 0.7411], [0.4294, 0.8854, 0.5739, 0.2666, 0.6274]])
    want = torch.tensor([[0.2309, 0.2385, 0.1401, 0.2493, 0.1412], [0.2019, 0.1431, 0.2448, 0.2837, 0.1265],
                         [0.2401, 0.1707, 0.2249, 0.1664, 0.1979], [0.1724, 0.2719, 0.1991, 0.1465, 0.2101]])
    assert torch.allclose(s.softmax(logits.to(DEV), temperature=1.0).cpu(), want, atol=1e-4)
    prob = torch.tensor([[0.2499, 0.2592, 0.1085, 0.2718, 0.1106], [0.2205, 0.0942, 0.2912, 0.3452, 0.0489],
                         [0.2522, 0.1602, 0.2346, 0.1532, 0.2000], [0.1543, 0.3182, 0.2062, 0.0958, 0.2255]])
    want = torch.tensor([[0.0, 0.4882, 0.0, 0.5118, 0.0], [0.0, 0.0, 0.0, 1.0, 0.0],
                         [0.5181, 0.0, 0.4819, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0, 0.0]])
    assert torch.allclose(s.top_p_renorm_probs(prob.to(DEV), 0.3).cpu(), want, atol=1e-4)
    want = torch.tensor([[0.3201, 0.3319, 0.0, 0.3480, 0.0], [0.2573, 0.0, 0.3398, 0.4028, 0.0],
                         [0.3672, 0.0, 0.3416, 0.0, 0.2912], [0.0, 0.4243, 0.2750, 0.0, 0.3007]])
    assert torch.allclose(s.top_k_renorm_probs(prob.to(DEV), 3).cpu(), want, atol=1e-4)
    logits = torch.tensor([[1.9269, 1.4873, 0.9007, -2.1055, -0.7581], [1.0783, 0.8008, 1.6806, 0.3559, -0.6866],
                           [-0.4934, 0.2415, -0.2316, 0.0418, -0.2516], [0.8599, -0.3097, -0.3957, 0.8034, -0.6216]])
    want = torch.tensor([[1.9269, 1.4873, 0.9007, -inf, -inf], [1.0783, 0.8008, 1.6806, -inf, -inf],
                         [-inf, 0.2415, -0.2316, 0.0418, -inf], [0.8599, -0.3097, -inf, 0.8034, -inf]])
    got = s.top_k_mask_logits(logits.to(DEV), 3).cpu()
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.allclose(got[~torch.isinf(got)], want[~torch.isinf(want)], atol=1e-4)


# ---------------------------------------------------------------- 5. frequencies
def _draw_counts(fn, vocab, n):
    idx = torch.zeros(n, dtype=torch.int32, device=DEV)
    samples = fn(idx)
    assert samples.shape == (n,)
    return torch.bincount(samples.cpu().long(), minlength=vocab)


def _check_cosine(counts, target, n, what):
    assert bool(torch.all(counts[target.reshape(-1) == 0] == 0)), f"{what}: a token outside the support was drawn"
    cos = R.cosine(counts, target)
    print(f"{what}: N={n} cosine={cos:.5f}")
    # expectation >= 0.995 by the choice of N (sampling_ref.draws_needed); the bar is the reference's
    assert cos > 0.99, f"{what}: cosine {cos} with N={n}"


@pytest.mark.parametrize("dist", DISTS, ids=lambda d: d.__name__)
@pytest.mark.parametrize("vocab", VOCABS)
def test_frequencies_follow_the_distribution(vocab, dist):
    s = sampling()
    torch.manual_seed(42)
    for zero_ratio in (0.0, 0.5, 0.9):
        g = _gen()
        logits = dist((1, vocab), g)
        logits[0, torch.randperm(vocab, generator=g)[: int(vocab * zero_ratio)]] = float("-inf")
        target = R.softmax_ref(logits)
        probs = target.float().to(DEV)
        n = R.draws_needed(target)
        counts = _draw_counts(lambda idx: s.sampling_from_probs(probs, indices=idx), vocab, n)
        _check_cosine(counts, target, n, f"from_probs v={vocab} {dist.__name__} zero={zero_ratio}")
        x = logits.to(DEV)
        counts = _draw_counts(lambda idx: s.sampling_from_logits(x, indices=idx), vocab, n)
        _check_cosine(counts, target, n, f"from_logits v={vocab} {dist.__name__} zero={zero_ratio}")
    logits = dist((1, vocab), _gen())
    base = R.softmax_ref(logits)
    probs = base.float()
    o = R.RowOracle(probs)
    x = probs.to(DEV)
    for k in [k for k in KS if k <= vocab]:
        target = R.renorm(probs, o.top_k_mask(k))
        n = R.draws_needed(target)
        counts = _draw_counts(lambda idx: s.top_k_sampling_from_probs(x, k, indices=idx), vocab, n)
        _check_cosine(counts, target, n, f"top_k {k} v={vocab} {dist.__name__}")
    for p in (0.1, 0.5, 0.9):
        target = R.renorm(probs, o.top_p_mask(p))
        n = R.draws_needed(target)
        counts = _draw_counts(lambda idx: s.top_p_sampling_from_probs(x, p, indices=idx), vocab, n)
        # the support is checked with the reference's slack, the frequencies against the exact set
        assert bool(torch.all(counts[~o.top_p_mask(p, 1e-4).reshape(-1)] == 0))
        cos = R.cosine(counts, target)
        print(f"top_p {p} v={vocab} {dist.__name__}: N={n} cosine={cos:.5f}")
        assert cos > 0.99, (p, cos, n)


@pytest.mark.parametrize("dist", DISTS, ids=lambda d: d.__name__)
def test_counts_are_binomial_on_a_small_vocabulary(dist):
    """vocab 111, N = 2 M: every token with N p >= 50 within 6 standard deviations of N p, the rest pooled."""
    s = sampling()
    torch.manual_seed(4242)
    vocab, n = 111, 2_000_000
    logits = dist((1, vocab), _gen(11))
    probs = R.softmax_ref(logits).float()
    o = R.RowOracle(probs)
    x, lx = probs.to(DEV), logits.to(DEV)
    cases = {
        "from_probs": (lambda idx: s.sampling_from_probs(x, indices=idx), probs.double()),
        "from_logits": (lambda idx: s.sampling_from_logits(lx, indices=idx), R.softmax_ref(logits)),
        "top_k 10": (lambda idx: s.top_k_sampling_from_probs(x, 10, indices=idx), R.renorm(probs, o.top_k_mask(10))),
        "top_k 100": (lambda idx: s.top_k_sampling_from_probs(x, 100, indices=idx), R.renorm(probs, o.top_k_mask(100))),
        "top_p 0.5": (lambda idx: s.top_p_sampling_from_probs(x, 0.5, indices=idx), R.renorm(probs, o.top_p_mask(0.5))),
        "top_p 0.9": (lambda idx: s.top_p_sampling_from_probs(x, 0.9, indices=idx), R.renorm(probs, o.top_p_mask(0.9))),
        "min_p 0.1": (lambda idx: s.min_p_sampling_from_probs(x, 0.1, indices=idx),
                      R.renorm(probs, R.min_p_mask(probs, 0.1))),
        "joint 20 0.9": (lambda idx: s.top_k_top_p_sampling_from_probs(x, 20, 0.9, indices=idx, filter_apply_order="joint"),
                         R.renorm(probs, R.top_k_top_p_mask(probs, 20, 0.9, "joint"))),
        "top_k_first 20 0.9": (lambda idx: s.top_k_top_p_sampling_from_probs(x, 20, 0.9, indices=idx),
                               R.renorm(probs, R.top_k_top_p_mask(probs, 20, 0.9, "top_k_first"))),
    }
    for name, (fn, target) in cases.items():
        target = target / target.sum()
        counts = _draw_counts(fn, vocab, n)
        bad = R.binomial_outliers(counts, target, n)
        print(f"binomial {dist.__name__} {name}: outliers {bad}")
        assert not bad, (name, bad)


# ---------------------------------------------------------------- 6. reproducibility
def test_reproducibility_and_generator_bookkeeping():
    s = sampling()
    batch, vocab = 989, 32000
    probs = rand_probs(batch, vocab).to(DEV)
    g1 = torch.Generator(DEV)
    g1.manual_seed(2024)
    g2 = g1.clone_state()
    a = s.top_p_sampling_from_probs(probs, 0.9, generator=g1)
    b = s.top_p_sampling_from_probs(probs, 0.9, generator=g2)
    assert torch.equal(a, b)
    # the reference's increments (flashinfer/sampling.py:111, 145, 186, 227, 271, 305, 444), rounded up to 4
    assert g1.get_state().view(torch.int64).tolist() == [2024, (batch * 32 + 3) // 4 * 4]
    c = s.top_p_sampling_from_probs(probs, 0.9, generator=g1)
    assert not torch.equal(a, c)
    for fn, inc in ((lambda g: s.sampling_from_probs(probs, generator=g), batch),
                    (lambda g: s.sampling_from_logits(probs, generator=g), batch * vocab),
                    (lambda g: s.top_k_sampling_from_probs(probs, 50, generator=g), batch * 32),
                    (lambda g: s.min_p_sampling_from_probs(probs, 0.1, generator=g), batch),
                    (lambda g: s.top_k_top_p_sampling_from_probs(probs, 50, 0.9, filter_apply_order="joint", generator=g),
                     batch * 32)):
        g = torch.Generator(DEV)
        g.manual_seed(5)
        fn(g)
        assert g.get_state().view(torch.int64).tolist() == [5, (inc + 3) // 4 * 4]
    # generator=None is the device's default generator: consecutive calls differ, torch.manual_seed governs
    torch.manual_seed(9)
    a = s.sampling_from_probs(probs)
    b = s.sampling_from_probs(probs)
    assert not torch.equal(a, b)
    torch.manual_seed(9)
    assert torch.equal(s.sampling_from_probs(probs), a)
    # a draw depends on (seed, offset, output row) only, not on the rest of the batch
    g = torch.Generator(DEV)
    g.manual_seed(31)
    full = s.top_k_sampling_from_probs(probs, 50, generator=g)
    g.manual_seed(31)
    g.set_state(torch.tensor([31, batch * 32 - 8 * 32], dtype=torch.int64).view(torch.uint8))
    part = s.top_k_sampling_from_probs(probs[:8], 50, generator=g)
    assert torch.equal(part, full[:8])


@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
def test_sampling_from_logits_equals_sampling_from_own_softmax(batch, vocab):
    """ref: tests/utils/test_sampling.py:361-409, with this library's softmax on both sides."""
    s = sampling()
    cases = [("top_k_first", 100, 0.1, 5.0, torch.randn), ("top_k_first", 100, 0.5, 5.0, torch.randn),
             ("joint", int(vocab * 0.5), 0.1, 5.0, torch.rand), ("joint", int(vocab * 0.1), 0.5, 5.0, torch.rand)]
    for order, k, p, scale, noise in cases:
        logits = (noise(batch, vocab, generator=_gen()) * scale).to(DEV)
        g1 = torch.Generator(DEV)
        g1.manual_seed(42)
        g2 = g1.clone_state()
        a = s.top_k_top_p_sampling_from_logits(logits, k, p, filter_apply_order=order, generator=g1)
        b = s.top_k_top_p_sampling_from_probs(s.softmax(logits), k, p, filter_apply_order=order, generator=g2)
        diff = int((a != b).sum())
        print(f"alignment b={batch} v={vocab} {order} k={k} p={p}: {diff} of {batch} differ")
        assert diff == 0, (order, k, p, diff)


# ---------------------------------------------------------------- 7. chain speculative sampling
@pytest.mark.parametrize("onehot_target", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5, 7])
@pytest.mark.parametrize("vocab", VOCABS)
@pytest.mark.parametrize("batch", BATCHES)
def test_chain_speculative_sampling(batch, vocab, n, onehot_target):
    """ref: tests/utils/test_sampling.py:492-557 (inputs made on the device, as there)."""
    s = sampling()
    torch.manual_seed(42)
    draft = torch.rand(batch, n, vocab, device=DEV)
    draft = draft / draft.sum(dim=-1, keepdim=True)
    draft_ids = torch.randint(vocab, (batch, n), device=DEV)
    if onehot_target:
        target_ids = torch.randint(vocab, (batch, n + 1), device=DEV)
        target_ids[..., :n] = draft_ids
        target = torch.zeros(batch, n + 1, vocab, device=DEV)
        target.scatter_(2, target_ids.unsqueeze(-1), 1)
    else:
        target = torch.rand(batch, n + 1, vocab, device=DEV)
        target = target / target.sum(dim=-1, keepdim=True)
    accepted = torch.zeros(batch, dtype=torch.int32, device=DEV)
    emitted = torch.zeros(batch, dtype=torch.int32, device=DEV)
    out, acc, emi = s.chain_speculative_sampling(draft, draft_ids, target, accepted, emitted)
    assert acc is accepted and emi is emitted and out.dtype == torch.int32
    if onehot_target:
        assert torch.equal(out.long(), target_ids)
        assert bool(torch.all(emitted == n)) and bool(torch.all(accepted == n))
    else:
        assert R.chain_structure_errors(out, draft_ids, emitted, vocab) == []
        assert bool(torch.all(accepted >= emitted)) and bool(torch.all(accepted <= n))
    # counters accumulate across calls
    first, first_accepted = emitted.clone(), accepted.clone()
    out2, _, _ = s.chain_speculative_sampling(draft, draft_ids, target, accepted, emitted)
    assert torch.equal(emitted - first + 1, (out2 != -1).sum(dim=1).int())
    delta = accepted - first_accepted
    assert bool(torch.all(delta >= emitted - first)) and bool(torch.all(delta <= n))


@pytest.mark.parametrize("vocab", VOCABS)
def test_chain_accepts_everything_when_draft_equals_target(vocab):
    s = sampling()
    torch.manual_seed(1)
    batch, n = 99, 5
    target = torch.rand(batch, n + 1, vocab, device=DEV)
    target[..., : vocab // 2] = 0  # the bonus token must come from the other half
    target = target / target.sum(dim=-1, keepdim=True)
    draft = target[:, :n].contiguous()
    draft_ids = torch.multinomial(draft.reshape(-1, vocab), 1).reshape(batch, n)
    out, acc, emi = s.chain_speculative_sampling(draft, draft_ids, target)
    assert torch.equal(out[:, :n].long(), draft_ids)
    assert bool(torch.all(acc == n)) and bool(torch.all(emi == n))
    bonus = out[:, n].long()
    assert bool(torch.all(target[torch.arange(batch), n, bonus] > 0))


# ---------------------------------------------------------------- 8. degenerate rows have a defined result
def test_degenerate_rows():
    s = sampling()
    torch.manual_seed(0)
    vocab = 1000
    zeros = torch.zeros(3, vocab, device=DEV)
    probs = rand_probs(3, vocab).to(DEV)
    top = probs.argmax(dim=-1).int().cpu()
    # a row without a positive entry gives token 0 from every sampler
    for got in (s.sampling_from_probs(zeros), s.top_k_sampling_from_probs(zeros, 5), s.top_p_sampling_from_probs(zeros, 0.5),
                s.min_p_sampling_from_probs(zeros, 0.5), s.top_k_top_p_sampling_from_probs(zeros, 5, 0.5),
                s.top_k_top_p_sampling_from_probs(zeros, 5, 0.5, filter_apply_order="joint"),
                s.sampling_from_logits(torch.full((3, vocab), float("-inf"), device=DEV))):
        assert got.cpu().tolist() == [0, 0, 0]
    # top_k > vocab and top_k = 0 switch the filter off
    for k in (vocab + 1, 0):
        got = s.top_k_sampling_from_probs(probs, k).cpu()
        assert bool(torch.all((got >= 0) & (got < vocab)))
        assert torch.allclose(s.top_k_renorm_probs(probs, k), probs, atol=1e-6)
        assert torch.equal(s.top_k_mask_logits(probs, k), probs)
    # top_p = 0 keeps the maximum only
    assert torch.equal(s.top_p_sampling_from_probs(probs, 0.0).cpu(), top)
    assert torch.equal(s.top_k_top_p_sampling_from_probs(probs, 0, 0.0, filter_apply_order="joint").cpu(), top)
    r = s.top_p_renorm_probs(probs, 0.0).cpu()
    assert torch.equal((r != 0).sum(dim=1), torch.ones(3, dtype=torch.long)) and torch.equal(r.argmax(dim=-1).int(), top)
    # a NaN entry is never drawn and does not stop a call
    bad = probs.clone()
    bad[:, 7] = float("nan")
    for got in (s.sampling_from_probs(bad), s.top_k_sampling_from_probs(bad, 5), s.top_p_sampling_from_probs(bad, 0.5),
                s.min_p_sampling_from_probs(bad, 0.1)):
        got = got.cpu()
        assert bool(torch.all((got >= 0) & (got < vocab) & (got != 7)))


# ---------------------------------------------------------------- 9. check_nan
def test_check_nan_raises():
    s = sampling()
    probs = rand_probs(4, 128).to(DEV)
    probs[2, 5] = float("nan")
    for call in (lambda: s.sampling_from_probs(probs, check_nan=True),
                 lambda: s.top_p_sampling_from_probs(probs, 0.5, check_nan=True),
                 lambda: s.top_k_sampling_from_probs(probs, 5, check_nan=True),
                 lambda: s.min_p_sampling_from_probs(probs, 0.1, check_nan=True),
                 lambda: s.top_k_top_p_sampling_from_probs(probs, 5, 0.5, filter_apply_order="joint", check_nan=True)):
        with pytest.raises(ValueError, match="Input probs contains NaN."):
            call()
    with pytest.raises(ValueError, match="Input logits contains NaN."):
        s.sampling_from_logits(probs, check_nan=True)
