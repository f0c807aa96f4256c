"""CPU oracle and inputs of the sigmoid routing methods, DeepSeekV3 and Llama4 (tests/test_moe_sigmoid_routing_cpu.py,
tests/test_moe_sigmoid_routing_gpu.py): plain torch, fp64, no kernel.

The oracle is written from the formulas of include/fi_mi355.h (fi_moe_route_sigmoid).  The ids it returns are compared
exactly, so the inputs are made such that no decision of the routing -- which of two experts has the larger biased
score, which of two groups the larger score -- is closer than MARGIN = 2^-16.  An f32 device evaluates sigmoid, one add
and one sum of two values below 2 to within about 2^-20, so it cannot flip a decision that the fp64 oracle makes with
that margin: 16x headroom.
"""
import torch

DEEPSEEK_V3, LLAMA4 = 2, 3
MARGIN = 2.0 ** -16


def grouped(n_group) -> bool:
    return n_group is not None and n_group > 1


def scores_ref(logits: torch.Tensor, bias: torch.Tensor):
    """(s, b) fp64 [T, E]: s = sigmoid(logit) with NaN as -inf, b = s + bias."""
    x = logits.double()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    s = torch.sigmoid(x)
    return s, s + bias.double()


def group_scores_ref(b: torch.Tensor, n_group: int) -> torch.Tensor:
    """[T, n_group]: the sum of the two largest b of experts [g * epg, (g + 1) * epg)."""
    T, E = b.shape
    return b.view(T, n_group, E // n_group).topk(2, dim=-1).values.sum(-1)


def route_sigmoid_ref(logits, bias, n_group, topk_group, top_k, scale, method):
    """logits [T, E], bias [E] (ignored by LLAMA4) -> (ids int32 [T, top_k], weights fp64 [T, top_k]).  Stable descending
    sorts: ties to the lower expert and the lower group.  An expert of a dropped group sorts behind every candidate,
    whatever its score."""
    x = logits.double()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    T, E = x.shape
    if method == LLAMA4:
        assert top_k == 1
        ids = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :1]
        return ids.to(torch.int32), torch.sigmoid(torch.gather(x, 1, ids))
    assert method == DEEPSEEK_V3
    s, b = scores_ref(logits, bias)
    ids = choose_ref(b, n_group, topk_group, top_k)
    chosen = torch.gather(s, 1, ids)
    factor = 1.0 if scale is None else float(scale)
    return ids.to(torch.int32), chosen * factor / (chosen.sum(-1, keepdim=True) + 1e-20)


def choose_ref(b: torch.Tensor, n_group, topk_group, top_k: int) -> torch.Tensor:
    """Biased scores [T, E] (any float dtype; group scores are summed in it) -> ids int64 [T, top_k]."""
    T, E = b.shape
    candidate = torch.ones(T, E, dtype=torch.bool)
    if grouped(n_group):
        assert E % n_group == 0 and E // n_group >= 2 and 1 <= topk_group <= n_group
        top_groups = torch.sort(group_scores_ref(b, n_group), dim=-1, descending=True, stable=True).indices[:, :topk_group]
        kept = torch.zeros(T, n_group, dtype=torch.bool).scatter_(1, top_groups, True)
        candidate = kept.repeat_interleave(E // n_group, dim=1)
    assert bool((candidate.sum(-1) >= top_k).all())
    by_score = torch.sort(b, dim=-1, descending=True, stable=True).indices
    dropped_last = torch.sort((~torch.gather(candidate, 1, by_score)).to(torch.int8), dim=-1, stable=True).indices
    return torch.gather(by_score, 1, dropped_last)[:, :top_k]


def min_gap(v: torch.Tensor) -> torch.Tensor:
    """[T, n >= 2] -> [T]: the smallest distance between two entries of a row."""
    s = torch.sort(v, dim=-1).values
    return (s[:, 1:] - s[:, :-1]).min(-1).values


def decision_gaps(logits: torch.Tensor, bias: torch.Tensor, n_group):
    """(smallest gap between two experts' b, smallest gap between two group scores or None), over all rows."""
    _, b = scores_ref(logits, bias)
    experts = min_gap(b).min().item()
    groups = min_gap(group_scores_ref(b, n_group)).min().item() if grouped(n_group) else None
    return experts, groups


def sigmoid_case(T: int, E: int, n_group, seed: int, dtype=torch.float32):
    """(logits [T, E] of ``dtype``, bias f32 [E], draws) for DeepSeekV3 routing with every decision gap >= MARGIN.

    A token's biased scores are a random permutation of the grid 0.25 + i * step + r * 2^-16, r random in [0, 8); the
    bias of an expert is a bf16-exact multiple of 1 / 32 in [-1 / 8, 1 / 8], so the sigmoid the logit must produce lies
    in [1 / 8, 7 / 8].  The logit is rounded to ``dtype``, the fp64 scores are recomputed from the rounded inputs, and the
    token is drawn again (seeded by the number of the draw) until all its gaps hold.  step is 2^-10 for f32 logits; a
    bf16 logit moves the sigmoid by up to 2^-10, so there the step is 2^-7 and E <= 64.  ``draws`` is the number of draws
    over all tokens."""
    step = 2.0 ** -10 if dtype == torch.float32 else 2.0 ** -7
    assert dtype in (torch.float32, torch.bfloat16) and E * step <= 0.5
    g = torch.Generator().manual_seed(seed)
    bias = torch.randint(-4, 5, (E,), generator=g).double() / 32
    assert torch.equal(bias.to(torch.bfloat16).double(), bias)
    rows, draws = [], 0
    for t in range(T):
        for attempt in range(1000):
            gt = torch.Generator().manual_seed((seed * 1000 + t) * 1000 + attempt)
            target = 0.25 + torch.randperm(E, generator=gt).double() * step \
                + torch.randint(0, 8, (E,), generator=gt).double() * 2.0 ** -16
            p = target - bias
            row = torch.log(p / (1 - p)).to(dtype).unsqueeze(0)
            draws += 1
            experts, groups = decision_gaps(row, bias, n_group)
            if experts >= MARGIN and (groups is None or groups >= MARGIN):
                break
        else:
            raise AssertionError(f"no draw of token {t} keeps the margin")
        rows.append(row)
    return torch.cat(rows), bias.float(), draws
