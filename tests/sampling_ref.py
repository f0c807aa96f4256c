"""fp64 CPU statement of what flashinfer.sampling computes: sort-based masks, renormalisation, the speculative
chain's structure, and the Philox4x32-10 stream.  Plain helper for tests/test_sampling_*.py (torch on the CPU only).

The masks restate the bodies of the reference's tests (ref: tests/utils/test_sampling.py:226-490): top-k keeps
``p >= k-th largest`` (ties at the pivot included, :255-257), top-p keeps the entries whose ascending cumulative sum
exceeds ``1 - p`` (:234-237, with the slack ``eps`` the reference allows its sampler at the boundary), min-p keeps
``p >= min_p * max p`` (:298-304), "joint" is the intersection of top-k and top-p on the given probabilities
(:333-343) and "top_k_first" is top-k, renormalise, top-p (flashinfer/sampling.py:1153-1162).
"""
import math

import torch


def _per_row(x, batch, dtype):
    """scalar or 1D tensor -> [batch, 1] tensor"""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(dtype).reshape(batch, 1)
    return torch.full((batch, 1), x, dtype=dtype)


def softmax_ref(logits: torch.Tensor, temperature=1.0) -> torch.Tensor:
    x = logits.detach().cpu().double()
    return torch.softmax(x / _per_row(temperature, x.shape[0], torch.float64), dim=-1)


class RowOracle:
    """One descending fp64 sort of [batch, vocab] rows; every mask below is read off it."""

    def __init__(self, values: torch.Tensor):
        self.p = values.detach().cpu().double()
        self.sorted_desc, self.order_desc = torch.sort(self.p, dim=-1, descending=True)

    def top_k_mask(self, k) -> torch.Tensor:
        kk = _per_row(k, self.p.shape[0], torch.int64)
        return self.p >= torch.gather(self.sorted_desc, 1, kk - 1)

    def top_p_mask(self, top_p, eps: float = 0.0) -> torch.Tensor:
        pp = _per_row(top_p, self.p.shape[0], torch.float64)
        cdf = torch.cumsum(torch.flip(self.sorted_desc, dims=[-1]), dim=-1)  # ascending, inclusive
        keep_sorted = cdf > (1.0 - pp) - eps
        mask = torch.zeros_like(keep_sorted)
        mask.scatter_(1, torch.flip(self.order_desc, dims=[-1]), keep_sorted)
        return mask


def top_k_mask(probs: torch.Tensor, k) -> torch.Tensor:
    """{i : p_i >= k-th largest p} per row; works for logits too.  k: int or [batch] tensor, 1 <= k <= vocab."""
    return RowOracle(probs).top_k_mask(k)


def top_p_mask(probs: torch.Tensor, top_p, eps: float = 0.0) -> torch.Tensor:
    """entries whose ascending inclusive cumulative sum exceeds (1 - top_p) - eps, i.e. the smallest set of the
    largest entries whose mass reaches top_p (plus the slack)."""
    return RowOracle(probs).top_p_mask(top_p, eps)


def min_p_mask(probs: torch.Tensor, min_p) -> torch.Tensor:
    # the comparison the kernel has to reproduce is the f32 one: p >= f32(min_p * max p)
    p = probs.detach().cpu().float()
    mp = _per_row(min_p, p.shape[0], torch.float32)
    return p >= mp * p.max(dim=-1, keepdim=True).values


def renorm(probs: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    p = probs.detach().cpu().double() * mask
    return p / p.sum(dim=-1, keepdim=True)


def top_k_top_p_mask(probs: torch.Tensor, k, top_p, order: str, eps: float = 0.0) -> torch.Tensor:
    if order == "joint":
        return top_k_mask(probs, k) & top_p_mask(probs, top_p, eps)
    assert order == "top_k_first"
    mk = top_k_mask(probs, k)
    return mk & top_p_mask(renorm(probs, mk), top_p, eps)


def draws_needed(target: torch.Tensor, floor: int = 200_000) -> int:
    """N for the frequency check.  For N independent draws from p the expected cosine between the empirical
    frequencies and p is 1 / sqrt(1 + (1 - S) / (N S)), S = sum p^2; N = 99 (1 - S) / S puts it at 0.995."""
    s = float((target.double() ** 2).sum())
    return max(floor, math.ceil(99.0 * (1.0 - s) / s))


def cosine(counts: torch.Tensor, target: torch.Tensor) -> float:
    f = counts.double()
    t = target.double().reshape(-1)
    return float((f @ t) / (f.norm() * t.norm()))


def binomial_outliers(counts: torch.Tensor, target: torch.Tensor, n: int, sigmas: float = 6.0, min_expect: float = 50.0):
    """Tokens with N p >= min_expect whose count is more than `sigmas` standard deviations sqrt(N p (1 - p)) from
    N p; the remaining tokens are pooled into one bin that is tested the same way.  Returns a list of
    (token or 'pool', count, expected, sigma)."""
    p = target.double().reshape(-1)
    c = counts.double().reshape(-1)
    big = n * p >= min_expect
    bad = []
    for i in torch.nonzero(big).flatten().tolist():
        sd = math.sqrt(n * float(p[i]) * (1 - float(p[i])))
        if abs(float(c[i]) - n * float(p[i])) > sigmas * sd:
            bad.append((i, float(c[i]), n * float(p[i]), sd))
    pp, cc = float(p[~big].sum()), float(c[~big].sum())
    sd = math.sqrt(max(n * pp * (1 - pp), 0.0))
    if abs(cc - n * pp) > sigmas * sd + 1e-9:
        bad.append(("pool", cc, n * pp, sd))
    return bad


def chain_structure_errors(output_token_ids, draft_token_ids, emitted_num, vocab: int):
    """The reference's structural checks on a speculative chain (ref: tests/utils/test_sampling.py:546-557)."""
    out = output_token_ids.cpu()
    draft = draft_token_ids.cpu()
    errors = []
    if not bool(torch.all(out[out >= 0] < vocab)) or not bool(torch.all(out >= -1)):
        errors.append("token out of range")
    if tuple(out.shape) != (draft.shape[0], draft.shape[1] + 1):
        errors.append("shape")
    mism = out[:, :-1] != draft
    for row in range(out.shape[0]):
        idx = torch.nonzero(mism[row]).flatten()
        if len(idx) > 0:
            if not bool(torch.all(idx[1:] == idx[:-1] + 1)):
                errors.append(f"row {row}: mismatches not contiguous")
            if not bool(torch.all(out[row, idx[0] + 1:] == -1)):
                errors.append(f"row {row}: tokens after the first resampled one are not -1")
    if not bool(torch.all(emitted_num.cpu() + 1 == (out != -1).sum(dim=1))):
        errors.append("emitted + 1 != count(!= -1)")
    return errors


_M32 = 0xFFFFFFFF


def philox4x32_10(seed: int, offset: int, row: int, block: int = 0):
    """Philox4x32-10 (Salmon et al., SC'11) with key = seed and counter = (offset lo, offset hi, row, block): the four
    32-bit words the kernels draw from."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    c = [offset & _M32, (offset >> 32) & _M32, row & _M32, block & _M32]
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _M32, (p0 >> 32) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + 0x9E3779B9) & _M32
        k1 = (k1 + 0xBB67AE85) & _M32
    return c
