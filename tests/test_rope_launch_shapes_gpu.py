"""GPU: the standalone RoPE kernel (csrc/rope.hip) at the sizes where its launch changes, and at long positions.

rope_fill_and_launch picks heads_per_thread = min(heads, max(1, heads * nnz * tph / 65536)) (tph = threads per token)
and caps the grid at 256 * 16 workgroups of 256 threads, with a grid-stride loop behind the cap.  Every shape below
is the smallest that reaches one regime; next to it stands the arithmetic, and an assert recomputes the regime from
the launcher's constants as of this commit, so that retuning them fails the test instead of silently losing coverage.

Outputs are always visible when unwritten: the in-place forms (where a skipped row keeps its input, which the oracle
comparison and `assert_every_row_changed` catch since all positions are >= 1), or outputs pre-filled with NaN.
Tolerances are those of tests/test_rope_gpu.py.
"""
import pytest
import torch

from attn_inputs import append_problem
from oracle import rope_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: dict(rtol=1e-3, atol=1e-3), torch.bfloat16: dict(rtol=2.0 ** -7, atol=8e-3)}  # test_rope_gpu.py

# csrc/rope.hip, rope_fill_and_launch, as of this commit
ROPE_SPLIT_THREADS = 65536          # heads_per_thread = min(heads, max(1, heads * nnz * tph / 65536))
ROPE_GRID_ITEMS = 256 * 16 * 256    # grid cap 256 * 16 workgroups x 256 threads = 1,048,576 items per pass


def threads_per_token(head_dim, rotary_dim):
    cph, rot_chunks = head_dim // 8, rotary_dim // 8
    return rot_chunks // 2 + (cph - rot_chunks + 1) // 2


def heads_per_thread(hq, hk, nnz, head_dim, rotary_dim):
    heads = hq + hk
    return min(heads, max(1, heads * nnz * threads_per_token(head_dim, rotary_dim) // ROPE_SPLIT_THREADS))


def launch_items(hq, hk, nnz, head_dim, rotary_dim):
    hpt = heads_per_thread(hq, hk, nnz, head_dim, rotary_dim)
    return nnz * threads_per_token(head_dim, rotary_dim) * (-(-(hq + hk) // hpt))


def packed_qkv(nnz, hq, hk, d, dtype, seed):
    """(qkv, q view, k view): q and k are strided views of one packed [nnz, (hq + 2 hk) d] tensor."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    qkv = torch.randn(nnz, (hq + 2 * hk) * d, device=DEV, generator=g).to(dtype)
    return (qkv,) + qk_views(qkv, hq, hk, d)


def qk_views(qkv, hq, hk, d):
    nnz = qkv.shape[0]
    return qkv[:, : hq * d].view(nnz, hq, d), qkv[:, hq * d: (hq + hk) * d].view(nnz, hk, d)


def random_positions(nnz, seed, lo=1, hi=4000):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (nnz,), generator=g, dtype=torch.int32)


def bits(x):
    return x.contiguous().view(torch.int16)


def assert_every_row_changed(after, before):
    """in place: a row the kernel skipped still holds its input (positions >= 1 rotate every row visibly)"""
    same = (bits(after) == bits(before)).flatten(1).all(dim=1)
    assert not bool(same.any()), f"{int(same.sum())} rows were left as they were, first {int(same.nonzero()[0])}"


def assert_matches_oracle(q_got, k_got, q_in, k_in, pos, rot, interleave, dtype, scale=1.0, theta=1e4, a=0.0, b=0.0,
                          what=""):
    q_ref, k_ref = RR.apply_rope_pos_ids_ref(q_in.float().cpu(), k_in.float().cpu(), pos.cpu(), rot, interleave,
                                             scale, theta, a, b)
    torch.testing.assert_close(q_got.float().cpu(), q_ref.float(), **TOL[dtype], msg=lambda m: f"{what} q: {m}")
    torch.testing.assert_close(k_got.float().cpu(), k_ref.float(), **TOL[dtype], msg=lambda m: f"{what} k: {m}")


def run_inplace_and_check(hq, hk, nnz, d, rot, dtype, interleave, seed):
    import flashinfer

    qkv, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed)
    qkv0 = qkv.clone()
    q0, k0 = qk_views(qkv0, hq, hk, d)
    pos = random_positions(nnz, seed + 1).to(DEV)
    flashinfer.apply_rope_pos_ids_inplace(q, k, pos, rotary_dim=rot, interleave=interleave)
    assert_matches_oracle(q, k, q0, k0, pos, rot, interleave, dtype)
    assert_every_row_changed(q, q0)
    assert_every_row_changed(k, k0)
    assert torch.equal(bits(qkv[:, (hq + hk) * d:]), bits(qkv0[:, (hq + hk) * d:])), "the v columns were written"
    if rot < d:
        assert torch.equal(bits(q[..., rot:]), bits(q0[..., rot:])) and torch.equal(bits(k[..., rot:]), bits(k0[..., rot:]))


def rope_out_of_place(q, k, pos, hq, hk, d, **kw):
    """apply_rope_pos_ids into outputs that were filled with NaN first: the public wrapper allocates its outputs
    itself, so the same launch is also made through the wrapper's own helper on NaN-filled views of a packed buffer,
    and the two must agree bit for bit.  Returns (q_out, k_out) of the pre-filled run."""
    import flashinfer
    from flashinfer import rope as rope_mod

    out = torch.full((q.shape[0], (hq + 2 * hk) * d), float("nan"), dtype=q.dtype, device=DEV)
    q_out, k_out = qk_views(out, hq, hk, d)
    rope_mod._run(q, k, q_out, k_out, pos, kw.get("rotary_dim"), kw.get("interleave", False),
                  kw.get("rope_scale", 1.0), kw.get("rope_theta", 1e4))
    assert not bool(torch.isnan(q_out).any() or torch.isnan(k_out).any()), "part of the output was never written"
    assert bool(torch.isnan(out[:, (hq + hk) * d:]).all()), "the launch wrote outside q_out / k_out"
    q_pub, k_pub = flashinfer.apply_rope_pos_ids(q, k, pos, **kw)
    assert torch.equal(bits(q_pub), bits(q_out)) and torch.equal(bits(k_pub), bits(k_out))
    return q_out, k_out


# ---- A1 / A2: one thread walks several heads ------------------------------------------------------------------------

@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_partial_head_groups_straddling_q_and_k(dtype, interleave):
    # head_dim 128, full rotation: tph = 8.  10 heads * 3300 tokens * 8 / 65536 = 4.03 -> heads_per_thread 4:
    # groups {q0-3}, {q4, q5, q6, k0} (straddles q/k), {k1, k2} (short last group).  ~8 MB.
    hq, hk, nnz, d = 7, 3, 3300, 128
    assert threads_per_token(d, d) == 8
    hpt = heads_per_thread(hq, hk, nnz, d, d)
    assert hpt == 4 and (hq + hk) % hpt != 0 and hq % hpt != 0, hpt
    assert launch_items(hq, hk, nnz, d, d) <= ROPE_GRID_ITEMS  # one pass: this shape isolates the head grouping
    run_inplace_and_check(hq, hk, nnz, d, d, dtype, interleave, seed=10)


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hq,hk,full_trips,remainder", [(4, 1, 1, 1), (9, 2, 2, 3)])
def test_all_heads_in_one_thread(hq, hk, full_trips, remainder, dtype, interleave):
    # nnz * tph = 8200 * 8 = 65600 >= 65536 -> heads * 65600 / 65536 >= heads -> heads_per_thread = heads:
    # 5 heads = one unrolled-by-4 trip + 1 remainder; 11 heads = two unrolled trips + 3 remainder
    nnz, d = 8200, 128
    assert nnz * threads_per_token(d, d) >= ROPE_SPLIT_THREADS
    hpt = heads_per_thread(hq, hk, nnz, d, d)
    assert hpt == hq + hk and divmod(hpt, 4) == (full_trips, remainder), hpt
    run_inplace_and_check(hq, hk, nnz, d, d, dtype, interleave, seed=20 + hq)


# ---- A3: the grid-stride loop takes a second pass -------------------------------------------------------------------

@pytest.mark.parametrize("interleave", [False, True])
def test_grid_stride_second_pass(interleave):
    """head_dim 256: tph = 16; 1 + 1 heads, 65600 tokens: heads_per_thread 2, one head group, 65600 * 16 = 1,049,600
    items against 1,048,576 per pass -> the last 1024 items (tokens 65536 ... 65599) belong to the second pass.
    ~67 MB of q + k.  The f64 oracle runs on a subset of rows; the whole output is checked on the GPU for what any
    rotation keeps, the norm of every pair."""
    import flashinfer

    dtype = torch.float16
    hq, hk, nnz, d = 1, 1, 65600, 256
    assert threads_per_token(d, d) == 16 and heads_per_thread(hq, hk, nnz, d, d) == 2
    items = launch_items(hq, hk, nnz, d, d)
    assert items == 1_049_600 and ROPE_GRID_ITEMS < items <= 2 * ROPE_GRID_ITEMS, items
    first_second_pass_row = ROPE_GRID_ITEMS // threads_per_token(d, d)
    assert first_second_pass_row == 65536 < nnz
    qkv, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed=30)
    qkv0 = qkv.clone()
    q0, k0 = qk_views(qkv0, hq, hk, d)
    pos = random_positions(nnz, 31).to(DEV)
    flashinfer.apply_rope_pos_ids_inplace(q, k, pos, interleave=interleave)
    rows = torch.cat((torch.arange(256), torch.arange(first_second_pass_row - 64, nnz),
                      torch.randperm(nnz, generator=torch.Generator().manual_seed(32))[:2048])).unique().to(DEV)
    assert_matches_oracle(q[rows], k[rows], q0[rows], k0[rows], pos[rows], d, interleave, dtype)
    assert_every_row_changed(q, q0)
    assert_every_row_changed(k, k0)
    assert torch.equal(bits(qkv[:, (hq + hk) * d:]), bits(qkv0[:, (hq + hk) * d:])), "the v columns were written"
    rtol, atol = TOL[dtype]["rtol"], TOL[dtype]["atol"]
    for got, src in ((q, q0), (k, k0)):
        n_got = RR.pair_norm_sq(got.float(), d, interleave)
        n_src = RR.pair_norm_sq(src.float(), d, interleave)
        bad = (n_got - n_src).abs() > 2 * rtol * n_src + atol ** 2
        assert not bool(bad.any()), f"{int(bad.sum())} pairs changed their norm, first at {bad.nonzero()[0].tolist()}"


# ---- A4: an odd number of pass-through chunks -----------------------------------------------------------------------

@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,rot,nnz", [(72, 64, 45), (40, 32, 45), (72, 64, 3300)])
def test_odd_pass_through_chunk_count(d, rot, nnz, dtype, interleave):
    """(72, 64): 9 chunks per head, 8 rotary -> 1 pass-through chunk, tph = 4 + 1; (40, 32): 5 chunks, 4 rotary ->
    1 pass-through chunk, tph = 2 + 1.  The pass-through thread's second chunk (c0 + 1) lies past the row.
    nnz 45: heads_per_thread 1.  (72, 64) at nnz 3300: 10 * 3300 * 5 / 65536 = 2.5 -> heads_per_thread 2, groups
    {q0,q1} {q2,q3} {q4,q5} {q6,k0} {k1,k2}."""
    hq, hk = (7, 3) if nnz == 3300 else (3, 2)
    pass_chunks = d // 8 - rot // 8
    assert pass_chunks % 2 == 1 and threads_per_token(d, rot) == rot // 16 + 1
    hpt = heads_per_thread(hq, hk, nnz, d, rot)
    assert hpt == (2 if nnz == 3300 else 1), hpt
    run_inplace_and_check(hq, hk, nnz, d, rot, dtype, interleave, seed=40 + d)
    # out of place: the pass-through part has to be copied, bit for bit
    _, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed=41 + d)
    pos = random_positions(nnz, 42).to(DEV)
    q_out, k_out = rope_out_of_place(q, k, pos, hq, hk, d, rotary_dim=rot, interleave=interleave)
    assert_matches_oracle(q_out, k_out, q, k, pos, rot, interleave, dtype)
    assert torch.equal(bits(q_out[..., rot:]), bits(q[..., rot:])), "q pass-through elements differ from the input"
    assert torch.equal(bits(k_out[..., rot:]), bits(k[..., rot:])), "k pass-through elements differ from the input"


# ---- A5: the fused append in the multi-head regime ------------------------------------------------------------------

def slots_view(cache, layout):
    """5-D cache -> [pages * page_size, 2, heads, d] (a copy), one row per slot."""
    c = cache if layout == "NHD" else cache.transpose(2, 3)  # -> [P, 2, ps, H, D]
    return c.permute(0, 2, 1, 3, 4).reshape(-1, 2, c.shape[3], c.shape[4])


@pytest.mark.parametrize("q_inplace", [False, True])
@pytest.mark.parametrize("layout", ["NHD", "HND"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,rot,interleave", [(128, 128, False), (128, 128, True), (72, 64, False)])
def test_fused_append_with_several_heads_per_thread(d, rot, interleave, dtype, layout, q_inplace):
    """apply_rope_append_paged_kv_cache == apply_rope_pos_ids + append_paged_kv_cache bit for bit (the criterion of
    test_page_cascade_gpu.py) where one thread walks a head group that holds q and k heads: 7 + 3 heads, 3300 tokens,
    heads_per_thread 4 at head_dim 128 (tph 8), 2 at (72, 64) (tph 5)."""
    import flashinfer

    hq, hk, ps = 7, 3, 16
    lens, hist = [1, 1500, 700, 1099], [5, 0, 37, 16]
    nnz = sum(lens)
    hpt = heads_per_thread(hq, hk, nnz, d, rot)
    assert nnz == 3300 and hpt == (4 if d == 128 else 2) and hq % hpt != 0, hpt
    pt = append_problem(lens, hist, ps, spare_pages=9, seed=50)
    shape = (pt["total_pages"], 2, ps, hk, d) if layout == "NHD" else (pt["total_pages"], 2, hk, ps, d)
    cache_a = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    cache_b = torch.full(shape, float("nan"), dtype=dtype, device=DEV)
    qkv, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed=51)
    v = qkv[:, (hq + hk) * d:].view(nnz, hk, d)
    pos_ids = pt["positions"] + 7  # rotation positions that differ from the cache positions by a constant
    args = (pt["batch_indices"], pt["positions"])
    table = (pt["kv_indices"], pt["kv_indptr"], pt["last"])
    q_ref, k_rot = rope_out_of_place(q, k, pos_ids, hq, hk, d, rotary_dim=rot, interleave=interleave, rope_scale=2.0,
                                     rope_theta=5e4)
    flashinfer.append_paged_kv_cache(k_rot, v, *args, cache_a, *table, kv_layout=layout)
    k0, v0 = k.clone(), v.clone()
    q_out = q if q_inplace else torch.full_like(q.contiguous(), float("nan"))
    ret = flashinfer.apply_rope_append_paged_kv_cache(q, k, v, *args, cache_b, *table, kv_layout=layout, rotary_dim=rot,
                                                      interleave=interleave, rope_scale=2.0, rope_theta=5e4,
                                                      pos_ids=pos_ids, q_out=q_out)
    assert ret is q_out
    assert torch.equal(bits(q_out), bits(q_ref))
    assert torch.equal(bits(cache_a), bits(cache_b))
    assert torch.equal(bits(k), bits(k0)) and torch.equal(bits(v), bits(v0)), "the append inputs were modified"
    # every targeted slot is fully written, every other slot keeps its fill
    slots = slots_view(cache_b, layout)
    hit = torch.zeros(slots.shape[0], dtype=torch.bool, device=DEV)
    hit[pt["slot"]] = True
    assert int(hit.sum()) == nnz
    assert bool(torch.isnan(slots[~hit]).all()), "a slot outside the append was written"
    assert not bool(torch.isnan(slots[hit]).any()), "part of an appended row was not written"
    assert torch.equal(bits(slots[pt["slot"], 0]), bits(k_rot)) and torch.equal(bits(slots[pt["slot"], 1]), bits(v))


# ---- A6: llama-3.1 frequency scaling with explicit positions --------------------------------------------------------

@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("factors", [{}, dict(low_freq_factor=2, high_freq_factor=8, old_context_len=4096)],
                         ids=["default", "low2-high8-ctx4096"])
def test_llama31_pos_ids_forms(factors, dtype, interleave):
    """apply_llama31_rope_pos_ids and its in-place form at the shape of test_partial_head_groups_straddling_q_and_k
    (heads_per_thread 4).  The out-of-place form allocates its own outputs; positions >= 1 keep a stale copy of the
    input from passing, and the in-place form must give the same bits."""
    import flashinfer

    hq, hk, nnz, d = 7, 3, 3300, 128
    assert heads_per_thread(hq, hk, nnz, d, d) == 4
    a, b = RR.llama31_smooth(**factors)
    qkv, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed=60)
    qkv0 = qkv.clone()
    q0, k0 = qk_views(qkv0, hq, hk, d)
    pos = random_positions(nnz, 61).to(DEV)
    q_o, k_o = flashinfer.apply_llama31_rope_pos_ids(q, k, pos, interleave=interleave, **factors)
    assert torch.equal(bits(qkv), bits(qkv0)), "the out-of-place form wrote its input"
    flashinfer.apply_llama31_rope_pos_ids_inplace(q, k, pos, interleave=interleave, **factors)
    assert_matches_oracle(q, k, q0, k0, pos, d, interleave, dtype, 8.0, 5e5, a, b, what="in place")
    assert_every_row_changed(q, q0)
    assert_every_row_changed(k, k0)
    assert torch.equal(bits(q_o), bits(q)) and torch.equal(bits(k_o), bits(k))


# ---- B1: sin / cos alone at long positions --------------------------------------------------------------------------

B1_POSITIONS = [1, 255, 1608, 1609, 4095, 32768, 131071, 524287, 1048575, 16777215]


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sincos_at_long_positions_theta_one(dtype, interleave):
    """rope_theta = 1: 1 / theta is exactly 1, log2(1) = 0 and exp2(0) = 1, so every pair's frequency is exactly 1 and
    the angle is exactly pos (an integer below 2^24 is an f32 number).  What is left is fast_sincos(pos): the
    Cody-Waite reduction and the hardware sin / cos, whose own domain ends at 256 revolutions (1608 / 1609 are either
    side of it).  The ordinary tolerance and nothing more."""
    hq, hk, d = 2, 1, 64
    extra = random_positions(200, 70, lo=1, hi=1 << 24)
    pos = torch.cat((torch.tensor(B1_POSITIONS, dtype=torch.int32), extra)).to(DEV)
    assert int(pos.min()) >= 1 and int(pos.max()) < 1 << 24
    _, q, k = packed_qkv(pos.numel(), hq, hk, d, dtype, seed=71)
    q_out, k_out = rope_out_of_place(q, k, pos, hq, hk, d, interleave=interleave, rope_theta=1.0, rope_scale=1.0)
    freq = RR.rope_freqs(d, interleave, 1.0, 1.0)
    assert bool((freq == 1.0).all())
    assert_matches_oracle(q_out, k_out, q, k, pos, d, interleave, dtype, 1.0, 1.0)


# ---- B2: real frequencies at long positions, within the f32 angle budget ---------------------------------------------

B2_POSITIONS = [4000, 32767, 131071]
B2_FORMS = {"plain-1e4": dict(theta=1e4, scale=1.0, llama31=False), "llama31-5e5": dict(theta=5e5, scale=8.0, llama31=True)}


@pytest.mark.parametrize("interleave", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,rot", [(128, 128), (256, 128)])
@pytest.mark.parametrize("form", list(B2_FORMS))
def test_long_positions_within_f32_angle_budget(form, d, rot, dtype, interleave):
    """An f32 angle pos * freq cannot match f64 at position 1e5 (the reference computes it in f32 as well).  Per
    element the kernel gets the ordinary tolerance plus hypot(x0, x1) * delta_theta, delta_theta from
    oracle.rope_ref.angle_budget (constants justified on the CPU by tests/test_rope_budget_cpu.py).  Two assertions
    on the oracle alone keep that budget from hiding a failure."""
    import flashinfer

    f = B2_FORMS[form]
    hq, hk = 2, 1
    pos = torch.cat((torch.tensor(B2_POSITIONS, dtype=torch.int32), random_positions(64, 80, lo=1, hi=131072)))
    assert int(pos.max()) == 131071
    nnz = pos.numel()
    a, b = RR.llama31_smooth() if f["llama31"] else (0.0, 0.0)
    qkv, q, k = packed_qkv(nnz, hq, hk, d, dtype, seed=81)
    qkv0 = qkv.clone()
    if f["llama31"]:
        flashinfer.apply_llama31_rope_pos_ids_inplace(q, k, pos.to(DEV), rotary_dim=rot, interleave=interleave)
    else:
        flashinfer.apply_rope_pos_ids_inplace(q, k, pos.to(DEV), rotary_dim=rot, interleave=interleave)
    rtol, atol = TOL[dtype]["rtol"], TOL[dtype]["atol"]
    dtheta = RR.angle_budget(pos, rot, interleave, f["scale"], f["theta"], a, b)  # [nnz, rot]
    assert float(dtheta.max()) <= 0.08, float(dtheta.max())
    worst, over, count = 0.0, 0, 0
    for got, src in zip(qk_views(qkv, hq, hk, d), qk_views(qkv0, hq, hk, d)):
        x = src.double().cpu()
        ref = RR.apply_rope_pos_ids_ref(x, x, pos, rot, interleave, f["scale"], f["theta"], a, b)[0]
        allow = atol + rtol * ref.abs()
        allow[..., :rot] += RR.pair_hypot(x, rot, interleave) * dtheta[:, None, :]
        err = (got.double().cpu() - ref).abs()
        worst = max(worst, float((err / allow).max()))
        over += int((allow > 4 * atol).sum())
        count += allow.numel()
        bad = err > allow
        assert not bool(bad.any()), f"{int(bad.sum())} elements over the allowance, worst ratio {float((err / allow).max()):.3f}"
        assert torch.equal(bits(got[..., rot:]), bits(src[..., rot:]))
    print(f"B2 {form} d={d} rot={rot} {dtype} interleave={interleave}: worst error / allowance = {worst:.3f}, "
          f"max delta_theta = {float(dtheta.max()):.4f} rad, share of elements allowed > 4 atol = {over / count:.3f}")
    assert over / count < 0.60, over / count
