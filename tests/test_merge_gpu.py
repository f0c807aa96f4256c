"""GPU parity: cascade merge operators against the oracle (ref: tests/attention/test_shared_prefix_kernels.py:229-303)."""
import pytest
import torch

from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("seq_len,heads,d", [(1, 1, 64), (77, 32, 128), (512, 8, 256), (0, 4, 128)])
def test_merge_state(dtype, seq_len, heads, d):
    import flashinfer

    torch.manual_seed(0)
    va, vb = torch.randn(seq_len, heads, d).to(dtype), torch.randn(seq_len, heads, d).to(dtype)
    sa, sb = torch.randn(seq_len, heads) * 5, torch.randn(seq_len, heads) * 5
    v, s = flashinfer.merge_state(va.to(DEV), sa.to(DEV), vb.to(DEV), sb.to(DEV))
    v_ref, s_ref = R.merge_state_ref(va.float(), sa, vb.float(), sb)
    tol = 1e-3 if dtype != torch.bfloat16 else 8e-3
    torch.testing.assert_close(v.float().cpu(), v_ref.float(), rtol=tol, atol=tol)
    torch.testing.assert_close(s.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("use_mask", [False, True])
def test_merge_state_in_place(use_mask):
    import flashinfer

    torch.manual_seed(1)
    n, h, d = 129, 8, 128
    v, vo = torch.randn(n, h, d).half(), torch.randn(n, h, d).half()
    s, so = torch.randn(n, h) * 4, torch.randn(n, h) * 4
    mask = (torch.rand(n) > 0.5) if use_mask else None
    vd, sd = v.to(DEV).clone(), s.to(DEV).clone()
    flashinfer.merge_state_in_place(vd, sd, vo.to(DEV), so.to(DEV), mask=None if mask is None else mask.to(DEV))
    v_ref, s_ref = R.merge_state_ref(v.float(), s, vo.float(), so)
    if mask is not None:
        v_ref = torch.where(mask[:, None, None], v_ref, v.double())
        s_ref = torch.where(mask[:, None], s_ref, s.double())
    torch.testing.assert_close(vd.float().cpu(), v_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(sd.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)
    if mask is not None:  # untouched rows are bit-identical
        assert torch.equal(vd.cpu()[~mask], v[~mask])


@pytest.mark.parametrize("sets", [1, 2, 8, 33])
def test_merge_states(sets):
    import flashinfer

    torch.manual_seed(2)
    n, h, d = 64, 32, 128
    v = torch.randn(n, sets, h, d).half()
    s = torch.randn(n, sets, h) * 6
    vm, sm = flashinfer.merge_states(v.to(DEV), s.to(DEV))
    v_ref, s_ref = R.merge_states_ref(v.float(), s)
    torch.testing.assert_close(vm.float().cpu(), v_ref.float(), rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(sm.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)


MERGE_N = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 97, 129, 300]
V_BAR = {torch.float16: 1e-3, torch.bfloat16: 8e-3}  # the bars of the tests above


def _states(n, d, dtype, seed, rows=3, heads=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, n, heads, d, generator=g).to(dtype), torch.randn(rows, n, heads, generator=g) * 6


def _f32_bar(v, s, v_ref):
    """max(1e-5, 4 x the error of the f32 evaluation of the oracle's formula on the CPU): the kernel sums in f32 too,
    in another order over four waves."""
    v32, _ = R.merge_states_ref(v, s, dtype=torch.float32)
    return max(1e-5, 4 * (v32.double() - v_ref).abs().max().item())


@pytest.mark.parametrize("dtype,d", [(torch.float32, d) for d in (64, 128, 256, 32, 96, 192, 512)]
                         + [(dt, d) for dt in (torch.float16, torch.bfloat16) for d in (64, 80, 128, 512)],
                         ids=lambda x: str(x).replace("torch.", ""))
def test_merge_states_at_the_edges_of_its_loops(dtype, d):
    """merge_states with n on both sides of the four-wave split (4), the round of 32 entries in flight and the group of
    64.  f32 states of head_dim 64 / 128 / 256 run merge_n_f32_kernel<1|2|4> -- the kernel behind every split-KV
    decode, prefill and MLA run -- every other shape the generic kernel.
    f32 bar: the f32 evaluation of the oracle on the CPU is within 1.4e-6 of the fp64 oracle for every (D, n) here
    (measured, worst at D = 96), so 4 x that stays under the 1e-5 floor and the bar is 1e-5 throughout."""
    import flashinfer

    for n in MERGE_N:
        v, s = _states(n, d, dtype, seed=1000 * d + n)
        vm, sm = flashinfer.merge_states(v.to(DEV), s.to(DEV))
        v_ref, s_ref = R.merge_states_ref(v.float(), s)
        bar = _f32_bar(v, s, v_ref) if dtype == torch.float32 else V_BAR[dtype]
        torch.testing.assert_close(vm.float().cpu(), v_ref.float(), rtol=bar, atol=bar, msg=lambda m: f"n={n}: {m}")
        torch.testing.assert_close(sm.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4, msg=lambda m: f"n={n}: {m}")


@pytest.mark.parametrize("n", [1, 5, 65])
def test_merge_states_f32_unaligned_view_takes_the_fallback(n):
    """v four bytes into its allocation: contiguous, so the wrapper's .contiguous() keeps the pointer, and not
    16-byte aligned, so the vector kernel's 8-byte loads are out and launch_merge_n falls back to the generic kernel."""
    import flashinfer

    d = 128
    v, s = _states(n, d, torch.float32, seed=n)
    buf = torch.zeros(v.numel() + 1, device=DEV)
    vd = buf[1:].view(v.shape)
    vd.copy_(v)
    assert vd.data_ptr() % 16 == 4 and vd.contiguous().data_ptr() == vd.data_ptr()
    vm, sm = flashinfer.merge_states(vd, s.to(DEV))
    v_ref, s_ref = R.merge_states_ref(v, s)
    bar = _f32_bar(v, s, v_ref)
    torch.testing.assert_close(vm.cpu(), v_ref.float(), rtol=bar, atol=bar)
    torch.testing.assert_close(sm.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)
    aligned = flashinfer.merge_states(v.to(DEV), s.to(DEV))  # the vector kernel on the same values
    torch.testing.assert_close(vm, aligned[0], rtol=bar, atol=bar)


@pytest.mark.parametrize("d", [64, 128, 256, 96])
def test_ragged_merge_of_f32_partials(d):
    """fi_variable_length_merge_states as the split-KV paths call it: f32 partials, rows of 0, 1, 64, 65, 129 and 2
    entries.  Rows without entries give zeros and FI_NEG_INF."""
    from attn_inputs import indptr_of
    from flashinfer import _lib

    counts = [0, 1, 64, 65, 0, 129, 2]
    indptr = indptr_of(counts)
    nnz, h = int(indptr[-1]), 3
    g = torch.Generator().manual_seed(d)
    v, s = torch.randn(nnz, h, d, generator=g), torch.randn(nnz, h, generator=g) * 6
    v_d, s_d, ip_d = v.to(DEV), s.to(DEV), indptr.to(DEV)  # kept alive across the asynchronous launch
    for out_dtype in (torch.float32, torch.float16):
        vo = torch.full((len(counts), h, d), 7.0, dtype=out_dtype, device=DEV)
        so = torch.full((len(counts), h), 7.0, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().fi_variable_length_merge_states(
            v_d.data_ptr(), s_d.data_ptr(), ip_d.data_ptr(), vo.data_ptr(), so.data_ptr(), len(counts), h, d,
            _lib.FI_DTYPE_F32, _lib.fi_dtype(out_dtype), _lib.current_stream(vo.device)), "vlms")
        torch.cuda.synchronize()
        v_ref, s_ref = R.variable_length_merge_states_ref(v, s, indptr)
        bar = V_BAR[out_dtype] if out_dtype != torch.float32 else max(
            1e-5, 4 * (R.variable_length_merge_states_ref(v, s, indptr, torch.float32)[0].double() - v_ref).abs().max().item())
        torch.testing.assert_close(vo.float().cpu(), v_ref.float(), rtol=bar, atol=bar)
        torch.testing.assert_close(so.cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)
        for r in (0, 4):
            assert torch.all(vo[r] == 0) and torch.all(so[r] == _lib.FI_NEG_INF)


# The two encodings of a state that saw no key (csrc/merge_kernel.h): what the attention kernels write, and what the
# reference's callers pass; v = 0 in both.
EMPTY_S = {"kernel_sentinel": R.NEG_INF_SENTINEL, "minus_inf": float("-inf")}


def _reads_as_empty(v_e, s_e, dtype, d):
    """(v_e, s_e) [rows, H, D] / [rows, H] on the GPU merged with a live state returns that live state."""
    import flashinfer

    g = torch.Generator().manual_seed(99)
    live_v = torch.randn(*v_e.shape, generator=g).to(dtype).to(DEV)
    live_s = (torch.randn(*s_e.shape, generator=g) * 6).to(DEV)
    bar = 1e-5 if dtype == torch.float32 else V_BAR[dtype]
    for args in ((v_e, s_e, live_v, live_s), (live_v, live_s, v_e, s_e)):
        vm, sm = flashinfer.merge_state(*args)
        torch.testing.assert_close(vm.float(), live_v.float(), rtol=bar, atol=bar)
        torch.testing.assert_close(sm, live_s, rtol=1e-4, atol=1e-4)
    vm, sm = flashinfer.merge_states(torch.stack([v_e, live_v], 1), torch.stack([s_e, live_s], 1))
    torch.testing.assert_close(vm.float(), live_v.float(), rtol=bar, atol=bar)
    torch.testing.assert_close(sm, live_s, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("encoding", EMPTY_S)
@pytest.mark.parametrize("dtype,d", [(torch.float32, 128), (torch.float32, 96), (torch.float16, 128),
                                     (torch.bfloat16, 64)], ids=lambda x: str(x).replace("torch.", ""))
def test_merge_states_with_empty_entries(dtype, d, encoding):
    """Empty entries among live ones contribute nothing: the result is the oracle's over the live entries alone.  A
    row of nothing but empty entries gives v = 0 and an s that still reads as empty."""
    import flashinfer

    bar = 1e-5 if dtype == torch.float32 else V_BAR[dtype]
    for n in (2, 5, 33, 65, 130):
        v, s = _states(n, d, dtype, seed=7 * n + d, rows=4)
        dead = torch.rand(4, n, 3, generator=torch.Generator().manual_seed(n)) < 0.4
        dead[..., 0, :] = False  # at least one live entry per (row, head) ...
        dead[3] = True  # ... but for the last row, which holds nothing
        v[dead] = 0
        s[dead] = EMPTY_S[encoding]
        vm, sm = flashinfer.merge_states(v.to(DEV), s.to(DEV))
        assert torch.isfinite(vm).all() and not sm.isnan().any()
        # the oracle over the live entries alone: a dead entry's weight is exactly 0 in f64 under either encoding
        s_live = torch.where(dead, torch.full_like(s, float("-inf")), s)
        v_ref, s_ref = R.merge_states_ref(v[:3].float(), s_live[:3])
        torch.testing.assert_close(vm[:3].float().cpu(), v_ref.float(), rtol=bar, atol=bar)
        torch.testing.assert_close(sm[:3].cpu(), s_ref.float(), rtol=1e-4, atol=1e-4)
        assert torch.count_nonzero(vm[3]) == 0
        _reads_as_empty(vm[3:], sm[3:], dtype, d)


@pytest.mark.parametrize("in_place", [False, True], ids=["merge_state", "in_place"])
@pytest.mark.parametrize("encoding", EMPTY_S)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=lambda x: str(x).replace("torch.", ""))
def test_merge_state_with_empty_states(dtype, encoding, in_place):
    """(empty, live), (live, empty) and (empty, empty), one row each: never NaN; a live state comes back as it was;
    two empty states give v = 0 and an s that still reads as empty."""
    import flashinfer

    h, d = 4, 128
    g = torch.Generator().manual_seed(3)
    live_v, live_s = torch.randn(h, d, generator=g).to(dtype), torch.randn(h, generator=g) * 6
    e_v, e_s = torch.zeros(h, d, dtype=dtype), torch.full((h,), EMPTY_S[encoding])
    va, sa = torch.stack([e_v, live_v, e_v]).to(DEV), torch.stack([e_s, live_s, e_s]).to(DEV)
    vb, sb = torch.stack([live_v, e_v, e_v]).to(DEV), torch.stack([live_s, e_s, e_s]).to(DEV)
    if in_place:
        vm, sm = va.clone(), sa.clone()
        flashinfer.merge_state_in_place(vm, sm, vb, sb)
    else:
        vm, sm = flashinfer.merge_state(va, sa, vb, sb)
    assert not vm.isnan().any() and not sm.isnan().any()
    bar = 1e-5 if dtype == torch.float32 else V_BAR[dtype]
    for r in (0, 1):
        torch.testing.assert_close(vm[r].float().cpu(), live_v.float(), rtol=bar, atol=bar)
        torch.testing.assert_close(sm[r].cpu(), live_s, rtol=1e-4, atol=1e-4)
    assert torch.count_nonzero(vm[2]) == 0
    _reads_as_empty(vm[2:], sm[2:], dtype, d)


def test_merge_with_empty_state_is_identity():
    import flashinfer

    n, h, d = 5, 4, 128
    v = torch.randn(n, h, d).half().to(DEV)
    s = torch.randn(n, h).to(DEV)
    e_v = torch.zeros_like(v)
    e_s = torch.full_like(s, R.NEG_INF_SENTINEL)
    vm, sm = flashinfer.merge_state(v, s, e_v, e_s)
    torch.testing.assert_close(vm, v, rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(sm, s, rtol=1e-5, atol=1e-5)
