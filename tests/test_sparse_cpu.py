"""CPU: flashinfer.sparse keeps the reference's signatures, convert_bsr_mask_layout equals its restatement, the two
oracles of tests/sparse_ref.py agree with each other, and the new C entry points are declared, exported, bound and
refuse null arguments through fi_last_error().  No kernel is launched here."""
import inspect
import json
import os

import pytest
import torch

import sparse_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_signatures.json")
SYMBOLS = ("fi_block_mask_row_pages", "fi_block_mask_to_page_indices",
           "fi_block_sparse_indices_to_vector_sparse_offsets")


def _params(fn):
    return [{"name": p.name, **({} if p.default is inspect.Parameter.empty else {"default": p.default})}
            for p in inspect.signature(fn).parameters.values()]


def test_signatures_match_the_reference():
    """tests/golden/sparse_signatures.json: parameter names and defaults of the reference's two classes and two
    functions, read from its flashinfer/sparse.py and flashinfer/page.py with ``ast``."""
    import flashinfer
    from flashinfer import page, sparse

    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden["classes"]) == ["BlockSparseAttentionWrapper", "VariableBlockSparseAttentionWrapper"]
    for cls_name, members in golden["classes"].items():
        cls = getattr(sparse, cls_name)
        assert getattr(flashinfer, cls_name) is cls
        assert {"__init__", "reset_workspace_buffer", "plan", "forward", "run"} <= set(members)
        for name, params in members.items():
            if isinstance(params, str):  # an alias, e.g. begin_forward = plan
                assert getattr(cls, name) is getattr(cls, params), f"{cls_name}.{name}"
            else:
                assert _params(getattr(cls, name)) == params, f"{cls_name}.{name}"
    modules = {"flashinfer.sparse": sparse, "flashinfer.page": page}
    assert len(golden["functions"]) == 2
    for qualified, params in golden["functions"].items():
        module, name = qualified.rsplit(".", 1)
        assert _params(getattr(modules[module], name)) == params, qualified
    assert flashinfer.sparse is sparse
    assert flashinfer.block_sparse_indices_to_vector_sparse_offsets is page.block_sparse_indices_to_vector_sparse_offsets


@pytest.mark.parametrize("R,C", [(1, 1), (3, 5), (16, 4)])
def test_convert_bsr_mask_layout_equals_the_restatement(R, C):
    from flashinfer.sparse import convert_bsr_mask_layout

    indptr, indices, _ = S.bsr_pattern(6, 9, seed=R)
    nnz = int(indptr[-1])
    mask = torch.rand(nnz, R, C, generator=torch.Generator().manual_seed(C)) < 0.5
    got = convert_bsr_mask_layout(mask, indptr)
    assert got.shape == (nnz * R * C,) and got.dtype == mask.dtype
    assert torch.equal(got, S.bsr_mask_layout(mask, indptr))


@pytest.mark.parametrize("R,C,M,N,hq,hkv", [(4, 2, 30, 24, 4, 2), (1, 3, 7, 27, 2, 2)])
def test_gathered_and_dense_oracles_agree(R, C, M, N, hq, hkv):
    """Non-causal attention does not depend on the order of the keys: gathering a block row's KV rows in the
    (unsorted) order of ``indices`` and masking the dense score matrix are the same function."""
    g = torch.Generator().manual_seed(5)
    indptr, indices, block_map = S.bsr_pattern(-(-M // R), N // C, seed=9)
    assert any(torch.any(indices[int(a):int(b)][1:] < indices[int(a):int(b)][:-1])
               for a, b in zip(indptr[:-1], indptr[1:])), "the pattern must hold an unsorted row"
    q = torch.randn(M, hq, 16, generator=g)
    k, v = torch.randn(N, hkv, 16, generator=g), torch.randn(N, hkv, 16, generator=g)
    o_g, lse_g = S.bsr_attention_gathered(q, k, v, indptr, indices, R, C)
    o_d, lse_d = S.bsr_attention_dense(q, k, v, indptr, indices, R, C)
    torch.testing.assert_close(o_g, o_d, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(lse_g, lse_d, rtol=1e-12, atol=1e-12)
    empty = slice(R, 2 * R)  # block row 1 selects nothing
    assert torch.all(o_g[empty] == 0) and torch.all(lse_g[empty] == S.NEG_INF_LSE)
    assert torch.equal(S.bsr_dense_mask(indptr, indices, M, N, R, C)[::R, ::C][: len(block_map)], block_map)


def test_expansion_restatement_on_a_hand_case():
    block_map = torch.tensor([[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[1, 1, 0], [0, 0, 0], [1, 0, 0]]], dtype=torch.bool)
    col_sz = torch.tensor([[4, 2, 6], [2, 8, 2]], dtype=torch.int32)
    pages, indptr, indices = S.expand_block_mask(block_map, col_sz, 2)
    assert pages.tolist() == [3, 5, 4, 5, 0, 1]
    assert indptr.tolist() == [0, 3, 8, 12, 17, 17, 18]
    assert indices.tolist() == [3, 4, 5, 0, 1, 3, 4, 5, 2, 3, 4, 5, 6, 7, 8, 9, 10, 6]


def test_new_symbols_are_declared_exported_and_bound(fi_lib):
    from flashinfer import _lib

    header = open(os.path.join(ROOT, "include", "fi_mi355.h")).read()
    for name in SYMBOLS:
        assert f"FI_API int {name}(" in header, name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(fi_lib, name), name
    assert fi_lib.fi_abi_version() == 2


def test_null_arguments_are_reported(fi_lib):
    assert fi_lib.fi_block_mask_row_pages(None, None, 2, 3, 4, 1, 8, None, None) != 0
    assert b"null" in fi_lib.fi_last_error()
    assert fi_lib.fi_block_mask_to_page_indices(None, None, None, 2, 3, 4, 1, 8, 0, 0, None, None) != 0
    assert b"null" in fi_lib.fi_last_error()
    assert fi_lib.fi_block_sparse_indices_to_vector_sparse_offsets(None, None, None, None, None, 16, 1, 3, 16, 0, 0,
                                                                   None) != 0
    assert b"null" in fi_lib.fi_last_error()
    # a granule that does not divide kv_len, and page numbers past int32, without touching any tensor
    buf = (torch.zeros(64, dtype=torch.int32)).data_ptr()
    assert fi_lib.fi_block_mask_row_pages(buf, buf, 1, 1, 1, 3, 8, buf, None) != 0
    assert b"granule" in fi_lib.fi_last_error()
    assert fi_lib.fi_block_mask_row_pages(buf, buf, 4, 1, 1, 1, 2 ** 29, buf, None) != 0
    assert b"int32" in fi_lib.fi_last_error()


@pytest.mark.parametrize("cls", ["BlockSparseAttentionWrapper", "VariableBlockSparseAttentionWrapper"])
def test_cpu_workspace_is_refused(cls):
    import flashinfer

    with pytest.raises(RuntimeError, match="GPU"):
        getattr(flashinfer, cls)(torch.zeros(1024, dtype=torch.uint8))
    with pytest.raises(ValueError, match="backend"):
        getattr(flashinfer, cls)(torch.zeros(1024, dtype=torch.uint8), backend="trtllm")
