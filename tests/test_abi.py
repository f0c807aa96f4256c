"""CPU: the C-ABI library loads and exports every symbol include/fi_mi355.h declares; host-side argument
validation reports through fi_last_error(); the ctypes binding read from the header lays every struct out as the
compiler does.  No kernel is launched here."""
import ctypes as C
import keyword
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fi_mi355.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"FI_API\s+[\w\s\*]+?\b(fi_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_entry_points():
    syms = declared_symbols()
    assert "fi_batch_decode_plan" in syms and "fi_batch_decode_run" in syms
    assert "fi_last_error" in syms


def test_library_exports_every_declared_symbol(fi_lib):
    from flashinfer import _lib

    missing = [s for s in declared_symbols() if not hasattr(fi_lib, s)]
    assert not missing, f"library does not export: {missing}"
    # and the Python binding knows every one of them
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared_symbols()


def test_abi_version_and_cu_count(fi_lib):
    assert fi_lib.fi_abi_version() == 2
    assert fi_lib.fi_num_compute_units() > 0


def test_errors_are_reported_not_thrown(fi_lib):
    from flashinfer import _lib

    info = (C.c_int64 * _lib.FI_DECODE_PLAN_INFO_LEN)()
    # null pinned buffer / indptr
    rc = fi_lib.fi_batch_decode_plan(None, 0, None, None, 0, None, 1, 8, 8, 16, 0, 128, 0, 0, 0, -1, info, None)
    assert rc != 0
    assert b"null" in fi_lib.fi_last_error()
    # num_qo_heads not a multiple of num_kv_heads
    buf = (C.c_char * 4096)()
    indptr = (C.c_int32 * 2)(0, 4)
    rc = fi_lib.fi_batch_decode_plan(None, 0, None, buf, 4096, indptr, 1, 7, 2, 16, 0, 128, 0, 0, 0, -1, info, None)
    assert rc != 0 and b"multiple" in fi_lib.fi_last_error()
    # unsupported head_dim
    rc = fi_lib.fi_batch_decode_plan(None, 0, None, buf, 4096, indptr, 1, 8, 2, 16, 0, 96, 0, 0, 0, -1, info, None)
    assert rc != 0 and b"unsupported" in fi_lib.fi_last_error()
    # run with a plan_info that is not a plan
    with pytest.raises(RuntimeError, match="plan"):
        _lib.check(fi_lib.fi_batch_decode_run(None, 0, None, 0, info, _lib.FI_DECODE_PLAN_INFO_LEN, None, None), "run")


def test_product_path_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "flashinfer-ai_amd", "flashinfer")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            text = open(os.path.join(pkg, name)).read()
            assert "oracle" not in text.replace("oracle/", ""), f"{name} references the oracle"


def test_ops_fail_loudly_on_cpu_tensors():
    import torch

    import flashinfer

    q = torch.zeros(4, 64, dtype=torch.float16)
    k = torch.zeros(8, 4, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        flashinfer.single_decode_with_kv_cache(q, k, k)
    with pytest.raises(RuntimeError, match="GPU"):
        flashinfer.merge_state(torch.zeros(1, 1, 64), torch.zeros(1, 1), torch.zeros(1, 1, 64), torch.zeros(1, 1))


def host_clang():
    """The clang beside hipcc: the compiler the library itself is built with."""
    hipcc = shutil.which("hipcc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if hipcc:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang")):
        if os.path.exists(cand):
            return cand
    pytest.fail(f"no clang under {rocm}: the library cannot be built without it either")


def compiler_layouts(tmp_path, names):
    """{struct tag: ([(byte offset, field name), ...] top level in order, sizeof)} from clang's record-layout dump."""
    src = tmp_path / "layouts.c"
    src.write_text(f'#include "{HEADER}"\n' + "".join(f"{n} var_{n};\n" for n in names))
    cmd = [host_clang(), "-c", "-Xclang", "-fdump-record-layouts", str(src), "-o", str(tmp_path / "layouts.o")]
    dump = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout
    layouts = {}
    for record in dump.split("*** Dumping AST Record Layout")[1:]:
        lines = record.strip().splitlines()
        tag = re.match(r"\s*0 \| struct (\w+)$", lines[0]).group(1)
        # a top-level member is indented by exactly three columns after the bar; a nested record's own fields by more
        fields = [(int(off), name) for off, name in re.findall(r"^\s*(\d+) \|   \S.*?(\w+)$", record, re.M)]
        size = int(re.search(r"\[sizeof=(\d+)", record).group(1))
        layouts[tag] = (fields, size)
    return layouts


def test_struct_layouts_match_the_compiler(tmp_path):
    from flashinfer import _lib

    structs = _lib._ABI.structs
    assert "fi_paged_kv_t" in structs and "fi_batch_prefill_params_t" in structs
    layouts = compiler_layouts(tmp_path, list(structs))
    for name, cls in structs.items():
        fields, size = layouts[name[:-2]]  # the header names every typedef <struct tag>_t
        ours = [(getattr(cls, f).offset, f) for f, _ in cls._fields_]
        assert ours == [(off, f + "_" if keyword.iskeyword(f) else f) for off, f in fields], name
        assert C.sizeof(cls) == size, name


@pytest.mark.parametrize("snippet,offender", [
    ("typedef struct fi_x { int32_t a; fi_unknown_t b; } fi_x_t;", "fi_unknown_t"),
    ("FI_API int fi_f(int32_t a, const fi_missing_t* params);", "fi_missing_t"),
    ("enum fi_e { FI_E_A = 0, FI_E_B };", "FI_E_B"),
    ("FI_API int fi_unfinished(int32_t a)\nFI_API int fi_next(void);", "fi_unfinished"),
])
def test_parser_refuses_what_it_cannot_read(snippet, offender):
    from flashinfer import _abi

    with pytest.raises(_abi.HeaderError, match=offender):
        _abi.parse(snippet)


def test_every_parsed_prototype_is_bound(fi_lib):
    from flashinfer import _lib

    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    counts = {name: 0 if params.strip() == "void" else params.count(",") + 1
              for name, params in re.findall(r"FI_API\s[^;(]*?\b(fi_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(counts) == sorted(_lib.EXPORTED_SYMBOLS)
    for name, count in counts.items():
        fn = getattr(fi_lib, name)
        assert len(fn.argtypes) == count, name
        assert fn.restype is (C.c_char_p if name == "fi_last_error" else C.c_int), name
