"""Write tests/golden/mx_signatures.json: the public MX functions of the reference's flashinfer/fp8_quantization.py and
flashinfer/gemm.py with their parameter names, order and defaults, the aliases gemm.py keeps, and the names the
reference's top level re-exports from fp8_quantization, read by an AST walk (no import of the reference is needed).

    python tools/gen_mx_signatures.py <reference checkout> [output.json]
"""
import ast
import json
import os
import sys

PUBLIC = {
    "fp8_quantization": ["mxfp8_quantize", "mxfp8_dequantize_host"],
    "gemm": ["group_gemm_mxfp8_mxfp4_nt_groupwise"],
}
ALIASES = {"gemm": ["group_gemm_mxfp4_nt_groupwise"]}


def signatures(tree: ast.Module, public) -> dict:
    functions = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in public:
            a = node.args
            assert not (a.posonlyargs or a.kwonlyargs or a.vararg or a.kwarg), node.name
            names = [x.arg for x in a.args]
            first_default = len(names) - len(a.defaults)
            functions[node.name] = [
                {"name": n, **({"default": ast.literal_eval(a.defaults[i - first_default])} if i >= first_default else {})}
                for i, n in enumerate(names)
            ]
    missing = [n for n in public if n not in functions]
    assert not missing, missing
    return functions


def aliases(tree: ast.Module, wanted) -> dict:
    """module-level `new = old` assignments among the wanted names"""
    found = {}
    for node in tree.body:
        if (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
                and node.targets[0].id in wanted and isinstance(node.value, ast.Name)):
            found[node.targets[0].id] = node.value.id
    missing = [n for n in wanted if n not in found]
    assert not missing, missing
    return found


def main() -> None:
    ref = sys.argv[1]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "mx_signatures.json")
    init = ast.parse(open(os.path.join(ref, "flashinfer", "__init__.py")).read())
    modules = {}
    for module, public in PUBLIC.items():
        tree = ast.parse(open(os.path.join(ref, "flashinfer", module + ".py")).read())
        exported = sorted(
            al.asname or al.name for node in init.body
            if isinstance(node, ast.ImportFrom) and node.module == module and node.level == 1 for al in node.names)
        modules[module] = {
            "functions": signatures(tree, public),
            "aliases": aliases(tree, ALIASES.get(module, [])),
            "top_level": [n for n in exported if n in public],
        }
    with open(out, "w") as f:
        json.dump(modules, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {m: len(v["functions"]) for m, v in modules.items()})


if __name__ == "__main__":
    main()
