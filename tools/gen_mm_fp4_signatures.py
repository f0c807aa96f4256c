"""Write tests/golden/mm_fp4_signatures.json: the parameter names, order and defaults of ``mm_fp4`` in the reference's
flashinfer/gemm.py and whether the reference's top level re-exports it, read by an AST walk (no import of the reference
is needed).  A default that is no literal (``torch.bfloat16``) is recorded as its source text.

    python tools/gen_mm_fp4_signatures.py <reference checkout> [output.json]
"""
import ast
import json
import os
import sys

PUBLIC = {"gemm": ["mm_fp4"]}


def default_of(node: ast.expr):
    try:
        return ast.literal_eval(node)
    except ValueError:
        return ast.unparse(node)


def signatures(tree: ast.Module, public) -> dict:
    functions = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in public:
            a = node.args
            assert not (a.posonlyargs or a.kwonlyargs or a.vararg or a.kwarg), node.name
            names = [x.arg for x in a.args]
            first_default = len(names) - len(a.defaults)
            functions[node.name] = [
                {"name": n, **({"default": default_of(a.defaults[i - first_default])} if i >= first_default else {})}
                for i, n in enumerate(names)
            ]
    missing = [n for n in public if n not in functions]
    assert not missing, missing
    return functions


def main() -> None:
    ref = sys.argv[1]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "mm_fp4_signatures.json")
    init = ast.parse(open(os.path.join(ref, "flashinfer", "__init__.py")).read())
    modules = {}
    for module, public in PUBLIC.items():
        tree = ast.parse(open(os.path.join(ref, "flashinfer", module + ".py")).read())
        exported = sorted(
            al.asname or al.name for node in init.body
            if isinstance(node, ast.ImportFrom) and node.module == module and node.level == 1 for al in node.names)
        modules[module] = {"functions": signatures(tree, public), "top_level": [n for n in exported if n in public]}
    with open(out, "w") as f:
        json.dump(modules, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {m: len(v["functions"]) for m, v in modules.items()})


if __name__ == "__main__":
    main()
