"""Write tests/golden/norm_activation_signatures.json: the public functions of the reference's flashinfer/norm.py and
flashinfer/activation.py with their parameter names, order and defaults, and the names the reference's top level
re-exports from the two modules, read by an AST walk (no import of the reference is needed).

    python tools/gen_norm_activation_signatures.py <reference checkout> [output.json]
"""
import ast
import json
import os
import sys

PUBLIC = {
    "norm": ["rmsnorm", "fused_add_rmsnorm", "gemma_rmsnorm", "gemma_fused_add_rmsnorm"],
    "activation": ["silu_and_mul", "gelu_and_mul", "gelu_tanh_and_mul"],
}


def signatures(path: str, public) -> dict:
    functions = {}
    for node in ast.parse(open(path).read()).body:
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


def main() -> None:
    ref = sys.argv[1]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden",
                                                             "norm_activation_signatures.json")
    init = ast.parse(open(os.path.join(ref, "flashinfer", "__init__.py")).read())
    modules = {}
    for module, public in PUBLIC.items():
        exported = sorted(
            al.asname or al.name for node in init.body
            if isinstance(node, ast.ImportFrom) and node.module == module and node.level == 1 for al in node.names)
        modules[module] = {
            "functions": signatures(os.path.join(ref, "flashinfer", module + ".py"), public),
            # the reference also re-exports its nvfp4 quantising silu; fp4 is out of scope here
            "top_level": [n for n in exported if n in public],
        }
    with open(out, "w") as f:
        json.dump(modules, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, {m: len(v["functions"]) for m, v in modules.items()})


if __name__ == "__main__":
    main()
