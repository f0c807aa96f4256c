"""Write tests/golden/sampling_signatures.json: the public functions of the reference's flashinfer/sampling.py with
their parameter names, order and defaults, read by an AST walk (no import of the reference is needed).

    python tools/gen_sampling_signatures.py <reference checkout> [output.json]
"""
import ast
import json
import os
import sys

PUBLIC = [
    "get_seed_and_offset", "softmax", "sampling_from_logits", "sampling_from_probs", "top_p_sampling_from_probs",
    "top_k_sampling_from_probs", "min_p_sampling_from_probs", "top_k_top_p_sampling_from_logits",
    "top_k_top_p_sampling_from_probs", "top_p_renorm_probs", "top_k_renorm_probs", "top_k_mask_logits",
    "chain_speculative_sampling",
]


def main() -> None:
    ref = sys.argv[1]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "sampling_signatures.json")
    tree = ast.parse(open(os.path.join(ref, "flashinfer", "sampling.py")).read())
    functions, aliases = {}, {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in PUBLIC:
            a = node.args
            assert not (a.posonlyargs or a.kwonlyargs or a.vararg or a.kwarg), node.name
            names = [x.arg for x in a.args]
            first_default = len(names) - len(a.defaults)
            functions[node.name] = [
                {"name": n, **({"default": ast.literal_eval(a.defaults[i - first_default])} if i >= first_default else {})}
                for i, n in enumerate(names)
            ]
        elif (isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name)
              and isinstance(node.value, ast.Name) and node.value.id in PUBLIC):
            aliases[node.targets[0].id] = node.value.id
    missing = [n for n in PUBLIC if n not in functions]
    assert not missing, missing
    init = ast.parse(open(os.path.join(ref, "flashinfer", "__init__.py")).read())
    top_level = sorted(
        al.asname or al.name for node in init.body
        if isinstance(node, ast.ImportFrom) and node.module == "sampling" and node.level == 1 for al in node.names)
    with open(out, "w") as f:
        json.dump({"functions": functions, "aliases": aliases, "top_level": top_level}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(functions), "functions")


if __name__ == "__main__":
    main()
