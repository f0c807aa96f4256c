"""Write tests/golden/fp4_signatures.json: the MX functions of the reference's flashinfer/fp4_quantization.py with their
parameter names, order and defaults, the alias the module keeps, and which of them the reference's top level
re-exports, read by an AST walk (no import of the reference is needed).  The file holds names and defaults only.

    python tools/gen_fp4_signatures.py <reference checkout> [output.json]
"""
import ast
import json
import os
import sys

from gen_mx_signatures import aliases, signatures

MODULE = "fp4_quantization"
PUBLIC = ["fp4_quantize", "mxfp4_quantize", "block_scale_interleave", "e2m1_and_ufp8sf_scale_to_float",
          "mxfp4_dequantize", "mxfp4_dequantize_host"]
ALIASES = ["nvfp4_block_scale_interleave"]


def main() -> None:
    ref = sys.argv[1]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "tests", "golden", "fp4_signatures.json")
    init = ast.parse(open(os.path.join(ref, "flashinfer", "__init__.py")).read())
    tree = ast.parse(open(os.path.join(ref, "flashinfer", MODULE + ".py")).read())
    exported = sorted(
        al.asname or al.name for node in init.body
        if isinstance(node, ast.ImportFrom) and node.module == MODULE and node.level == 1 for al in node.names)
    entry = {
        "functions": signatures(tree, PUBLIC),
        "aliases": aliases(tree, ALIASES),
        "top_level": [n for n in exported if n in PUBLIC + ALIASES],
    }
    with open(out, "w") as f:
        json.dump({MODULE: entry}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(entry["functions"]), "functions")


if __name__ == "__main__":
    main()
