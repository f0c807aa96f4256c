"""Wide-group decode: matrix-core kernel vs the VALU kernel."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from bench_decode_sweep import run
which = sys.argv[1] if len(sys.argv) > 1 else "wide"
if which == "wide":
    run(hq=64, tag="G=8 hq=64 bs64 kv8192")
    run(hq=128, tag="G=16 hq=128 bs64 kv8192")
    run(hq=64, hkv=4, tag="G=16 hq=64/4 bs64 kv8192")
    run(hq=40, hkv=8, tag="G=5 hq=40 bs64 kv8192")
    run(hq=64, b=4, L=65536, tag="G=8 bs4 kv65536")
    run(hq=64, b=256, L=2048, tag="G=8 bs256 kv2048")
    run(hq=64, layout="HND", tag="G=8 HND")
    run(hq=64, dtype=torch.float8_e4m3fn, tag="G=8 fp8 kv")
else:  # narrow groups: where is the crossover?
    run(tag="C2 G=4")
    run(hq=16, tag="G=2")
    run(hq=8, tag="G=1")
    run(dtype=torch.float8_e4m3fn, tag="C2 fp8 kv G=4")
    run(hq=8, dtype=torch.float8_e4m3fn, tag="fp8 kv G=1")
    run(b=1, L=131072, tag="bs1 kv131072")
