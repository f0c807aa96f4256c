"""A fixed set of small calls, one per outcome of the kernel choices (choose_decode in csrc/decode.hip, choose_gemm
in csrc/gemm.hip), to be run under a kernel trace:
    rocprofv3 --kernel-trace --stats -- python tools/kernel_names.py [NAME=VALUE ...]
NAME=VALUE sets a switch of INTEGRATION.md in this process (flashinfer._lib.set_option); a library without
set_option takes the switches from the environment only.  The sorted (kernel name, calls) list of the trace must
not depend on the way a switch was given, nor change when the choice is not meant to (profiles/kernel_choice_trace.md).
The GEMM shapes are sized for the thresholds at 256 CUs."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "flashinfer-ai_amd"))
import torch, flashinfer
from flashinfer import _lib

for arg in sys.argv[1:]:
    name, value = arg.split("=", 1)
    if not hasattr(_lib, "set_option"):
        sys.exit(f"this library has no set_option: give {arg} through the environment")
    _lib.set_option(name, int(value))

DEV = torch.device("cuda:0")
FP8 = torch.float8_e4m3fn
torch.manual_seed(0)
ws = torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)


def decode(group, kv_dtype, d, mode="NONE", hkv=2, ps=16, kv_lens=(700, 33, 2048)):
    pages = torch.tensor([-(-l // ps) for l in kv_lens])
    indptr = torch.cat([torch.zeros(1, dtype=torch.long), pages.cumsum(0)]).to(torch.int32).to(DEV)
    total = int(pages.sum())
    indices = torch.randperm(total).to(torch.int32).to(DEV)
    last = torch.tensor([(l - 1) % ps + 1 for l in kv_lens], dtype=torch.int32, device=DEV)
    cache = torch.randn(total, 2, ps, hkv, d, device=DEV).to(kv_dtype)
    q = torch.randn(len(kv_lens), group * hkv, d, device=DEV, dtype=torch.bfloat16)
    w = flashinfer.BatchDecodeWithPagedKVCacheWrapper(ws, "NHD")
    w.plan(indptr, indices, last, group * hkv, hkv, d, ps, q_data_type=torch.bfloat16, kv_data_type=kv_dtype,
           pos_encoding_mode=mode)
    w.run(q, cache)


def gemm(ms, n, k=128):
    """One group: the plain GEMM; several: the grouped one.  Operands and scales of ones (power-of-two scales)."""
    cum = sum(ms)
    a = torch.ones(cum, k, device=DEV).to(FP8)
    sa = torch.ones(k // 128, cum, device=DEV)
    if len(ms) == 1:
        flashinfer.gemm_fp8_nt_groupwise(a, torch.ones(n, k, device=DEV).to(FP8), sa,
                                         torch.ones(k // 128, -(-n // 128), device=DEV), scale_major_mode="MN")
    else:
        m_indptr = torch.tensor([0] + list(torch.tensor(ms).cumsum(0)), dtype=torch.int32, device=DEV)
        flashinfer.group_gemm_fp8_nt_groupwise(a, torch.ones(len(ms), n, k, device=DEV).to(FP8), sa,
                                               torch.ones(len(ms), k // 128, -(-n // 128), device=DEV), m_indptr)


for group in (1, 4, 8, 32):
    decode(group, torch.bfloat16, 128)
decode(4, FP8, 128)
decode(8, FP8, 128)
decode(4, torch.bfloat16, 256)
decode(1, FP8, 256)
decode(4, torch.bfloat16, 128, "ROPE_LLAMA")
decode(32, FP8, 128, "ROPE_LLAMA")
decode(8, torch.bfloat16, 128, "ALIBI")
decode(32, torch.bfloat16, 128, "ALIBI")
# by default, at 256 CUs (256 x 256 tiles / 256 x 128 tiles of the call):
gemm([128], 256)          # 1 / 2: the 128 x 128 kernel alone
gemm([4096], 2048)        # 128 / 256: hardware-scale 256 x 256 variant in front of the 128 x 128 kernel
gemm([8192], 2048)        # 256 / 512: ... in front of the persistent 256 x 128 kernel
gemm([8192], 8192)        # 1024: both 256 x 256 variants, nothing after them
gemm([64] * 64, 1536)     # groups of 64 rows: the persistent 128 x 256 kernel alone
gemm([128] * 64, 1536)    # groups of 128 rows: the hardware-scale variant in front of the 128 x 256 kernel
torch.cuda.synchronize()
print("kernel_names: done")
