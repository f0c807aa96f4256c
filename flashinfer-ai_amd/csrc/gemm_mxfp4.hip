// Grouped GEMM with MXFP8 activations and MXFP4 weights on the block-scaled MFMA of gfx950.
//
// What it replaces: the reference's CUTLASS kernel behind group_gemm_mxfp8_mxfp4_nt_groupwise
// (include/flashinfer/gemm/group_gemm_mxfp4_groupwise_sm100.cuh, flashinfer/gemm.py:2814-2949).
//   d[r, j] = sum_k a[r, k] 2^(sa[r, k/32] - 127) . e2m1(b[g, j, k]) 2^(sb[g, j, k/32] - 127)   for r in group g
//   a (cum_m, k) e4m3 / e5m2, b (G, n, k/2) bytes (k = 2i in the low nibble of byte i), scales E8M0 bytes in the
//   swizzled layout of mx_layout.h (offsets and sizes), f32 accumulation, one rounding to f16 / bf16.
//
// Structure.  v_mfma_scale_f32_16x16x128_f8f6f4 multiplies a [16][128] by a [128][16] operand and scales every run of 32
// k elements of every row by its own E8M0 byte: the MX format itself, so the weight nibbles and both tensors' scale
// bytes go from memory into the instruction's operands unchanged -- no dequantisation, no f32 scale multiply.
// The product is computed TRANSPOSED (d^T = b a^T): 16 weight rows are the MFMA's row operand (fp4, cbsz 4) and 16
// tokens its column operand (fp8, blgp 0 / 1), so a group of 4 ... 16 tokens costs one column block, not a 128-row tile
// of padding.  A workgroup of 4 waves owns 128 weight rows x 16 MB tokens (MB = 1, 2, 4 by the mean rows per group);
// each wave owns 32 of the weight rows and streams them from global memory straight into registers, 16 bytes per
// lane per MFMA, every weight byte fetched once per token tile.  The token fragments (32 bytes per lane) and the
// scale dwords come the same way, from L2 after the first workgroup.  There is no LDS stage and no barrier: the
// loads of k step s + 1 are in flight while the MFMAs of step s run, and the other waves of the CU cover the rest.
//
// Operand lane maps (lane l, c = l & 15, q = l >> 4), as found on the hardware with one-hot operands (the bit-exact
// tests of tests/test_mx_gpu.py pin them):
//   row operand (fp4)     lane l holds row c, k = 32 q .. 32 q + 31 as 16 bytes in memory order (low nibble first),
//                         in the first 4 of the operand's 8 registers
//   column operand (fp8)  lane l holds column c, k = 16 q .. 16 q + 15 in registers 0-3 and k = 64 + 16 q .. 64 + 16 q + 15
//                         in registers 4-7, bytes in memory order: NOT the 32 consecutive elements of the fp4 map
//   scales                lane l supplies, in byte 0 of the scale register (op_sel 0), the byte of (row c, k block q)
//                         resp. (column c, k block q), k block q = k 32 q .. 32 q + 31 -- for the fp4 operand the
//                         block the lane holds, for the fp8 operand NOT the elements the lane holds
//   result                register i of lane l is (row 4 q + i, column c)
#include "gemm_mx.h"

namespace fi {

constexpr int kMxThreads = 256;
constexpr int kMxTileN = 128;  // weight rows per workgroup: 4 waves x 2 blocks of 16

struct MxGemmParams {
  const uint8_t* a;
  const uint8_t* b;
  const uint8_t* a_scale;
  const uint8_t* b_scale;
  void* d;
  const int32_t* m_indptr;  // [G + 1] device
  int32_t num_groups, cum_m, n, k;
  int32_t out_dtype;
  int32_t num_m_tiles_bound;  // grid bound on (group, token tile) pairs
  int32_t n_tiles;
};

template <bool A_E5M2, int MB>
__global__ void __launch_bounds__(kMxThreads) group_gemm_mxfp4_kernel(const MxGemmParams p) {
  constexpr int TM = 16 * MB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;

  // token tiles fastest: the tiles of one group that share a weight tile run next to each other
  const int nt = blockIdx.x / p.num_m_tiles_bound;
  const int mt_global = blockIdx.x - nt * p.num_m_tiles_bound;
  int g = 0, m_begin = 0, m_end = 0, mt = 0;
  if (!find_group_tile<TM>(p.m_indptr, p.num_groups, mt_global, lane, g, m_begin, m_end, mt)) return;
  const int N = p.n, K = p.k;
  const int m0 = m_begin + mt * TM;
  m_end = min(m_end, p.cum_m);  // rows at or past cum_m do not exist whatever m_indptr says
  const int n0 = nt * kMxTileN + 32 * wave;
  if (m_begin < 0 || m0 >= m_end || n0 >= N) return;  // whole waves leave; there is no barrier below
  const int ksteps = K >> 7;
  const int nkb = K >> 5;

  // ---- per-lane sources; rows past the edge of n or of the group re-read the last valid row and are masked at the store
  const uint8_t* const b_tile = p.b + ((int64_t)g * N + n0) * (K >> 1);
  const uint8_t* const a_tile = p.a + (int64_t)m0 * K;
  const uint8_t* const sb_base = p.b_scale + (int64_t)g * mx_sf_rows(N, true) * nkb;
  const uint8_t* const sa_base = p.a_scale + mx_sf_row_offset(m_begin, g) * nkb;
  uint32_t w_off[2], sw_off[2], a_off[MB], sa_off[MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int row = min(n0 + 16 * nb + c, N - 1);
    w_off[nb] = (uint32_t)(row - n0) * (uint32_t)(K >> 1) + q * 16;
    sw_off[nb] = (uint32_t)mx_sf_offset(row, 0, nkb);
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int row = min(m0 + 16 * mb + c, m_end - 1);
    a_off[mb] = (uint32_t)(row - m0) * (uint32_t)K + q * 16;
    sa_off[mb] = (uint32_t)mx_sf_offset(row - m_begin, 0, nkb);
  }

  struct StepRegs {
    u32x4 w[2];
    u32x4 a[MB][2];
    uint32_t sw[2], sa[MB];
  };
  // k step ks: 64 weight bytes and 128 token bytes per row, and the aligned dword of its four scales
  auto load = [&](int ks, StepRegs& r) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      r.w[nb] = *(const u32x4*)(b_tile + (w_off[nb] + (uint32_t)ks * 64));
      r.sw[nb] = *(const uint32_t*)(sb_base + (sw_off[nb] + (uint32_t)ks * 512));
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const uint8_t* src = a_tile + (a_off[mb] + (uint32_t)ks * 128);
      r.a[mb][0] = *(const u32x4*)src;
      r.a[mb][1] = *(const u32x4*)(src + 64);
      r.sa[mb] = *(const uint32_t*)(sa_base + (sa_off[mb] + (uint32_t)ks * 512));
    }
  };

  f32x4 acc[2][MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const StepRegs& r) {
    i32x8g fw[2];
    int ew[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      fw[nb] = mx_fp4_frag(r.w[nb]);
      ew[nb] = mx_scale_byte(r.sw[nb], q);
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const i32x8g fa = {(int)r.a[mb][0][0], (int)r.a[mb][0][1], (int)r.a[mb][0][2], (int)r.a[mb][0][3],
                         (int)r.a[mb][1][0], (int)r.a[mb][1][1], (int)r.a[mb][1][2], (int)r.a[mb][1][3]};
      const int ea = mx_scale_byte(r.sa[mb], q);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) acc[nb][mb] = mx_mfma<A_E5M2 ? 1 : 0>(fw[nb], ew[nb], fa, ea, acc[nb][mb]);
    }
  };

  // the loads run one k step ahead of the MFMAs; the step past the end re-loads the last one (no branch around a load)
  StepRegs r0, r1;
  load(0, r0);
  int ks = 0;
  for (; ks + 1 < ksteps; ks += 2) {
    load(ks + 1, r1);
    compute(r0);
    load(min(ks + 2, ksteps - 1), r0);
    compute(r1);
  }
  if (ks < ksteps) compute(r0);

  // ---- store: a lane holds 4 consecutive n of one token
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      mx_store_piece(p.d, p.out_dtype, m0 + 16 * mb + c, m_end, n0 + 16 * nb + 4 * q, N, acc[nb][mb], 1.0f);
}

template <bool A_E5M2>
static void launch_mxfp4(const MxGemmParams& p_in, hipStream_t stream) {
  MxGemmParams p = p_in;
  p.n_tiles = ceil_div(p.n, kMxTileN);
  // token tile by the mean rows per group (the groups' sizes live on the device): a tile the mean group fills
  with_mx_token_blocks(ceil_div<int64_t>(p.cum_m, p.num_groups), [&](auto mb_c) {
    constexpr int MB = decltype(mb_c)::value;
    // every group adds at most one partial tile on top of cum_m / TM
    p.num_m_tiles_bound = p.cum_m / (16 * MB) + p.num_groups;
    group_gemm_mxfp4_kernel<A_E5M2, MB>
        <<<dim3((uint32_t)p.num_m_tiles_bound * (uint32_t)p.n_tiles), dim3(kMxThreads), 0, stream>>>(p);
  });
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_group_gemm_mxfp8_mxfp4_nt_groupwise(const fi_group_gemm_mxfp4_params_t* p, fi_stream_t stream) {
  const char* who = "group_gemm_mxfp8_mxfp4_nt_groupwise";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->num_groups >= 0 && p->cum_m >= 0 && p->n >= 0 && p->k >= 0,
             "%s: negative size (num_groups %d, cum_m %d, n %d, k %d)", who, p->num_groups, p->cum_m, p->n, p->k);
  if (p->num_groups == 0 || p->cum_m == 0 || p->n == 0) return 0;
  FI_REQUIRE(p->a && p->b && p->a_scale && p->b_scale && p->d && p->m_indptr, "%s: null tensor", who);
  FI_REQUIRE(p->a_dtype == FI_DTYPE_FP8_E4M3 || p->a_dtype == FI_DTYPE_FP8_E5M2, "%s: a dtype %d is not fp8 (e4m3 / e5m2)",
             who, p->a_dtype);
  const bool aligned = ((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->d % 8) == 0 &&
                       ((uintptr_t)p->a_scale % 4) == 0 && ((uintptr_t)p->b_scale % 4) == 0;
  const int64_t nkb = p->k / kMxBlock;
  if (const int e = mx_check_common(
          who, p->d_dtype, p->n, p->k, aligned, "d 8-byte and the scales 4-byte", p->a_scale_bytes,
          mx_sf_rows_grouped(p->cum_m, p->num_groups) * nkb, "(cum_m + 127 G) / 128 * 128 rows", p->b_scale_bytes,
          (int64_t)p->num_groups * mx_sf_rows(p->n, true) * nkb, p->num_groups, "n padded to 128 per group",
          (int64_t)(p->cum_m / 16 + p->num_groups) * ceil_div(p->n, kMxTileN)))
    return e;
  MxGemmParams g{};
  g.a = (const uint8_t*)p->a;
  g.b = (const uint8_t*)p->b;
  g.a_scale = (const uint8_t*)p->a_scale;
  g.b_scale = (const uint8_t*)p->b_scale;
  g.d = p->d;
  g.m_indptr = p->m_indptr;
  g.num_groups = p->num_groups;
  g.cum_m = p->cum_m;
  g.n = p->n;
  g.k = p->k;
  g.out_dtype = p->d_dtype;
  if (p->a_dtype == FI_DTYPE_FP8_E5M2) launch_mxfp4<true>(g, (hipStream_t)stream);
  else launch_mxfp4<false>(g, (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
