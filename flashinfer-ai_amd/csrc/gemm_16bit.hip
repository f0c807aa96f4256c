// Grouped f16 / bf16 NT GEMM for gfx950 with a fused row gather and a fused SwiGLU epilogue: the two matrix multiplies of
// the unquantised mixture-of-experts layer (cutlass_fused_moe, flashinfer/fused_moe/core.py:758-786 of the reference,
// whose CUTLASS grouped GEMM this replaces).  Contract in include/fi_mi355.h, design in DESIGN.md 3.13c.
//   d[r, :] = a[row(r), :] . b[g]^T   for m_indptr[g] <= r < m_indptr[g + 1],  row(r) = a_row_ids ? a_row_ids[r] / div : r
//   a (*, k) and b (G, n, k) of one 16-bit dtype, f32 accumulation on v_mfma_f32_32x32x16_{f16,bf16}, one rounding.
//
// Tile.  One workgroup (4 waves of 64 x 64, each 2 x 2 blocks of 32 x 32) owns 128 rows of one group x 128 rows of b[g]
// and walks k in steps of 64 elements = 128 bytes per row: the operand image of a step is the [rows][128 bytes] form
// whose 16-byte chunks image_chunk / image_off (gemm_common.h) swizzle, and a lane's 8 k elements of an MFMA are one
// ds_read_b128.  As in the fp8 kernels the product is computed TRANSPOSED (d^T = b a^T): the row of d sits on the
// lane and four consecutive columns in four consecutive accumulator registers, which pack into 8 bytes.
//
// Staging.  Operands go global -> LDS directly (global_load_lds_dwordx4, 1 KiB = 8 image rows per wave instruction, 8
// instructions per wave and step), kStages - 1 steps ahead through a ring of kStages 32 KB stages; the swizzle is
// applied on the global side (the lane that writes slot ch of a row fetches chunk image_chunk(row, ch)).  Every lane
// brings its own source address, so the gather costs nothing: the lanes of an A row read a[a_row_ids[r] / div] instead
// of a[r] and no permuted copy of the activations exists.  Rows past the end of the group (or past n) re-read the
// last valid row and are masked at the store.  Synchronisation is wait_vmcnt_barrier (common.h).
//
// SwiGLU.  b[g] is [2 I, k]: rows [0, I) the linear half (w3), rows [I, 2 I) the gate (w1).  A workgroup's 128 image
// rows of b are then the SAME 64 columns c0 .. c0 + 63 of both halves, ordered so that wave column wn holds columns
// c0 + 32 wn .. + 31 of w3 in its block 0 and of w1 in its block 1: register r of acc[0][mb] and of acc[1][mb] are x2
// and x1 of one output element, and the lane writes act = x1 sigmoid(alpha x1) (clamp(x2, -limit, limit) + beta), x1
// capped at limit, straight from the f32 accumulators as one 128 x 64 tile of [cum_m, I].
//
// Output.  Each wave turns a 64 x 32 block through 5 KB of LDS stage 0 (free after the loop's last barrier) and stores
// 64-byte row pieces, 16 bytes per lane.
#include <type_traits>

#include "gemm_common.h"

namespace fi {

constexpr int kG16Threads = 256;
constexpr int kG16StepBytes = 128;                            // 64 k elements of a row
constexpr int kG16StageBytes = (kBM + kBN) * kG16StepBytes;   // A rows 0-127, B rows 128-255
constexpr int kG16Stages = 2;                                 // ring depth (2 against 3, measured)
constexpr int kG16Pieces = kG16StageBytes / 1024 / 4;         // DMA instructions per wave and step

struct Gemm16Params {
  const uint8_t* a;
  const int32_t* a_row_ids;
  const uint8_t* b;
  uint16_t* d;
  const int32_t* m_indptr;
  const float* alpha;
  const float* beta;
  const float* limit;
  int32_t num_groups, cum_m, a_rows, a_row_ids_div, n, k;
  int32_t num_m_tiles_bound, n_tiles;
};

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

// c + b a^T over 16 k elements: lane l of either operand holds row l & 31, k elements 8 (l >> 5) .. + 7 of the 16
template <int DT>
__device__ __forceinline__ f32x16g mfma_16bit(const u32x4& b, const u32x4& a, const f32x16g& c) {
  if constexpr (DT == FI_DTYPE_BF16)
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, b), __builtin_bit_cast(f16x8, a), c, 0, 0, 0);
}

template <int DT, bool SWIGLU, int STAGES>
__global__ void __launch_bounds__(kG16Threads) group_gemm_16bit_kernel(const Gemm16Params p) {
  static_assert(STAGES == 2 || STAGES == 3, "ring depth");
  // one array: the compiler tells a DMA target from an LDS read by constant offsets inside ONE object
  __shared__ __attribute__((aligned(1024))) uint8_t smem[STAGES][kG16StageBytes];
  constexpr int kBOff = kBM * kG16StepBytes;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lq = lane & 31, lh = lane >> 5;

  // ---- tile assignment: XCD-contiguous logical id, banded order inside the XCD's range (gemm.hip) ----
  const int logical = xcd_share(p.num_m_tiles_bound * p.n_tiles, blockIdx.x & 7).start + (blockIdx.x >> 3);
  constexpr int kBandM = 8;
  int mt_global, nt, g, m_begin, m_end, mt;
  band_tile_of<kBandM>(logical, p.num_m_tiles_bound, p.n_tiles, mt_global, nt);
  if (!find_group_tile<kBM>(p.m_indptr, p.num_groups, mt_global, lane, g, m_begin, m_end, mt)) return;
  m_end = min(m_end, p.cum_m);  // rows at or past cum_m do not exist whatever m_indptr says
  const int m0 = m_begin + mt * kBM;
  if (m_begin < 0 || m0 >= m_end) return;  // the whole workgroup leaves, before any barrier
  const int N = p.n, K = p.k;
  const int I = N >> 1;                       // SWIGLU: columns of d
  const int n0 = nt * (SWIGLU ? kBN / 2 : kBN);  // first column of d
  const int ksteps = K >> 6;
  const uint8_t* const Bg = p.b + (int64_t)g * N * K * 2;

  // ---- DMA sources: wave w owns pieces 4 w .. 4 w + 3 of A and of B; a piece is 8 image rows, lane i -> slot i & 7 of
  // row i >> 3
  const uint8_t* src[kG16Pieces];
#pragma unroll
  for (int j = 0; j < kG16Pieces; ++j) {
    const int row = 8 * (4 * wave + (j & 3)) + (lane >> 3);  // of the tile's 128 A resp. B rows
    const int ch = image_chunk(row, lane & 7);
    if (j < kG16Pieces / 2) {
      int64_t r = min(m0 + row, m_end - 1);
      if (p.a_row_ids) r = min(max(p.a_row_ids[r] / p.a_row_ids_div, 0), p.a_rows - 1);
      src[j] = p.a + (r * K + ch * 8) * 2;
    } else {
      // SWIGLU: block (row >> 5) & 1 of wave column row >> 6 is the linear (0) resp. gate (1) half of the same columns
      const int br = SWIGLU ? ((row >> 5) & 1) * I + n0 + 32 * (row >> 6) + (row & 31) : min(n0 + row, N - 1);
      src[j] = Bg + ((int64_t)br * K + ch * 8) * 2;
    }
  }
  auto dma = [&](int ks, int stage) {
#pragma unroll
    for (int j = 0; j < kG16Pieces; ++j) {
      const int q = (j < kG16Pieces / 2 ? 0 : kBM / 8) + 4 * wave + (j & 3);
      lds_dma16(src[j] + (int64_t)ks * kG16StepBytes, &smem[stage][q * 1024]);
    }
  };

  f32x16g acc[2][2];  // [n block][m block]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- k loop: step ks reads stage ks % STAGES while the DMA of step ks + STAGES - 1 runs ----
  dma(0, 0);
  if (STAGES == 3 && ksteps > 1) dma(1, 1);
  if (STAGES == 3 && ksteps > 1) wait_vmcnt_barrier<kG16Pieces>();
  else wait_vmcnt_barrier<0>();
  auto k_step = [&](auto buf_c, const int ks) {
    constexpr int buf = decltype(buf_c)::value;  // == ks % STAGES
    // into the stage read in step ks - 1: every wave's reads of it finished in front of that step's barrier
    if (ks + STAGES - 1 < ksteps) dma(ks + STAGES - 1, (buf + STAGES - 1) % STAGES);
    const uint8_t* const stage = &smem[buf][0];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // 16 k elements: chunk 2 kk + lh of the row
      u32x4 fa[2], fb[2];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) fa[mb] = *(const u32x4*)(stage + image_off(64 * wm + 32 * mb + lq, 2 * kk + lh));
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        fb[nb] = *(const u32x4*)(stage + kBOff + image_off(64 * wn + 32 * nb + lq, 2 * kk + lh));
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) acc[nb][mb] = mfma_16bit<DT>(fb[nb], fa[mb], acc[nb][mb]);
    }
    // the next step's operands landed (all waves' pieces: barrier); with three stages the pieces of the step after it
    // stay in flight
    if (STAGES == 3 && ks + 2 < ksteps) wait_vmcnt_barrier<kG16Pieces>();
    else wait_vmcnt_barrier<0>();
  };
  for (int ks = 0; ks < ksteps; ks += STAGES) {
    k_step(std::integral_constant<int, 0>{}, ks);
    if (ks + 1 < ksteps) k_step(std::integral_constant<int, 1>{}, ks + 1);
    if constexpr (STAGES == 3)
      if (ks + 2 < ksteps) k_step(std::integral_constant<int, 2>{}, ks + 2);
  }

  // ---- epilogue: v[mb] is a 64 (m) x 32 block of d at column `col`; a lane holds row 32 mb + lq, register 4 r4 + i is
  // column 8 r4 + 4 lh + i
  constexpr int kOutStride = 80;
  uint8_t* const scratch = &smem[0][0] + wave * (64 * kOutStride);
  const int width = SWIGLU ? I : N;
  auto store_block = [&](const f32x16g (&v)[2], int col) {
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        *(u32x2*)(scratch + (32 * mb + lq) * kOutStride + (8 * r4 + 4 * lh) * 2) = pack4_16bit(v[mb], 4 * r4, DT);
#pragma unroll
    for (int i2 = 0; i2 < 4; ++i2) {
      const int idx = lane + 64 * i2;
      const int r = idx >> 2, c = idx & 3;
      const u32x4 piece = *(const u32x4*)(scratch + r * kOutStride + c * 16);
      const int m = m0 + 64 * wm + r;
      if (m < m_end) store_row_piece(p.d + (int64_t)m * width + col + 8 * c, piece, true);
    }
  };
  if constexpr (SWIGLU) {
    const float alpha = p.alpha ? p.alpha[g] : 1.f;
    const float beta = p.beta ? p.beta[g] : 0.f;
    const float limit = p.limit ? p.limit[g] : INFINITY;
    f32x16g act[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float x1 = fminf(acc[1][mb][r], limit);
        const float x2 = fminf(fmaxf(acc[0][mb][r], -limit), limit) + beta;
        act[mb][r] = x1 * (1.0f / (1.0f + expf(-alpha * x1))) * x2;
      }
    store_block(act, n0 + 32 * wn);
  } else {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int col = n0 + 64 * wn + 32 * nb;
      if (col < N) store_block(acc[nb], col);  // n is a multiple of 64: a block is inside or outside
    }
  }
}

template <int DT, bool SWIGLU>
static void launch_gemm_16bit(const Gemm16Params& p, hipStream_t stream) {
  group_gemm_16bit_kernel<DT, SWIGLU, kG16Stages>
      <<<dim3((uint32_t)p.num_m_tiles_bound * (uint32_t)p.n_tiles), dim3(kG16Threads), 0, stream>>>(p);
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_group_gemm_16bit_nt(const fi_group_gemm_16bit_params_t* p, fi_stream_t stream) {
  const char* who = "group_gemm_16bit_nt";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->num_groups >= 0 && p->cum_m >= 0 && p->n >= 0 && p->k >= 0 && p->a_rows >= 0,
             "%s: negative size (num_groups %d, cum_m %d, a_rows %d, n %d, k %d)", who, p->num_groups, p->cum_m, p->a_rows,
             p->n, p->k);
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "%s: dtype %d is not f16 or bf16", who, p->dtype);
  const bool swiglu = p->epilogue == FI_GEMM16_EPILOGUE_SWIGLU;
  FI_REQUIRE(swiglu || p->epilogue == FI_GEMM16_EPILOGUE_NONE, "%s: epilogue %d is not provided", who, p->epilogue);
  FI_REQUIRE(p->num_groups <= FI_MOE_MAX_EXPERTS, "%s: num_groups %d is not in [0, %d]", who, p->num_groups,
             FI_MOE_MAX_EXPERTS);
  FI_REQUIRE(p->k > 0 && p->k % 64 == 0, "%s: k %d must be a positive multiple of 64", who, p->k);
  FI_REQUIRE(p->n % (swiglu ? 128 : 64) == 0, "%s: n %d must be a multiple of %d%s", who, p->n, swiglu ? 128 : 64,
             swiglu ? " (both halves of the SwiGLU weight a multiple of 64 rows)" : "");
  const int gates = (p->alpha != nullptr) + (p->beta != nullptr) + (p->limit != nullptr);
  FI_REQUIRE(gates == 0 || (gates == 3 && swiglu), "%s: alpha, beta and limit come all three or not at all, with the SwiGLU "
             "epilogue only", who);
  if (p->num_groups == 0 || p->cum_m == 0 || p->n == 0) return 0;
  FI_REQUIRE(p->a && p->b && p->d && p->m_indptr, "%s: null tensor", who);
  FI_REQUIRE(((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->d % 16) == 0,
             "%s: a, b and d must be 16-byte aligned", who);
  FI_REQUIRE(((uintptr_t)p->m_indptr % 4) == 0 && ((uintptr_t)p->a_row_ids % 4) == 0 && ((uintptr_t)p->alpha % 4) == 0 &&
                 ((uintptr_t)p->beta % 4) == 0 && ((uintptr_t)p->limit % 4) == 0,
             "%s: m_indptr, a_row_ids, alpha, beta and limit must be 4-byte aligned", who);
  if (p->a_row_ids)
    FI_REQUIRE(p->a_rows >= 1 && p->a_row_ids_div >= 1, "%s: a_row_ids needs a_rows %d >= 1 and a_row_ids_div %d >= 1", who,
               p->a_rows, p->a_row_ids_div);
  else
    FI_REQUIRE(p->a_rows >= p->cum_m, "%s: a holds %d rows, cum_m %d needed", who, p->a_rows, p->cum_m);
  Gemm16Params g{};
  g.a = (const uint8_t*)p->a;
  g.a_row_ids = p->a_row_ids;
  g.b = (const uint8_t*)p->b;
  g.d = (uint16_t*)p->d;
  g.m_indptr = p->m_indptr;
  g.alpha = p->alpha;
  g.beta = p->beta;
  g.limit = p->limit;
  g.num_groups = p->num_groups;
  g.cum_m = p->cum_m;
  g.a_rows = p->a_rows;
  g.a_row_ids_div = p->a_row_ids_div;
  g.n = p->n;
  g.k = p->k;
  // every group adds at most one partial tile on top of cum_m / 128
  g.num_m_tiles_bound = p->cum_m / kBM + p->num_groups;
  g.n_tiles = swiglu ? p->n / kBN : ceil_div(p->n, kBN);
  FI_REQUIRE((int64_t)g.num_m_tiles_bound * g.n_tiles < (1ll << 31), "%s: too many tiles", who);
  hipStream_t st = (hipStream_t)stream;
  if (p->dtype == FI_DTYPE_BF16) {
    if (swiglu) launch_gemm_16bit<FI_DTYPE_BF16, true>(g, st);
    else launch_gemm_16bit<FI_DTYPE_BF16, false>(g, st);
  } else {
    if (swiglu) launch_gemm_16bit<FI_DTYPE_F16, true>(g, st);
    else launch_gemm_16bit<FI_DTYPE_F16, false>(g, st);
  }
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
