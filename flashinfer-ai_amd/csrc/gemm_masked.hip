// Masked batched fp8 GEMM for expert-parallel MoE decode: fi_batch_gemm_fp8_nt_masked.
//
// What it replaces: the reference's batch_deepgemm_fp8_nt_groupwise (flashinfer/gemm.py:3121-3256, over
// deep_gemm.py m_grouped_fp8_gemm_nt_masked).  The layout is the low-latency all-to-all's: a (E, m, k) e4m3, b (E, n, k)
// e4m3, a_scale (E, m, k / 128) f32, b_scale (E, n / 128, k / 128) f32, d (E, m, n) f16 / bf16, and masked_m[e] on the
// DEVICE says how many leading rows of expert e are real.  With r = min(masked_m[e], m):
//   d[e, i, j] = sum_kb a_scale[e, i, kb] b_scale[e, j / 128, kb] sum_{k in block kb} a[e, i, k] b[e, j, k]     i < r
// f32 accumulation, one rounding.  Rows r .. m - 1 of a and a_scale are never loaded and those of d never stored.
//
// The regime is 1 .. 64 live rows per expert: every weight byte is read once and used for a handful of rows, so the
// kernel is built as a weight STREAM and the tile is BM tokens x 128 weight rows, BM = 16 / 32 / 64 / 128.
//
// Work comes from the device.  The grid is fixed (a multiple of the compute units, a multiple of 8).  Every workgroup
// reads masked_m, counts ceil(r / BM) row tiles per expert (thread t: experts 4 t .. 4 t + 3, so E <= 1024) and
// prefix-sums them with block_incl_scan into LDS: tile_start[e].  With R row tiles in all, row tile rt belongs to the
// expert found by a binary search of tile_start (uniform, LDS broadcasts).  Row tiles are dealt to the 8 XCDs
// interleaved -- XCD x (workgroups b with b & 7 == x) owns row tiles x, x + 8, ... , with one row tile per expert
// that is experts x, x + 8, ... -- and an XCD's workgroups walk its (row tile, n tile) pairs n tile fastest, strided by
// the XCD's workgroup count: the workgroups in flight together read DIFFERENT 128-row weight tiles, and a weight tile
// is read by ceil(r / BM) workgroups (one in the regime this is for), so every byte of b leaves HBM once.
//
// The product is computed TRANSPOSED (d^T = b a^T) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales: 16
// weight rows are the row operand, 16 tokens the column operand, one instruction covers a whole 128-wide k block.
// Each k block's product goes into a fresh accumulator that is folded into the running sum by one FMA with
// a_scale[row] * b_scale (the vector pipe idles in a streaming kernel), as gemm.hip folds its groupwise scales.  A
// row's sum is taken in the order of the k blocks whatever BM is, so the result does not depend on expected_m.
//
// Operand maps (lane l, c = l & 15, g = l >> 4).  The contraction index may be permuted freely as long as both
// operands use the same permutation (decode_fp8_kernel.h); here a lane holds 32 CONSECUTIVE bytes of its row:
//   row operand (weights)   lane (c, g): weight row c, bytes 32 g .. 32 g + 31 of the k block: registers 0-3 the 16-byte
//                           chunk 2 g, registers 4-7 chunk 2 g + 1
//   column operand (tokens) lane (c, g): token c, the same bytes
//   result                  register i of lane l is (weight row 4 g + i, token c): 4 consecutive n of one token, 8 bytes
// Weights: a wave owns 32 weight rows (two blocks of 16) and nobody else reads them, so they never touch LDS.  A
// load instruction has the 8 lanes (c = 2 p and 2 p + 1, g = 0 .. 3) fetch the 8 chunks of ONE row -- the first
// instruction of a block the even rows, the second the odd rows -- so every instruction reads 8 whole 128-byte lines,
// non-temporal; a swap between neighbouring lanes (one DPP move per register) then hands each lane the two chunks of
// its own row.  The stream runs P k blocks ahead in a ring of registers (P = 4; 2 at BM = 128).
// Tokens: the BM x 128-byte slab of a k block is shared by the 4 waves: global -> registers (P k blocks ahead, in
// the same ring, so that waiting for it never drains the weight stream) -> LDS image [BM][128 bytes] with the chunk
// swizzle of gemm_common.h (image_off; the 16-lane groups of the fragment reads hit 16 distinct slots), two buffers,
// one barrier per k block that waits for LDS only.  The slab's BM a_scale words travel with it.  Rows of the tile at
// or past r re-read row r - 1 (loads clamped) and are masked at the store.
#include "gemm_common.h"

namespace fi {

struct MaskedGemmParams {
  const uint8_t* a;
  const uint8_t* b;
  const float* a_scale;
  const float* b_scale;
  void* d;
  const int32_t* masked_m;
  int32_t num_experts, m, n, k;
  int32_t out_dtype;
};

constexpr int kMaskedThreads = 256;
constexpr int kMaskedWaves = kMaskedThreads / 64;
constexpr int kMaskedMaxExperts = 4 * kMaskedThreads;
constexpr int kMaskedWaveRows = kBN / kMaskedWaves;  // weight rows per wave: 2 blocks of 16

__device__ __forceinline__ f32x4 mfma_fp8_k128(const i32x8g& w, const i32x8g& x) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, f32x4{0.f, 0.f, 0.f, 0.f}, /*e4m3*/ 0, /*e4m3*/ 0, 0,
                                                          0x7F7F7F7F, 0, 0x7F7F7F7F);
}

template <int BM>
__global__ void __launch_bounds__(kMaskedThreads, 2) gemm_masked_kernel(const MaskedGemmParams p) {
  static_assert(BM == 16 || BM == 32 || BM == 64 || BM == 128, "row tile heights");
  constexpr int MB = BM / 16;            // token blocks of the tile
  constexpr int P = BM == 128 ? 2 : 4;   // k blocks in flight
  constexpr int AV = BM >= 32 ? BM / 32 : 1;  // 16-byte pieces of the token slab per thread (32 rows per pass)
  static_assert(P % 2 == 0, "the LDS buffer of k block i + j must be j & 1");

  __shared__ __attribute__((aligned(1024))) uint8_t a_img[2][BM * kBK];
  __shared__ float a_sc[2][BM];
  __shared__ int32_t tile_start[kMaskedMaxExperts];
  __shared__ int32_t wave_tot[kMaskedWaves];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const bool odd = (c & 1) != 0;
  const int E = p.num_experts, M = p.m, N = p.n, K = p.k;
  const int NT = N >> 7, KB = K >> 7;

  // ---- the live row tiles: tile_start[e] = row tiles of the experts below e, R = all of them ----
  int R;
  {
    int cnt[4], mine = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * tid + i;
      const int rows = e < E ? min(max(p.masked_m[e], 0), M) : 0;
      cnt[i] = (rows + BM - 1) / BM;
      mine += cnt[i];
    }
    int total;
    int run = block_incl_scan<kMaskedWaves>(mine, wave_tot, total) - mine;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tile_start[4 * tid + i] = run;  // experts past E: R, never found
      run += cnt[i];
    }
    __syncthreads();
    R = __builtin_amdgcn_readfirstlane(total);
  }

  // ---- this XCD's (row tile, n tile) pairs, n tile fastest, strided by its workgroups ----
  const int xcd = blockIdx.x & 7, wg_step = gridDim.x >> 3;
  const int my_pairs = ((R - xcd + 7) >> 3) * NT;

  // per-lane pieces that do not depend on the tile
  const int a_row = tid >> 3;                                   // + 32 v: row of the slab this thread stages
  const bool stages_a = a_row < BM, stages_sc = tid < BM;
  uint32_t w_off[2][2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      w_off[nb][h] = (uint32_t)(16 * nb + ((c & ~1) | h)) * (uint32_t)K + (uint32_t)(2 * g + (c & 1)) * 16;
  uint32_t x_rd[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) x_rd[mb] = (uint32_t)image_off(16 * mb + c, 2 * g);

  struct Gen {  // what k block i needs beyond the LDS image: the weights of i, the token slab and scales of i + 1
    u32x4 w[2][2];
    u32x4 a[AV];
    float sa, sb;
  };

  for (int pair = blockIdx.x >> 3; pair < my_pairs; pair += wg_step) {
    const int rq = pair / NT, nt = pair - rq * NT;
    const int rt = xcd + 8 * rq;
    int lo = 0, hi = E - 1;  // the last expert whose first tile is at or below rt: it owns rt
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tile_start[mid] <= rt) lo = mid;
      else hi = mid - 1;
    }
    const int e = __builtin_amdgcn_readfirstlane(lo);
    const int m0 = (rt - __builtin_amdgcn_readfirstlane(tile_start[e])) * BM;
    const int m_end = min(__builtin_amdgcn_readfirstlane(p.masked_m[e]), M);  // > m0: the tile is live
    const int n0 = nt * kBN + kMaskedWaveRows * wave;

    const uint8_t* const w_tile = p.b + ((int64_t)e * N + n0) * K;
    const uint8_t* const a_tile = p.a + (int64_t)e * M * K;
    const float* const sa_tile = p.a_scale + (int64_t)e * M * KB;
    const float* const sb_tile = p.b_scale + ((int64_t)e * NT + nt) * KB;
    uint32_t a_off[AV];
#pragma unroll
    for (int v = 0; v < AV; ++v) {
      const int row = 32 * v + a_row;
      a_off[v] = (uint32_t)min(m0 + row, m_end - 1) * (uint32_t)K + (uint32_t)(image_chunk(row, tid & 7) << 4);
    }
    const uint32_t sa_off = (uint32_t)min(m0 + tid, m_end - 1) * (uint32_t)KB;

    auto load_slab = [&](int kb, u32x4* a, float& sa) {
#pragma unroll
      for (int v = 0; v < AV; ++v) a[v] = *(const u32x4*)(a_tile + (a_off[v] + (uint32_t)kb * kBK));
      sa = sa_tile[sa_off + kb];
    };
    auto store_slab = [&](int buf, const u32x4* a, float sa) {
      if (stages_a) {
#pragma unroll
        for (int v = 0; v < AV; ++v) *(u32x4*)&a_img[buf][(32 * v + a_row) * kBK + (tid & 7) * 16] = a[v];
      }
      if (stages_sc) a_sc[buf][tid] = sa;
    };
    // a k block past the end re-loads the last one (no branch around a load)
    auto load_gen = [&](int i, Gen& r) {
      const uint32_t kw = (uint32_t)min(i, KB - 1);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          r.w[nb][h] = __builtin_nontemporal_load((const u32x4*)(w_tile + (w_off[nb][h] + kw * kBK)));
      r.sb = sb_tile[kw];
      load_slab(min(i + 1, KB - 1), r.a, r.sa);
    };

    f32x4 acc[2][MB];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

    Gen r[P];
    {
      u32x4 a0[AV];
      float sa0;
      load_slab(0, a0, sa0);
#pragma unroll
      for (int j = 0; j < P; ++j) load_gen(j, r[j]);
      store_slab(0, a0, sa0);  // the last tile's readers of buffer 0 are behind that tile's last barrier
      lds_barrier();
    }

    for (int i = 0; i < KB; i += P) {
#pragma unroll
      for (int j = 0; j < P; ++j) {
        if (i + j < KB) {
          const int buf = j & 1;
          store_slab(buf ^ 1, r[j].a, r[j].sa);  // k block i + j + 1; its readers of that buffer are behind a barrier
          const i32x8g fw[2] = {weight_frag(r[j].w[0][0], r[j].w[0][1], odd), weight_frag(r[j].w[1][0], r[j].w[1][1], odd)};
          const float sb = r[j].sb;
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            const uint8_t* const x = &a_img[buf][x_rd[mb]];
            const i32x8g fx = fp8_frag(x, &a_img[buf][x_rd[mb] ^ 16]);
            const float s = a_sc[buf][16 * mb + c] * sb;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
              const f32x4 part = mfma_fp8_k128(fw[nb], fx);
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[nb][mb][q] += s * part[q];
            }
          }
          lds_barrier();
          load_gen(i + j + P, r[j]);
        }
      }
    }

    // ---- store: a lane's 4 consecutive n of token c, 8 bytes; rows at or past m_end stay as they are ----
    uint16_t* const d_tile = (uint16_t*)p.d + (int64_t)e * M * N + n0 + 4 * g;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int row = m0 + 16 * mb + c;
      if (row < m_end) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          *(u32x2*)(d_tile + (int64_t)row * N + 16 * nb) = pack4_16bit(acc[nb][mb], 0, p.out_dtype);
      }
    }
  }
}

// smallest row tile that holds expected_m rows, 128 at most
static int masked_row_tile(int expected_m) { return expected_m <= 16 ? 16 : expected_m <= 32 ? 32 : expected_m <= 64 ? 64 : 128; }

static void launch_gemm_masked(const MaskedGemmParams& p, int bm, int cus, hipStream_t stream) {
  // two workgroups per compute unit (registers and LDS allow that for every BM), a multiple of 8 so that every XCD
  // has the same number
  const dim3 grid((uint32_t)std::max(8, 2 * cus / 8 * 8)), block(kMaskedThreads);
  switch (bm) {
    case 16: gemm_masked_kernel<16><<<grid, block, 0, stream>>>(p); break;
    case 32: gemm_masked_kernel<32><<<grid, block, 0, stream>>>(p); break;
    case 64: gemm_masked_kernel<64><<<grid, block, 0, stream>>>(p); break;
    default: gemm_masked_kernel<128><<<grid, block, 0, stream>>>(p); break;
  }
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_gemm_fp8_nt_masked(const fi_batch_gemm_fp8_nt_masked_params_t* p, fi_stream_t stream) {
  const char* who = "batch_gemm_fp8_nt_masked";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->num_experts >= 0 && p->m >= 0 && p->n >= 0 && p->k >= 0, "%s: negative size (E %d, m %d, n %d, k %d)", who,
             p->num_experts, p->m, p->n, p->k);
  FI_REQUIRE(p->num_experts <= kMaskedMaxExperts, "%s: %d experts, at most %d", who, p->num_experts, kMaskedMaxExperts);
  FI_REQUIRE(p->n % 128 == 0, "%s: n %d must be a multiple of 128", who, p->n);
  FI_REQUIRE(p->k > 0 && p->k % 128 == 0, "%s: k %d must be a positive multiple of 128", who, p->k);
  FI_REQUIRE(p->expected_m >= 1, "%s: expected_m %d must be at least 1", who, p->expected_m);
  FI_REQUIRE(p->d_dtype == FI_DTYPE_F16 || p->d_dtype == FI_DTYPE_BF16, "%s: output dtype %d is not f16 / bf16", who, p->d_dtype);
  FI_REQUIRE(p->a_stride_e == (int64_t)p->m * p->k && p->b_stride_e == (int64_t)p->n * p->k &&
                 p->d_stride_e == (int64_t)p->m * p->n,
             "%s: a, b and d must be contiguous (expert strides %lld, %lld, %lld for m %d, n %d, k %d)", who,
             (long long)p->a_stride_e, (long long)p->b_stride_e, (long long)p->d_stride_e, p->m, p->n, p->k);
  if (p->num_experts == 0 || p->m == 0 || p->n == 0) return 0;
  FI_REQUIRE(p->a && p->b && p->a_scale && p->b_scale && p->d && p->masked_m, "%s: null tensor", who);
  FI_REQUIRE(((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->d % 8) == 0 &&
                 ((uintptr_t)p->a_scale % 4) == 0 && ((uintptr_t)p->b_scale % 4) == 0 && ((uintptr_t)p->masked_m % 4) == 0,
             "%s: a / b must be 16-byte, d 8-byte, the scales and masked_m 4-byte aligned", who);
  // 32-bit offsets inside an expert's a and inside a wave's 32 weight rows
  FI_REQUIRE((int64_t)p->m * p->k < (1ll << 31) && (int64_t)kMaskedWaveRows * p->k < (1ll << 31),
             "%s: problem too large for 32-bit tile offsets (m %d, k %d)", who, p->m, p->k);
  FI_REQUIRE((int64_t)p->num_experts * ceil_div(p->m, 16) * (p->n / 128) < (1ll << 31), "%s: too many tiles", who);
  MaskedGemmParams g{};
  g.a = (const uint8_t*)p->a;
  g.b = (const uint8_t*)p->b;
  g.a_scale = p->a_scale;
  g.b_scale = p->b_scale;
  g.d = p->d;
  g.masked_m = p->masked_m;
  g.num_experts = p->num_experts;
  g.m = p->m;
  g.n = p->n;
  g.k = p->k;
  g.out_dtype = p->d_dtype;
  launch_gemm_masked(g, masked_row_tile(p->expected_m), fi_num_compute_units(), (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
