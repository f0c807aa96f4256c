// Segment GEMM for multi-LoRA batches on gfx950 (SegmentGEMMWrapper, flashinfer/gemm.py:1300-1553 of the reference, whose
// CUTLASS grouped GEMM this replaces).  Contract in include/fi_mi355.h, design in DESIGN.md 3.17.
//   y[r, :] = x[r, :] . W[weight(s)]   for the rows r of segment s,  weight(s) = weight_indices ? weight_indices[s] : s
//   x (rows, d_in), y (rows, d_out) and W of one 16-bit dtype; W[w] is (d_out, d_in) ("column major": k contiguous) or
//   (d_in, d_out) ("row major": n contiguous); f32 accumulation on v_mfma_f32_16x16x32_{f16,bf16}, one rounding.
//
// A LoRA step has a rank (8 .. 128) on one side, so one side of the product is SKINNY and the 128 x 128 tile of
// gemm_16bit.hip would be padding.  Everything here is built from one unit, a wave's k step:
//   32 k elements x 64 (or 32) columns of W as the MFMA's A operand, 16 rows of x as its B operand (d^T = W^T x^T).
// The product is transposed and the columns of a 32-column PAIR of blocks are dealt to the two blocks so that
//   block b, operand row rho  <->  column 8 (rho >> 2) + 4 b + (rho & 3)  of the pair:
// lane (c = lane & 15, g = lane >> 4) then holds, in the four accumulator registers of block 0 and of block 1, columns
// 8 g .. 8 g + 7 of row c of y -- one 16-byte store, no turn through LDS.
//
// Weight operand of a step (WeightStep): column major, lane (c, g) loads its 16 bytes W[n(c, b)][32 ks + 8 g .. + 7]
// straight into the operand registers.  Row major, the wave loads the step's 32 k rows x 64 columns as coalesced
// 16-byte chunks (8 lanes per 128-byte row), writes them to a wave-private LDS piece and reads the operand back
// TRANSPOSED with ds_read_b64_tr_b16: the 16 lanes of group g present rows 8 g + (c >> 2) (+ 4 for the second read),
// columns 8 (c & 3) + 4 b .. + 3, and lane c receives column 8 (c >> 2) + 4 b + (c & 3) of four rows -- the same
// operand as above.  No workgroup barrier: the LDS operations of one wave execute in order.
//
// Two forms, chosen on the host from (d_in, d_out) alone (segment_gemm_long_k below):
//   long k (shrink): a workgroup owns 16 rows x <= 64 columns; its four waves take the k steps 4 i + w, so one
//     iteration of the workgroup reads 256 contiguous bytes of every row, each wave keeps f32 partial accumulators over
//     its steps (kLongBatch steps of loads in flight), and the four partials are summed through LDS in wave order and
//     rounded once.
//   wide n (expand, and every other shape): a workgroup owns 32 rows x 256 columns, wave w columns 64 w .. + 63.  The x
//     tile of 128 k elements is staged once per workgroup in LDS (two buffers, one barrier per 128 k) and read by every
//     wave as the B operand of two row blocks, so a weight operand is used twice.
// k tail: d_in % 8 == 0, so a lane's 16 bytes are inside or outside; outside they are zero in BOTH operands.  n tail
// (d_out % 8 == 0 likewise) and row tail: clamped or zero on the way in, masked at the store.
//
// Segments: segment_records_kernel (one workgroup) turns seg_lens or seg_indptr (int64, device) and weight_indices
// into int32 records {first row, end row, first tile, weight id} in the caller's workspace, the tile total in front;
// a workgroup finds its segment by binary search on "first tile".  The grid is the host bound ceil(rows / TILE_M) +
// batch_size, so there is no device-to-host copy.  Bounds are clamped into [0, rows]; a segment of negative length or
// with a weight id outside [0, num_weights) gets no tiles.
#include "gemm_common.h"

namespace fi {

constexpr int kSegThreads = 256;
constexpr int kSegHeaderInts = 4;     // ws[0]: tile total; the records follow, 16 bytes each
constexpr int kLongTileM = 16;        // rows per workgroup, long-k form
constexpr int kWideTileM = 32;        // rows per workgroup, wide-n form
constexpr int kWideTileN = 256;       // columns per workgroup, wide-n form
constexpr int kLongBatch = 4;         // k steps of loads a long-k wave keeps in flight
constexpr int kWStagePitch = 144;     // row-major stage: 32 k rows of 128 bytes, padded
constexpr int kWStageBytes = 32 * kWStagePitch;
constexpr int kXChunkK = 128;         // k elements of x per LDS stage, wide-n form
constexpr int kXPitch = kXChunkK * 2 + 16;  // 16 rows of a ds_read_b128 lane group hit 16 distinct 4-bank windows

struct SegGemmParams {
  const uint8_t* x;
  const uint8_t* w;
  uint16_t* y;
  const int32_t* ws;
  int32_t d_in, d_out, batch_size, n_tiles;
};

using i32x4 = __attribute__((ext_vector_type(4))) int32_t;
using bf16x8s = __attribute__((ext_vector_type(8))) __bf16;
using f16x8s = __attribute__((ext_vector_type(8))) _Float16;
using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;

// c + a b over 32 k elements: lane (c, g) of a holds row c, of b column c, k elements 8 g .. 8 g + 7; register j of the
// result is row 4 g + j, column c
template <int DT>
__device__ __forceinline__ f32x4 seg_mfma(const u32x4& a, const u32x4& b, const f32x4& c) {
  if constexpr (DT == FI_DTYPE_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8s, a), __builtin_bit_cast(bf16x8s, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8s, a), __builtin_bit_cast(f16x8s, b), c, 0, 0, 0);
}

// ---- segment records ----
__global__ void __launch_bounds__(kSegThreads) segment_records_kernel(const int64_t* seg_lens, const int64_t* seg_indptr,
                                                                      const int64_t* weight_indices, int32_t* ws,
                                                                      int batch_size, int rows, int num_weights, int tile_m) {
  __shared__ int64_t wave_tot[kSegThreads / 64];
  const int64_t R = rows;
  int64_t row_base = 0, tile_base = 0;  // rows resp. tiles of the segments of earlier passes
  for (int base = 0; base < batch_size; base += kSegThreads) {
    const int i = base + (int)threadIdx.x;
    const bool live = i < batch_size;
    int64_t begin = 0, end = 0;
    if (seg_indptr) {
      if (live) {
        begin = min(max(seg_indptr[i], (int64_t)0), R);
        end = min(max(seg_indptr[i + 1], (int64_t)0), R);
      }
    } else {
      const int64_t len = live ? min(max(seg_lens[i], (int64_t)0), R) : 0;
      int64_t total;
      const int64_t incl = block_incl_scan<kSegThreads / 64>(len, wave_tot, total);
      begin = min(row_base + incl - len, R);
      end = min(row_base + incl, R);
      row_base = min(row_base + total, R);
    }
    int64_t wid = live ? (weight_indices ? weight_indices[i] : (int64_t)i) : -1;
    if (wid < 0 || wid >= num_weights) wid = -1;
    const int64_t tiles = (wid >= 0 && end > begin) ? (end - begin + tile_m - 1) / tile_m : 0;
    int64_t tiles_total;
    const int64_t first = tile_base + block_incl_scan<kSegThreads / 64>(tiles, wave_tot, tiles_total) - tiles;
    if (live)
      *(i32x4*)(ws + kSegHeaderInts + 4 * (int64_t)i) =
          i32x4{(int32_t)begin, (int32_t)end, (int32_t)min(first, (int64_t)INT32_MAX), (int32_t)wid};
    tile_base += tiles_total;
  }
  if (threadIdx.x == 0) ws[0] = (int32_t)min(tile_base, (int64_t)INT32_MAX);
}

// The rows [m0, m_end) and the weight of tile t, false when there is none (the grid bound counts one partial tile per
// segment).  Uniform per workgroup.
template <int TILE_M>
__device__ __forceinline__ bool segment_of_tile(const SegGemmParams& p, int t, int& m0, int& m_end, int& wid) {
  if (t >= p.ws[0]) return false;
  const i32x4* const rec = (const i32x4*)(p.ws + kSegHeaderInts);
  // the last segment whose first tile is <= t: the segments behind it that start at the same tile are empty
  const int s = smallest_fitting<int>(0, p.batch_size, [&](int i) { return rec[i][2] <= t; }) - 1;
  if (s < 0) return false;
  const i32x4 r = rec[s];
  const int64_t first_row = r[0] + (int64_t)(t - r[2]) * TILE_M;
  m0 = (int)first_row, m_end = r[1], wid = r[3];
  return wid >= 0 && r[0] >= 0 && first_row < m_end;
}

// ---- the weight operand of one k step: P pairs of blocks = 32 P columns from column n0 on ----
// fetch() issues the global loads of step ks, operand() hands out the 2 P MFMA operands (block b of pair p at 2 p + b).
template <bool COLMAJOR, int P>
struct WeightStep {
  u32x4 raw[2 * P];

  __device__ __forceinline__ void fetch(const uint8_t* wg, int d_in, int d_out, int n0, int ks, int lane) {
    const u32x4 zero = {0, 0, 0, 0};
    if constexpr (COLMAJOR) {
      const int c = lane & 15, g = lane >> 4;
      const int k = 32 * ks + 8 * g;
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {
        const int n = n0 + 32 * (i >> 1) + 8 * (c >> 2) + 4 * (i & 1) + (c & 3);
        raw[i] = (k < d_in && n < d_out) ? *(const u32x4*)(wg + ((int64_t)n * d_in + k) * 2) : zero;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {  // chunk lane + 64 i of the step's 32 rows x 4 P chunks of 8 columns
        const int idx = lane + 64 * i;
        const int k = 32 * ks + idx / (4 * P), n = n0 + 8 * (idx % (4 * P));
        raw[i] = (k < d_in && n < d_out) ? *(const u32x4*)(wg + ((int64_t)k * d_out + n) * 2) : zero;
      }
    }
  }

  // Row major: through `stage`, this wave's kWStageBytes of LDS.  The wave barriers keep the compiler from moving the
  // writes of the next step in front of these reads.
  __device__ __forceinline__ void operand(uint8_t* stage, int lane, u32x4 (&a)[2 * P]) const {
    if constexpr (COLMAJOR) {
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) a[i] = raw[i];
    } else {
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {
        const int idx = lane + 64 * i;
        *(u32x4*)(stage + (idx / (4 * P)) * kWStagePitch + (idx % (4 * P)) * 16) = raw[i];
      }
      __builtin_amdgcn_wave_barrier();
      const int c = lane & 15, g = lane >> 4;
      const uint8_t* const rd = stage + (8 * g + (c >> 2)) * kWStagePitch + (c & 3) * 16;
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) {
        const uint8_t* const at = rd + 64 * (i >> 1) + 8 * (i & 1);
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(at));
        const s16x4 hi =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(at + 4 * kWStagePitch));
        a[i] = __builtin_bit_cast(u32x4, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
};

// columns 8 g .. 8 g + 7 of a pair for row c: block 0 holds the lower four, block 1 the upper four
template <int DT>
__device__ __forceinline__ u32x4 pack_pair(const f32x4& b0, const f32x4& b1) {
  return u32x4{pack_16bit(b0[0], b0[1], DT), pack_16bit(b0[2], b0[3], DT), pack_16bit(b1[0], b1[1], DT),
               pack_16bit(b1[2], b1[3], DT)};
}

// ---- long-k form ----
template <int DT, bool COLMAJOR, int P>
__global__ void __launch_bounds__(kSegThreads) segment_gemm_long_k_kernel(const SegGemmParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t w_stage[COLMAJOR ? 1 : 4][COLMAJOR ? 16 : kWStageBytes];
  __shared__ f32x4 partial[4][2 * P][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int t = blockIdx.x / p.n_tiles, n0 = (blockIdx.x % p.n_tiles) * (32 * P);
  int m0, m_end, wid;
  if (!segment_of_tile<kLongTileM>(p, t, m0, m_end, wid)) return;  // the whole workgroup, before any barrier
  const int d_in = p.d_in, d_out = p.d_out;
  const int ksteps = (d_in + 31) >> 5;
  const uint8_t* const wg = p.w + (int64_t)wid * d_in * d_out * 2;
  const uint8_t* const xrow = p.x + (int64_t)min(m0 + c, m_end - 1) * d_in * 2;  // rows past the end repeat the last

  f32x4 acc[2 * P];
#pragma unroll
  for (int i = 0; i < 2 * P; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // wave w owns the steps 4 i + w; a step past the end loads nothing (k >= d_in) and adds zeros
  for (int ks0 = wave; ks0 < ksteps; ks0 += 4 * kLongBatch) {
    WeightStep<COLMAJOR, P> ws[kLongBatch];
    u32x4 xb[kLongBatch];
#pragma unroll
    for (int u = 0; u < kLongBatch; ++u) {
      const int ks = ks0 + 4 * u;
      const int k = 32 * ks + 8 * g;
      xb[u] = k < d_in ? *(const u32x4*)(xrow + k * 2) : u32x4{0, 0, 0, 0};
      ws[u].fetch(wg, d_in, d_out, n0, ks, lane);
    }
#pragma unroll
    for (int u = 0; u < kLongBatch; ++u) {
      u32x4 a[2 * P];
      ws[u].operand(w_stage[COLMAJOR ? 0 : wave], lane, a);
#pragma unroll
      for (int i = 0; i < 2 * P; ++i) acc[i] = seg_mfma<DT>(a[i], xb[u], acc[i]);
    }
  }

  // the four partial tiles, summed in wave order; wave w < P rounds and stores pair w
#pragma unroll
  for (int i = 0; i < 2 * P; ++i) partial[wave][i][lane] = acc[i];
  __syncthreads();
  if (wave >= P) return;
  f32x4 sum[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    sum[b] = partial[0][2 * wave + b][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) sum[b] += partial[w][2 * wave + b][lane];
  }
  const int m = m0 + c, n = n0 + 32 * wave + 8 * g;
  if (m < m_end && n < d_out) store_row_piece(p.y + (int64_t)m * d_out + n, pack_pair<DT>(sum[0], sum[1]), true);
}

// ---- wide-n form ----
template <int DT, bool COLMAJOR>
__global__ void __launch_bounds__(kSegThreads) segment_gemm_wide_n_kernel(const SegGemmParams p) {
  constexpr int P = 2, MB = kWideTileM / 16, STEPS = kXChunkK / 32;
  __shared__ __attribute__((aligned(16))) uint8_t w_stage[COLMAJOR ? 1 : 4][COLMAJOR ? 16 : kWStageBytes];
  __shared__ __attribute__((aligned(16))) uint8_t x_stage[2][kWideTileM * kXPitch];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int t = blockIdx.x / p.n_tiles, n0 = (blockIdx.x % p.n_tiles) * kWideTileN + 64 * wave;
  int m0, m_end, wid;
  if (!segment_of_tile<kWideTileM>(p, t, m0, m_end, wid)) return;  // the whole workgroup, before any barrier
  const int d_in = p.d_in, d_out = p.d_out;
  const int chunks = (d_in + kXChunkK - 1) / kXChunkK;
  const uint8_t* const wg = p.w + (int64_t)wid * d_in * d_out * 2;

  // x staging: thread tid brings 16-byte piece tid & 15 of tile rows tid >> 4 and 16 + (tid >> 4); 16 lanes read 256
  // contiguous bytes
  const int xs_row = tid >> 4, xs_ch = tid & 15;
  const uint8_t* xsrc[MB];
#pragma unroll
  for (int h = 0; h < MB; ++h) xsrc[h] = p.x + (int64_t)min(m0 + 16 * h + xs_row, m_end - 1) * d_in * 2;
  u32x4 xr[MB];
  auto load_x = [&](int kc) {
    const int k = kXChunkK * kc + 8 * xs_ch;
#pragma unroll
    for (int h = 0; h < MB; ++h) xr[h] = k < d_in ? *(const u32x4*)(xsrc[h] + k * 2) : u32x4{0, 0, 0, 0};
  };

  f32x4 acc[MB][2 * P];
#pragma unroll
  for (int h = 0; h < MB; ++h)
#pragma unroll
    for (int i = 0; i < 2 * P; ++i) acc[h][i] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x(0);
  for (int kc = 0; kc < chunks; ++kc) {
    uint8_t* const xs = x_stage[kc & 1];
    // this buffer was last read in chunk kc - 2: every wave left those reads before the barrier of chunk kc - 1
#pragma unroll
    for (int h = 0; h < MB; ++h) *(u32x4*)(xs + (16 * h + xs_row) * kXPitch + xs_ch * 16) = xr[h];
    WeightStep<COLMAJOR, P> ws[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s)
      if (32 * (STEPS * kc + s) < d_in) ws[s].fetch(wg, d_in, d_out, n0, STEPS * kc + s, lane);
    __syncthreads();
    if (kc + 1 < chunks) load_x(kc + 1);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      if (32 * (STEPS * kc + s) >= d_in) break;
      u32x4 a[2 * P], xb[MB];
#pragma unroll
      for (int h = 0; h < MB; ++h) xb[h] = *(const u32x4*)(xs + (16 * h + c) * kXPitch + (4 * s + g) * 16);
      ws[s].operand(w_stage[COLMAJOR ? 0 : wave], lane, a);
#pragma unroll
      for (int h = 0; h < MB; ++h)
#pragma unroll
        for (int i = 0; i < 2 * P; ++i) acc[h][i] = seg_mfma<DT>(a[i], xb[h], acc[h][i]);
    }
  }

#pragma unroll
  for (int h = 0; h < MB; ++h)
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const int m = m0 + 16 * h + c, n = n0 + 32 * q + 8 * g;
      if (m < m_end && n < d_out)
        store_row_piece(p.y + (int64_t)m * d_out + n, pack_pair<DT>(acc[h][2 * q], acc[h][2 * q + 1]), true);
    }
}

// The form of a call: the long-k form when the output is at most 128 columns wide and the reduction long enough to
// give each of the four waves at least two k steps.  A function of the shape alone.
static bool segment_gemm_long_k(int d_in, int d_out) { return d_out <= 128 && d_in >= 256; }

template <int DT, bool COLMAJOR>
static void launch_segment_gemm(const SegGemmParams& p, bool long_k, uint32_t grid, hipStream_t stream) {
  if (!long_k) segment_gemm_wide_n_kernel<DT, COLMAJOR><<<dim3(grid), dim3(kSegThreads), 0, stream>>>(p);
  else if (p.d_out <= 32) segment_gemm_long_k_kernel<DT, COLMAJOR, 1><<<dim3(grid), dim3(kSegThreads), 0, stream>>>(p);
  else segment_gemm_long_k_kernel<DT, COLMAJOR, 2><<<dim3(grid), dim3(kSegThreads), 0, stream>>>(p);
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_segment_gemm(const fi_segment_gemm_params_t* p, fi_stream_t stream) {
  const char* who = "segment_gemm";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->rows >= 0 && p->d_in >= 0 && p->d_out >= 0 && p->batch_size >= 0 && p->num_weights >= 0,
             "%s: negative size (rows %d, d_in %d, d_out %d, batch_size %d, num_weights %d)", who, p->rows, p->d_in,
             p->d_out, p->batch_size, p->num_weights);
  FI_REQUIRE(p->dtype == FI_DTYPE_F16 || p->dtype == FI_DTYPE_BF16, "%s: dtype %d is not f16 or bf16", who, p->dtype);
  FI_REQUIRE(p->d_in % 8 == 0 && p->d_out % 8 == 0, "%s: d_in %d and d_out %d must be multiples of 8", who, p->d_in,
             p->d_out);
  FI_REQUIRE(p->seg_lens || p->seg_indptr, "%s: neither seg_lens nor seg_indptr", who);
  if (p->rows == 0 || p->batch_size == 0 || p->d_out == 0 || p->num_weights == 0) return 0;
  FI_REQUIRE(p->d_in > 0, "%s: d_in must be positive", who);
  FI_REQUIRE(p->x && p->weights && p->y && p->int_workspace, "%s: null tensor", who);
  FI_REQUIRE(((uintptr_t)p->x % 16) == 0 && ((uintptr_t)p->weights % 16) == 0 && ((uintptr_t)p->y % 16) == 0 &&
                 ((uintptr_t)p->int_workspace % 16) == 0,
             "%s: x, weights, y and int_workspace must be 16-byte aligned", who);
  FI_REQUIRE(((uintptr_t)p->seg_lens % 8) == 0 && ((uintptr_t)p->seg_indptr % 8) == 0 &&
                 ((uintptr_t)p->weight_indices % 8) == 0,
             "%s: seg_lens, seg_indptr and weight_indices must be 8-byte aligned", who);
  const int64_t need = 4 * ((int64_t)kSegHeaderInts + 4 * (int64_t)p->batch_size);
  FI_REQUIRE(p->int_workspace_bytes >= need, "%s: int_workspace of %lld bytes cannot hold %d segment records (%lld bytes)",
             who, (long long)p->int_workspace_bytes, p->batch_size, (long long)need);
  const bool long_k = segment_gemm_long_k(p->d_in, p->d_out);
  const int tile_m = long_k ? kLongTileM : kWideTileM;
  SegGemmParams g{};
  g.x = (const uint8_t*)p->x;
  g.w = (const uint8_t*)p->weights;
  g.y = (uint16_t*)p->y;
  g.ws = (const int32_t*)p->int_workspace;
  g.d_in = p->d_in;
  g.d_out = p->d_out;
  g.batch_size = p->batch_size;
  g.n_tiles = long_k ? ceil_div(p->d_out, p->d_out <= 32 ? 32 : 64) : ceil_div(p->d_out, kWideTileN);
  // every segment adds at most one partial tile on top of rows / tile_m
  const int64_t grid = ((int64_t)ceil_div(p->rows, tile_m) + p->batch_size) * g.n_tiles;
  FI_REQUIRE(grid < (1ll << 31), "%s: too many tiles", who);
  hipStream_t st = (hipStream_t)stream;
  segment_records_kernel<<<dim3(1), dim3(kSegThreads), 0, st>>>(p->seg_indptr ? nullptr : p->seg_lens, p->seg_indptr,
                                                                p->weight_indices, (int32_t*)p->int_workspace,
                                                                p->batch_size, p->rows, p->num_weights, tile_m);
  const bool colmajor = p->weight_column_major != 0;
  if (p->dtype == FI_DTYPE_BF16) {
    if (colmajor) launch_segment_gemm<FI_DTYPE_BF16, true>(g, long_k, (uint32_t)grid, st);
    else launch_segment_gemm<FI_DTYPE_BF16, false>(g, long_k, (uint32_t)grid, st);
  } else {
    if (colmajor) launch_segment_gemm<FI_DTYPE_F16, true>(g, long_k, (uint32_t)grid, st);
    else launch_segment_gemm<FI_DTYPE_F16, false>(g, long_k, (uint32_t)grid, st);
  }
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
