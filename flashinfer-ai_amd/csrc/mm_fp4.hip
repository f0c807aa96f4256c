// Dense MXFP4 x MXFP4 matmul on the block-scaled MFMA of gfx950: fi_mm_mxfp4.
//
// What it replaces: the reference's mm_fp4 in its MXFP4 mode (use_nvfp4=False, block_size=32; flashinfer/gemm.py:2012-2160).
//   d[r, j] = alpha . sum_k e2m1(a[r, k]) 2^(sa[r, k/32] - 127) . e2m1(b[j, k]) 2^(sb[j, k/32] - 127)
//   a (m, k/2) and b (n, k/2) bytes (k = 2i in the low nibble of byte i), scales E8M0 bytes in the swizzled 128x4 layout
//   of mx_layout.h, f32 accumulation, alpha (a device float, optional) multiplied in f32, one rounding to f16 / bf16.
//
// v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4 takes both operands as fp4 and scales every run of 32 k
// elements of every row and column by its own E8M0 byte, so nibbles and scale bytes go from memory into the
// instruction unchanged.  As in gemm_mxfp4.hip the product is computed TRANSPOSED (d^T = b a^T): 16 weight rows are the
// MFMA's row operand, 16 tokens its column operand, and a lane ends up with 4 consecutive n of one token (8 bytes).
//
// Two kernels, one entry point (FI_MM_FP4_KERNEL: 0 / unset = by m, 1 = streaming, 2 = tiled):
//
//   streaming (few rows)  A wave owns 32 weight rows x 16 MB tokens (MB = 1, 2, 4) and streams its weight bytes from
//       global memory straight into registers, kStreamDepth k steps ahead, no LDS stage for the operands.  There is no
//       expert dimension to fill the chip, so while 128-row workgroups would leave compute units without one, the 4
//       waves of a workgroup share 32 weight rows and SPLIT K: wave w takes the k steps w, w + 4, ... (n = 8192 gives 256
//       workgroups), the four partial sums meet in LDS and wave 0 adds them in wave order, so the result does not
//       depend on scheduling: no float atomics, no second launch.  With rows enough, every wave runs all of k for its
//       own 32 rows and nothing is reduced.
//   tiled (many rows)     128 tokens x 128 weight rows per workgroup, 4 waves of 64 x 64.  Both operands and the 512-byte
//       scale blocks of two k steps (2 x 128 elements = 128 bytes per row) go global -> LDS by global_load_lds, 16
//       bytes per lane for the operands, into one of two buffers; the DMA of stage s + 1 flies while stage s computes.
//       The LDS image is linear, [row][128 bytes]; the 16-byte chunk a lane FETCHES is chunk (slot ^ key(row)),
//       key(row) = (row >> 1) & 7, which makes the 16-lane groups of the ds_read_b128 fragment reads hit 16 distinct
//       slots.  The swizzled scale layout is already grouped by 128 rows x 4 k blocks: the block of (row tile, k step)
//       is 512 contiguous bytes and a row's dword holds its four scales.  Rows past the edge of m or n re-read the
//       last valid row and are masked at the store.
//
// Operand lane maps with BOTH operands fp4 (lane l, c = l & 15, q = l >> 4).  gemm_mxfp4.hip had the fp4 map as the row
// operand only; as the column operand it was a supposition (that it mirrors the row operand), pinned since by the
// one-hot tests of tests/test_mm_fp4_gpu.py, which are bit-exact and fail on any other nibble order, k permutation,
// row / column swap or scale-block assignment:
//   row operand (fp4)     lane l holds row c, k = 32 q .. 32 q + 31 as 16 bytes in memory order (low nibble first), in
//                         the first 4 of the operand's 8 registers
//   column operand (fp4)  the mirror: lane l holds column c, k = 32 q .. 32 q + 31, 16 bytes, registers 0-3
//   scales                byte 0 of the scale register (op_sel 0) of lane l is the byte of (row c, k block q) resp.
//                         (column c, k block q): for both operands the block the lane holds
//   result                register i of lane l is (row 4 q + i, column c)
#include "gemm_mx.h"

namespace fi {

struct MmFp4Params {
  const uint8_t* a;  // tokens (m, k/2)
  const uint8_t* b;  // weights (n, k/2)
  const uint8_t* a_scale;
  const uint8_t* b_scale;
  const float* alpha;  // device, may be null
  void* d;
  int32_t m, n, k;
  int32_t out_dtype;
  int32_t m_tiles, n_tiles;
};

// one block-scaled MFMA: 16 weight rows (w, scale dword sw) x 16 tokens (x, scale dword sx) over 128 k; q picks the
// lane's k block out of the row's dword of four scales
__device__ __forceinline__ f32x4 mfma_fp4(const u32x4& w, uint32_t sw, const u32x4& x, uint32_t sx, int q, const f32x4& acc) {
  return mx_mfma</*blgp fp4*/ 4>(mx_fp4_frag(w), mx_scale_byte(sw, q), mx_fp4_frag(x), mx_scale_byte(sx, q), acc);
}

// alpha as a wave-uniform value, fetched (and waited for) where the kernel starts: left to the epilogue the load makes
// every store wait for the one before it
__device__ __forceinline__ float load_alpha(const MmFp4Params& p) {
  return p.alpha ? __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, *p.alpha))) : 1.0f;
}

// ---- streaming kernel ------------------------------------------------------------------------------------------------
constexpr int kFp4Threads = 256;
constexpr int kStreamWaves = kFp4Threads / 64;
constexpr int kStreamRows = 32;  // weight rows per wave: 2 blocks of 16
constexpr int kStreamDepth = 4;  // k steps a wave keeps in flight

// SPLITK: the workgroup owns 32 weight rows and its waves split k; otherwise it owns 128 and every wave runs all of k
// for its own 32 and nothing is reduced (launch_mm_fp4 splits while 128-row workgroups would not fill the chip)
template <int MB, bool SPLITK>
__global__ void __launch_bounds__(kFp4Threads) mm_fp4_stream_kernel(const MmFp4Params p) {
  constexpr int TM = 16 * MB;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  // token tiles fastest: the tiles that share a weight tile run next to each other.  The grid is exact.
  const int nt = blockIdx.x / p.m_tiles;
  const int m0 = (blockIdx.x - nt * p.m_tiles) * TM;
  const int n0 = SPLITK ? nt * kStreamRows : (nt * kStreamWaves + wave) * kStreamRows;
  const int M = p.m, N = p.n, K = p.k;
  const int ksteps = K >> 7, nkb = K >> 5;
  const float alpha = load_alpha(p);
  if (!SPLITK && n0 >= N) return;  // whole waves leave; without the split there is no barrier below
  // this wave's k steps: wave, wave + 4, ... of the split, else all of them
  constexpr int kStride = SPLITK ? kStreamWaves : 1;
  const int first = SPLITK ? wave : 0;
  const int steps = first < ksteps ? (ksteps - first + kStride - 1) / kStride : 0;

  // Per-lane sources.  A LOAD has lane l fetch chunk l & 3 of row l >> 2, so that four neighbouring lanes read one
  // row's 64 contiguous bytes (with the MFMA's own map, row l & 15, every lane of a quad is in another row 4 KB-multiples
  // away and the load unit looks up 64 cache lines per instruction instead of 16); to_fragment() then moves the 16
  // bytes of lane 4 c + q to lane (c, q).  The scale dwords are fetched by the lanes that use them.  Rows past the edge
  // of n or m re-read the last valid row and are masked at the store.
  const int lr = lane >> 2, lch = lane & 3;
  const int frag_src = (4 * c + q) * 4;
  auto to_fragment = [&](const u32x4& v) {
    return u32x4{(uint32_t)__builtin_amdgcn_ds_bpermute(frag_src, (int)v[0]), (uint32_t)__builtin_amdgcn_ds_bpermute(frag_src, (int)v[1]),
                 (uint32_t)__builtin_amdgcn_ds_bpermute(frag_src, (int)v[2]), (uint32_t)__builtin_amdgcn_ds_bpermute(frag_src, (int)v[3])};
  };
  const uint8_t* const b_tile = p.b + (int64_t)n0 * (K >> 1);
  const uint8_t* const a_tile = p.a + (int64_t)m0 * (K >> 1);
  uint32_t w_off[2], sw_off[2], a_off[MB], sa_off[MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    w_off[nb] = (uint32_t)(min(n0 + 16 * nb + lr, N - 1) - n0) * (uint32_t)(K >> 1) + lch * 16;
    sw_off[nb] = (uint32_t)mx_sf_offset(min(n0 + 16 * nb + c, N - 1), 0, nkb);
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    a_off[mb] = (uint32_t)(min(m0 + 16 * mb + lr, M - 1) - m0) * (uint32_t)(K >> 1) + lch * 16;
    sa_off[mb] = (uint32_t)mx_sf_offset(min(m0 + 16 * mb + c, M - 1), 0, nkb);
  }

  struct StepRegs {
    u32x4 w[2], a[MB];
    uint32_t sw[2], sa[MB];
  };
  // this wave's i-th k step: 64 bytes per row of either operand and the aligned dword of its four scales
  auto load = [&](int i, StepRegs& r) {
    const uint32_t ks = (uint32_t)(first + kStride * i);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      r.w[nb] = *(const u32x4*)(b_tile + (w_off[nb] + ks * 64));
      r.sw[nb] = *(const uint32_t*)(p.b_scale + (sw_off[nb] + ks * 512));
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      r.a[mb] = *(const u32x4*)(a_tile + (a_off[mb] + ks * 64));
      r.sa[mb] = *(const uint32_t*)(p.a_scale + (sa_off[mb] + ks * 512));
    }
  };

  f32x4 acc[2][MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (steps > 0) {
    // a ring of kStreamDepth steps; a slot past the end re-loads the last step (no branch around a load)
    StepRegs r[kStreamDepth];
#pragma unroll
    for (int j = 0; j < kStreamDepth; ++j) load(min(j, steps - 1), r[j]);
    for (int i = 0; i < steps; i += kStreamDepth) {
#pragma unroll
      for (int j = 0; j < kStreamDepth; ++j) {
        if (i + j < steps) {
          const u32x4 fw[2] = {to_fragment(r[j].w[0]), to_fragment(r[j].w[1])};
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            const u32x4 fx = to_fragment(r[j].a[mb]);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[nb][mb] = mfma_fp4(fw[nb], r[j].sw[nb], fx, r[j].sa[mb], q, acc[nb][mb]);
          }
        }
        load(min(i + j + kStreamDepth, steps - 1), r[j]);
      }
    }
  }

  if constexpr (SPLITK) {
    // the k split meets in LDS; wave 0 adds the partial sums in wave order
    __shared__ __attribute__((aligned(16))) f32x4 partial[kStreamWaves - 1][2 * MB][64];
    if (wave != 0) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) partial[wave - 1][nb * MB + mb][lane] = acc[nb][mb];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int w = 0; w < kStreamWaves - 1; ++w) acc[nb][mb] += partial[w][nb * MB + mb][lane];
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      mx_store_piece(p.d, p.out_dtype, m0 + 16 * mb + c, M, n0 + 16 * nb + 4 * q, N, acc[nb][mb], alpha);
}

// ---- tiled kernel ----------------------------------------------------------------------------------------------------
constexpr int kTile = 128;                   // rows of either operand per workgroup
constexpr int kStageSteps = 2;               // k steps per LDS stage
constexpr int kRowBytes = 64 * kStageSteps;  // bytes of a row per stage (a k step is 128 e2m1 codes = 64 bytes)
constexpr int kOpBytes = kTile * kRowBytes;  // 16 KB per operand per stage
constexpr int kScOff = 2 * kOpBytes;         // [tokens step 0 | tokens step 1 | weights step 0 | weights step 1] x 512 B
constexpr int kStageBytes = kScOff + 2 * kStageSteps * 512;
constexpr int kBandM = 8;                    // token tiles per band of the tile order
static_assert(kRowBytes == 128, "the operand images are image_off()'s: 8 chunks of 16 bytes per row");

__global__ void __launch_bounds__(kFp4Threads) mm_fp4_tile_kernel(const MmFp4Params p) {
  // one array: [stage][tokens 16 KB | weights 16 KB | scales 2 KB]
  __shared__ __attribute__((aligned(1024))) uint8_t smem[2][kStageBytes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, q = lane >> 4;
  const int wn = wave & 1, wm = wave >> 1;  // the wave's 64 weight rows and 64 tokens of the tile
  const int M = p.m, N = p.n, K = p.k;
  const int ksteps = K >> 7;
  const int nstages = (ksteps + kStageSteps - 1) / kStageSteps;
  const float alpha = load_alpha(p);  // before the first DMA: an ordinary load beside one in flight drains it

  // tile order: bands of kBandM token tiles x all weight tiles, token tiles fastest inside a band, so the workgroups
  // in flight together share few rows of both operands
  int mt, nt;
  band_tile_of<kBandM>(blockIdx.x, p.m_tiles, p.n_tiles, mt, nt);
  const int m0 = mt * kTile, n0 = nt * kTile;

  // DMA geometry: a piece = one wave instruction = 8 rows x 128 bytes = 1 KiB of the stage image, written linearly
  // (lane i -> byte 16 i of the piece); the swizzle is on the GLOBAL side.  Wave w owns pieces 8 w .. 8 w + 7 of the 32:
  // waves 0, 1 the tokens, waves 2, 3 the weights.  With an odd number of k steps the last stage's second half does not
  // exist: its lanes re-read the row's last 16 bytes (min below) and its MFMAs are skipped.
  const bool tokens = wave < 2;
  const uint8_t* const op_tile = tokens ? p.a + (int64_t)m0 * (K >> 1) : p.b + (int64_t)n0 * (K >> 1);
  const uint32_t last_chunk = (uint32_t)(K >> 1) - 16;
  uint32_t row_off[8], ch_off[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = 8 * (8 * (wave & 1) + j) + (lane >> 3);
    const int r = tokens ? min(m0 + row, M - 1) - m0 : min(n0 + row, N - 1) - n0;
    row_off[j] = (uint32_t)r * (uint32_t)(K >> 1);
    ch_off[j] = (uint32_t)(image_chunk(row, lane & 7) << 4);
  }
  // the scale blocks travel the same way, 4 bytes per lane: wave w & 1 brings the 512 bytes of the stage's step w & 1
  const uint8_t* const sc_tile = tokens ? p.a_scale + (int64_t)mt * ksteps * 512 : p.b_scale + (int64_t)nt * ksteps * 512;
  auto dma = [&](int s, int stage) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t off = row_off[j] + min((uint32_t)s * kRowBytes + ch_off[j], last_chunk);
      lds_dma16(op_tile + off, &smem[stage][(8 * wave + j) * 1024]);
    }
    const uint8_t* const sc = sc_tile + (int64_t)min(kStageSteps * s + (wave & 1), ksteps - 1) * 512 + lane * 4;
#pragma unroll
    for (int j = 0; j < 2; ++j) lds_dma4(sc + j * 256, &smem[stage][kScOff + wave * 512 + j * 256]);
  };

  // fragment and scale addresses of the stage's first k step; the second is chunk + 4 (address ^ 64), scales + 512
  uint32_t x_rd[4], w_rd[4], sx_rd[4], sw_rd[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int xr = 64 * wm + 16 * i + c, wr = 64 * wn + 16 * i + c;
    x_rd[i] = (uint32_t)image_off(xr, q);
    w_rd[i] = (uint32_t)(kOpBytes + image_off(wr, q));
    sx_rd[i] = (uint32_t)(kScOff + (xr & 31) * 16 + (xr >> 5) * 4);
    sw_rd[i] = (uint32_t)(kScOff + kStageSteps * 512 + (wr & 31) * 16 + (wr >> 5) * 4);
  }

  f32x4 acc[4][4];  // [weight block][token block]
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const uint8_t* stage, int h) {
    u32x4 fx[4];
    uint32_t sx[4];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      fx[mb] = *(const u32x4*)(stage + (x_rd[mb] ^ (h * 64)));
      sx[mb] = *(const uint32_t*)(stage + (sx_rd[mb] + h * 512));
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const u32x4 fw = *(const u32x4*)(stage + (w_rd[nb] ^ (h * 64)));
      const uint32_t sw = *(const uint32_t*)(stage + (sw_rd[nb] + h * 512));
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) acc[nb][mb] = mfma_fp4(fw, sw, fx[mb], sx[mb], q, acc[nb][mb]);
    }
  };

  dma(0, 0);
  for (int s = 0; s < nstages; ++s) {
    // stage s landed, for every wave's pieces (barrier); every wave is also done reading the other buffer (stage s - 1)
    wait_vmcnt_barrier<0>();
    if (s + 1 < nstages) dma(s + 1, (s + 1) & 1);
    const uint8_t* const stage = &smem[s & 1][0];
    compute(stage, 0);
    if (kStageSteps * s + 1 < ksteps) compute(stage, 1);
  }

#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
      mx_store_piece(p.d, p.out_dtype, m0 + 64 * wm + 16 * mb + c, M, n0 + 64 * wn + 16 * nb + 4 * q, N, acc[nb][mb], alpha);
}

// The choice between the kernels (DESIGN.md 3.15 has the sweep).  The streaming kernel's time is the weights' streaming
// time plus a term in m n k; the tiled kernel's is flat while its tiles fit the chip once and about the weights'
// streaming time once there is a tile per compute unit.  Both scale with k, so the switch is in m n: at n = 8192 /
// 16384 / 28672 the measured crossing is near m = 180 / 85 / 30, m n = 1.5 / 1.4 / 0.9 M; with a tile per compute
// unit (n = 57344) the tiled kernel wins from 8 rows.
constexpr int64_t kStreamMaxMN = 3 << 19;  // 1.5 M
constexpr int kTiledMinM = 8;
static bool choose_streaming(int m, int n, int cus) {
  const int64_t tiles = (int64_t)ceil_div(m, kTile) * ceil_div(n, kTile);
  if (tiles >= cus) return m < kTiledMinM;
  return (int64_t)m * n < kStreamMaxMN;
}

static void launch_mm_fp4(MmFp4Params p, bool stream_kernel, int cus, hipStream_t stream) {
  if (!stream_kernel) {
    p.m_tiles = ceil_div(p.m, kTile);
    p.n_tiles = ceil_div(p.n, kTile);
    mm_fp4_tile_kernel<<<dim3((uint32_t)p.m_tiles * (uint32_t)p.n_tiles), dim3(kFp4Threads), 0, stream>>>(p);
    return;
  }
  with_mx_token_blocks(p.m, [&](auto mb_c) {
    constexpr int MB = decltype(mb_c)::value;
    p.m_tiles = ceil_div(p.m, 16 * MB);
    // k is split over the waves while 128-row workgroups would leave compute units without one
    if ((int64_t)p.m_tiles * ceil_div(p.n, kStreamWaves * kStreamRows) < cus) {
      p.n_tiles = ceil_div(p.n, kStreamRows);
      mm_fp4_stream_kernel<MB, true><<<dim3((uint32_t)p.m_tiles * (uint32_t)p.n_tiles), dim3(kFp4Threads), 0, stream>>>(p);
    } else {
      p.n_tiles = ceil_div(p.n, kStreamWaves * kStreamRows);
      mm_fp4_stream_kernel<MB, false><<<dim3((uint32_t)p.m_tiles * (uint32_t)p.n_tiles), dim3(kFp4Threads), 0, stream>>>(p);
    }
  });
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_mm_mxfp4(const fi_mm_mxfp4_params_t* p, fi_stream_t stream) {
  const char* who = "mm_mxfp4";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->m >= 0 && p->n >= 0 && p->k >= 0, "%s: negative size (m %d, n %d, k %d)", who, p->m, p->n, p->k);
  if (p->m == 0 || p->n == 0) return 0;
  FI_REQUIRE(p->a && p->b && p->a_scale && p->b_scale && p->d, "%s: null tensor", who);
  const bool aligned = ((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->d % 8) == 0 &&
                       ((uintptr_t)p->a_scale % 4) == 0 && ((uintptr_t)p->b_scale % 4) == 0 && ((uintptr_t)p->alpha % 4) == 0;
  const int64_t nkb = p->k / kMxBlock;
  if (const int e = mx_check_common(who, p->d_dtype, p->n, p->k, aligned, "d 8-byte, the scales and alpha 4-byte",
                                    p->a_scale_bytes, mx_sf_rows<int64_t>(p->m, true) * nkb, "m padded to 128",
                                    p->b_scale_bytes, mx_sf_rows<int64_t>(p->n, true) * nkb, 1, "n padded to 128",
                                    (int64_t)ceil_div(p->m, 16) * ceil_div(p->n, kStreamRows)))
    return e;
  MmFp4Params g{};
  g.a = (const uint8_t*)p->a;
  g.b = (const uint8_t*)p->b;
  g.a_scale = (const uint8_t*)p->a_scale;
  g.b_scale = (const uint8_t*)p->b_scale;
  g.alpha = p->alpha;
  g.d = p->d;
  g.m = p->m;
  g.n = p->n;
  g.k = p->k;
  g.out_dtype = p->d_dtype;
  const int choice = option(OPT_MM_FP4_KERNEL).value_or(0);
  FI_REQUIRE(choice >= 0 && choice <= 2, "%s: FI_MM_FP4_KERNEL=%d is not 0 (choose), 1 (streaming) or 2 (tiled)", who, choice);
  const int cus = fi_num_compute_units();
  launch_mm_fp4(g, choice == 1 || (choice == 0 && choose_streaming(p->m, p->n, cus)), cus, (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
