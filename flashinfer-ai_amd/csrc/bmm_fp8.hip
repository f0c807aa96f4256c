// Batched fp8 matmul with one scale per tensor: fi_bmm_fp8.
//
// What it replaces: the reference's bmm_fp8 (flashinfer/gemm.py:2227-2318, cuBLASLt / cuDNN / CUTLASS behind it):
//   d[b, i, j] = dtype(a_scale * b_scale * sum_k a[b, i, k] * w[b, j, k])
// a (batch, m, k) fp8, w (batch, n, k) fp8 -- the storage of the reference's column-major (batch, k, n) B --, the two
// scales one f32 each on the DEVICE, d (batch, m, n) f16 / bf16.  f32 accumulation over the whole of k, one multiply by
// a_scale * b_scale, one rounding.  Either operand may be e4m3 or e5m2, not both e5m2.  k % 16 == 0 and n % 8 == 0 are
// all the shapes owe: nothing is a multiple of 128.
//
// The regimes are a per-tensor-scaled linear layer at decode (batch 1, a handful of tokens, n and k in the thousands)
// and the absorbed MLA projections (batch = heads, (k, n) = (128, 512) / (512, 128)): few rows per weight byte, so the
// kernel is the weight STREAM of gemm_masked.hip -- same instruction, same operand maps, same ring -- without the block
// scales.  A dense prefill-size GEMM is computed correctly but not tuned for: that wants a 256-wide MFMA-bound tile.
//
// The product is computed TRANSPOSED (d^T = w a^T) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 scales; the two
// operand formats are arguments of the instruction.  Lane l = (c = l & 15, g = l >> 4) holds 32 consecutive bytes of
// its row: bytes 32 g .. 32 g + 31 of the k block, of weight row c (row operand) resp. token c (column operand);
// register i of the result is (weight row 4 g + i, token c): 4 consecutive n of one token, 8 bytes of d.
// ONE accumulator chain: the instruction's C operand carries the sum from k block to k block; the scale product,
// loaded once per workgroup, is applied in the epilogue.
//
// Weights go from global memory into registers (load_weights below: every instruction reads whole 128-byte lines,
// non-temporal; weight_frag of gemm_common.h hands each lane its own row's chunks), P k blocks ahead in a ring.
//
// Tails.  k: the last k block may hold 1 .. 7 16-byte chunks only.  A chunk at or past k is not loaded -- its lane
// re-reads the first chunk of the block, which exists -- and is replaced by zero codes (0x00 is zero in both formats)
// where the registers are used, for both operands.  n and m: weight rows at or past n and token rows at or past m
// re-read the last valid row of the batch entry and are masked at the store.
//
// Tiles: BM tokens (16 / 32 / 64 / 128: the smallest that holds m, 128 beyond) x a weight tile.  A unit is one
// (batch, weight tile), units ordered weight tile fastest; the host knows them all, the grid is the list.  Workgroup w
// runs on XCD w & 7: it takes unit (w & 7) + 8 * ((w >> 3) / m_tiles) and row tile (w >> 3) % m_tiles.  Workgroups in
// flight together so read different weight tiles, and the row tiles of a unit are neighbours on ONE XCD: at m > 128 the
// weight tile comes from HBM once and from that XCD's L2 after.  (The grid is rounded up to whole units per XCD; a
// workgroup past the last unit returns at once.)
//
// Two wave arrangements, one loop (SPLIT_K):
//   waves along n: the weight tile is 128 rows, wave v owns rows 32 v .. 32 v + 31 and walks every k block.  The BM x 128
//     byte token slab of a k block is shared: global -> registers (in the ring, one block ahead of its weights) -> LDS
//     image with the chunk swizzle of gemm_common.h, two buffers, one barrier per k block that waits for LDS only.
//   waves along k: for few tokens and too few 128-row tiles to occupy the chip.  The weight tile is 32 rows, wave v
//     takes k blocks v, v + 4, ... and loads its token fragments from global memory in the MFMA's layout (the 4 lanes
//     g of a token read one 128-byte line); nothing is shared, no barrier in the loop.  The 4 partial sums meet in LDS
//     and are added in wave order ((p0 + p1) + p2) + p3.  BM <= 32 only; four times the workgroups.
// Within an arrangement a result's sum is taken in an order that depends on k alone: not on BM, not on scheduling.
#include "gemm_common.h"

namespace fi {

struct BmmFp8Params {
  const uint8_t* a;
  const uint8_t* b;
  const float* a_scale;
  const float* b_scale;
  void* d;
  int64_t a_stride, b_stride, d_stride;  // batch strides, elements
  int32_t batch, m, n, k;
  int32_t out_dtype;
  int32_t m_tiles, n_tiles;  // row tiles of BM; weight tiles of 128 rows (waves along n) or 32 (waves along k)
  int32_t a_is_e5m2, b_is_e5m2;
};

constexpr int kBmmThreads = 256;
constexpr int kBmmWaves = kBmmThreads / 64;
constexpr int kBmmWaveRows = 32;  // weight rows of a wave: 2 blocks of 16

// c + w x over one 128-wide k block; W_E5M2 / X_E5M2: the formats of the weights (row operand) and tokens
template <bool W_E5M2, bool X_E5M2>
__device__ __forceinline__ f32x4 mfma_fp8_k128(const i32x8g& w, const i32x8g& x, const f32x4& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, c, W_E5M2 ? 1 : 0, X_E5M2 ? 1 : 0, 0, 0x7F7F7F7F, 0,
                                                          0x7F7F7F7F);
}

__device__ __forceinline__ u32x4 keep_or_zero(const u32x4& v, bool keep) { return keep ? v : u32x4{0u, 0u, 0u, 0u}; }

template <int BM, bool SPLIT_K, bool W_E5M2, bool X_E5M2>
__global__ void __launch_bounds__(kBmmThreads, 2) bmm_fp8_kernel(const BmmFp8Params p) {
  static_assert(BM == 16 || BM == 32 || BM == 64 || BM == 128, "row tile heights");
  static_assert(!SPLIT_K || BM <= 32, "waves along k: few tokens only");
  constexpr int MB = BM / 16;                   // token blocks of the tile
  constexpr int P = BM == 128 ? 2 : 4;          // k blocks in flight
  constexpr int AV = BM >= 32 ? BM / 32 : 1;    // 16-byte pieces of the token slab per thread (32 rows per pass)
  constexpr int XV = SPLIT_K ? 2 * MB : AV;     // 16-byte token pieces in a ring entry
  constexpr int KSTEP = SPLIT_K ? kBmmWaves : 1;
  constexpr int WG_ROWS = SPLIT_K ? kBmmWaveRows : kBN;
  static_assert(P % 2 == 0, "the LDS buffer of k block i + j must be j & 1");
  // waves along n: the token image, 2 buffers; waves along k: the partial sums [wave][2 MB fragments][lane]
  constexpr int LDS_BYTES = SPLIT_K ? kBmmWaves * 2 * MB * 64 * 16 : 2 * BM * kBK;
  __shared__ __attribute__((aligned(1024))) uint8_t lds[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const bool odd = (c & 1) != 0;
  const int M = p.m, N = p.n, K = p.k;
  const int KB = (K + kBK - 1) >> 7;
  const int tail = (K - (KB - 1) * kBK) >> 4;  // 16-byte chunks of the last k block: 1 .. 8
  const bool has_tail = tail < 8;

  // ---- the tile ----
  const int slot = blockIdx.x >> 3;
  const int unit = (blockIdx.x & 7) + 8 * (slot / p.m_tiles);
  if (unit >= p.batch * p.n_tiles) return;
  const int m0 = (slot % p.m_tiles) * BM;
  const int bi = unit / p.n_tiles, nt = unit - bi * p.n_tiles;
  const int n0 = nt * WG_ROWS + (SPLIT_K ? 0 : kBmmWaveRows * wave);
  const float scale = p.a_scale[0] * p.b_scale[0];

  // ---- per-lane sources: a row past the edge is the last valid row, a chunk past k the block's first chunk ----
  const int nb0 = min(n0, N - 1);  // the wave's first weight row, inside the batch entry
  const uint8_t* const w_tile = p.b + (int64_t)bi * p.b_stride + (int64_t)nb0 * K;
  const uint8_t* const a_tile = p.a + (int64_t)bi * p.a_stride;
  const int w_chunk = 2 * g + (c & 1);
  const bool w_ok = w_chunk < tail;
  uint32_t w_row[2][2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int h = 0; h < 2; ++h) w_row[nb][h] = (uint32_t)(min(n0 + 16 * nb + ((c & ~1) | h), N - 1) - nb0) * (uint32_t)K;
  // tokens.  Waves along n: thread t stages slot t & 7 of rows (t >> 3) + 32 v, which holds chunk a_chunk (the key
  // of image_chunk repeats every 16 rows).  Waves along k: the lane's own chunks 2 g and 2 g + 1 of tokens 16 mb + c.
  const int a_row = tid >> 3;
  const int a_chunk = image_chunk(a_row, tid & 7);
  const bool a_ok = a_chunk < tail, stages_a = a_row < BM;
  const bool x_ok[2] = {2 * g < tail, 2 * g + 1 < tail};
  uint32_t x_row[SPLIT_K ? MB : AV];
  if constexpr (SPLIT_K) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) x_row[mb] = (uint32_t)min(m0 + 16 * mb + c, M - 1) * (uint32_t)K;
  } else {
#pragma unroll
    for (int v = 0; v < AV; ++v) x_row[v] = (uint32_t)min(m0 + 32 * v + a_row, M - 1) * (uint32_t)K;
  }
  uint32_t x_rd[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) x_rd[mb] = (uint32_t)image_off(16 * mb + c, 2 * g);

  // byte offset in a row of chunk `chunk` of k block kb, or of the block's first chunk when that chunk is past k
  auto chunk_off = [&](int kb, int chunk, bool ok) {
    return (uint32_t)kb * kBK + ((kb == KB - 1 && !ok) ? 0u : (uint32_t)chunk * 16);
  };

  // this wave's k blocks: first, first + KSTEP, ... ; an index past the last one names a valid block (loaded, unused)
  const int kb_first = SPLIT_K ? wave : 0;
  const int cnt = SPLIT_K ? (KB - wave + KSTEP - 1) / KSTEP : KB;
  auto block_of = [&](int i) { return min(kb_first + KSTEP * i, KB - 1); };

  struct Gen {  // the weights of the wave's i-th block; its token fragments (along k) or the slab of the block after it
    u32x4 w[2][2];
    u32x4 x[XV];
  };
  // a 16-row weight block in two loads: the 8 lanes (c = 2 q, 2 q + 1; g) fetch the 8 chunks of ONE row, the first
  // load the even rows, the second the odd ones
  auto load_weights = [&](int kb, u32x4 (*w)[2]) {
    const uint32_t off = chunk_off(kb, w_chunk, w_ok);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int h = 0; h < 2; ++h) w[nb][h] = __builtin_nontemporal_load((const u32x4*)(w_tile + (w_row[nb][h] + off)));
  };
  auto load_slab = [&](int kb, u32x4* x) {
    const uint32_t off = chunk_off(kb, a_chunk, a_ok);
#pragma unroll
    for (int v = 0; v < AV; ++v) x[v] = *(const u32x4*)(a_tile + (x_row[v] + off));
  };
  auto load_frags = [&](int kb, u32x4* x) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int h = 0; h < 2; ++h) x[2 * mb + h] = *(const u32x4*)(a_tile + (x_row[mb] + chunk_off(kb, 2 * g + h, x_ok[h])));
  };
  auto store_slab = [&](int buf, int kb, const u32x4* x) {
    const bool keep = !(kb == KB - 1 && has_tail) || a_ok;
    if (stages_a) {
#pragma unroll
      for (int v = 0; v < AV; ++v)
        *(u32x4*)&lds[buf * (BM * kBK) + (32 * v + a_row) * kBK + (tid & 7) * 16] = keep_or_zero(x[v], keep);
    }
  };
  auto load_gen = [&](int i, Gen& r) {
    load_weights(block_of(i), r.w);
    if constexpr (SPLIT_K) load_frags(block_of(i), r.x);
    else load_slab(block_of(i + 1), r.x);
  };

  f32x4 acc[2][MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

  Gen r[P];
  if constexpr (SPLIT_K) {
#pragma unroll
    for (int j = 0; j < P; ++j) load_gen(j, r[j]);
  } else {
    u32x4 a0[AV];
    load_slab(0, a0);
#pragma unroll
    for (int j = 0; j < P; ++j) load_gen(j, r[j]);
    store_slab(0, 0, a0);
    lds_barrier();
  }

  for (int i = 0; i < cnt; i += P) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (i + j < cnt) {
        const int kb = kb_first + KSTEP * (i + j);
        const bool cut = kb == KB - 1 && has_tail;  // uniform: this block's chunks past k become zero codes
        const int buf = j & 1;
        // the slab of k block kb + 1; the readers of that buffer are behind the last barrier
        if constexpr (!SPLIT_K) store_slab(buf ^ 1, block_of(i + j + 1), r[j].x);
        i32x8g fw[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          fw[nb] = weight_frag(keep_or_zero(r[j].w[nb][0], !cut || w_ok), keep_or_zero(r[j].w[nb][1], !cut || w_ok), odd);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          i32x8g fx;
          if constexpr (SPLIT_K) {
            const u32x4 lo = keep_or_zero(r[j].x[2 * mb], !cut || x_ok[0]);
            const u32x4 hi = keep_or_zero(r[j].x[2 * mb + 1], !cut || x_ok[1]);
            fx = i32x8g{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
          } else {
            const uint8_t* const img = &lds[buf * (BM * kBK)];
            fx = fp8_frag(img + x_rd[mb], img + (x_rd[mb] ^ 16));
          }
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) acc[nb][mb] = mfma_fp8_k128<W_E5M2, X_E5M2>(fw[nb], fx, acc[nb][mb]);
        }
        if constexpr (!SPLIT_K) lds_barrier();
        load_gen(i + j + P, r[j]);
      }
    }
  }

  // ---- store: a lane's 4 consecutive n of token c, 8 bytes (n % 8 == 0: all four inside n or none) ----
  uint16_t* const d_tile = (uint16_t*)p.d + (int64_t)bi * p.d_stride;
  auto store_frag = [&](int nb, int mb, const f32x4& sum) {
    const int row = m0 + 16 * mb + c, col = n0 + 16 * nb + 4 * g;
    if (row < M && col < N) *(u32x2*)(d_tile + ((int64_t)row * N + col)) = pack4_16bit(sum * scale, 0, p.out_dtype);
  };
  if constexpr (SPLIT_K) {
    f32x4* const part = (f32x4*)lds;  // [wave][fragment nb * MB + mb][lane]
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) part[(wave * 2 * MB + nb * MB + mb) * 64 + lane] = acc[nb][mb];
    __syncthreads();
    if (wave < 2 * MB) {  // wave f adds fragment f, in wave order
      f32x4 sum = part[wave * 64 + lane];
#pragma unroll
      for (int v = 1; v < kBmmWaves; ++v) sum += part[(v * 2 * MB + wave) * 64 + lane];
      store_frag(wave / MB, wave % MB, sum);
    }
  } else {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) store_frag(nb, mb, acc[nb][mb]);
  }
}

// smallest row tile that holds m rows, 128 at most
static int bmm_row_tile(int m) { return m <= 16 ? 16 : m <= 32 ? 32 : m <= 64 ? 64 : 128; }

// Waves along k: a row tile of at most 32 tokens, at least one k block per wave, and fewer 128-row tiles than compute
// units -- the 32-row tiles then put four times the workgroups on the chip.
static bool bmm_waves_along_k(int batch, int m, int n, int k, int cus) {
  const int bm = bmm_row_tile(m);
  const int64_t wide_tiles = (int64_t)batch * ceil_div(m, bm) * ceil_div(n, kBN);
  return bm <= 32 && ceil_div(k, kBK) >= kBmmWaves && wide_tiles < cus;
}

template <int BM, bool SPLIT_K>
static void launch_bmm_fp8_tile(const BmmFp8Params& p, dim3 grid, hipStream_t stream) {
  GemmParams fmt{};
  fmt.a_is_e5m2 = p.a_is_e5m2;
  fmt.b_is_e5m2 = p.b_is_e5m2;
  with_fp8_formats(fmt, [&](auto w_e5m2, auto x_e5m2) {
    constexpr bool W = decltype(w_e5m2)::value, X = decltype(x_e5m2)::value;
    if constexpr (!(W && X))  // both e5m2: refused by the caller
      bmm_fp8_kernel<BM, SPLIT_K, W, X><<<grid, dim3(kBmmThreads), 0, stream>>>(p);
  });
}

static void launch_bmm_fp8(BmmFp8Params p, int cus, hipStream_t stream) {
  const int bm = bmm_row_tile(p.m);
  const bool split_k = bmm_waves_along_k(p.batch, p.m, p.n, p.k, cus);
  p.m_tiles = ceil_div(p.m, bm);
  p.n_tiles = ceil_div(p.n, split_k ? kBmmWaveRows : kBN);
  // whole units per XCD: unit u lives on XCD u & 7
  const dim3 grid((uint32_t)(ceil_div(p.batch * p.n_tiles, 8) * 8 * p.m_tiles));
  if (split_k) {
    if (bm == 16) launch_bmm_fp8_tile<16, true>(p, grid, stream);
    else launch_bmm_fp8_tile<32, true>(p, grid, stream);
    return;
  }
  switch (bm) {
    case 16: launch_bmm_fp8_tile<16, false>(p, grid, stream); break;
    case 32: launch_bmm_fp8_tile<32, false>(p, grid, stream); break;
    case 64: launch_bmm_fp8_tile<64, false>(p, grid, stream); break;
    default: launch_bmm_fp8_tile<128, false>(p, grid, stream); break;
  }
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_bmm_fp8(const fi_bmm_fp8_params_t* p, fi_stream_t stream) {
  const char* who = "bmm_fp8";
  FI_REQUIRE(p, "%s: null params", who);
  FI_REQUIRE(p->batch >= 0 && p->m >= 0 && p->n >= 0 && p->k >= 0, "%s: negative size (batch %d, m %d, n %d, k %d)", who,
             p->batch, p->m, p->n, p->k);
  const bool a_fp8 = p->a_dtype == FI_DTYPE_FP8_E4M3 || p->a_dtype == FI_DTYPE_FP8_E5M2;
  const bool b_fp8 = p->b_dtype == FI_DTYPE_FP8_E4M3 || p->b_dtype == FI_DTYPE_FP8_E5M2;
  FI_REQUIRE(a_fp8 && b_fp8, "%s: operand dtypes %d, %d are not e4m3 / e5m2", who, p->a_dtype, p->b_dtype);
  FI_REQUIRE(!(p->a_dtype == FI_DTYPE_FP8_E5M2 && p->b_dtype == FI_DTYPE_FP8_E5M2),
             "%s: both operands e5m2: at least one must be e4m3", who);
  FI_REQUIRE(p->d_dtype == FI_DTYPE_F16 || p->d_dtype == FI_DTYPE_BF16, "%s: output dtype %d is not f16 / bf16", who, p->d_dtype);
  FI_REQUIRE(p->k > 0 && p->k % 16 == 0, "%s: k %d must be a positive multiple of 16", who, p->k);
  FI_REQUIRE(p->n % 8 == 0, "%s: n %d must be a multiple of 8", who, p->n);
  FI_REQUIRE(p->a_stride_b >= (int64_t)p->m * p->k && p->b_stride_b >= (int64_t)p->n * p->k &&
                 p->d_stride_b >= (int64_t)p->m * p->n,
             "%s: batch strides %lld, %lld, %lld are smaller than a batch entry (m %d, n %d, k %d)", who,
             (long long)p->a_stride_b, (long long)p->b_stride_b, (long long)p->d_stride_b, p->m, p->n, p->k);
  FI_REQUIRE(p->a_stride_b % 16 == 0 && p->b_stride_b % 16 == 0 && p->d_stride_b % 4 == 0,
             "%s: the batch strides of a / b must be multiples of 16, that of d of 4 (got %lld, %lld, %lld)", who,
             (long long)p->a_stride_b, (long long)p->b_stride_b, (long long)p->d_stride_b);
  if (p->batch == 0 || p->m == 0 || p->n == 0) return 0;
  FI_REQUIRE(p->a && p->b && p->a_scale && p->b_scale && p->d, "%s: null tensor", who);
  FI_REQUIRE(((uintptr_t)p->a % 16) == 0 && ((uintptr_t)p->b % 16) == 0 && ((uintptr_t)p->d % 8) == 0 &&
                 ((uintptr_t)p->a_scale % 4) == 0 && ((uintptr_t)p->b_scale % 4) == 0,
             "%s: a / b must be 16-byte, d 8-byte, the scales 4-byte aligned", who);
  // 32-bit offsets inside a batch entry of a and inside a wave's 32 weight rows
  FI_REQUIRE((int64_t)p->m * p->k < (1ll << 31) && (int64_t)kBmmWaveRows * p->k < (1ll << 31),
             "%s: problem too large for 32-bit tile offsets (m %d, k %d)", who, p->m, p->k);
  FI_REQUIRE(((int64_t)p->batch * ceil_div(p->n, kBmmWaveRows) + 8) * ceil_div(p->m, 16) < (1ll << 31), "%s: too many tiles", who);
  BmmFp8Params g{};
  g.a = (const uint8_t*)p->a;
  g.b = (const uint8_t*)p->b;
  g.a_scale = p->a_scale;
  g.b_scale = p->b_scale;
  g.d = p->d;
  g.a_stride = p->a_stride_b;
  g.b_stride = p->b_stride_b;
  g.d_stride = p->d_stride_b;
  g.batch = p->batch;
  g.m = p->m;
  g.n = p->n;
  g.k = p->k;
  g.out_dtype = p->d_dtype;
  g.a_is_e5m2 = p->a_dtype == FI_DTYPE_FP8_E5M2;
  g.b_is_e5m2 = p->b_dtype == FI_DTYPE_FP8_E5M2;
  launch_bmm_fp8(g, fi_num_compute_units(), (hipStream_t)stream);
  FI_HIP_CALL(hipGetLastError());
  return 0;
}
