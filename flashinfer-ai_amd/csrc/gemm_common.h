// Shared by the matrix-multiply translation units (gemm.hip, gemm_big.hip, gemm_mxfp4.hip, mm_fp4.hip): the fp8
// launch parameters, and the decisions every tiled kernel makes the same way -- LDS image swizzle, tile order,
// (group, m tile) lookup, scale geometry, fp8 fragments and MFMA, output packing.
#pragma once
#include <type_traits>

#include "common.h"

namespace fi {

using f32x16g = __attribute__((ext_vector_type(16))) float;
using i32x8g = __attribute__((ext_vector_type(8))) int;

constexpr int kGemmThreads = 256;
constexpr int kBM = 128, kBN = 128, kBK = 128;

struct GemmParams {
  const uint8_t* a;
  const uint8_t* b;
  const float* a_scale;
  const float* b_scale;
  void* d;
  const int32_t* m_indptr;  // [G+1] device; NULL: one group of m_total rows
  int32_t num_groups, m_total, n, k;
  int32_t a_gran_m;         // 1 or 128
  int32_t scale_k_major;    // 0: "MN" major, 1: "K" major
  int32_t out_dtype;
  int32_t num_m_tiles_bound;  // grid bound on (group, m tile) pairs
  int32_t num_m_tiles_bound_ws;  // the same for the 256-row tiles of the producer/consumer kernel
  int32_t n_tiles;
  int32_t a_is_e5m2, b_is_e5m2;
  // 256 x 256 kernel only: device word written by scales_pow2_check_kernel before the launch -- 0: every a / b scale
  // is an exact power of two (what the reference's quantiser produces, flashinfer/testing/utils.py:96-98), so the
  // scales can ride the MFMA's hardware block scales; non-zero (or a null pointer): the general fold path
  const uint32_t* pow2_flag;
};

// ---- LDS operand image: [rows][128 bytes], the 16-byte chunks of a row XOR-swizzled by the row so that the 16-lane
// groups of a ds_read_b128 fragment read hit 16 distinct slots.  A kernel that writes the image linearly by DMA
// applies the same key on the global side: the lane that writes slot `ch` of `row` fetches chunk image_chunk(row, ch).
__device__ __forceinline__ int image_chunk(int row, int ch) { return ch ^ ((row >> 1) & 7); }
__device__ __forceinline__ int image_off(int row, int ch) { return row * 128 + (image_chunk(row, ch) << 4); }

// ---- tile order ----
// XCD `xcd`'s contiguous share of `total` tiles (workgroup b runs on XCD b & 7): the shares differ by at most one
struct TileShare {
  int start, count;
};
__device__ __forceinline__ TileShare xcd_share(int total, int xcd) {
  const int qn = total >> 3, rn = total & 7;
  return {xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn, qn + (xcd < rn ? 1 : 0)};
}
// Banded order: bands of BAND_M m tiles x all n tiles, m fastest inside a band (the last band may be short), so that
// the workgroups in flight together share few rows of both operands.  (mt, nt) of tile in_band of band `band`.
template <int BAND_M>
__device__ __forceinline__ void band_tile(int band, int in_band, int m_tiles, int& mt, int& nt) {
  const int band_m = min(BAND_M, m_tiles - band * BAND_M);
  nt = in_band / band_m;
  mt = band * BAND_M + (in_band - nt * band_m);
}
template <int BAND_M>
__device__ __forceinline__ void band_tile_of(int logical, int m_tiles, int n_tiles, int& mt, int& nt) {
  const int band = logical / (BAND_M * n_tiles);
  band_tile<BAND_M>(band, logical - band * (BAND_M * n_tiles), m_tiles, mt, nt);
}

// ---- (group, m tile) lookup ----
// Lane i's view of group gi = base + i: its rows [lo, hi) and, in `start`, the tiles of the groups of lower lanes
struct GroupRows {
  int lo, hi, start;
  template <int TILE_M>
  __device__ __forceinline__ int tiles() const { return (hi - lo + TILE_M - 1) / TILE_M; }
};
template <int TILE_M>
__device__ __forceinline__ GroupRows lane_group_rows(const int32_t* m_indptr, int num_groups, int gi) {
  GroupRows r;
  r.lo = gi < num_groups ? m_indptr[gi] : 0;
  r.hi = gi < num_groups ? m_indptr[gi + 1] : 0;
  r.start = wave_incl_scan(r.tiles<TILE_M>()) - r.tiles<TILE_M>();
  return r;
}
// The lane whose group holds tile mt_global: a ballot and three readlanes, no load (a lane past the groups has no tiles)
template <int TILE_M>
__device__ __forceinline__ bool lookup_group_tile(const GroupRows& r, int mt_global, int& g, int& m_begin, int& m_end,
                                                  int& mt) {
  const uint64_t hit = __ballot(mt_global >= r.start && mt_global < r.start + r.tiles<TILE_M>());
  if (!hit) return false;
  g = __builtin_ctzll(hit);
  m_begin = __builtin_amdgcn_readlane(r.lo, g);
  m_end = __builtin_amdgcn_readlane(r.hi, g);
  mt = mt_global - __builtin_amdgcn_readlane(r.start, g);
  return true;
}

// (group, m tile) of the mt_global-th m tile from the running count of tiles per group, on the device (the
// reference's arg-prep kernel group_gemm_fp8_groupwise_sm100.cuh:35-72 also sizes the groups on the device, no
// host sync).  Wave-parallel: 64 groups per pass -- lane i loads m_indptr[i], [i + 1], an inclusive scan over
// the lanes gives each group's first tile -- so that 256 experts cost 4 passes, not 256 dependent loads.
// Every lane of every wave runs it with the same arguments and gets the same (uniform) answer.
template <int TILE_M>
__device__ __forceinline__ bool find_group_tile(const int32_t* m_indptr, int num_groups, int mt_global, int lane,
                                                int& g, int& m_begin, int& m_end, int& mt) {
  int first = 0;  // tiles in the groups of earlier passes
  for (int base = 0; base < num_groups; base += 64) {
    GroupRows r = lane_group_rows<TILE_M>(m_indptr, num_groups, base + lane);
    const int incl = r.start + r.tiles<TILE_M>();
    r.start += first;
    if (lookup_group_tile<TILE_M>(r, mt_global, g, m_begin, m_end, mt)) {
      g += base;
      return true;
    }
    first += __builtin_amdgcn_readlane(incl, 63);
  }
  return false;
}

// (group, m tile) of a kernel's mt_global-th TILE_M-row tile, false when there is none (the grid bound counts one
// partial tile per group).  Without groups: one group of m_total rows.  `cached`: gc holds lane_group_rows of all
// (<= 64) groups; else the looping search.  Uniform per workgroup.
template <int TILE_M>
__device__ __forceinline__ bool group_of_tile(const GemmParams& p, int mt_global, int lane, bool cached,
                                              const GroupRows& gc, int& g, int& m_begin, int& m_end, int& mt) {
  g = 0, m_begin = 0, m_end = p.m_total, mt = mt_global;
  if (!p.m_indptr) return mt_global * TILE_M < p.m_total;
  if (cached) return lookup_group_tile<TILE_M>(gc, mt_global, g, m_begin, m_end, mt);
  return find_group_tile<TILE_M>(p.m_indptr, p.num_groups, mt_global, lane, g, m_begin, m_end, mt);
}

// Row of a_scale for row m of a, m_begin being the first row of m's group (0 without groups).  gran_m == 128: a
// group's scale rows start at m_begin / 128 and block the group's rows from its first one, as the reference offsets
// the scale pointer per group (group_gemm_fp8_groupwise_sm100.cuh:52-69, sf_m_offset) -- never past the global row's
// block, so a_scale's ceil(m_total / 128) rows cover it.
__device__ __forceinline__ int a_scale_row(int gran_m, int m_begin, int m) {
  return gran_m == 1 ? m : m_begin / gran_m + (m - m_begin) / gran_m;
}

// Where a call's scales lie, in floats: a_scale is [m_cnt rows][kblocks] ("K" major) or [kblocks][m_cnt], b_scale
// [groups][n_sblocks][kblocks] or [groups][kblocks][n_sblocks].  The scale of k block kb is a_stride resp. b_stride
// times kb past the offset of its row (a_row) resp. of its group's 128-row block of B (b_block).
struct ScaleGeom {
  int kblocks, m_cnt, n_sblocks, a_stride, b_stride;
  bool k_major;
  __host__ __device__ int64_t a_row(int mi) const { return k_major ? (int64_t)mi * kblocks : mi; }
  __host__ __device__ int64_t b_block(int g, int nb) const {
    return k_major ? ((int64_t)g * n_sblocks + nb) * kblocks : (int64_t)g * kblocks * n_sblocks + nb;
  }
};
__host__ __device__ inline ScaleGeom scale_geom(const GemmParams& p) {
  ScaleGeom s;
  s.kblocks = p.k / kBK;
  s.m_cnt = p.a_gran_m == 1 ? p.m_total : (p.m_total + p.a_gran_m - 1) / p.a_gran_m;
  s.n_sblocks = (p.n + 127) / 128;
  s.k_major = p.scale_k_major != 0;
  s.a_stride = s.k_major ? 1 : s.m_cnt;
  s.b_stride = s.k_major ? 1 : s.n_sblocks;
  return s;
}

// ---- fp8 fragments and the 32x32x64 MFMA.  MA_E5M2 / MB_E5M2 are the formats of the MFMA's A operand (= matrix B
// of the GEMM) and B operand (= matrix A).
// a lane's 32 bytes of a row as the MFMA's eight operand registers, from two 16-byte LDS reads
__device__ __forceinline__ i32x8g fp8_frag(const uint8_t* p_lo, const uint8_t* p_hi) {
  const u32x4 lo = *(const u32x4*)p_lo, hi = *(const u32x4*)p_hi;
  return i32x8g{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// the same in a stage whose per-lane address is `base`: k half kk flips chunk bit 2, the second 16 bytes chunk bit 0,
// 32-row block blk adds a literal
__device__ __forceinline__ i32x8g fp8_frag(const uint8_t* stage, uint32_t base, int kk, int blk) {
  return fp8_frag(stage + ((base ^ (kk << 6)) + blk * 32 * kBK), stage + ((base ^ (kk << 6) ^ 16) + blk * 32 * kBK));
}
// c + b a with E8M0 block scales eb, ea (byte 0); the default 127 is the unit scale: the plain fp8 product at twice
// the rate of the non-scaled fp8 MFMA (MI355X_MICROARCH.md, matrix cores)
template <bool MA_E5M2, bool MB_E5M2>
__device__ __forceinline__ f32x16g mfma_fp8(const i32x8g& b, const i32x8g& a, const f32x16g& c, int eb = 0x7F7F7F7F,
                                            int ea = 0x7F7F7F7F) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b, a, c, MA_E5M2 ? 1 : 0, MB_E5M2 ? 1 : 0, 0, eb, 0, ea);
}
// b a into a zero accumulator
template <bool MA_E5M2, bool MB_E5M2>
__device__ __forceinline__ f32x16g mfma_fp8_zero(const i32x8g& b, const i32x8g& a) {
  f32x16g z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return mfma_fp8<MA_E5M2, MB_E5M2>(b, a, z);
}

// ---- output ----
// two floats rounded to dt (f16 / bf16) in one dword, `lo` in the low half
__device__ __forceinline__ uint32_t pack_16bit(float lo, float hi, int dt) {
  return (uint32_t)f32_to_16bit(lo, dt) | ((uint32_t)f32_to_16bit(hi, dt) << 16);
}
// four consecutive accumulators v[i] .. v[i + 3] as two such dwords
template <class V>
__device__ __forceinline__ u32x2 pack4_16bit(const V& v, int i, int dt) {
  return u32x2{pack_16bit(v[i], v[i + 1], dt), pack_16bit(v[i + 2], v[i + 3], dt)};
}
// 16 bytes of a row of d: one store, or two 8-byte stores when d is only 8-byte aligned.  NT: non-temporal.
template <bool NT = false>
__device__ __forceinline__ void store_row_piece(uint16_t* dst, const u32x4& v, bool d_aligned16) {
  if (!d_aligned16) {
    *(u32x2*)dst = u32x2{v[0], v[1]};
    *(u32x2*)(dst + 4) = u32x2{v[2], v[3]};
  } else if constexpr (NT) {
    __builtin_nontemporal_store(v, (u32x4*)dst);
  } else {
    *(u32x4*)dst = v;
  }
}

// The power-of-two verdict of a call: kPow2Words words, one per workgroup of the check kernel (non-zero = that
// workgroup saw a scale that is not a positive normal power of two).  No word is ever reset: every call's check
// kernel rewrites all of its slot's words, so there is no memset node in front of it.
constexpr int kPow2Words = 64;
__device__ __forceinline__ bool fi_scales_are_pow2(const uint32_t* flag) {
  return flag != nullptr && !__any(flag[threadIdx.x & (kPow2Words - 1)] != 0);
}

// f(std::bool_constant<MA_E5M2>{}, std::bool_constant<MB_E5M2>{}) for the call's fp8 formats: the MFMA A operand is
// GEMM matrix B, the MFMA B operand GEMM matrix A
template <class F>
void with_fp8_formats(const GemmParams& p, F&& f) {
  auto with_ma = [&](auto ma) {
    if (p.a_is_e5m2) f(ma, std::true_type{});
    else f(ma, std::false_type{});
  };
  if (p.b_is_e5m2) with_ma(std::true_type{});
  else with_ma(std::false_type{});
}

// 256 x 256 tile persistent kernel (gemm_big.hip); p.num_m_tiles_bound counts 256-row tiles.
// A call's flag words (kPow2Words), or nullptr under a stream capture before the first eager call.
uint32_t* pow2_flag_slot(hipStream_t stream);
// The check kernel: writes p.pow2_flag (non-null) from p's scales.
void launch_pow2_check(const GemmParams& p, hipStream_t stream);
// hws: the hardware-scale variant (does the call when fi_scales_are_pow2(p.pow2_flag), else returns at once);
// otherwise the fold variant (the reverse).
void launch_gemm_big(const GemmParams& p, bool hws, int grid, hipStream_t stream);

}  // namespace fi
