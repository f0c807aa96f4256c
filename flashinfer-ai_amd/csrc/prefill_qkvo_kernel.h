// Ragged / single-request prefill with separate head dims for Q.K (192) and P.V (128): the non-absorbed form of
// DeepSeek-style MLA (128 "nope" + 64 rope dims per q / k head, 128-dim v heads), f16 and bf16.
//
// What it replaces: the reference's FA2 prefill instantiated at HEAD_DIM_QK 192 / HEAD_DIM_VO 128
// (include/flashinfer/attention/prefill.cuh, aot.py:568).
//
// The arithmetic is batch_prefill_kernel's (prefill_kernel.h): GQA-packed rows, S^T = K . Q^T with Q held in
// registers, P taken straight from the S^T accumulators as the B operand of O^T += V^T . P^T, V^T read with
// ds_read_b64_tr_b16, deferred rescale, the three bf16 P.V modes.  What differs:
//   * K rows are 192 dims (12 MFMA k-steps, 384-byte LDS rows), V rows 128 dims (4 O^T blocks, 256-byte rows), each
//     with its own strides: v may be a strided view of a fused projection output.
//   * No page table: ragged (kv_indptr) or dense single-request K / V, so each thread computes its rows' addresses
//     itself (no per-tile row-offset table).
//   * LDS: K double-buffered (2 x 24 KiB) and V single-buffered (16 KiB), 64 KiB per workgroup, so two 4-wave
//     workgroups share a CU as at head_dim 128.  With one V buffer the V rows of tile t+1 are written after every
//     wave's P.V of tile t: two barriers per tile instead of one.
//   * Plain logits only (causal / non-causal, sliding window, sm_scale): no fp8, RoPE, ALiBi, soft cap or masks.
#pragma once
#include "prefill_kernel.h"

namespace fi {

constexpr int kQkvoDimQK = 192;
constexpr int kQkvoDimVO = 128;
constexpr int kQkvoSmemBytes = 2 * kTileKV * kQkvoDimQK * 2 + kTileKV * kQkvoDimVO * 2;  // 64 KiB

struct PrefillQkvoParams {
  const void* q;
  const void* k;
  const void* v;
  void* o;                       // [rows, num_qo_heads, 128] contiguous
  float* lse;
  const int32_t* qo_indptr;      // NULL: single request (single_qo_len / single_kv_len)
  const int32_t* kv_indptr;
  const int32_t* request_indices;  // work list (NULL: request 0)
  const int32_t* qo_tile_indices;
  const int32_t* kv_tile_indices;  // NULL: no split through the work list
  const int32_t* merge_indptr;
  float* tmp_o;                    // split-KV partial states [entry][num_qo_heads][128] and lse
  float* tmp_lse;
  const int32_t* kv_chunk_size_ptr;  // plan's device copy (graph replays read the current plan's value)
  int64_t q_stride_n, q_stride_h;
  int64_t k_stride_n, k_stride_h;  // host checks stride_n < 2^31
  int64_t v_stride_n, v_stride_h;
  int32_t kv_chunk_size;
  int32_t num_kv_chunks;           // single-request split: work = q tile * chunks + chunk
  int32_t num_work;
  int32_t num_qo_heads, num_kv_heads, group_size;
  FastDiv group_div;
  int32_t single_qo_len, single_kv_len;
  int32_t causal;
  int32_t window_left;  // < 0 off
  float sm_scale;
};

// PMODE as batch_prefill_kernel (bf16 only; f16 ignores it): 0 single bf16 P, 1 hi + lo bf16 P, 2 P.V on the f16 MFMA
template <int T16, int PMODE>
__global__ void __launch_bounds__(kPrefillThreads, 2) prefill_qkvo_kernel(const PrefillQkvoParams p) {
  using M = MfmaType<T16>;
  using frag_t = typename M::frag;
  constexpr bool P_HI_LO = PMODE == 1 && T16 == FI_DTYPE_BF16;
  constexpr bool PV_F16 = PMODE == 2 && T16 == FI_DTYPE_BF16;
  constexpr int TPV = PV_F16 ? FI_DTYPE_F16 : T16;
  using MPV = MfmaType<TPV>;
  constexpr int KROWB = kQkvoDimQK * 2;  // 384 bytes per K row in LDS
  constexpr int VROWB = kQkvoDimVO * 2;  // 256
  constexpr int KSTEPS = kQkvoDimQK / 16;  // 12
  constexpr int DBLK = kQkvoDimVO / 32;    // 4
  constexpr int KTILE_BYTES = kTileKV * KROWB;
  constexpr int V_LDS = 2 * KTILE_BYTES;   // the single V image follows the two K images

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 31;
  const int lh = lane >> 5;

  // ---- which (request, q tile, kv chunk, kv head): XCD-contiguous logical ids, as batch_prefill_kernel ----
  const int total = p.num_work * p.num_kv_heads;
  int logical;
  {
    const int b = blockIdx.x;
    const int xcd = b & 7, slot = b >> 3;
    const int qn = total >> 3, rn = total & 7;
    logical = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + slot;
  }
  const int kv_head = logical / p.num_work;
  const int work = logical - kv_head * p.num_work;
  int req = 0, q_tile = work, kv_chunk = 0;
  const bool split = p.kv_tile_indices != nullptr || p.num_kv_chunks > 1;
  if (p.request_indices) {
    req = p.request_indices[work];
    q_tile = p.qo_tile_indices[work];
    if (req < 0) return;  // padding item of a fixed-shape (graph) launch; uniform for the workgroup
    if (p.kv_tile_indices) kv_chunk = p.kv_tile_indices[work];
  } else if (p.num_kv_chunks > 1) {
    q_tile = work / p.num_kv_chunks;
    kv_chunk = work - q_tile * p.num_kv_chunks;
  }
  int qo_start = 0, qo_len, kv_len, kv_start = 0;
  if (p.qo_indptr) {
    qo_start = p.qo_indptr[req];
    qo_len = p.qo_indptr[req + 1] - qo_start;
    kv_start = p.kv_indptr[req];
    kv_len = p.kv_indptr[req + 1] - kv_start;
  } else {
    qo_len = p.single_qo_len;
    kv_len = p.single_kv_len;
  }
  const int G = p.group_size;
  const int packed_len = qo_len * G;
  const int row0 = q_tile * kTileQ + wave * 32;
  const int pr = row0 + lq;
  const bool row_valid = pr < packed_len;
  // a wave none of whose rows exist only stages K / V (wave-uniform)
  const bool wave_active = row0 < packed_len;
  const int prc = row_valid ? pr : (packed_len > 0 ? packed_len - 1 : 0);
  const int qo_idx = (int)fast_div((uint32_t)prc, p.group_div);
  const int hg = prc - qo_idx * G;
  const int qo_head = kv_head * G + hg;
  const int q_pos = kv_len - qo_len + qo_idx;

  // ---- Q fragments: lane (q, h) holds Q[q][16 ks + 8 h + 0..7], 12 k-steps ----
  frag_t qf[KSTEPS];
  {
    const int64_t qb = (int64_t)(qo_start + qo_idx) * p.q_stride_n + (int64_t)qo_head * p.q_stride_h;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)
      qf[ks] = __builtin_bit_cast(frag_t, *(const u32x4*)((const uint16_t*)p.q + qb + 16 * ks + 8 * lh));
  }
  const float c_log2 = p.sm_scale * kLog2e;

  // ---- kv range of this workgroup (as batch_prefill_kernel) ----
  int kv_end = kv_len;
  if (p.causal) {
    const int last_pr = min(q_tile * kTileQ + kTileQ, packed_len) - 1;
    const int last_qo = last_pr >= 0 ? (int)fast_div((uint32_t)last_pr, p.group_div) : 0;
    kv_end = min(kv_len, max(0, kv_len - qo_len + last_qo + 1));
  }
  int kv_begin = 0;
  if (p.window_left >= 0) {
    const int first_pr = min(q_tile * kTileQ, max(packed_len - 1, 0));
    const int first_qo = (int)fast_div((uint32_t)first_pr, p.group_div);
    kv_begin = max(kv_len - qo_len + first_qo - p.window_left, 0) / kTileKV * kTileKV;
  }
  if (split) {
    const int kv_chunk_size = p.kv_chunk_size_ptr ? *p.kv_chunk_size_ptr : p.kv_chunk_size;
    kv_begin += kv_chunk * kv_chunk_size;
    kv_end = min(kv_end, kv_begin + kv_chunk_size);
  }
  const int tile_base = kv_begin / kTileKV;
  const int num_tiles = kv_end > kv_begin ? (kv_end - kv_begin + kTileKV - 1) / kTileKV : 0;
  const int vis_hi_raw = p.causal ? min(kv_len - 1, q_pos) : kv_len - 1;
  const int vis_lo_raw = p.window_left >= 0 ? max(q_pos - p.window_left, 0) : 0;
  const bool sees_none = vis_hi_raw < vis_lo_raw;
  const int vis_lo = sees_none ? 0x40000000 : vis_lo_raw;
  const int vis_hi = sees_none ? 0x40000000 : vis_hi_raw;
  const int first_qo_wave = (int)fast_div((uint32_t)min(row0, max(packed_len - 1, 0)), p.group_div);
  const int min_qpos_wave = kv_len - qo_len + first_qo_wave;

  // ---- staging: thread (r0, c8) moves 16-byte chunk c8 (+ 8 seg) of tile rows r0 and r0 + 32 ----
  // K: 3 segments of 8 chunks per row, V: 2; every pass reads 8 rows x 128 contiguous bytes per wave.
  const int r0 = tid >> 3, c8 = tid & 7;
  const char* const k_thr = (const char*)p.k + ((int64_t)kv_head * p.k_stride_h + c8 * 8) * 2;
  const char* const v_thr = (const char*)p.v + ((int64_t)kv_head * p.v_stride_h + c8 * 8) * 2;
  const uint32_t k_sn = (uint32_t)p.k_stride_n, v_sn = (uint32_t)p.v_stride_n;
  struct KStage {
    u32x4 r[2][3];
  };
  struct VStage {
    u32x4 r[2][2];
  };
  // token (row of the ragged / dense tensor) of tile row r0 + 32 h, clamped into the request
  auto tok = [&](int tile, int h) -> uint32_t {
    return (uint32_t)(kv_start + max(min(tile * kTileKV + r0 + 32 * h, kv_len - 1), 0));
  };
  auto issue_k = [&](int tile, KStage& st) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const char* rowp = k_thr + (uint64_t)tok(tile, h) * k_sn * 2;
#pragma unroll
      for (int s = 0; s < 3; ++s) st.r[h][s] = *(const u32x4*)(rowp + 128 * s);
    }
  };
  auto issue_v = [&](int tile, VStage& st) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const char* rowp = v_thr + (uint64_t)tok(tile, h) * v_sn * 2;
#pragma unroll
      for (int s = 0; s < 2; ++s) st.r[h][s] = *(const u32x4*)(rowp + 128 * s);
    }
  };
  // K image for ds_read_b128: chunk ch of row r at (ch ^ ((r >> 1) & 7)); with the 96-dword row pitch the 16 rows of
  // a ds_read_b128 lane group then hit 16 distinct 4-dword bank windows.  The XOR stays inside an aligned 8-chunk
  // segment.  V image for ds_read_b64_tr_b16: batch_prefill_kernel's 256-byte-row layout.
  const int k_wr = r0 * KROWB + ((c8 ^ ((r0 >> 1) & 7)) << 4);
  const int v_wr = r0 * VROWB + ((((c8 >> 2) ^ (r0 & 3))) << 6) + ((c8 & 3) << 4);
  auto write_k = [&](int buf, const KStage& st) {
    char* kb = smem + buf * KTILE_BYTES;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 3; ++s) *(u32x4*)(kb + k_wr + 32 * h * KROWB + 128 * s) = st.r[h][s];
  };
  auto write_v = [&](const VStage& st) {
    char* vb = smem + V_LDS;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 vw = st.r[h][s];
        if constexpr (PV_F16) {
          // bf16 -> f16 (batch_prefill_kernel's write_v: exact for 2^-14 <= |v| < 65504)
          typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const uint32_t raw = st.r[h][s][w];
            const f16x2_t h2 = {(_Float16)__builtin_bit_cast(float, raw << 16),
                                (_Float16)__builtin_bit_cast(float, raw & 0xffff0000u)};
            vw[w] = __builtin_bit_cast(uint32_t, h2);
          }
        }
        // segment s = chunks 8 s .. 8 s + 7: 64-byte group (2 s + (c8 >> 2)) ^ (r & 3) = the s = 0 group ^ 2 s
        *(u32x4*)(vb + ((v_wr + 32 * h * VROWB) ^ (s << 7))) = vw;
      }
  };

  // ---- per-lane LDS read addresses ----
  // K fragment of k-step ks: row lq (+ 32 kb), chunk (2 ks + lh) ^ sw = 8 (ks >> 2) + ((2 (ks & 3)) ^ lh ^ sw): the
  // lane constant k_rd_base carries lh ^ sw in bits 4-6, above bit 6 only row bits (384 = 3 x 128)
  int k_rd_base = lq * KROWB + ((lh ^ ((lq >> 1) & 7)) << 4);
  auto k_rd = [&](int ks) { return (k_rd_base ^ ((2 * (ks & 3)) << 4)) + 128 * (ks >> 2); };
  const int q4 = (lane & 15) >> 2, p4 = lane & 3, gpar = (lane >> 4) & 1;
  int v_rd_base;
  {
    const int row = 4 * lh + q4;
    v_rd_base = row * VROWB + ((row & 3) << 6) + (16 * gpar + 4 * p4) * 2;
  }
  auto v_rd = [&](int db) { return v_rd_base ^ (db << 6); };

  f32x16 o_acc[DBLK];
#pragma unroll
  for (int db = 0; db < DBLK; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[db][r] = 0.f;
  float m_run = -1.0e30f, l_run = 0.f;

  if (num_tiles > 0) {
    // K rows two tiles ahead (kst), V rows one tile ahead (vst, issued after QK^T), as batch_prefill_kernel
    KStage kst;
    VStage vst;
    issue_k(tile_base, kst);
    issue_v(tile_base, vst);
    write_k(0, kst);
    write_v(vst);
    issue_k(tile_base + min(1, num_tiles - 1), kst);
    __syncthreads();
    auto tile_body = [&](auto buf_c, const int t) {
      constexpr int buf = decltype(buf_c)::value;
      const int t_next = tile_base + min(t + 1, num_tiles - 1);
      if (!wave_active) {
        write_k(buf ^ 1, kst);
        issue_k(tile_base + min(t + 2, num_tiles - 1), kst);
        issue_v(t_next, vst);
        __syncthreads();
        write_v(vst);
        __syncthreads();
        return;
      }
      asm volatile("" : "+v"(k_rd_base), "+v"(v_rd_base));
      write_k(buf ^ 1, kst);  // K rows of tile t+1 (its buffer was last read before the previous closing barrier)
      issue_k(tile_base + min(t + 2, num_tiles - 1), kst);
      const char* kb = smem + buf * KTILE_BYTES;
      const char* vb = smem + V_LDS;
      const int tile0 = (tile_base + t) * kTileKV;

      // ---- S^T = K Q^T: 24 MFMAs, K fragments kQkPrefetch ahead ----
      f32x16 s_acc[2];
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) s_acc[kbk][r] = 0.f;
      {
        constexpr int NK = 2 * KSTEPS;
        constexpr int PF = kQkPrefetch;
        u32x4 kf[NK];
        auto rd = [&](int i) { return *(const u32x4*)(kb + (i / KSTEPS) * 32 * KROWB + k_rd(i % KSTEPS)); };
#pragma unroll
        for (int i = 0; i < PF; ++i) kf[i] = rd(i);
#pragma unroll
        for (int i = 0; i < NK; ++i) {
          if (i + PF < NK) kf[i + PF] = rd(i + PF);
          s_acc[i / KSTEPS] = M::mfma(__builtin_bit_cast(frag_t, kf[i]), qf[i % KSTEPS], s_acc[i / KSTEPS]);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, PF, 0);
#pragma unroll
        for (int i = 0; i < NK - PF; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, PF, 0);
      }
      __builtin_amdgcn_sched_barrier(0);

      issue_v(t_next, vst);  // V rows of tile t+1

      // ---- mask: visible kv range [vis_lo, vis_hi] of this lane's query ----
      const bool need_mask = (tile0 + kTileKV > kv_len) || (p.causal && tile0 + kTileKV - 1 > min_qpos_wave) ||
                             (p.window_left >= 0);
      if (need_mask) {
        const unsigned span = (unsigned)(vis_hi - vis_lo);
        const int base_idx = tile0 + 4 * lh - vis_lo;
#pragma unroll
        for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const unsigned rel = (unsigned)(base_idx + 32 * kbk + (r & 3) + 8 * (r >> 2));
            s_acc[kbk][r] = rel <= span ? s_acc[kbk][r] : -INFINITY;
          }
      }

      // ---- online softmax, base 2, deferred rescale (batch_prefill_kernel) ----
      float mx = s_acc[0][0];
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s_acc[kbk][r]);
      mx = fmaxf(mx, swap_halves(mx));
      constexpr float kRescaleLog2 = 6.f;
      constexpr float kPShift = PV_F16 ? 9.f : 0.f;
      const float m_true = fmaxf(m_run, mx * c_log2);
      if (__any(m_true - m_run > kRescaleLog2)) {
        const float alpha = fast_exp2(m_run - m_true);
        m_run = m_true;
        l_run *= alpha;
#pragma unroll
        for (int db = 0; db < DBLK; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o_acc[db][r] *= alpha;
      }
      float psum = 0.f;
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s_acc[kbk][r] = fast_exp2(__builtin_fmaf(s_acc[kbk][r], c_log2, kPShift - m_run));
          psum += s_acc[kbk][r];
        }
      l_run += psum;

      // ---- O^T += V^T P^T ----
#pragma unroll
      for (int kbk = 0; kbk < 2; ++kbk) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          u32x4 w;
          [[maybe_unused]] u32x4 w_lo;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float a = s_acc[kbk][8 * s2 + 2 * j], b = s_acc[kbk][8 * s2 + 2 * j + 1];
            w[j] = pack2<TPV>(a, b);
            if constexpr (P_HI_LO) {
              const float a_hi = __builtin_bit_cast(float, w[j] << 16);
              const float b_hi = __builtin_bit_cast(float, w[j] & 0xffff0000u);
              w_lo[j] = pack2<T16>(a - a_hi, b - b_hi);
            }
          }
          using pv_frag_t = typename MPV::frag;
          const pv_frag_t pfrag = __builtin_bit_cast(pv_frag_t, w);
#pragma unroll
          for (int db = 0; db < DBLK; ++db) {
            const char* base = vb + (32 * kbk + 16 * s2) * VROWB + v_rd(db);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
            const s16x4 hi =
                __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 8 * VROWB));
            using s16x8 = __attribute__((ext_vector_type(8))) short;
            const s16x8 a8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            o_acc[db] = MPV::mfma(__builtin_bit_cast(pv_frag_t, a8), pfrag, o_acc[db]);
            if constexpr (P_HI_LO)
              o_acc[db] = M::mfma(__builtin_bit_cast(frag_t, a8), __builtin_bit_cast(frag_t, w_lo), o_acc[db]);
          }
        }
      }

      __syncthreads();  // every wave is done with V(t)
      write_v(vst);     // V rows of tile t+1
      __syncthreads();
    };
    int t = 0;
    for (; t + 1 < num_tiles; t += 2) {
      tile_body(std::integral_constant<int, 0>{}, t);
      tile_body(std::integral_constant<int, 1>{}, t + 1);
    }
    if (t < num_tiles) tile_body(std::integral_constant<int, 0>{}, t);
  }

  // ---- finalize ----
  l_run += swap_halves(l_run);
  const bool empty = !(l_run > 0.f);
  const float inv = empty ? 0.f : 1.0f / l_run;
  const float lse_val = empty ? FI_NEG_INF : m_run + fast_log2(l_run) - (PV_F16 ? 9.f : 0.f);
  if (row_valid && split) {
    const int64_t entry = p.merge_indptr ? (int64_t)p.merge_indptr[qo_start + qo_idx] + kv_chunk
                                         : (int64_t)(qo_start + qo_idx) * p.num_kv_chunks + kv_chunk;
    const int64_t ob = (entry * p.num_qo_heads + qo_head) * kQkvoDimVO;
#pragma unroll
    for (int db = 0; db < DBLK; ++db)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int d0 = 32 * db + 8 * r4 + 4 * lh;
        *(f32x4*)(p.tmp_o + ob + d0) = f32x4{o_acc[db][4 * r4 + 0] * inv, o_acc[db][4 * r4 + 1] * inv,
                                             o_acc[db][4 * r4 + 2] * inv, o_acc[db][4 * r4 + 3] * inv};
      }
    if (lh == 0) p.tmp_lse[entry * p.num_qo_heads + qo_head] = lse_val;
  } else if (row_valid) {
    const int64_t ob = ((int64_t)(qo_start + qo_idx) * p.num_qo_heads + qo_head) * kQkvoDimVO;
#pragma unroll
    for (int db = 0; db < DBLK; ++db)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int d0 = 32 * db + 8 * r4 + 4 * lh;
        const uint32_t w0 = pack2<T16>(o_acc[db][4 * r4 + 0] * inv, o_acc[db][4 * r4 + 1] * inv);
        const uint32_t w1 = pack2<T16>(o_acc[db][4 * r4 + 2] * inv, o_acc[db][4 * r4 + 3] * inv);
        *(u32x2*)((uint16_t*)p.o + ob + d0) = u32x2{w0, w1};
      }
    if (p.lse && lh == 0) p.lse[(int64_t)(qo_start + qo_idx) * p.num_qo_heads + qo_head] = lse_val;
  }
}

}  // namespace fi
