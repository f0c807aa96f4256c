// Contiguous-layout grouped fp8 GEMM for expert-parallel MoE prefill: the kernel of fi_group_gemm_fp8_nt_contiguous.
//
// What it replaces: the reference's group_deepgemm_fp8_nt_groupwise (flashinfer/gemm.py:2991-3118, over deep_gemm.py
// m_grouped_fp8_gemm_nt_contiguous).  The layout is the normal-mode all-to-all's: a (m, k) e4m3, b (G, n, k) e4m3,
// a_scale (m, k / 128) f32, b_scale (G, n / 128, k / 128) f32, d (m, n) f16 / bf16, and m_indices[r] on the DEVICE
// names the group of row r.  Segments are padded to multiples of 128 rows, so block i (rows 128 i .. 128 i + 127, the
// last one possibly short) belongs to ONE group g = m_indices[128 i], or to none (g < 0 or g >= G: dead).  Rows of a
// live block with a negative index are tail padding.  For the live rows r of a live block
//   d[r, j] = sum_kb a_scale[r, kb] b_scale[g, j / 128, kb] sum_{k in block kb} a[r, k] b[g, j, k]
// f32 accumulation, k blocks in ascending order, one rounding.
//
// Group lookup.  The tile is 128 rows = exactly one layout block, by 256 columns, so the (group, m tile) search of the
// m_indptr kernels (find_group_tile: a wave scan over the groups) is one scalar load of m_indices[128 i].  A dead
// block costs that load and nothing else: every workgroup first lists the live blocks in LDS (one load per block and
// a workgroup scan; up to 2032 blocks = 260 096 rows, past that dead blocks are skipped where they lie) and the walk
// deals out live tiles only.  A live tile then reads its 128 indices once (two loads per lane) and keeps
// the rows' liveness as two ballots in scalar registers: loads of a dead row (tail padding, or at / past m) are
// clamped to the tile's first row, which is live by definition, and the row is masked at the store, so nothing of a
// padding row -- NaN included -- reaches memory.
//
// Walk.  A persistent grid, one 512-thread workgroup per compute unit, XCD-aligned: XCD x (workgroups b with
// b & 7 == x) owns a contiguous share of the (live block, n tile) pairs in banded order -- bands of 8 blocks x all n tiles,
// block fastest -- and its workgroups stride through it.  The workgroups of an XCD in flight together so work on
// consecutive blocks of the same n tile; neighbouring blocks usually belong to one expert, so they read the same
// b[g, n tile] panel from the XCD's L2.
//
// Main loop, per 128-wide k block: 8 waves as 2 (m) x 4 (n), wave tile 64 x 64, the product TRANSPOSED (d^T = b a^T,
// m on the lane) on v_mfma_scale_f32_32x32x64_f8f6f4 with unit hardware scales into a fresh accumulator that one FMA
// per element folds into the running sum with a_scale[row, kb] b_scale[g, nb, kb] (two-level accumulation, as gemm.hip).
// Operands go global -> LDS by DMA (1 KiB per wave instruction, the image swizzle applied on the global side), two k
// blocks ahead through a ring of three 52 KB stages [a 128 rows | b 256 rows | scales].  a_scale is K-major here: the
// tile's 128 scales of a k block are a 4-byte gather with a row stride, and they ride the same DMA -- lane L of a wave
// fetches the scale of row 64 wm + L into the stage -- so the loop holds no ordinary global load.  Waits are by hand:
// vmcnt(8) (this wave's 8 DMA instructions of the block after next stay in flight) or vmcnt(0), then s_barrier
// (wait_vmcnt_barrier; tools/isa_guard.py checks the counts).
//
// Output: through LDS stage 2 (free at a tile border, while the next tile's first two blocks land in stages 0 and 1)
// as 64-byte row pieces, 16 bytes per lane.
#include <type_traits>

#include "gemm_common.h"

namespace fi {

constexpr int kCgThreads = 512;
constexpr int kCgTM = 128, kCgTN = 256;
constexpr int kCgScOff = (kCgTM + kCgTN) * kBK;                // 48 KB of operands, then the scales
constexpr int kCgStage = kCgScOff + (kCgThreads / 64) * 512;  // per wave: 64 a scales, 64 x the b scale
constexpr int kCgBandM = 8;                                   // blocks per band of the walk
constexpr int kCgList = 3 * kCgStage;                         // behind the stages: the scan's scratch, the live blocks
constexpr int kCgListBytes = 4096;                            // what the 160 KB leave
constexpr int kCgMaxListed = (kCgListBytes - 32) / 2;         // 16-bit block ids

__global__ void __launch_bounds__(kCgThreads, 1) group_gemm_fp8_contig_kernel(const ContigGemmParams p) {
  // ONE array: the compiler tells a DMA target from an LDS read by constant offsets inside one object
  __shared__ __attribute__((aligned(1024))) uint8_t smem[kCgList + kCgListBytes];
  constexpr int kBOff = kCgTM * kBK;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lq = lane & 31, lh = lane >> 5;
  const int M = p.m, N = p.n, K = p.k;
  const int kblocks = K / kBK, n_sblocks = N / 128;
  uint32_t a_rd_base = (uint32_t)image_off(64 * wm + lq, 2 * lh);
  uint32_t b_rd_base = (uint32_t)(kBOff + image_off(64 * wn + lq, 2 * lh));

  // ---- the live blocks, in order: every workgroup lists them in LDS (512 first-row indices per pass, a workgroup scan
  // for their places), so that the walk below deals out live tiles only -- dead blocks, which an oversized buffer
  // has at its end and a layout may have anywhere, would otherwise leave the workgroups they fall to idle.  More
  // blocks than the list holds: the walk covers every block and skips the dead ones where they lie.
  const int m_blocks = (M + kCgTM - 1) / kCgTM, n_tiles = (N + kCgTN - 1) / kCgTN;
  const bool listed = m_blocks <= kCgMaxListed;
  const uint16_t* const live_blk = (const uint16_t*)&smem[kCgList + 32];
  int walk_blocks = m_blocks;
  if (listed) {
    int run = 0;
    for (int base = 0; base < m_blocks; base += kCgThreads) {
      const int blk = base + tid;
      const int first = blk < m_blocks ? p.m_indices[blk * kCgTM] : -1;
      const int flag = first >= 0 && first < p.num_groups;
      int total;
      const int pos = run + block_incl_scan<kCgThreads / 64>(flag, (int*)&smem[kCgList], total) - flag;
      if (flag) *(uint16_t*)&smem[kCgList + 32 + 2 * pos] = (uint16_t)blk;
      run += total;
    }
    __syncthreads();
    walk_blocks = __builtin_amdgcn_readfirstlane(run);
  }

  // ---- this XCD's contiguous share of the (block, n tile) pairs, strided by its workgroups ----
  const TileShare share = xcd_share(walk_blocks * n_tiles, blockIdx.x & 7);
  int logical = share.start + (blockIdx.x >> 3);
  const int logical_end = share.start + share.count, logical_step = gridDim.x >> 3;

  f32x16g acc[2][2];  // [n block][m block]; register r of a block: n = 8 (r / 4) + 4 lh + r % 4, m = lq
  int out_m0 = 0, out_n0 = 0;        // tile whose accumulators are waiting to be stored
  uint64_t out_live0 = 0, out_live1 = 0;  // and its live rows
  bool have_out = false;
  constexpr int kOutStride = 80;
  const bool d_aligned16 = (((uintptr_t)p.d) & 15) == 0;
  // bit `row` of the 128 live bits (two ballots, in scalar registers)
  auto row_live = [](uint64_t live0, uint64_t live1, int row) { return (((row & 64) ? live1 : live0) >> (row & 63)) & 1; };
  auto store_tile = [&]() {
    uint8_t* const scratch = &smem[2 * kCgStage] + wave * (64 * kOutStride);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          *(u32x2*)(scratch + (32 * mb + lq) * kOutStride + (8 * r4 + 4 * lh) * 2) =
              pack4_16bit(acc[nb][mb], 4 * r4, p.out_dtype);
#pragma unroll
      for (int i2 = 0; i2 < 4; ++i2) {
        const int idx = lane + 64 * i2;
        const int r = idx >> 2, c = idx & 3;
        const u32x4 v = *(const u32x4*)(scratch + r * kOutStride + c * 16);
        const int row = 64 * wm + r;
        const int n = out_n0 + 64 * wn + 32 * nb + 8 * c;
        if (!row_live(out_live0, out_live1, row) || n >= N) continue;  // tail padding, rows at or past m, the short last n tile
        store_row_piece((uint16_t*)p.d + (int64_t)(out_m0 + row) * N + n, v, d_aligned16);
      }
    }
  };

  for (; logical < logical_end; logical += logical_step) {
    int blk, nt;
    band_tile_of<kCgBandM>(logical, walk_blocks, n_tiles, blk, nt);
    if (listed) blk = __builtin_amdgcn_readfirstlane(live_blk[blk]);
    const int m0 = blk * kCgTM;
    const int n0 = nt * kCgTN;
    // the block's group: one scalar load (m_indices does not change under the kernel: the constant address space
    // makes the uniform load an s_load_dword behind the kernel's own stores); a dead block (unlisted walk) ends here
    const int g = *(const __attribute__((address_space(4))) int32_t*)(uintptr_t)(p.m_indices + m0);
    if (g < 0 || g >= p.num_groups) continue;
    // the block's live rows (row 0 is: g >= 0)
    const int r0 = m0 + lane, r1 = m0 + 64 + lane;
    const int idx0 = p.m_indices[min(r0, M - 1)], idx1 = p.m_indices[min(r1, M - 1)];
    const uint64_t live0 = __ballot(r0 < M && idx0 >= 0), live1 = __ballot(r1 < M && idx1 >= 0);

    // LDS-DMA geometry: the stage image is [384 rows][128 B] (a rows 0-127, b rows 128-383) and a piece = one wave
    // instruction = 8 rows = 1 KiB of it, written linearly (lane i -> byte 16 i of the piece).  The XOR swizzle is
    // applied on the GLOBAL side: lane i fetches chunk (i & 7) ^ key(row) of row (i >> 3).  Wave w owns pieces
    // 6 w .. 6 w + 5 of the 48.  A dead row of a re-reads row 0 of the tile, a row of b past n the last row.
    const uint8_t* const a_tile = p.a + (int64_t)m0 * K;
    const uint8_t* const b_tile = p.b + ((int64_t)g * N + n0) * K;
    uint32_t d_off[6];
#pragma unroll
    for (int j2 = 0; j2 < 6; ++j2) {
      const int row = 8 * (6 * wave + j2) + (lane >> 3);
      const int ch = image_chunk(row, lane & 7);
      const int r = row < kCgTM ? (row_live(live0, live1, row & (kCgTM - 1)) ? row : 0) : min(n0 + row - kCgTM, N - 1) - n0;
      d_off[j2] = (uint32_t)r * (uint32_t)K + ch * 16;
    }
    // scale sources for the DMA: one a-scale pointer per lane (row 64 wm + lane of the tile, clamped like the row
    // itself), the b scale of this wave's 128-wide block fetched by every lane
    const int nsb = min((n0 + 64 * wn) / 128, n_sblocks - 1);
    const float* const b_sc = p.b_scale + ((int64_t)g * n_sblocks + nsb) * kblocks;
    const int sc_row = 64 * wm + lane;
    const float* const a_sc = p.a_scale + (int64_t)(m0 + (row_live(live0, live1, sc_row) ? sc_row : 0)) * kblocks;
    auto dma = [&](int kb, int stage) {
      const uint32_t koff = (uint32_t)(kb * kBK);
#pragma unroll
      for (int j2 = 0; j2 < 6; ++j2) {
        const int q = 6 * wave + j2;
        lds_dma16((q < kCgTM / 8 ? a_tile : b_tile) + (d_off[j2] + koff), &smem[stage * kCgStage + q * 1024]);
      }
      lds_dma4(a_sc + kb, &smem[stage * kCgStage + kCgScOff + wave * 512]);
      lds_dma4(b_sc + kb, &smem[stage * kCgStage + kCgScOff + wave * 512 + 256]);
    };
    // the next tile's first two blocks go out BEFORE the finished tile is converted and stored (stages 0 and 1; the
    // store's scratch is stage 2): with one workgroup per CU nothing else would cover the round trip
    dma(0, 0);
    if (kblocks > 1) dma(1, 1);
    const bool stored = have_out;
    if (have_out) store_tile();
    out_m0 = m0;
    out_n0 = n0;
    out_live0 = live0;
    out_live1 = live1;
    have_out = true;
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i2][j2][r] = 0.f;
    // Block 0 landed.  The output stores are younger than both blocks and vmcnt retires in order, so with stores in
    // the queue the only count that is sure to cover block 0 is 0.  (Also: every wave is done with the stage 2
    // scratch before step 0's DMA.)
    if (kblocks > 1 && !stored) wait_vmcnt_barrier<8>();
    else wait_vmcnt_barrier<0>();
    f32x16g p_carry;  // block (1, 1) of the previous k step, folded at the start of the next one
#pragma unroll
    for (int r = 0; r < 16; ++r) p_carry[r] = 0.f;
    float s_carry = 0.f;

    auto k_step = [&](auto par_c, const int kb) {
      constexpr int buf = decltype(par_c)::value;  // == kb % 3
      if (kb + 2 < kblocks) dma(kb + 2, (buf + 2) % 3);  // block kb + 2 into the stage read in step kb - 1
      const float* const sc = (const float*)(&smem[buf * kCgStage + kCgScOff + wave * 512]);
      const float sa[2] = {sc[lq], sc[32 + lq]};
      const float sb = sc[64 + lane];
      asm volatile("" : "+v"(a_rd_base), "+v"(b_rd_base));  // fragment addresses are recomputed here, not kept
      const uint8_t* const stage = &smem[buf * kCgStage];
      auto fold = [&](int nb, int mb, const f32x16g& part, float s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][mb][r] += s * part[r];
        asm volatile("" : "+v"(acc[nb][mb]));  // IR-level sinking ignores sched_barrier: pin the fold here
      };
      const float s0 = sa[0] * sb, s1 = sa[1] * sb;
      i32x8g fa0[2], fa1[2], fb0[2], fb1[2];
      // The two MFMAs of a 32 x 32 block are dependent (same accumulator), so the previous block's fold sits between
      // them, in the shadow of the first; the fold carried over from the previous k step hides the fragment reads.
      fa0[0] = fp8_frag(stage, a_rd_base, 0, 0);
      fb0[0] = fp8_frag(stage, b_rd_base, 0, 0);
      fa0[1] = fp8_frag(stage, a_rd_base, 1, 0);
      fb0[1] = fp8_frag(stage, b_rd_base, 1, 0);
      fa1[0] = fp8_frag(stage, a_rd_base, 0, 1);
      fa1[1] = fp8_frag(stage, a_rd_base, 1, 1);
      fold(1, 1, p_carry, s_carry);
      __builtin_amdgcn_sched_barrier(0);
      f32x16g p00 = mfma_fp8_zero<false, false>(fb0[0], fa0[0]);
      __builtin_amdgcn_sched_barrier(0);
      fb1[0] = fp8_frag(stage, b_rd_base, 0, 1);
      fb1[1] = fp8_frag(stage, b_rd_base, 1, 1);
      __builtin_amdgcn_sched_barrier(0);
      p00 = mfma_fp8<false, false>(fb0[1], fa0[1], p00);
      f32x16g p01 = mfma_fp8_zero<false, false>(fb0[0], fa1[0]);
      __builtin_amdgcn_sched_barrier(0);
      fold(0, 0, p00, s0);
      __builtin_amdgcn_sched_barrier(0);
      p01 = mfma_fp8<false, false>(fb0[1], fa1[1], p01);
      f32x16g p10 = mfma_fp8_zero<false, false>(fb1[0], fa0[0]);
      __builtin_amdgcn_sched_barrier(0);
      fold(0, 1, p01, s1);
      __builtin_amdgcn_sched_barrier(0);
      p10 = mfma_fp8<false, false>(fb1[1], fa0[1], p10);
      f32x16g p11 = mfma_fp8_zero<false, false>(fb1[0], fa1[0]);
      __builtin_amdgcn_sched_barrier(0);
      fold(1, 0, p10, s0);
      __builtin_amdgcn_sched_barrier(0);
      p11 = mfma_fp8<false, false>(fb1[1], fa1[1], p11);
      p_carry = p11;
      s_carry = s1;
      // block kb + 1 must have landed (all waves' pieces: barrier); the 8 instructions of block kb + 2 stay in flight
      if (kb + 2 < kblocks) wait_vmcnt_barrier<8>();
      else wait_vmcnt_barrier<0>();
      __builtin_amdgcn_sched_barrier(0);  // no mixing of two k steps either
    };
    {
      int kb = 0;
      for (; kb + 2 < kblocks; kb += 3) {
        k_step(std::integral_constant<int, 0>{}, kb);
        k_step(std::integral_constant<int, 1>{}, kb + 1);
        k_step(std::integral_constant<int, 2>{}, kb + 2);
      }
      if (kb < kblocks) k_step(std::integral_constant<int, 0>{}, kb);
      if (kb + 1 < kblocks) k_step(std::integral_constant<int, 1>{}, kb + 1);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[1][1][r] += s_carry * p_carry[r];
  }
  if (have_out) store_tile();
}

void launch_gemm_contig(const ContigGemmParams& p, int grid, hipStream_t stream) {
  group_gemm_fp8_contig_kernel<<<dim3(grid), dim3(kCgThreads), 0, stream>>>(p);
}

}  // namespace fi
