// Batch / single prefill: host planner, dispatcher and C-ABI entry points.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "merge_kernel.h"
#include "prefill_kernel.h"
#include "prefill_plan.h"
#include "prefill_qkvo_kernel.h"

namespace fi {

typedef hipError_t (*prefill_launch_fn)(const PrefillKernelParams&, int, hipStream_t);

#define FI_PF_DECL(T, K, Q, D) \
  hipError_t prefill_launch_##T##_##K##_##Q##_##D(const PrefillKernelParams&, int, hipStream_t);
#define FI_PF_DECL_D(T, K, Q) FI_PF_DECL(T, K, Q, 64) FI_PF_DECL(T, K, Q, 128) FI_PF_DECL(T, K, Q, 256)
// 16-bit q: kv of the same type, or fp8 kv upcast on the fly (ref: prefill.cuh:637-647, 993-1004)
FI_PF_DECL_D(0, 0, 0) FI_PF_DECL_D(0, 2, 0) FI_PF_DECL_D(0, 3, 0)
FI_PF_DECL_D(1, 1, 1) FI_PF_DECL_D(1, 2, 1) FI_PF_DECL_D(1, 3, 1)
// fp8 q + fp8 kv (ref FA3 fp8 path), output type picks the compute type
FI_PF_DECL_D(0, 2, 2) FI_PF_DECL_D(1, 2, 2) FI_PF_DECL_D(0, 3, 3) FI_PF_DECL_D(1, 3, 3)
#undef FI_PF_DECL
#undef FI_PF_DECL_D

hipError_t prefill_fp8_launch(const PrefillKernelParams& p, int out_dtype, int e5m2, int head_dim, hipStream_t stream);

// fp8-native kernel (MX-scaled MFMA for both contractions): e4m3 or e5m2 q/k/v, plain logits, no fused RoPE, no
// sliding window, no custom mask.  fp8 runs with any of those go through the upcast-to-16-bit kernel.
static bool use_fp8_native(const PrefillKernelParams& kp, int q_dt, int kv_dt, int rope) {
  return (q_dt == FI_DTYPE_FP8_E4M3 || q_dt == FI_DTYPE_FP8_E5M2) && kv_dt == q_dt && !rope && !kp.use_alibi &&
         kp.logits_soft_cap == 0.f && kp.window_left < 0 && !kp.custom_mask;
}

static prefill_launch_fn find_prefill(int t16, int kvs, int qs, int d) {
#define FI_TRY(T, K, Q)                                       \
  if (t16 == T && kvs == K && qs == Q) {                      \
    if (d == 64) return prefill_launch_##T##_##K##_##Q##_64;  \
    if (d == 128) return prefill_launch_##T##_##K##_##Q##_128; \
    if (d == 256) return prefill_launch_##T##_##K##_##Q##_256; \
    return nullptr;                                           \
  }
  FI_TRY(0, 0, 0) FI_TRY(0, 2, 0) FI_TRY(0, 3, 0)
  FI_TRY(1, 1, 1) FI_TRY(1, 2, 1) FI_TRY(1, 3, 1)
  FI_TRY(0, 2, 2) FI_TRY(1, 2, 2) FI_TRY(0, 3, 3) FI_TRY(1, 3, 3)
#undef FI_TRY
  return nullptr;
}

// compute type for (q dtype, o dtype)
static int compute_type(int q_dt, int o_dt) {
  if (q_dt == FI_DTYPE_F16 || q_dt == FI_DTYPE_BF16) return q_dt;
  return o_dt;  // fp8 q: f16 or bf16 output decides
}

// A measured batch: per request the q tiles, the kv span its chunks are cut from and the query rows; the totals.
struct BatchShape {
  int n;
  const int64_t *q_tiles, *kv_len, *qo_rows;
  int64_t total_q_tiles, max_kv_len;
};

static_assert(kPlanTileQ == kTileQ && kPlanTileKV == kTileKV, "prefill_plan.h restates the kernels' tile sizes");

int64_t resident_items(int num_kv_heads) {
  return std::max<int64_t>((int64_t)fi_num_compute_units() * 2 / num_kv_heads, 1);
}

// q tiles and kv spans (ref: PrefillSplitQOKVIndptr, scheduler.cuh:495-614, with packed_qo_len = qo_len * G and a
// fixed 128-row q tile).  `store` holds the three per-request arrays `s` points into.
static int measure_batch(const int32_t* qo_indptr_h, const int32_t* kv_len_arr_h, int batch_size, int group,
                         bool causal, int window_left, std::vector<int64_t>& store, BatchShape& s) {
  store.resize((size_t)batch_size * 3);
  int64_t *q_tiles = store.data(), *kv_len = q_tiles + batch_size, *qo_rows = kv_len + batch_size;
  s = BatchShape{batch_size, q_tiles, kv_len, qo_rows, 0, 1};
  for (int b = 0; b < batch_size; ++b) {
    qo_rows[b] = qo_indptr_h[b + 1] - qo_indptr_h[b];
    FI_REQUIRE(qo_rows[b] >= 0, "batch_prefill_plan: qo_indptr must be non-decreasing");
    FI_REQUIRE(kv_len_arr_h[b] >= 0, "batch_prefill_plan: negative kv length");
    q_tiles[b] = ceil_div<int64_t>(qo_rows[b] * group, kTileQ);
    kv_len[b] = kv_span(kv_len_arr_h[b], qo_rows[b], causal, window_left);
    s.total_q_tiles += q_tiles[b];
    s.max_kv_len = std::max(s.max_kv_len, kv_len[b]);
  }
  return 0;
}

// Chunk choice by price.  The reference rule cuts as fine as max_items allows.  On this part that over-splits whenever
// the batch has rows to merge: every chunk writes, and the merge reads back, an f32 partial row per query row and head
// (bs 1, qo = kv = 1024: 82 us split in two against 31 us whole; bs 2, 512 x 4096: 132 against 95), while few-row
// requests gain a lot (bs 1, 16 x 8192: 28 against 159 us).  So the candidates chunk, 2 x chunk, 4 x chunk ... and
// "whole" (returned as the kv span rounded up to a kv tile) are priced with a two-term model -- workgroup rounds per CU
// x tokens per item x 20 ns (per 256 of head_dim_qk + head_dim_vo), plus for a split 6 us + partial-state bytes at
// 3 TB/s -- and the cheapest wins (ties: the coarser).
static int64_t price_kv_chunk(int64_t ref_chunk, const BatchShape& s, int num_kv_heads, int num_qo_heads,
                              int head_dim_qk, int head_dim_vo) {
  const int64_t cus = fi_num_compute_units();
  const int64_t tok_ns = std::max<int64_t>(20 * (head_dim_qk + head_dim_vo) / 256, 1);
  auto cost_ns = [&](int64_t chunk, bool split) {
    int64_t items = 0, entries = 0;
    for (int b = 0; b < s.n; ++b) {
      const int64_t nc = split ? ceil_div<int64_t>(s.kv_len[b], chunk) : 1;
      items += s.q_tiles[b] * nc;
      entries += s.qo_rows[b] * nc;
    }
    int64_t t = ceil_div<int64_t>(items * num_kv_heads, cus) * std::min(chunk, s.max_kv_len) * tok_ns;
    if (split) t += 6000 + entries * num_qo_heads * head_dim_vo * 8 / 3000;
    return t;
  };
  const int64_t whole = ceil_div<int64_t>(s.max_kv_len, kTileKV) * kTileKV;
  int64_t best = whole, best_cost = cost_ns(whole, false);
  for (int64_t c = ref_chunk; c < s.max_kv_len; c *= 2) {
    const int64_t t = cost_ns(c, true);
    if (t < best_cost || (t == best_cost && c > best && best != whole)) {
      best = c;
      best_cost = t;
    }
  }
  return best;
}

struct KvChunk { int64_t size; bool split_kv; };  // split_kv: the launch writes partial states and merges them

// The kv chunk of a batch, or of one request (split_single_kv).  graph_items: the items a graph plan's launch is padded
// to, 0 for a plan that is not captured.
static KvChunk choose_kv_chunk(const BatchShape& s, int num_qo_heads, int num_kv_heads, int head_dim_qk,
                               int head_dim_vo, size_t float_ws_bytes, int64_t graph_items, int fixed_split_size,
                               bool disable_split_kv) {
  // chunk sizes are multiples of one 64-row kv tile and at least 128 tokens (ref: min_kv_chunk_size)
  const int64_t chunk_unit = kTileKV;
  int64_t kv_chunk = ceil_div<int64_t>(s.max_kv_len, chunk_unit) * chunk_unit;  // one chunk = no split
  if (disable_split_kv || s.n <= 0) return {kv_chunk, false};
  const int64_t max_items = resident_items(num_kv_heads);
  auto items_at = [&](int64_t chunk) {
    int64_t n = 0;
    for (int b = 0; b < s.n; ++b) n += s.q_tiles[b] * ceil_div<int64_t>(s.kv_len[b], chunk);
    return n;
  };
  if (fixed_split_size > 0) {
    kv_chunk = ceil_div<int64_t>(fixed_split_size, chunk_unit) * chunk_unit;
  } else {
    // ref: PrefillBinarySearchKVChunkSize, scheduler.cuh:101-130 (in units of 64 tokens)
    kv_chunk = chunk_unit * smallest_fitting(128 / chunk_unit, ceil_div<int64_t>(s.max_kv_len, chunk_unit),
                                             [&](int64_t n) { return items_at(n * chunk_unit) > max_items; });
    // Graph plans keep the reference rule (they always split).
    if (!graph_items) kv_chunk = price_kv_chunk(kv_chunk, s, num_kv_heads, num_qo_heads, head_dim_qk, head_dim_vo);
  }
  // Load balance (not in the reference, whose rule above only ever splits a batch of fewer than max_items items): a
  // mixed batch -- many short requests and a few long ones with few query rows -- otherwise ends in a tail of
  // single workgroups walking the long requests (reference benchmark bench_batch_attention.py, 122 x (600, 1) + 8 x
  // (10000, 17): 0.23 ms for 0.3 GB).  With W = sum of q tiles x kv length, the ideal makespan is W / max_items;
  // chunks of at most half of that (and >= 256 tokens) let the longest-first work list even out.  A batch whose long
  // requests also have many query rows has a large W and keeps its single chunk; graph plans keep the reference
  // rule (their item count must stay under the captured bound).
  // Only where the reference rule left every request whole AND the batch is uneven (longest request >= twice the
  // mean item): an even batch gains nothing from more items (decode-only 128 x 8192 through this wrapper: -6 %), and
  // a batch the reference rule already cut is compute-bound prefill (4 x (4096, 128): -12 % when cut finer).
  if (fixed_split_size <= 0 && !graph_items && kv_chunk >= s.max_kv_len && s.total_q_tiles > 0) {
    int64_t work = 0;
    for (int b = 0; b < s.n; ++b) work += s.q_tiles[b] * s.kv_len[b];
    const int64_t bal = ceil_div<int64_t>(std::max<int64_t>(work / (2 * max_items), 256), chunk_unit) * chunk_unit;
    if (s.max_kv_len * s.total_q_tiles >= 2 * work && 2 * bal <= s.max_kv_len && items_at(bal) <= 8 * max_items)
      kv_chunk = bal;
  }
  // the partial states must fit the caller's float workspace: grow the chunks until they do (a plan
  // that cannot split at all is still correct, only less parallel)
  if (fixed_split_size <= 0) {
    auto ws_need = [&](int64_t chunk) {
      int64_t entries = 0;
      for (int b = 0; b < s.n; ++b) entries += s.qo_rows[b] * ceil_div<int64_t>(s.kv_len[b], chunk);
      int64_t lse_entries = entries;
      if (graph_items)  // the fixed lse region of a graph plan (see fi_batch_prefill_plan)
        lse_entries = std::max(entries, std::max(items_at(chunk), graph_items) *
                                            (ceil_div<int64_t>(kTileQ, num_qo_heads / num_kv_heads) + 1));
      return (entries * num_qo_heads * head_dim_vo + lse_entries * num_qo_heads + 64) * (int64_t)sizeof(float);
    };
    while (kv_chunk < s.max_kv_len && ws_need(kv_chunk) > (int64_t)float_ws_bytes) kv_chunk *= 2;
  }
  // a fixed-shape (graph) launch always takes the split path so that the kernel sequence does not
  // depend on the page table (ref: scheduler.cuh:129)
  return {kv_chunk, kv_chunk < s.max_kv_len || graph_items};
}

struct WorkItem { int32_t req, tile, kvt; };  // request, q tile, kv chunk

// work list, costliest first (requests by rows per q tile x kv_len descending; for causal masks the later = heavier q
// tiles first) so the tail of the launch is made of the cheapest items (ref LPT idea: scheduler.cuh:900-946)
static std::vector<WorkItem> build_work_list(const BatchShape& s, const int32_t* kv_len_arr_h, int group, bool causal,
                                             int64_t kv_chunk, bool split_kv) {
  std::vector<int> order(s.n);
  std::iota(order.begin(), order.end(), 0);
  // (cost of a request's items ~ rows of a q tile x kv length: in a mixed batch the compute-bound full tiles of a
  // prefill request go out before the memory-bound one-row items of equally long decode requests and run beside
  // them, instead of forming the tail -- bench_batch_attention.py's 254 x (8192, 1) + (8192, 4096))
  auto item_cost = [&](int b) {
    const int64_t rows = std::min<int64_t>(s.qo_rows[b] * group, kTileQ);
    return (int64_t)kv_len_arr_h[b] * std::max<int64_t>(rows, 1);
  };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return item_cost(a) > item_cost(b); });
  std::vector<WorkItem> w;
  for (int b : order) {
    const int64_t ntiles = s.q_tiles[b];
    const int64_t nchunks = split_kv ? ceil_div<int64_t>(s.kv_len[b], kv_chunk) : 1;
    for (int64_t t = 0; t < ntiles; ++t)
      for (int64_t c = 0; c < nchunks; ++c) w.push_back({b, (int32_t)(causal ? ntiles - 1 - t : t), (int32_t)c});
  }
  // Mixed batches: a q tile with many rows is compute-bound, one with a few rows (decode-like) streams its keys at
  // HBM rate.  Listed one kind after the other they run as two phases; interleaved in proportion (each kind keeps its
  // costliest-first order) the two kinds share the CUs and overlap.  Pure batches (one kind only) are unchanged.
  std::vector<size_t> wide, narrow;
  for (size_t i = 0; i < w.size(); ++i) {
    const int64_t rows_left = s.qo_rows[w[i].req] * group - (int64_t)w[i].tile * kTileQ;
    (std::min<int64_t>(rows_left, kTileQ) * 2 >= kTileQ ? wide : narrow).push_back(i);
  }
  if (wide.empty() || narrow.empty()) return w;
  std::vector<WorkItem> mixed;
  const size_t n = w.size();
  size_t iw = 0, in = 0;
  for (size_t k = 0; k < n; ++k) {
    // wide items are due when their share of the first k + 1 slots falls behind
    const bool take_wide = in >= narrow.size() || (iw < wide.size() && iw * n <= k * wide.size());
    mixed.push_back(w[take_wide ? wide[iw++] : narrow[in++]]);
  }
  return mixed;
}

}  // namespace fi

using namespace fi;

extern "C" FI_API int fi_batch_prefill_plan(
    void* float_ws, size_t float_ws_bytes, void* int_ws, void* pinned_int_ws, size_t int_ws_bytes,
    const int32_t* qo_indptr_h, const int32_t* kv_indptr_h, const int32_t* kv_len_arr_h,
    int32_t total_num_rows, int32_t batch_size, int32_t num_qo_heads, int32_t num_kv_heads,
    int32_t page_size, int32_t enable_cuda_graph, int32_t head_dim_qk, int32_t head_dim_vo,
    int32_t causal, int32_t window_left, int32_t fixed_split_size, int32_t disable_split_kv,
    int64_t* plan_info_out, fi_stream_t stream) {
  (void)float_ws; (void)kv_indptr_h;
  FI_REQUIRE(pinned_int_ws && qo_indptr_h && kv_len_arr_h && plan_info_out,
             "batch_prefill_plan: null argument");
  FI_REQUIRE(batch_size >= 0 && page_size > 0, "batch_prefill_plan: bad batch size / page size");
  FI_REQUIRE(num_kv_heads > 0 && num_qo_heads % num_kv_heads == 0,
             "batch_prefill_plan: num_qo_heads (%d) must be a multiple of num_kv_heads (%d)",
             num_qo_heads, num_kv_heads);
  // (192, 128): the ragged / single prefill_qkvo kernel (fi_batch_prefill_qkvo_run)
  const bool qkvo = head_dim_qk == 192 && head_dim_vo == 128;
  FI_REQUIRE(head_dim_qk == head_dim_vo || qkvo,
             "batch_prefill_plan: head_dim_qk %d / head_dim_vo %d unsupported (equal, or 192 / 128)", head_dim_qk,
             head_dim_vo);
  FI_REQUIRE(qkvo || head_dim_qk == 64 || head_dim_qk == 128 || head_dim_qk == 256,
             "batch_prefill_plan: unsupported head_dim %d (64/128/256)", head_dim_qk);
  FI_REQUIRE(qo_indptr_h[0] == 0, "batch_prefill_plan: qo_indptr[0] must be 0");
  const int group = num_qo_heads / num_kv_heads;

  std::vector<int64_t> store;
  BatchShape shape;
  if (measure_batch(qo_indptr_h, kv_len_arr_h, batch_size, group, causal, window_left, store, shape)) return 1;
  // a graph launch is padded to the resident items, or the most items total_num_rows rows can make without a split
  const int64_t graph_bound =
      ceil_div<int64_t>((int64_t)total_num_rows * group, kTileQ) + std::max(batch_size, 1) - 1;
  const int64_t graph_items = enable_cuda_graph ? std::max(resident_items(num_kv_heads), graph_bound) : 0;
  const auto [kv_chunk, split_kv] = choose_kv_chunk(shape, num_qo_heads, num_kv_heads, head_dim_qk, head_dim_vo,
                                                    float_ws_bytes, graph_items, fixed_split_size, disable_split_kv);
  FI_REQUIRE(kv_chunk < (1ll << 31), "batch_prefill_plan: kv chunk too large");
  const std::vector<WorkItem> work = build_work_list(shape, kv_len_arr_h, group, causal, kv_chunk, split_kv);

  const size_t num_work = work.size(), padded = std::max(num_work, (size_t)graph_items);
  // partial-state ranges per qo row (ref merge_indptr, scheduler.cuh:597-600)
  const int64_t nrows_tab = split_kv ? (int64_t)std::max(total_num_rows, qo_indptr_h[batch_size]) : 0;
  OffsetAllocator ia(int_ws_bytes);
  const int64_t req_off = ia.alloc(std::max<size_t>(padded, 1) * sizeof(int32_t));
  const int64_t tile_off = ia.alloc(std::max<size_t>(padded, 1) * sizeof(int32_t));
  const int64_t kvt_off = ia.alloc(std::max<size_t>(padded, 1) * sizeof(int32_t));
  const int64_t mrg_off = ia.alloc((size_t)(nrows_tab + 1) * sizeof(int32_t));
  const int64_t chunk_off = ia.alloc(sizeof(int32_t));
  FI_REQUIRE(ia.ok, "batch_prefill_plan: int workspace too small (%zu bytes)", int_ws_bytes);
  int32_t* req_h = (int32_t*)((char*)pinned_int_ws + req_off);
  int32_t* tile_h = (int32_t*)((char*)pinned_int_ws + tile_off);
  int32_t* kvt_h = (int32_t*)((char*)pinned_int_ws + kvt_off);
  int32_t* mrg_h = (int32_t*)((char*)pinned_int_ws + mrg_off);
  for (size_t i = 0; i < padded; ++i) {
    req_h[i] = i < num_work ? work[i].req : -1;  // -1: padding item, the workgroup exits
    tile_h[i] = i < num_work ? work[i].tile : 0;
    kvt_h[i] = i < num_work ? work[i].kvt : 0;
  }
  *(int32_t*)((char*)pinned_int_ws + chunk_off) = (int32_t)kv_chunk;
  int64_t entries = 0;
  mrg_h[0] = 0;
  if (split_kv) {
    int64_t row = 0;
    for (int b = 0; b < batch_size; ++b) {
      const int64_t nchunks = ceil_div<int64_t>(shape.kv_len[b], kv_chunk);
      for (int64_t r = qo_indptr_h[b]; r < qo_indptr_h[b + 1]; ++r) {
        entries += nchunks;
        mrg_h[++row] = (int32_t)entries;
      }
    }
    FI_REQUIRE(entries < (1ll << 31), "batch_prefill_plan: too many partial states");
    for (; row < nrows_tab; ) mrg_h[++row] = (int32_t)entries;  // padded rows of a graph launch: empty
  }
  int64_t v_off = 0, s_off = 0;
  if (split_kv) {
    // lse region first, sized for the most partial states a launch of `padded` items can write (each
    // (row, chunk) pair belongs to one item of <= kTileQ / G + 1 rows): with a fixed-shape (graph) plan
    // both offsets are then the same for every plan, so a captured run() stays valid after a re-plan.
    // The outputs follow and may use the rest of the workspace.
    OffsetAllocator fa(float_ws_bytes);
    const int64_t rows_per_item = ceil_div<int64_t>(kTileQ, group) + 1;
    const int64_t lse_entries =
        enable_cuda_graph ? std::max<int64_t>(entries, (int64_t)padded * rows_per_item) : std::max<int64_t>(entries, 1);
    s_off = fa.alloc((size_t)lse_entries * num_qo_heads * sizeof(float));
    v_off = fa.alloc((size_t)std::max<int64_t>(entries, 1) * num_qo_heads * head_dim_vo * sizeof(float));
    FI_REQUIRE(fa.ok, "batch_prefill_plan: float workspace too small (%zu bytes, need %zu for %lld partial "
               "states)", float_ws_bytes,
               (size_t)entries * num_qo_heads * (head_dim_vo + 1) * sizeof(float), (long long)entries);
  }
  for (int i = 0; i < FI_PREFILL_PLAN_INFO_LEN; ++i) plan_info_out[i] = 0;
  plan_info_out[FI_PP_PADDED_BATCH_SIZE] = (int64_t)padded;
  plan_info_out[FI_PP_TOTAL_NUM_ROWS] = split_kv ? nrows_tab : total_num_rows;
  plan_info_out[FI_PP_KV_CHUNK_SIZE_PTR_OFFSET] = chunk_off;
  plan_info_out[FI_PP_CTA_TILE_Q] = kTileQ;
  plan_info_out[FI_PP_REQUEST_INDICES_OFFSET] = req_off;
  plan_info_out[FI_PP_QO_TILE_INDICES_OFFSET] = tile_off;
  plan_info_out[FI_PP_KV_TILE_INDICES_OFFSET] = kvt_off;
  plan_info_out[FI_PP_MERGE_INDPTR_OFFSET] = mrg_off;
  plan_info_out[FI_PP_BATCH_SIZE] = batch_size;
  plan_info_out[FI_PP_KV_CHUNK_SIZE] = kv_chunk;
  plan_info_out[FI_PP_V_OFFSET] = v_off;
  plan_info_out[FI_PP_S_OFFSET] = s_off;
  plan_info_out[FI_PP_NUM_WORK] = (int64_t)num_work;
  plan_info_out[FI_PP_ENABLE_CUDA_GRAPH] = enable_cuda_graph ? 1 : 0;
  plan_info_out[FI_PP_SPLIT_KV] = split_kv ? 1 : 0;
  // a (192, 128) plan carries its own tag: its partial states are sized for head_dim_vo 128, and only
  // fi_batch_prefill_qkvo_run runs it
  plan_info_out[FI_PP_MAGIC] = qkvo ? FI_PREFILL_QKVO_PLAN_MAGIC : FI_PREFILL_PLAN_MAGIC;
  if (int_ws && ia.used)
    FI_HIP_CALL(hipMemcpyAsync(int_ws, pinned_int_ws, ia.used, hipMemcpyHostToDevice,
                               (hipStream_t)stream));
  return 0;
}

namespace fi {

// What one prefill launch runs: the kernel instantiated for the dtypes and head_dim, or the fp8-native one.
struct PrefillLaunch {
  prefill_launch_fn fn;
  bool fp8_native, rope;
  int q_dtype, head_dim;
};

// The checks and PrefillKernelParams fields batch and single prefill share (A is fi_batch_prefill_params_t or
// fi_single_prefill_params_t: the fields read here have the same names in both), then the kernel choice.
template <class A>
static int check_and_fill_prefill(const char* who, const A& a, const void* k, const void* v, int kv_dt, int head_dim,
                                  int num_kv_heads, int page_size, int64_t stride_page, int64_t stride_n,
                                  int64_t stride_h, PrefillKernelParams& kp, PrefillLaunch& launch) {
  FI_REQUIRE(num_kv_heads > 0 && a.num_qo_heads % num_kv_heads == 0,
             "%s: num_qo_heads must be a multiple of num_kv_heads", who);
  const int q_dt = a.q_dtype, o_dt = a.o_dtype;
  FI_REQUIRE(o_dt == FI_DTYPE_F16 || o_dt == FI_DTYPE_BF16, "%s: output dtype must be f16/bf16", who);
  if (q_dt == FI_DTYPE_F16 || q_dt == FI_DTYPE_BF16) {
    FI_REQUIRE(o_dt == q_dt, "%s: output dtype must equal the 16-bit q dtype", who);
    FI_REQUIRE(kv_dt == q_dt || kv_dt == FI_DTYPE_FP8_E4M3 || kv_dt == FI_DTYPE_FP8_E5M2,
               "%s: kv dtype must equal q dtype or be fp8", who);
  } else {
    FI_REQUIRE((q_dt == FI_DTYPE_FP8_E4M3 || q_dt == FI_DTYPE_FP8_E5M2) && kv_dt == q_dt,
               "%s: fp8 attention needs q, k and v of one fp8 type (e4m3 or e5m2)", who);
  }
  launch.fn = find_prefill(compute_type(q_dt, o_dt), kv_dt, q_dt, head_dim);
  FI_REQUIRE(launch.fn, "%s: unsupported q/kv dtype %d/%d or head_dim %d", who, q_dt, kv_dt, head_dim);
  FI_REQUIRE(a.pos_encoding_mode != FI_POS_ALIBI || a.alibi_slopes, "%s: ALIBI needs alibi_slopes", who);
  // q, k and v are 1- or 2-byte types here, so 8 elements are 16 bytes (8 for fp8)
  FI_REQUIRE(((uintptr_t)a.q % 16) == 0 && a.q_stride_n % 8 == 0 && a.q_stride_h % 8 == 0,
             "%s: q rows must be aligned to 8 elements", who);
  FI_REQUIRE(stride_n % 8 == 0 && stride_h % 8 == 0 && stride_page % 8 == 0 && ((uintptr_t)k % 16) == 0 &&
                 ((uintptr_t)v % 16) == 0,
             "%s: k/v rows must be aligned to 8 elements", who);
  FI_REQUIRE(stride_page < (1ll << 31) && stride_n < (1ll << 31) && stride_page >= 0 && stride_n >= 0,
             "%s: kv page / token strides must be below 2^31 elements", who);
  memset(&kp, 0, sizeof(kp));
  kp.q = a.q;
  kp.o = a.o;
  kp.lse = a.lse;
  kp.k = k;
  kp.v = v;
  kp.alibi_slopes = a.alibi_slopes;
  kp.scale_q = a.scale_q;
  kp.scale_k = a.scale_k;
  kp.scale_v = a.scale_v;
  kp.q_stride_n = a.q_stride_n;
  kp.q_stride_h = a.q_stride_h;
  kp.kv_stride_page = stride_page;
  kp.kv_stride_n = stride_n;
  kp.kv_stride_h = stride_h;
  kp.num_qo_heads = a.num_qo_heads;
  kp.num_kv_heads = num_kv_heads;
  kp.group_size = a.num_qo_heads / num_kv_heads;
  kp.page_size = page_size;
  kp.page_div = FastDiv((uint32_t)page_size);
  kp.group_div = FastDiv((uint32_t)kp.group_size);
  // multi-item scoring is causal plus the per-item predicate (ref: prefill.cuh:845-856); plan() must have
  // been called with causal = true so that the kv range of a q tile ends at its last row
  kp.causal = a.mask_mode == FI_MASK_CAUSAL || a.mask_mode == FI_MASK_MULTIITEMSCORING;
  if (a.mask_mode == FI_MASK_CUSTOM) kp.custom_mask = a.custom_mask;
  kp.window_left = a.window_left;
  kp.use_alibi = a.pos_encoding_mode == FI_POS_ALIBI;
  kp.o_dtype = o_dt;
  kp.fp8_p_quant = q_dt == FI_DTYPE_FP8_E4M3 || q_dt == FI_DTYPE_FP8_E5M2;
  kp.logits_soft_cap = a.logits_soft_cap > 0.f ? a.logits_soft_cap : 0.f;
  kp.sm_scale = a.sm_scale;
  kp.rope_rcp_scale = a.rope_rcp_scale;
  kp.rope_rcp_theta = a.rope_rcp_theta;
  kp.bf16_pv_mode = a.bf16_pv_mode;
  launch.rope = a.pos_encoding_mode == FI_POS_ROPE_LLAMA;
  launch.fp8_native = use_fp8_native(kp, q_dt, kv_dt, launch.rope);
  launch.q_dtype = q_dt;
  launch.head_dim = head_dim;
  return 0;
}

// Binds a batch plan's workspace offsets to kernel params (KP: PrefillKernelParams or PrefillQkvoParams): work list
// and, for a split plan, kv tiles, merge indptr, partial states and chunk size.
template <class KP>
static int bind_batch_plan(const char* who, const int64_t* plan_info, void* float_ws, size_t float_ws_bytes,
                           void* int_ws, KP& kp) {
  auto iws = [&](int field) { return (const int32_t*)((const char*)int_ws + plan_info[field]); };
  kp.request_indices = iws(FI_PP_REQUEST_INDICES_OFFSET);
  kp.qo_tile_indices = iws(FI_PP_QO_TILE_INDICES_OFFSET);
  if (plan_info[FI_PP_SPLIT_KV]) {
    FI_REQUIRE(float_ws, "%s: a split-kv plan needs the float workspace", who);
    FI_REQUIRE((size_t)plan_info[FI_PP_V_OFFSET] <= float_ws_bytes, "%s: float workspace smaller than at plan()", who);
    kp.kv_tile_indices = iws(FI_PP_KV_TILE_INDICES_OFFSET);
    kp.merge_indptr = iws(FI_PP_MERGE_INDPTR_OFFSET);
    kp.tmp_o = (float*)((char*)float_ws + plan_info[FI_PP_V_OFFSET]);
    kp.tmp_lse = (float*)((char*)float_ws + plan_info[FI_PP_S_OFFSET]);
    kp.kv_chunk_size = (int32_t)plan_info[FI_PP_KV_CHUNK_SIZE];
    kp.kv_chunk_size_ptr = iws(FI_PP_KV_CHUNK_SIZE_PTR_OFFSET);
  }
  return 0;
}

// Splits a single request's kv axis when the q tiles alone (kp.num_work) cannot fill the chip, and the partial
// states ([qo_len, chunks, Hq, head_dim_vo] f32 + lse) fit the caller's scratch buffer: the batch planner's chunk
// choice for a batch of this one request.  Leaves kp unsplit otherwise.
template <class KP>
static void split_single_kv(KP& kp, void* tmp, size_t tmp_bytes, int qo_len, int kv_len, int window_left,
                            int head_dim_qk, int head_dim_vo) {
  const int64_t q_tiles = kp.num_work, rows = qo_len, span = kv_span(kv_len, qo_len, kp.causal, window_left);
  const KvChunk kc = choose_kv_chunk(BatchShape{1, &q_tiles, &span, &rows, q_tiles, span}, kp.num_qo_heads,
                                     kp.num_kv_heads, head_dim_qk, head_dim_vo, tmp_bytes, /*graph_items=*/0,
                                     /*fixed_split_size=*/0, /*disable_split_kv=*/false);
  const int64_t nchunks = ceil_div<int64_t>(span, kc.size);
  if (kc.split_kv && q_tiles * nchunks < (1ll << 30)) {
    kp.num_kv_chunks = (int32_t)nchunks;
    kp.kv_chunk_size = (int32_t)kc.size;
    kp.num_work = (int32_t)(q_tiles * nchunks);
    kp.tmp_o = (float*)tmp;
    size_t vbytes = (size_t)qo_len * nchunks * kp.num_qo_heads * head_dim_vo * sizeof(float);
    vbytes = (vbytes + 15) / 16 * 16;
    kp.tmp_lse = (float*)((char*)tmp + vbytes);
  }
}

// For a split kv axis (kp.tmp_o set), the n-way merge of the partial states of merge_rows query rows: ragged over
// kp.merge_indptr (batch), or kp.num_kv_chunks per row (single).  ref: VariableLengthMergeStates after the
// partition-kv kernel, prefill.cuh:2590-2671; the padding rows of a graph plan have no entries and are left alone.
// `sinks`: the attention sinks of the run (NULL: none), which the kernel left out of the partial states.
template <class KP>
static int merge_split_kv(const KP& kp, int head_dim_vo, int o_dtype, int32_t merge_rows, const float* sinks,
                          hipStream_t stream) {
  if (kp.tmp_o) {
    MergeNParams mp{kp.tmp_o, kp.tmp_lse, kp.merge_indptr, kp.o, kp.lse, kp.num_kv_chunks, merge_rows,
                    kp.num_qo_heads, head_dim_vo, FI_DTYPE_F32, o_dtype, /*skip_empty=*/kp.merge_indptr != nullptr,
                    sinks};
    FI_HIP_CALL(launch_merge_n(mp, stream));
  }
  return 0;
}

// The kernel, then the merge of a split kv axis.
static int launch_prefill(const PrefillKernelParams& kp, const PrefillLaunch& launch, int32_t merge_rows,
                          hipStream_t stream) {
  if (launch.fp8_native)
    FI_HIP_CALL(prefill_fp8_launch(kp, kp.o_dtype, launch.q_dtype == FI_DTYPE_FP8_E5M2, launch.head_dim, stream));
  else
    FI_HIP_CALL(launch.fn(kp, launch.rope, stream));
  return merge_split_kv(kp, launch.head_dim, kp.o_dtype, merge_rows, kp.sinks, stream);
}

}  // namespace fi

extern "C" FI_API int fi_batch_prefill_paged_run(void* float_ws, size_t float_ws_bytes, void* int_ws,
                                                 size_t int_ws_bytes, const int64_t* plan_info,
                                                 int32_t plan_info_len,
                                                 const fi_batch_prefill_params_t* a,
                                                 fi_stream_t stream_) {
  return fi_batch_prefill_paged_run_sinks(float_ws, float_ws_bytes, int_ws, int_ws_bytes, plan_info, plan_info_len, a,
                                          /*sinks=*/nullptr, stream_);
}

extern "C" FI_API int fi_batch_prefill_paged_run_sinks(void* float_ws, size_t float_ws_bytes, void* int_ws,
                                                       size_t int_ws_bytes, const int64_t* plan_info,
                                                       int32_t plan_info_len,
                                                       const fi_batch_prefill_params_t* a, const float* sinks,
                                                       fi_stream_t stream_) {
  (void)int_ws_bytes;
  // attention sinks exist for 16-bit queries only (the fp8-query kernels have no sink term): refused before anything
  // else, so before any launch
  FI_REQUIRE(!sinks || !a || a->q_dtype == FI_DTYPE_F16 || a->q_dtype == FI_DTYPE_BF16,
             "batch_prefill_paged_run: attention sinks need f16 / bf16 queries (q dtype %d)", a->q_dtype);
  FI_REQUIRE(!plan_info || plan_info_len != FI_PREFILL_PLAN_INFO_LEN ||
                 plan_info[FI_PP_MAGIC] != FI_PREFILL_QKVO_PLAN_MAGIC,
             "batch_prefill_paged_run: the plan is for head_dim_qk 192 / head_dim_vo 128, which runs through "
             "fi_batch_prefill_qkvo_run (ragged kv) only");
  FI_REQUIRE(plan_info && plan_info_len == FI_PREFILL_PLAN_INFO_LEN &&
                 plan_info[FI_PP_MAGIC] == FI_PREFILL_PLAN_MAGIC,
             "batch_prefill_paged_run: plan_info is not a prefill plan (call plan() first)");
  FI_REQUIRE(a && int_ws, "batch_prefill_paged_run: null argument");
  const fi_paged_kv_t& kv = a->kv;
  const int64_t num_work = plan_info[FI_PP_PADDED_BATCH_SIZE];
  if (num_work == 0 || kv.batch_size == 0) return 0;
  // kv.indices == NULL && kv.last_page_len == NULL: ragged KV (identity page table, every page full)
  FI_REQUIRE(a->q && a->o && a->qo_indptr && kv.k_data && kv.v_data && kv.indptr,
             "batch_prefill_paged_run: null tensor");
  FI_REQUIRE(kv.last_page_len || !kv.indices, "batch_prefill_paged_run: a page table needs last_page_len");
  FI_REQUIRE(kv.batch_size == plan_info[FI_PP_BATCH_SIZE], "batch_prefill_paged_run: batch size differs from the plan");
  FI_REQUIRE(a->mask_mode >= FI_MASK_NON_CAUSAL && a->mask_mode <= FI_MASK_MULTIITEMSCORING,
             "batch_prefill_paged_run: bad mask_mode %d", a->mask_mode);
  FI_REQUIRE(a->mask_mode != FI_MASK_CUSTOM || (a->custom_mask && a->mask_indptr),
             "batch_prefill_paged_run: mask_mode CUSTOM needs custom_mask and mask_indptr");
  FI_REQUIRE(a->mask_mode != FI_MASK_MULTIITEMSCORING ||
                 (a->prefix_len_ptr && a->token_pos_in_items_ptr && a->token_pos_in_items_len > 0),
             "batch_prefill_paged_run: mask_mode MULTIITEMSCORING needs prefix_len_ptr, token_pos_in_items_ptr and "
             "token_pos_in_items_len");
  FI_REQUIRE(a->mask_mode != FI_MASK_MULTIITEMSCORING ||
                 (a->q_dtype == FI_DTYPE_F16 || a->q_dtype == FI_DTYPE_BF16),
             "batch_prefill_paged_run: multi-item scoring needs 16-bit queries");
  PrefillKernelParams kp;
  PrefillLaunch launch;
  if (check_and_fill_prefill("batch_prefill_paged_run", *a, kv.k_data, kv.v_data, kv.dtype, kv.head_dim,
                             kv.num_kv_heads, kv.page_size, kv.stride_page, kv.stride_n, kv.stride_h, kp, launch))
    return 1;
  kp.qo_indptr = a->qo_indptr;
  kp.kv_indptr = kv.indptr;
  kp.kv_indices = kv.indices;
  kp.kv_last_page_len = kv.last_page_len;
  if (bind_batch_plan("batch_prefill_paged_run", plan_info, float_ws, float_ws_bytes, int_ws, kp)) return 1;
  kp.num_work = (int32_t)num_work;
  kp.sinks = sinks;
  if (a->mask_mode == FI_MASK_CUSTOM) kp.mask_indptr = a->mask_indptr;
  if (a->mask_mode == FI_MASK_MULTIITEMSCORING) {
    kp.prefix_len_ptr = a->prefix_len_ptr;
    kp.token_pos_in_items_ptr = a->token_pos_in_items_ptr;
    kp.token_pos_in_items_len = a->token_pos_in_items_len;
  }
  return launch_prefill(kp, launch, (int32_t)plan_info[FI_PP_TOTAL_NUM_ROWS], (hipStream_t)stream_);
}

extern "C" FI_API int fi_single_prefill_run(const fi_single_prefill_params_t* a, void* tmp,
                                            size_t tmp_bytes, fi_stream_t stream_) {
  FI_REQUIRE(a, "single_prefill_run: null params");
  if (a->qo_len == 0) return 0;
  FI_REQUIRE(a->q && a->k && a->v && a->o, "single_prefill_run: null tensor");
  FI_REQUIRE(a->mask_mode >= FI_MASK_NON_CAUSAL && a->mask_mode <= FI_MASK_CUSTOM,
             "single_prefill_run: bad mask_mode %d", a->mask_mode);
  FI_REQUIRE(a->mask_mode != FI_MASK_CUSTOM || a->custom_mask,
             "single_prefill_run: mask_mode CUSTOM needs custom_mask");
  // the dense k / v are an identity page table of 16-token pages
  const int vpage = 16;
  PrefillKernelParams kp;
  PrefillLaunch launch;
  if (check_and_fill_prefill("single_prefill_run", *a, a->k, a->v, a->kv_dtype, a->head_dim, a->num_kv_heads, vpage,
                             (int64_t)vpage * a->kv_stride_n, a->kv_stride_n, a->kv_stride_h, kp, launch))
    return 1;
  kp.num_work = (int32_t)ceil_div<int64_t>((int64_t)a->qo_len * kp.group_size, kTileQ);
  kp.single_qo_len = a->qo_len;
  kp.single_kv_len = a->kv_len;
  // split the kv axis when the caller lent a scratch buffer and there is no custom mask
  if (tmp && tmp_bytes > 0 && a->mask_mode != FI_MASK_CUSTOM)
    split_single_kv(kp, tmp, tmp_bytes, a->qo_len, a->kv_len, a->window_left, a->head_dim, a->head_dim);
  // partial states are [qo_len, chunks, Hq, D]: the dense n-way merge
  return launch_prefill(kp, launch, a->qo_len, (hipStream_t)stream_);
}

// ---- head_dim_qk 192 / head_dim_vo 128 (prefill_qkvo_kernel.h) ----

namespace fi {

hipError_t prefill_qkvo_launch(const PrefillQkvoParams& p, int dtype, int pmode, hipStream_t stream);

// The checks and PrefillQkvoParams fields batch and single runs share.
static int check_and_fill_qkvo(const char* who, const fi_prefill_qkvo_params_t& a, PrefillQkvoParams& kp) {
  FI_REQUIRE(a.q && a.k && a.v && a.o, "%s: null tensor", who);
  FI_REQUIRE(a.head_dim_qk == kQkvoDimQK && a.head_dim_vo == kQkvoDimVO,
             "%s: head_dim_qk %d / head_dim_vo %d unsupported (192 / 128)", who, a.head_dim_qk, a.head_dim_vo);
  FI_REQUIRE((a.q_dtype == FI_DTYPE_F16 || a.q_dtype == FI_DTYPE_BF16) && a.kv_dtype == a.q_dtype &&
                 a.o_dtype == a.q_dtype,
             "%s: q, k, v and o must share one 16-bit dtype (f16 / bf16; no fp8 at head_dim_qk 192 / head_dim_vo 128)",
             who);
  FI_REQUIRE(a.num_kv_heads > 0 && a.num_qo_heads > 0 && a.num_qo_heads % a.num_kv_heads == 0,
             "%s: num_qo_heads must be a multiple of num_kv_heads", who);
  FI_REQUIRE(a.mask_mode == FI_MASK_NON_CAUSAL || a.mask_mode == FI_MASK_CAUSAL,
             "%s: mask_mode %d unsupported (non-causal / causal; no custom mask or multi-item scoring)", who,
             a.mask_mode);
  FI_REQUIRE(a.pos_encoding_mode == FI_POS_NONE, "%s: pos_encoding_mode must be NONE (no fused RoPE / ALiBi)", who);
  FI_REQUIRE(!(a.logits_soft_cap > 0.f), "%s: logits_soft_cap is not supported", who);
  FI_REQUIRE(((uintptr_t)a.q % 16) == 0 && a.q_stride_n % 8 == 0 && a.q_stride_h % 8 == 0,
             "%s: q rows must be aligned to 8 elements", who);
  FI_REQUIRE(((uintptr_t)a.k % 16) == 0 && ((uintptr_t)a.v % 16) == 0 && a.k_stride_n % 8 == 0 &&
                 a.k_stride_h % 8 == 0 && a.v_stride_n % 8 == 0 && a.v_stride_h % 8 == 0,
             "%s: k / v rows must be aligned to 8 elements", who);
  FI_REQUIRE(a.k_stride_n >= 0 && a.k_stride_n < (1ll << 31) && a.v_stride_n >= 0 && a.v_stride_n < (1ll << 31),
             "%s: k / v token strides must be below 2^31 elements", who);
  memset(&kp, 0, sizeof(kp));
  kp.q = a.q;
  kp.k = a.k;
  kp.v = a.v;
  kp.o = a.o;
  kp.lse = a.lse;
  kp.q_stride_n = a.q_stride_n;
  kp.q_stride_h = a.q_stride_h;
  kp.k_stride_n = a.k_stride_n;
  kp.k_stride_h = a.k_stride_h;
  kp.v_stride_n = a.v_stride_n;
  kp.v_stride_h = a.v_stride_h;
  kp.num_qo_heads = a.num_qo_heads;
  kp.num_kv_heads = a.num_kv_heads;
  kp.group_size = a.num_qo_heads / a.num_kv_heads;
  kp.group_div = FastDiv((uint32_t)kp.group_size);
  kp.causal = a.mask_mode == FI_MASK_CAUSAL;
  kp.window_left = a.window_left;
  kp.sm_scale = a.sm_scale;
  return 0;
}

// the kernel, then for a split kv axis the n-way merge of merge_rows query rows (head_dim_vo wide)
static int launch_qkvo(const PrefillQkvoParams& kp, const fi_prefill_qkvo_params_t& a, int32_t merge_rows,
                       hipStream_t stream) {
  // bf16: P.V on the f16 MFMA by default; bf16_pv_mode 1 = hi + lo bf16 P, 3 = one bf16 rounding of P
  const int pmode = a.bf16_pv_mode == 1 ? 1 : a.bf16_pv_mode == 3 ? 0 : 2;
  FI_HIP_CALL(prefill_qkvo_launch(kp, a.q_dtype, pmode, stream));
  return merge_split_kv(kp, kQkvoDimVO, a.o_dtype, merge_rows, /*sinks=*/nullptr, stream);
}

}  // namespace fi

extern "C" FI_API int fi_batch_prefill_qkvo_run(void* float_ws, size_t float_ws_bytes, void* int_ws,
                                                size_t int_ws_bytes, const int64_t* plan_info, int32_t plan_info_len,
                                                const fi_prefill_qkvo_params_t* a, fi_stream_t stream_) {
  (void)int_ws_bytes;
  FI_REQUIRE(plan_info && plan_info_len == FI_PREFILL_PLAN_INFO_LEN,
             "batch_prefill_qkvo_run: plan_info is not a prefill plan (call plan() first)");
  // the tag also guarantees partial states sized for head_dim_vo 128 (a plan for equal head dims sized them for its
  // own head_dim)
  FI_REQUIRE(plan_info[FI_PP_MAGIC] == FI_PREFILL_QKVO_PLAN_MAGIC,
             "batch_prefill_qkvo_run: the plan was not made for head_dim_qk 192 / head_dim_vo 128");
  FI_REQUIRE(a && int_ws, "batch_prefill_qkvo_run: null argument");
  const int64_t num_work = plan_info[FI_PP_PADDED_BATCH_SIZE];
  FI_REQUIRE(a->batch_size == plan_info[FI_PP_BATCH_SIZE], "batch_prefill_qkvo_run: batch size differs from the plan");
  if (num_work == 0 || a->batch_size == 0) return 0;
  FI_REQUIRE(a->qo_indptr && a->kv_indptr, "batch_prefill_qkvo_run: null indptr");
  PrefillQkvoParams kp;
  if (check_and_fill_qkvo("batch_prefill_qkvo_run", *a, kp)) return 1;
  kp.qo_indptr = a->qo_indptr;
  kp.kv_indptr = a->kv_indptr;
  if (bind_batch_plan("batch_prefill_qkvo_run", plan_info, float_ws, float_ws_bytes, int_ws, kp)) return 1;
  kp.num_work = (int32_t)num_work;
  return launch_qkvo(kp, *a, (int32_t)plan_info[FI_PP_TOTAL_NUM_ROWS], (hipStream_t)stream_);
}

extern "C" FI_API int fi_single_prefill_qkvo_run(const fi_prefill_qkvo_params_t* a, void* tmp, size_t tmp_bytes,
                                                 fi_stream_t stream_) {
  FI_REQUIRE(a, "single_prefill_qkvo_run: null params");
  FI_REQUIRE(a->qo_len >= 0 && a->kv_len >= 0, "single_prefill_qkvo_run: negative length");
  if (a->qo_len == 0) return 0;
  PrefillQkvoParams kp;
  if (check_and_fill_qkvo("single_prefill_qkvo_run", *a, kp)) return 1;
  kp.num_work = (int32_t)ceil_div<int64_t>((int64_t)a->qo_len * kp.group_size, kTileQ);
  kp.single_qo_len = a->qo_len;
  kp.single_kv_len = a->kv_len;
  // split the kv axis when the caller lent a scratch buffer
  if (tmp && tmp_bytes > 0)
    split_single_kv(kp, tmp, tmp_bytes, a->qo_len, a->kv_len, a->window_left, kQkvoDimQK, kQkvoDimVO);
  // partial states are [qo_len, chunks, Hq, 128]: the dense n-way merge
  return launch_qkvo(kp, *a, a->qo_len, (hipStream_t)stream_);
}
