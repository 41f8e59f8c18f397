// Full-catalogue top-K retrieval: scores of a batch of queries against one table of a
// bank, fused with the selection of the k best per query (mrec.h "Retrieval", ABI 35).
//
//   score[b, i] = sum_d bf16(q[b, d]) bf16(T[i, d]) (+ w[i])       i in [low, high)
//   out[b, :]   = the k best eligible (score, id) by score descending, then id ascending
//
// The [B, items] score matrix never exists.  Phase 1 runs on a grid of query tiles x
// item splits.  A workgroup of four waves carries TK_TQ = 32 queries as the B operand of
// v_mfma_f32_32x32x16_bf16 (column = query) in registers for the whole launch and streams
// its split of the table TK_TI = 128 items at a time: wave w takes items 32 w .. 32 w + 31
// of the tile as the A operand (row = item), each lane loading its own fragment -- 8
// consecutive elements of its item's row -- straight from memory, TK_PF tiles ahead of
// their products (fp32 rows are rounded to bf16 where they are used, not where they are
// fetched: a fetched tile waits for nothing).  The
// C/D map (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) leaves the 16
// scores of ONE query in a lane's registers, so the query's threshold is one register.
//
// Selection (topk_select.h, shared with ncf_topk.hip): per query an LDS buffer of `cap`
// 64-bit keys, a count and a threshold; a lane whose score reaches the threshold's score
// offers the item (exclusion lookup, LDS append), and when a count passes `lim` = cap - TK_TI
// (a tile can add TK_TI keys to a query at the most) every buffer is sorted, cut to k, and
// the thresholds are raised.  The result is a function of the inputs alone.
#include "common.h"
#include "frag.h"
#include "topk_select.h"

namespace mrec {

constexpr int TK_TQ = 32;        // queries per workgroup
constexpr int TK_TI = 128;       // items per streamed tile: 32 per wave
constexpr int TK_PF = 3;         // tiles in flight per wave

struct TopkArgs {
  const char *table;  // the table's row 0 (bank data + row_offset[table] rows)
  int64_t row_bytes;
  int32_t low, high;
  int32_t w_off;  // byte offset of the first-order weight in a row, -1: none
  const void *q;
  int64_t ldq;
  int32_t q_bf16;
  int32_t cap, lim, P;  // buffer capacity, reduction trigger, pow2 >= cap
  const int64_t *ex_off;
  const int32_t *ex_items;
  int64_t ex_rows;
  const void *ex_row;
  int32_t ex_row64;
  int32_t tiles_per_split;
  TkOut o;
};

// D: the embedding size (8 is one zero-padded K-step); T: the bank's element type
template <int D, typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_scan_kernel(TopkArgs p) {
  constexpr int KS = D <= 16 ? 1 : D / 16;
  extern __shared__ __attribute__((aligned(16))) char tk_lds[];
  unsigned long long *buf = reinterpret_cast<unsigned long long *>(tk_lds);  // [TK_TQ][cap]
  unsigned long long *thr = buf + TK_TQ * p.cap;                             // [TK_TQ]
  int *cnt = reinterpret_cast<int *>(thr + TK_TQ);                           // [TK_TQ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t qrow = static_cast<int64_t>(blockIdx.x) * TK_TQ + r;  // this lane's query
  const bool qlive = qrow < p.o.batch;
  const bool klive = 8 * h < D;  // (D = 8: the upper half of the K-step is padding)
  if (tid < TK_TQ) cnt[tid] = 0, thr[tid] = 0;

  // the query tile as B fragments: element j of K-step s is q[qrow][16 s + 8 h + j]
  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = 0.f;
      if (qlive && klive) {
        const int64_t e = qrow * p.ldq + 16 * s + 8 * h + j;
        f[j] = p.q_bf16 ? bf16_to_f32(static_cast<const uint16_t *>(p.q)[e])
                        : static_cast<const float *>(p.q)[e];
      }
    }
    qf[s] = frag_pack8(f);
  }
  // the query's exclusion list [ex_lo, ex_hi)
  int64_t ex_lo = 0, ex_hi = 0;
  if (p.ex_off && qlive) {
    int64_t er = qrow;
    if (p.ex_row)
      er = p.ex_row64 ? static_cast<const int64_t *>(p.ex_row)[qrow]
                      : static_cast<int64_t>(static_cast<const int32_t *>(p.ex_row)[qrow]);
    if (er >= 0 && er < p.ex_rows) ex_lo = p.ex_off[er], ex_hi = p.ex_off[er + 1];
  }

  const int64_t n_items = static_cast<int64_t>(p.high) - p.low;
  const int64_t n_tiles = (n_items + TK_TI - 1) / TK_TI;
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * p.tiles_per_split;
  const int64_t t1 = t0 + p.tiles_per_split < n_tiles ? t0 + p.tiles_per_split : n_tiles;

  // raw 16-byte loads per lane and K-step, per tile (one of a bf16 row, two of an fp32 row);
  // TK_PF tiles are in flight, and frag_from_raw rounds an fp32 tile at use, so that a
  // fetched tile waits for nothing until its products
  constexpr int LPS = sizeof(T) == 2 ? 1 : 2, RV = KS * LPS;
  auto fetch = [&](int64_t tile, uint4 (&raw)[RV]) {
    const int64_t item = p.low + tile * TK_TI + 32 * wave + r;
    const bool live = tile < t1 && item < p.high && klive;
    const char *row = p.table + (live ? item : static_cast<int64_t>(p.low)) * p.row_bytes +
                      8 * h * static_cast<int>(sizeof(T));
#pragma unroll
    for (int i = 0; i < RV; ++i) {
      raw[i] = make_uint4(0, 0, 0, 0);
      // K-step i / LPS starts 16 elements after the one before it
      if (live) raw[i] = *reinterpret_cast<const uint4 *>(row + 16 * static_cast<int>(sizeof(T)) * (i / LPS) + 16 * (i % LPS));
    }
  };

  uint4 st[TK_PF][RV];
#pragma unroll
  for (int u = 0; u < TK_PF; ++u) fetch(t0 + u, st[u]);
  __syncthreads();
  for (int64_t tile = t0; tile < t1; ++tile) {
    bf16x8 af[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) af[s] = frag_from_raw<T>(st[0], s);
#pragma unroll
    for (int u = 0; u + 1 < TK_PF; ++u) {
#pragma unroll
      for (int i = 0; i < RV; ++i) st[u][i] = st[u + 1][i];
    }
    fetch(tile + TK_PF, st[TK_PF - 1]);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = mfma_32x32x16(af[s], qf[s], acc);
    const int64_t item0 = p.low + tile * TK_TI + 32 * wave + 4 * h;  // + (e & 3) + 8 (e >> 2)
    if (p.w_off >= 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t item = item0 + (e & 3) + 8 * (e >> 2);
        if (item < p.high) {
          const char *wp = p.table + item * p.row_bytes + p.w_off;
          acc[e] += sizeof(T) == 2 ? bf16_to_f32(*reinterpret_cast<const uint16_t *>(wp))
                                   : *reinterpret_cast<const float *>(wp);
        }
      }
    }
    const unsigned long long th = thr[r];
    const float th_s = tk_thr_score(th);
    int full = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t item = item0 + (e & 3) + 8 * (e >> 2);
      if (qlive && item < p.high)
        full |= tk_offer(acc[e], static_cast<int32_t>(item), th, th_s, p.ex_items, ex_lo, ex_hi, buf, cnt, r,
                         p.cap, p.lim);
    }
    if (__syncthreads_or(full)) tk_cut(buf, thr, cnt, TK_TQ, p.cap, p.o.k, p.P, tid);
  }
  // the split's k best of every query
  tk_finish(buf, cnt, TK_TQ, p.cap, p.P, static_cast<int64_t>(blockIdx.x) * TK_TQ, blockIdx.y, p.o, tid);
}

}  // namespace mrec

using namespace mrec;

namespace {

bool tk_dim_ok(int32_t D) { return D == 8 || D == 16 || D == 32 || D == 64; }

template <int D, typename T>
void tk_launch_scan(const TopkArgs &p, dim3 grid, size_t lds, hipStream_t s) {
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(topk_scan_kernel<D, T>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
    (void)hipGetLastError();
    return 1;
  }();
  (void)once;
  topk_scan_kernel<D, T><<<grid, TK_THREADS, lds, s>>>(p);
}

template <typename T>
void tk_launch_dim(int D, const TopkArgs &p, dim3 grid, size_t lds, hipStream_t s) {
  switch (D) {
    case 8: tk_launch_scan<8, T>(p, grid, lds, s); break;
    case 16: tk_launch_scan<16, T>(p, grid, lds, s); break;
    case 32: tk_launch_scan<32, T>(p, grid, lds, s); break;
    default: tk_launch_scan<64, T>(p, grid, lds, s); break;
  }
}

}  // namespace

extern "C" {

int32_t mrec_topk_supported(int32_t D, int32_t k, mrec_dtype bank_dtype) {
  return tk_dim_ok(D) && k >= 1 && k <= TK_MAXK && (bank_dtype == MREC_F32 || bank_dtype == MREC_BF16);
}

int32_t mrec_topk_tile_queries(void) { return TK_TQ; }
int32_t mrec_topk_tile_items(void) { return TK_TI; }

int32_t mrec_topk_splits(int64_t batch, int64_t n_items) {
  if (batch <= 0 || n_items <= 0) return 1;
  const int64_t qt = (batch + TK_TQ - 1) / TK_TQ, it = (n_items + TK_TI - 1) / TK_TI;
  // fill the CUs when the batch is small; the table is re-read once per query tile, so
  // no more splits than that takes
  int64_t s = (device_cus() + qt - 1) / qt;
  if (s > it) s = it;
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return static_cast<int32_t>(s < 1 ? 1 : s);
}

size_t mrec_topk_workspace_size(int64_t batch, int32_t k, int32_t splits) {
  return tk_workspace_size(batch, k, splits);
}

mrec_status mrec_topk(const mrec_topk_args *a, mrec_stream stream) {
  MREC_CHECK_ARG(a, "NULL arguments");
  const mrec_table_bank *bank = a->bank;
  MREC_CHECK_ARG(bank && bank->data && bank->row_offset && bank->rows, "NULL bank pointer");
  MREC_CHECK_ARG(bank->dtype == MREC_F32 || bank->dtype == MREC_BF16, "bank dtype must be F32/BF16");
  MREC_CHECK_ARG(mrec_topk_supported(bank->dim, a->k, bank->dtype),
                 "unsupported shape (mrec_topk_supported: dim in {8, 16, 32, 64}, 1 <= k <= 128)");
  MREC_CHECK_ARG(a->table >= 0 && a->table < bank->n_tables && bank->n_tables <= MREC_MAX_TABLES,
                 "table index out of range");
  const int eb = bank->dtype == MREC_F32 ? 4 : 2;
  const int64_t row_bytes = static_cast<int64_t>(bank->row_stride) * eb;
  MREC_CHECK_ARG(bank->row_stride >= bank->dim + (bank->has_w ? 1 : 0) && row_bytes >= 16 &&
                     row_bytes <= 256 && (row_bytes & (row_bytes - 1)) == 0,
                 "row_stride*elem_size must be a power of two in [16, 256] bytes holding [v | w]");
  MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(bank->data) & 15) == 0, "bank->data not 16B aligned");
  const int64_t rows = bank->rows[a->table], off = bank->row_offset[a->table];
  MREC_CHECK_ARG(rows >= 0 && off >= 0 && rows <= INT32_MAX, "the table must have 0 .. 2^31 - 1 rows");
  MREC_CHECK_ARG(a->low >= 0 && a->low <= a->high && a->high <= rows,
                 "need 0 <= low <= high <= the table's rows");
  MREC_CHECK_ARG(!a->use_w || bank->has_w, "use_w needs a bank with a first-order column");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->q_dtype == MREC_F32 || a->q_dtype == MREC_BF16, "q must be F32 or BF16");
  MREC_CHECK_ARG(a->ldq >= bank->dim, "ldq is smaller than the embedding size");
  MREC_CHECK_ARG(a->ld_out >= a->k, "ld_out is smaller than k");
  MREC_CHECK_ARG(a->batch == 0 || (a->q && a->out_ids && a->out_scores), "NULL pointer");
  const bool excl = a->excl_offsets != nullptr;
  MREC_CHECK_ARG(!excl || (a->excl_items && a->excl_n_rows >= 0),
                 "an exclusion needs offsets, items and n_rows >= 0");
  MREC_CHECK_ARG(excl || (!a->excl_items && !a->excl_row), "exclusion items or rows without offsets");
  MREC_CHECK_ARG(!a->excl_row || a->excl_row_dtype == MREC_I32 || a->excl_row_dtype == MREC_I64,
                 "excl_row must be int32 or int64");
  MREC_CHECK_ARG(a->splits >= 0 && a->splits <= TK_MAX_SPLITS, "splits must be in 0 .. 64 (0: the default)");
  const int64_t n_items = a->high - a->low;
  const int32_t splits = a->splits ? a->splits : mrec_topk_splits(a->batch, n_items);
  const size_t need = mrec_topk_workspace_size(a->batch, a->k, splits);
  if (need > 0 && a->batch > 0 && n_items > 0) {
    MREC_CHECK_ARG(a->workspace != nullptr && a->workspace_bytes >= need,
                   "workspace smaller than mrec_topk_workspace_size");
    MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0, "workspace not 8-byte aligned");
  }
  if (a->batch == 0) return MREC_OK;

  TopkArgs p{};
  p.table = static_cast<const char *>(bank->data) + off * row_bytes;
  p.row_bytes = row_bytes;
  p.low = static_cast<int32_t>(a->low);
  p.high = static_cast<int32_t>(a->high);
  p.w_off = a->use_w ? bank->dim * eb : -1;
  p.q = a->q;
  p.ldq = a->ldq;
  p.q_bf16 = a->q_dtype == MREC_BF16;
  p.o.batch = static_cast<int32_t>(a->batch);
  p.o.k = a->k;
  p.lim = 2 * a->k > 64 ? 2 * a->k : 64;
  p.cap = p.lim + TK_TI;
  p.P = tk_pow2_at_least(p.cap);
  p.ex_off = a->excl_offsets;
  p.ex_items = a->excl_items;
  p.ex_rows = a->excl_n_rows;
  p.ex_row = a->excl_row;
  p.ex_row64 = a->excl_row_dtype == MREC_I64;
  p.o.out_ids = a->out_ids;
  p.o.out_scores = a->out_scores;
  p.o.ld_out = a->ld_out;
  p.o.splits = 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_items == 0) return tk_launch_fill(p.o, s, "mrec_topk");
  const int64_t n_tiles = (n_items + TK_TI - 1) / TK_TI;
  p.o.splits = splits;
  p.tiles_per_split = static_cast<int32_t>((n_tiles + splits - 1) / splits);
  p.o.part = static_cast<unsigned long long *>(a->workspace);
  const dim3 grid(static_cast<unsigned>((a->batch + TK_TQ - 1) / TK_TQ), static_cast<unsigned>(splits));
  const size_t lds = static_cast<size_t>(TK_TQ) * p.cap * 8 + TK_TQ * (8 + 4);
  if (bank->dtype == MREC_BF16)
    tk_launch_dim<uint16_t>(bank->dim, p, grid, lds, s);
  else
    tk_launch_dim<float>(bank->dim, p, grid, lds, s);
  mrec_status st = launch_status("mrec_topk");
  if (st != MREC_OK || splits == 1) return st;
  return tk_launch_merge(p.o, s, "mrec_topk");
}

}  // extern "C"
