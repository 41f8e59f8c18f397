// The selection half of full-catalogue retrieval, shared by the scan kernels that feed it
// (topk.hip: a dot product with an item row; ncf_topk.hip: the NeuMF scorer).
//
// A candidate is the 64-bit key
//   [ordered bits of the score (-0.0 folded into +0.0) | 0xffffffff - id]
// whose unsigned order IS the total order (bigger = better), and whose value is unique per
// item: the k largest keys of a set do not depend on the order the set was built in.  Per
// query a scan workgroup keeps an LDS buffer of `cap` keys, a count and a threshold (the
// k-th best key after the last reduction, 0 before there are k).  A score that reaches the
// threshold's score forms the key, and if it beats the threshold the item is looked up in
// the query's exclusion list (binary search) and appended (LDS atomic on the count).  When
// a count passes `lim` = cap - (the keys one tile can add to a query) every buffer is
// sorted (a bitonic network over all queries at once, padded virtually to a power of two),
// cut to k, and the thresholds are raised.  A split ends with the same reduction and
// writes its k keys per query: decoded straight into the output when there is one split,
// else as keys into the workspace [B, splits, k], which phase 2 (one workgroup per query)
// sorts again and decodes.  Every item of the true top k passes every threshold, whatever
// the geometry, so the result is a function of the inputs alone.
#pragma once

#include "common.h"

namespace mrec {

constexpr int TK_THREADS = 256;
constexpr int TK_MAXK = 128;
constexpr int TK_MAX_SPLITS = 64;
constexpr int TK_MERGE_MAX = TK_MAX_SPLITS * TK_MAXK;  // keys phase 2 sorts in LDS

// what the end of a scan and phase 2 need: the partial lists and the output windows
struct TkOut {
  int32_t batch, k, splits;
  unsigned long long *part;  // [batch, splits, k] keys (splits > 1)
  int32_t *out_ids;
  float *out_scores;
  int64_t ld_out;
};

__device__ __forceinline__ uint32_t tk_ord(float s) {
  const uint32_t u = __float_as_uint(s + 0.f);  // -0.0 + 0.0 = +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float tk_unord(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ unsigned long long tk_key(float s, int32_t id) {
  return (static_cast<unsigned long long>(tk_ord(s)) << 32) | (0xffffffffu - static_cast<uint32_t>(id));
}
// key -> (id, score); the empty key 0 and a score of -inf give (-1, -inf)
__device__ __forceinline__ void tk_emit(unsigned long long key, int32_t *id, float *score) {
  const float s = key ? tk_unord(static_cast<uint32_t>(key >> 32)) : -INFINITY;
  *score = s;
  *id = s == -INFINITY ? -1 : static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(key));
}
// the score a candidate must reach to be worth a key (-inf before there are k)
__device__ __forceinline__ float tk_thr_score(unsigned long long th) {
  return th ? tk_unord(static_cast<uint32_t>(th >> 32)) : -INFINITY;
}

// Sort the first cnt[q] keys of each of nq buffers (buf + q * stride) descending, the
// whole workgroup together.  A bitonic network whose comparators all point the same way
// (the first step of a merge mirrors, the rest are half-cleaners): positions >= cnt[q]
// stand for the smallest key and never move, so any count <= P works.  Ends at a barrier.
// THREADS: the workgroup's size.
template <int THREADS = TK_THREADS>
__device__ __forceinline__ void tk_sort(unsigned long long *buf, int nq, int stride, const int *cnt,
                                        int P, int tid) {
  const int half = P >> 1;
  const int hs = __builtin_ctz(half);
  for (int size = 2; size <= P; size <<= 1) {
    for (int st = size >> 1; st > 0; st >>= 1) {
      const bool mirror = st == (size >> 1);
      // four comparators per thread and round, all their reads before any write (the
      // comparators of a step touch disjoint slots): four LDS round trips overlap
      for (int idx0 = tid; idx0 < nq * half; idx0 += 4 * THREADS) {
        unsigned long long *pi[4], *pj[4], x[4], y[4];
        bool on[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = idx0 + u * THREADS;
          const int qi = idx >> hs, p = idx & (half - 1);
          const int t = p & (st - 1), base = (p - t) << 1;
          const int i = base + t;
          const int j = mirror ? base + size - 1 - t : i + st;
          on[u] = idx < nq * half && j < cnt[idx < nq * half ? qi : 0];
          pi[u] = buf + (on[u] ? qi * stride + i : 0);
          pj[u] = buf + (on[u] ? qi * stride + j : 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *pi[u], y[u] = *pj[u];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (on[u] && x[u] < y[u]) *pi[u] = y[u], *pj[u] = x[u];
      }
      __syncthreads();
    }
  }
}

// Offer (s, id) to query r, whose threshold is th (score th_s) and whose exclusion list is
// ex_items[ex_lo, ex_hi).  -> the query's count has passed lim: a reduction is due.
__device__ __forceinline__ int tk_offer(float s, int32_t id, unsigned long long th, float th_s,
                                        const int32_t *ex_items, int64_t ex_lo, int64_t ex_hi,
                                        unsigned long long *buf, int *cnt, int r, int cap, int lim) {
  if (!(s >= th_s)) return 0;  // (false for a NaN)
  const unsigned long long key = tk_key(s, id);
  if (!(key > th)) return 0;
  int64_t lo = ex_lo, hi = ex_hi;  // lower bound of id
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (ex_items[mid] < id)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < ex_hi && ex_items[lo] == id) return 0;
  const int slot = atomicAdd(&cnt[r], 1);
  if (slot < cap) buf[r * cap + slot] = key;  // (always: cnt <= lim before the tile)
  return slot + 1 > lim;
}

// The reduction: every buffer sorted, cut to k, the thresholds raised.  Ends at a barrier.
template <int THREADS = TK_THREADS>
__device__ __forceinline__ void tk_cut(unsigned long long *buf, unsigned long long *thr, int *cnt, int nq,
                                       int cap, int k, int P, int tid) {
  tk_sort<THREADS>(buf, nq, cap, cnt, P, tid);
  if (tid < nq && cnt[tid] >= k) {
    thr[tid] = buf[tid * cap + k - 1];
    cnt[tid] = k;
  }
  __syncthreads();
}

// The end of a split: the k best of each of the workgroup's nq queries (b0 the first),
// as keys for phase 2 or decoded into the output.
template <int THREADS = TK_THREADS>
__device__ __forceinline__ void tk_finish(unsigned long long *buf, const int *cnt, int nq, int cap, int P,
                                          int64_t b0, int split, const TkOut &o, int tid) {
  tk_sort<THREADS>(buf, nq, cap, cnt, P, tid);
  for (int i = tid; i < nq * o.k; i += THREADS) {
    const int qi = i / o.k, j = i - qi * o.k;
    const int64_t b = b0 + qi;
    if (b >= o.batch) continue;
    const unsigned long long key = j < cnt[qi] ? buf[qi * cap + j] : 0ull;
    if (o.splits > 1) {
      o.part[(b * o.splits + split) * o.k + j] = key;
    } else {
      int32_t id;
      float s;
      tk_emit(key, &id, &s);
      o.out_ids[b * o.ld_out + j] = id;
      o.out_scores[b * o.ld_out + j] = s;
    }
  }
}

// Phase 2: the splits' lists of one query, sorted together; the first k decoded.
static __global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(TkOut o, int P) {
  extern __shared__ __attribute__((aligned(16))) char tk_merge_lds[];
  unsigned long long *buf = reinterpret_cast<unsigned long long *>(tk_merge_lds);  // [P]
  __shared__ int n_sh;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int n = o.splits * o.k;
  for (int i = tid; i < n; i += TK_THREADS) buf[i] = o.part[b * n + i];
  if (tid == 0) n_sh = n;
  __syncthreads();
  tk_sort(buf, 1, P, &n_sh, P, tid);
  for (int j = tid; j < o.k; j += TK_THREADS) {
    int32_t id;
    float s;
    tk_emit(buf[j], &id, &s);
    o.out_ids[b * o.ld_out + j] = id;
    o.out_scores[b * o.ld_out + j] = s;
  }
}

// an empty range: every slot is padding
static __global__ __launch_bounds__(TK_THREADS) void topk_fill_kernel(TkOut o) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * TK_THREADS + threadIdx.x;
  if (i >= static_cast<int64_t>(o.batch) * o.k) return;
  const int64_t b = i / o.k, j = i - b * o.k;
  o.out_ids[b * o.ld_out + j] = -1;
  o.out_scores[b * o.ld_out + j] = -INFINITY;
}

inline int tk_pow2_at_least(int v) {
  int p = 2;
  while (p < v) p <<= 1;
  return p;
}

// bytes of the partial lists [batch, splits, k]; splits = 0 sizes for any default
inline size_t tk_workspace_size(int64_t batch, int32_t k, int32_t splits) {
  if (batch <= 0 || k <= 0 || splits < 0 || splits == 1) return 0;
  if (splits == 0 || splits > TK_MAX_SPLITS) splits = TK_MAX_SPLITS;
  return static_cast<size_t>(batch) * splits * k * sizeof(unsigned long long);
}

static inline mrec_status tk_launch_fill(const TkOut &o, hipStream_t s, const char *who) {
  const int64_t total = static_cast<int64_t>(o.batch) * o.k;
  topk_fill_kernel<<<dim3(static_cast<unsigned>((total + TK_THREADS - 1) / TK_THREADS)), TK_THREADS, 0, s>>>(o);
  return launch_status(who);
}

static inline mrec_status tk_launch_merge(const TkOut &o, hipStream_t s, const char *who) {
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(topk_merge_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, TK_MERGE_MAX * 8);
    (void)hipGetLastError();
    return 1;
  }();
  (void)once;
  const int P2 = tk_pow2_at_least(o.splits * o.k);
  topk_merge_kernel<<<dim3(static_cast<unsigned>(o.batch)), TK_THREADS, static_cast<size_t>(P2) * 8, s>>>(o, P2);
  return launch_status(who);
}

}  // namespace mrec
