// Ranking: the pairwise losses (BPR, Top1), the rank of the positive among a row of
// candidate scores, and negative sampling (mrec.h "Ranking", ABI 31).
//
// They replace, on the device, BPRLoss / Top1Loss forward and backward
// (torchrec/loss/BPRLoss.py:15-23, Top1Loss.py:14-22), the argsort + argwhere of
// IMetric.get_pos_rank (IMetric.py:17-26) and the host loop of
// SimpleDataReader.train_neg_sample (SimpleDataReader.py:280-300).
#include <algorithm>

#include "common.h"
#include "frag.h"

namespace mrec {

// ---------------------------------------------------------------------------
// pairwise losses (sigmoid_stable, dsigmoid_stable: frag.h)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float pair_loss(int kind, float pos, float neg) {
  const float x = neg - pos;
  if (kind == MREC_PAIR_BPR) return x > 20.f ? x : log1pf(expf(x));  // torch's softplus
  return sigmoid_stable(x) + sigmoid_stable(neg * neg);
}

// dl/dpos, dl/dneg
__device__ __forceinline__ void pair_grad(int kind, float pos, float neg, float &dpos,
                                          float &dneg) {
  const float x = neg - pos;
  if (kind == MREC_PAIR_BPR) {
    const float s = x > 20.f ? 1.f : sigmoid_stable(x);  // softplus' under torch's threshold
    dpos = -s;
    dneg = s;
  } else {
    const float d = dsigmoid_stable(x);
    dpos = -d;
    dneg = d + 2.f * neg * dsigmoid_stable(neg * neg);
  }
}

// NONE: out[b] = l_b over a grid.  MEAN / SUM: ONE workgroup; thread t sums rows t,
// t + 1024, ... in order, then the wave butterfly, then the 16 wave partials in order
// (bce_fwd_kernel's reduction, head.hip): bitwise reproducible.
constexpr int PL_T = 1024;
__global__ __launch_bounds__(PL_T) void pair_loss_fwd_kernel(const float *__restrict__ x,
                                                             int64_t ld, int64_t B, int kind,
                                                             int reduction,
                                                             float *__restrict__ out) {
  __shared__ float red[PL_T / 64];
  const int64_t step = static_cast<int64_t>(gridDim.x) * PL_T;
  float acc = 0.f;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * PL_T + threadIdx.x; i < B; i += step) {
    const float l = pair_loss(kind, x[i * ld], x[i * ld + 1]);
    if (reduction == MREC_REDUCE_NONE)
      out[i] = l;
    else
      acc += l;
  }
  if (reduction == MREC_REDUCE_NONE) return;  // (uniform)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < PL_T / 64; ++i) s += red[i];
    if (reduction == MREC_REDUCE_MEAN) s = B > 0 ? s / static_cast<float>(B) : 0.f;
    out[0] = s;
  }
}

__global__ __launch_bounds__(256) void pair_loss_bwd_kernel(const float *__restrict__ x, int64_t ld,
                                                            int64_t B, int kind, int reduction,
                                                            const float *__restrict__ g,
                                                            float *__restrict__ dx) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= B) return;
  float up = reduction == MREC_REDUCE_NONE ? g[i] : g[0];
  if (reduction == MREC_REDUCE_MEAN) up /= static_cast<float>(B);
  float dpos, dneg;
  pair_grad(kind, x[i * ld], x[i * ld + 1], dpos, dneg);
  *reinterpret_cast<float2 *>(dx + 2 * i) = make_float2(up * dpos, up * dneg);
}

// ---------------------------------------------------------------------------
// rank of column 0: one wave per row, RK_ROWS rows per workgroup
// ---------------------------------------------------------------------------
constexpr int RK_ROWS = 4;
__global__ __launch_bounds__(64 * RK_ROWS) void rank_pos_kernel(const float *__restrict__ pred,
                                                                int64_t rows, int n, int64_t ld,
                                                                int32_t *__restrict__ rank) {
  const int lane = threadIdx.x & 63;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * RK_ROWS + (threadIdx.x >> 6);
  if (r >= rows) return;  // (wave-uniform)
  const float *row = pred + r * ld;
  const float p0 = row[0];
  int cnt = 0;
  for (int j = 1 + lane; j < n; j += 64) cnt += row[j] > p0 ? 1 : 0;  // false for any NaN
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) rank[r] = p0 != p0 ? n : 1 + cnt;
}

// ---------------------------------------------------------------------------
// negative sampling: one thread per output, a counter hash (mrec.h writes it down)
// ---------------------------------------------------------------------------
constexpr uint64_t NS_G = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t mix64(uint64_t z) {  // the splitmix64 finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// `key0` = mix(mix(seed + G) + step), formed on the host (it is the same for every output)
__global__ __launch_bounds__(256) void neg_sample_kernel(const void *__restrict__ uids, int is64,
                                                         int64_t total, int n_neg,
                                                         const int64_t *__restrict__ offsets,
                                                         const int32_t *__restrict__ items,
                                                         int64_t n_users, int32_t low,
                                                         uint64_t range, uint64_t key0,
                                                         int32_t *__restrict__ out,
                                                         int32_t *__restrict__ unresolved) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t b = i / n_neg;
  const int64_t u = is64 ? static_cast<const int64_t *>(uids)[b]
                         : static_cast<int64_t>(static_cast<const int32_t *>(uids)[b]);
  int64_t lo0 = 0, hi0 = 0;  // the user's items [lo0, hi0): empty for an unknown uid
  if (u >= 0 && u < n_users) {
    lo0 = offsets[u];
    hi0 = offsets[u + 1];
  }
  const uint64_t key = mix64(key0 + static_cast<uint64_t>(i));
  int32_t item = low;
  bool taken = true;
  for (int a = 0; a < MREC_NEG_MAX_ATTEMPTS && taken; ++a) {
    const uint64_t h = mix64(key + static_cast<uint64_t>(a + 1) * NS_G);
    item = static_cast<int32_t>(static_cast<int64_t>(low) +
                                static_cast<int64_t>(((h >> 32) * range) >> 32));
    int64_t lo = lo0, hi = hi0;  // lower bound of `item`
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (items[mid] < item)
        lo = mid + 1;
      else
        hi = mid;
    }
    taken = lo < hi0 && items[lo] == item;
  }
  out[i] = item;
  if (taken) atomicAdd(unresolved, 1);
}

}  // namespace mrec

using namespace mrec;

extern "C" {

static bool pair_args_ok(int32_t kind, int32_t reduction) {
  return (kind == MREC_PAIR_BPR || kind == MREC_PAIR_TOP1) &&
         (reduction == MREC_REDUCE_NONE || reduction == MREC_REDUCE_MEAN ||
          reduction == MREC_REDUCE_SUM);
}

mrec_status mrec_pair_loss_fwd(const float *x, int64_t ld, int64_t batch, int32_t kind,
                               int32_t reduction, float *out, mrec_stream stream) {
  MREC_CHECK_ARG(x && out, "NULL pointer");
  MREC_CHECK_ARG(batch >= 0 && batch <= (int64_t{1} << 40) && ld >= 2, "bad shape (batch < 0 or ld < 2)");
  MREC_CHECK_ARG(pair_args_ok(kind, reduction), "unknown kind or reduction");
  if (reduction == MREC_REDUCE_NONE && batch == 0) return MREC_OK;
  const unsigned blocks =
      reduction == MREC_REDUCE_NONE
          ? static_cast<unsigned>(std::min<int64_t>((batch + PL_T - 1) / PL_T, 4096))
          : 1u;
  pair_loss_fwd_kernel<<<blocks, PL_T, 0, static_cast<hipStream_t>(stream)>>>(x, ld, batch, kind,
                                                                             reduction, out);
  return launch_status("mrec_pair_loss_fwd");
}

mrec_status mrec_pair_loss_bwd(const float *x, int64_t ld, int64_t batch, int32_t kind,
                               int32_t reduction, const float *g, float *dx, mrec_stream stream) {
  MREC_CHECK_ARG(x && g && dx, "NULL pointer");
  MREC_CHECK_ARG(batch >= 0 && batch <= (int64_t{1} << 38) && ld >= 2, "bad shape (batch < 0 or ld < 2)");
  MREC_CHECK_ARG(pair_args_ok(kind, reduction), "unknown kind or reduction");
  MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(dx) & 7) == 0, "dx must be 8-byte aligned");
  if (batch == 0) return MREC_OK;
  pair_loss_bwd_kernel<<<dim3(static_cast<unsigned>((batch + 255) / 256)), 256, 0,
                         static_cast<hipStream_t>(stream)>>>(x, ld, batch, kind, reduction, g, dx);
  return launch_status("mrec_pair_loss_bwd");
}

mrec_status mrec_rank_pos(const float *pred, int64_t rows, int32_t n, int64_t ld, int32_t *rank,
                          mrec_stream stream) {
  MREC_CHECK_ARG(pred && rank, "NULL pointer");
  MREC_CHECK_ARG(rows >= 0 && rows <= (int64_t{1} << 32), "bad row count");
  MREC_CHECK_ARG(n >= 1, "n < 1");
  MREC_CHECK_ARG(ld >= n, "ld < n");
  if (rows == 0) return MREC_OK;
  rank_pos_kernel<<<dim3(static_cast<unsigned>((rows + RK_ROWS - 1) / RK_ROWS)), 64 * RK_ROWS, 0,
                    static_cast<hipStream_t>(stream)>>>(pred, rows, n, ld, rank);
  return launch_status("mrec_rank_pos");
}

mrec_status mrec_neg_sample(const void *uids, mrec_dtype uid_dtype, int64_t batch, int32_t n_neg,
                            const int64_t *offsets, const int32_t *items, int64_t n_users,
                            int32_t low, int32_t high, uint64_t seed, uint64_t step, int32_t *out,
                            int32_t *d_unresolved, mrec_stream stream) {
  MREC_CHECK_ARG(uids && offsets && items && out && d_unresolved, "NULL pointer");
  MREC_CHECK_ARG(uid_dtype == MREC_I32 || uid_dtype == MREC_I64, "uids must be int32 or int64");
  MREC_CHECK_ARG(batch >= 0 && n_users >= 0, "negative count");
  MREC_CHECK_ARG(n_neg >= 1, "n_neg < 1");
  MREC_CHECK_ARG(high > low, "high <= low");
  MREC_CHECK_ARG(batch <= (int64_t{1} << 38) / n_neg, "batch * n_neg too large");
  const int64_t total = batch * n_neg;
  if (total == 0) return MREC_OK;
  const uint64_t key0 = mix64(mix64(seed + NS_G) + step);
  const uint64_t range = static_cast<uint64_t>(static_cast<int64_t>(high) - low);
  neg_sample_kernel<<<dim3(static_cast<unsigned>((total + 255) / 256)), 256, 0,
                      static_cast<hipStream_t>(stream)>>>(uids, uid_dtype == MREC_I64, total, n_neg,
                                                          offsets, items, n_users, low, range, key0,
                                                          out, d_unresolved);
  return launch_status("mrec_neg_sample");
}

}  // extern "C"
