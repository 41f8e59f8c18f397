// Pooled multi-valued lookup (ABI 30): a field of a sample is a *bag* of bag_len ids
// and the output is the scaled sum of the bag's rows,
//   out[b, f*dim + d] = s_bf * sum_{valid j} row(f, id_bfj)[d],   s = 1 | 1/n | 1/sqrt(n)
// with n the bag's valid count -- the reference's SVD++ history term (SVDPP.py:49-55:
// gather [B, L] rows, mask id > 0, sum over L, divide by sqrt(valid count)).
//
// Row access as in emb_fwd.hip: a worker of LPR = row_bytes / 16 consecutive lanes
// owns one (bag, field), every lane reads 16 bytes of each row.  The bag is walked in
// groups of kPoolUnroll positions: the group's ids are loaded first, then its rows
// (unconditionally, from a clamped row, masked afterwards -- an out-of-range id is
// never dereferenced), so kPoolUnroll independent row loads are in flight per worker
// before the first add.  No LDS, no atomics.
//
// Summation order (fixed, so the result is bitwise reproducible run to run): fp32,
// one accumulator per element starting at -0.0f (the additive identity that keeps a
// lone -0.0f), the valid rows added in ascending bag position j = 0, 1, .. bag_len-1.
// Then ONE multiply by s and ONE rounding into the output dtype; a bag of one valid
// id under SUM is therefore a bit copy of its row, as mrec_emb_gather_fwd's.
//
// Deviation from the reference: an empty bag (n = 0) gives a zero row and s = 0; the
// reference divides 0 by sqrt(0) and returns NaN (SVDPP.py:54-55).
#include "common.h"

namespace mrec {

constexpr int kPoolUnroll = 4;  // row loads in flight per worker

struct PoolArgs {
  int64_t n_bags;
  int32_t bag_len;
  int32_t pool_mode;
  int32_t pad_mode;
  int64_t out_ld;
  float *w_out;
  float *bag_scale;
  int32_t *lookup_ids;
  int32_t *oob;
};

// the scale of a bag with n valid lookups: formed in double and rounded once, so it
// is the correctly rounded 1 / n or 1 / sqrt(n)
__device__ __forceinline__ float pool_scale(int mode, int n) {
  if (n == 0) return 0.f;
  if (mode == MREC_POOL_MEAN) return static_cast<float>(1.0 / static_cast<double>(n));
  if (mode == MREC_POOL_SQRTN) return static_cast<float>(1.0 / sqrt(static_cast<double>(n)));
  return 1.f;
}

template <typename T, typename O, int LPR, bool ADAM>
__global__ __launch_bounds__(256) void pool_kernel(BankArgs bank, IdsArgs ids, PoolArgs pa,
                                                   O *__restrict__ out) {
  constexpr int EPL = Vec<T>::EPL;
  constexpr int WPB = 256 / LPR;
  constexpr int U = kPoolUnroll;
  const int F = bank.n_tables;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * WPB + threadIdx.x / LPR;
  const int l = threadIdx.x % LPR;
  if (g >= pa.n_bags * F) return;  // whole workers
  const int64_t b = g / F;
  const int f = static_cast<int>(g - b * F);
  const int L = pa.bag_len;
  const int D = bank.dim;
  const int e0 = l * EPL;
  const int64_t rows = bank.rows[f];
  const int64_t roff = bank.row_offset[f];
  const int live = live_elems(bank, e0, EPL);
  const T *__restrict__ data = reinterpret_cast<const T *>(bank.data);
  const int64_t id_base = b * ids.stride;
  int32_t *__restrict__ lk =
      pa.lookup_ids ? pa.lookup_ids + (static_cast<int64_t>(f) * pa.n_bags + b) * L : nullptr;

  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = -0.f;
  int n = 0;
  bool any_oob = false;
#pragma unroll 1
  for (int j0 = 0; j0 < L; j0 += U) {
    // the group's ids (positions past the bag: the last position again, masked)
    int64_t id[U];
    if (ids.is64) {
      const int64_t *p = static_cast<const int64_t *>(ids.ptr[f]) + id_base;
#pragma unroll
      for (int u = 0; u < U; ++u) id[u] = p[min(j0 + u, L - 1)];
    } else {
      const int32_t *p = static_cast<const int32_t *>(ids.ptr[f]) + id_base;
#pragma unroll
      for (int u = 0; u < U; ++u) id[u] = p[min(j0 + u, L - 1)];
    }
    bool ok[U];
    uint4 raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool in_bag = j0 + u < L;
      const bool pad = pa.pad_mode == MREC_POOL_PAD_ZERO ? id[u] == 0 : id[u] < 0;
      const bool in_range = id[u] >= 0 && id[u] < rows;  // checked before the load
      ok[u] = in_bag && !pad && in_range;
      any_oob = any_oob || (in_bag && !pad && !in_range);
      const int64_t grow = ok[u] ? roff + id[u] : 0;
      raw[u] = *reinterpret_cast<const uint4 *>(data + grow * static_cast<int64_t>(bank.row_stride) + e0);
    }
    if (lk && l == 0) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (j0 + u < L) lk[j0 + u] = ok[u] ? static_cast<int32_t>(id[u]) : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u]) continue;  // (uniform over the worker)
      if constexpr (ADAM)  // a lazily updated Adam bank: the row as of the last step
        raw[u] = adam_current<T>(bank, roff + id[u], e0, live, raw[u], *bank.adam.d_t);
      float v[EPL];
      Vec<T>::to_f32(raw[u], v);
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] += v[e];
      ++n;
    }
  }
  if (any_oob && l == 0 && pa.oob) *pa.oob = 1;
  const float s = pool_scale(pa.pool_mode, n);
  if (l == 0) pa.bag_scale[b * F + f] = s;
  float r[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) r[e] = n ? s * acc[e] : 0.f;
  if (e0 + EPL <= D) {
    O *dst = out + b * pa.out_ld + static_cast<int64_t>(f) * D + e0;
    if constexpr (sizeof(O) == 4) {
#pragma unroll
      for (int e = 0; e < EPL; e += 4)
        *reinterpret_cast<float4 *>(dst + e) = make_float4(r[e], r[e + 1], r[e + 2], r[e + 3]);
    } else if constexpr (EPL == 8) {
      *reinterpret_cast<uint4 *>(dst) = make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]),
                                                   pack_bf16x2(r[4], r[5]), pack_bf16x2(r[6], r[7]));
    } else {
      *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]));
    }
  } else if (pa.w_out && bank.has_w && e0 == D) {
    pa.w_out[b * F + f] = r[0];
  }
}

template <typename T, typename O>
static void launch_pool(int lpr, const BankArgs &ba, const IdsArgs &ia, const PoolArgs &pa,
                        void *out, hipStream_t s) {
  const int64_t work = pa.n_bags * ba.n_tables;
  const int wpb = 256 / lpr;
  const dim3 grid(static_cast<unsigned>((work + wpb - 1) / wpb));
  O *o = static_cast<O *>(out);
#define MREC_PK(A)                                                              \
  switch (lpr) {                                                                \
    case 1: pool_kernel<T, O, 1, A><<<grid, 256, 0, s>>>(ba, ia, pa, o); break;  \
    case 2: pool_kernel<T, O, 2, A><<<grid, 256, 0, s>>>(ba, ia, pa, o); break;  \
    case 4: pool_kernel<T, O, 4, A><<<grid, 256, 0, s>>>(ba, ia, pa, o); break;  \
    case 8: pool_kernel<T, O, 8, A><<<grid, 256, 0, s>>>(ba, ia, pa, o); break;  \
    default: pool_kernel<T, O, 16, A><<<grid, 256, 0, s>>>(ba, ia, pa, o); break; \
  }
  if (ba.adam.kind) {
    MREC_PK(true)
  } else {
    MREC_PK(false)
  }
#undef MREC_PK
}

}  // namespace mrec

using namespace mrec;

extern "C" mrec_status mrec_emb_pool_fwd(const mrec_table_bank *bank, const mrec_ids *ids,
                                         int64_t n_bags, int32_t bag_len, int32_t pool_mode,
                                         int32_t pad_mode, void *out, mrec_dtype out_dtype,
                                         int64_t out_ld, float *w_out, float *bag_scale,
                                         int32_t *lookup_ids, int32_t *d_oob_flag,
                                         mrec_stream stream) {
  BankArgs ba;
  IdsArgs ia;
  int eb, lpr;
  mrec_status st = make_bank_args(bank, &ba, &eb, &lpr);
  if (st != MREC_OK) return st;
  if ((st = make_ids_args(ids, ba.n_tables, &ia)) != MREC_OK) return st;
  MREC_CHECK_ARG(n_bags >= 0, "n_bags < 0");
  MREC_CHECK_ARG(bag_len >= 1, "bag_len < 1");
  MREC_CHECK_ARG(n_bags < (int64_t(1) << 31) / bag_len / ba.n_tables,
                 "n_bags * bag_len * n_tables must be < 2^31");
  MREC_CHECK_ARG(pool_mode == MREC_POOL_SUM || pool_mode == MREC_POOL_MEAN ||
                     pool_mode == MREC_POOL_SQRTN,
                 "pool_mode must be MREC_POOL_SUM / _MEAN / _SQRTN");
  MREC_CHECK_ARG(pad_mode == MREC_POOL_PAD_ZERO || pad_mode == MREC_POOL_PAD_NEGATIVE,
                 "pad_mode must be MREC_POOL_PAD_ZERO / _PAD_NEGATIVE");
  MREC_CHECK_ARG(ia.chunk == 0, "bags take plain strided ids (chunk must be 0)");
  MREC_CHECK_ARG(ia.stride >= bag_len, "ids stride < bag_len");
  for (int f = 0; f < ba.n_tables; ++f)
    MREC_CHECK_ARG(ba.rows[f] < (int64_t(1) << 31), "rows per table must be < 2^31");
  MREC_CHECK_ARG(out != nullptr, "out is NULL");
  MREC_CHECK_ARG(bag_scale != nullptr, "bag_scale is NULL");
  MREC_CHECK_ARG(out_dtype == MREC_F32 || out_dtype == MREC_BF16, "out dtype must be F32/BF16");
  const int ob = out_dtype == MREC_F32 ? 4 : 2;
  MREC_CHECK_ARG(out_ld >= static_cast<int64_t>(ba.n_tables) * ba.dim, "out_ld < n_tables*dim");
  // a lane stores its 16 bytes of the row in the output dtype: 16 B, or 8 B when an
  // fp32 bank narrows to bf16
  const int sb = (bank->dtype == MREC_F32 && out_dtype == MREC_BF16) ? 8 : 16;
  MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & (sb - 1)) == 0 && (out_ld * ob) % sb == 0 &&
                     (ba.dim * ob) % sb == 0,
                 "out must be 16B aligned with 16B-multiple rows (8B: fp32 bank, bf16 out)");
  MREC_CHECK_ARG(w_out == nullptr || ba.has_w, "w_out requested but bank has no w column");
  if (n_bags == 0) return MREC_OK;
  PoolArgs pa{};
  pa.n_bags = n_bags;
  pa.bag_len = bag_len;
  pa.pool_mode = pool_mode;
  pa.pad_mode = pad_mode;
  pa.out_ld = out_ld;
  pa.w_out = w_out;
  pa.bag_scale = bag_scale;
  pa.lookup_ids = lookup_ids;
  pa.oob = d_oob_flag;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (bank->dtype == MREC_BF16) {
    if (out_dtype == MREC_BF16)
      launch_pool<uint16_t, uint16_t>(lpr, ba, ia, pa, out, s);
    else
      launch_pool<uint16_t, float>(lpr, ba, ia, pa, out, s);
  } else {
    if (out_dtype == MREC_BF16)
      launch_pool<float, uint16_t>(lpr, ba, ia, pa, out, s);
    else
      launch_pool<float, float>(lpr, ba, ia, pa, out, s);
  }
  return launch_status("mrec_emb_pool_fwd");
}
