// Normalised graph propagation, one LightGCN layer per launch (He et al., SIGIR 2020):
//
//   y[r]       = dinv[r] * sum_{c in N(r)} dinv[c] * src[c]          (fp32 accumulation)
//   next[r]    = y[r]                 fp32 or bf16, the next launch's gather source
//   acc_out[r] = acc_in[r] + y[r]     the running sum; the last launch divides by K + 1
//                                     and writes the output rows, pad columns zero
//
// A CSR row-gather SpMM: about 0.5 flop per gathered byte and no reuse of a gathered row
// inside a wave, so there is nothing for MFMA to do; the bound is gather latency and
// bandwidth.  A launch boundary is the grid-wide dependency between layers.
//
// Work split: one wave per work-list entry (graph.py builds the list once per graph).
// A row of up to GP_LONG_ROW neighbours is one entry and the wave finishes it; a longer
// row is cut into entries of GP_LONG_ROW consecutive neighbours whose fp32 partial sums go
// to a partial buffer, and a second small launch adds a row's partials in slot order and
// runs the same epilogue.  Long entries come first in the list, so the heavy waves start
// first.  Nothing depends on the grid: an entry is always one wave's work.
//
// Lane mapping: every lane loads 16 bytes of a gathered row, 4 fp32 or 8 bf16 values, so
// a row of D values takes LPR = D / 4 (fp32) or D / 8 (bf16) lanes and a wave gathers
// G = 64 / LPR neighbour rows per step (fp32: 32 / 16 / 8 / 4 for D = 8 / 16 / 32 / 64;
// bf16 keeps 16-byte loads and carries 8 values per lane, so G doubles).  Lane group g
// takes neighbours g, g + G, ... of each 64-index chunk; each lane accumulates its own
// columns with one fma per value, and at the end of the entry the groups are added by a
// butterfly over the group bits (LPR, 2 LPR, ..., 32), a fixed order.
//
// Index loads: a wave loads 64 column ids per chunk with one coalesced load, and each
// lane the dinv of its id; the lane groups get (id, dinv) by ds_bpermute (the LDS
// crossbar, no LDS allocated), never by re-reading.  Ids are loaded two chunks ahead and
// their dinv one chunk ahead, so neither load is waited for when its chunk starts.  Up to
// 8 row loads per lane are issued before the first is used.  Lanes past the end of an
// entry gather its last neighbour again with weight 0, so every address is a valid row.
#include "common.h"

namespace mrec {

constexpr int GP_THREADS = 256;
constexpr int GP_WAVES = GP_THREADS / 64;
constexpr int GP_LONG_ROW = MREC_GRAPH_LONG_ROW;

struct GpArgs {
  int64_t n_work, n_long;
  const int32_t *col;
  const float *dinv;
  const int4 *work;
  const int64_t *work_beg;
  const int32_t *long_row, *long_ptr;
  float *partial;
  const char *src;
  int64_t src_row_bytes;
  void *next;
  int next_bf16;
  const float *acc_in;
  int64_t ld_acc_in;
  float *acc_out;
  int64_t ld_acc_out;
  float divide;
  int zero_pad;
};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The epilogue of row `row` for the N columns [e0, e0 + N) this lane holds: y = dinv[row] t,
// the stored layer, the running sum (or the output).  N = 8, 4 (16-byte accesses) or 1.
template <int D, int N>
__device__ __forceinline__ void gp_finish(const GpArgs &a, int row, int e0, const float (&t)[N]) {
  const float dr = a.dinv[row];
  float y[N], s[N];
  const float *in = a.acc_in + row * a.ld_acc_in + e0;
  if constexpr (N == 1) {
    s[0] = in[0];
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
      const float4 v = reinterpret_cast<const float4 *>(in)[q];
      s[4 * q] = v.x, s[4 * q + 1] = v.y, s[4 * q + 2] = v.z, s[4 * q + 3] = v.w;
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    y[j] = dr * t[j];
    s[j] += y[j];
    if (a.divide != 0.f) s[j] = s[j] / a.divide;
  }
  if (a.next) {
    const int64_t o = static_cast<int64_t>(row) * D + e0;
    if (a.next_bf16) {
      uint16_t *p = static_cast<uint16_t *>(a.next) + o;
      if constexpr (N == 1) {
        p[0] = f32_to_bf16_rne(y[0]);
      } else if constexpr (N == 4) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]));
      } else {
        *reinterpret_cast<uint4 *>(p) = make_uint4(pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]),
                                                   pack_bf16x2(y[4], y[5]), pack_bf16x2(y[6], y[7]));
      }
    } else {
      float *p = static_cast<float *>(a.next) + o;
      if constexpr (N == 1) {
        p[0] = y[0];
      } else {
#pragma unroll
        for (int q = 0; q < N / 4; ++q)
          reinterpret_cast<float4 *>(p)[q] = make_float4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
      }
    }
  }
  float *out = a.acc_out + row * a.ld_acc_out + e0;
  if constexpr (N == 1) {
    out[0] = s[0];
  } else {
#pragma unroll
    for (int q = 0; q < N / 4; ++q)
      reinterpret_cast<float4 *>(out)[q] = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
  }
}

// columns [D, ld_acc_out) of an output row, by the whole wave (ld_acc_out is a multiple of 4)
template <int D>
__device__ __forceinline__ void gp_zero_pad(const GpArgs &a, int row, int lane) {
  if (!a.zero_pad) return;
  float *out = a.acc_out + row * a.ld_acc_out;
  for (int64_t c = D + 4 * lane; c < a.ld_acc_out; c += 256)
    *reinterpret_cast<float4 *>(out + c) = make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int D, bool SRC_BF16>
__global__ __launch_bounds__(GP_THREADS) void graph_prop_kernel(const GpArgs a) {
  using T = std::conditional_t<SRC_BF16, uint16_t, float>;
  constexpr int EPL = Vec<T>::EPL;    // values per lane: 16 bytes of a row
  constexpr int LPR = D / EPL;        // lanes per gathered row
  constexpr int G = 64 / LPR;         // neighbour rows per step
  constexpr int STEPS = 64 / G;       // steps per 64-index chunk
  constexpr int U = STEPS < 8 ? STEPS : 8;  // row loads in flight per lane
  const int lane = threadIdx.x & 63;
  const int64_t item = static_cast<int64_t>(blockIdx.x) * GP_WAVES + (threadIdx.x >> 6);
  if (item >= a.n_work) return;
  const int4 w = a.work[item];
  const int row = uniform(w.x), len = uniform(w.y), slot = uniform(w.z);
  const int grp = lane / LPR, sub = lane % LPR;

  float acc[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) acc[j] = 0.f;

  if (len > 0) {
    const int32_t *colp = a.col + a.work_beg[item];
    const int last = len - 1;
    const char *src = a.src + sub * 16;
    int c_a = colp[min(lane, last)];
    int c_b = colp[min(64 + lane, last)];
    float w_a = a.dinv[c_a];
    for (int base = 0; base < len; base += 64) {
      const int c = c_a;
      const float wc = w_a;
      c_a = c_b;
      c_b = colp[min(base + 128 + lane, last)];
      w_a = a.dinv[c_a];
      const int n = min(64, len - base);
#pragma unroll
      for (int s0 = 0; s0 < STEPS; s0 += U) {
        if (s0 * G >= n) break;
        uint4 v[U];
        float wv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int p = (s0 + u) * G + grp;
          const int ci = __shfl(c, p);
          const float wi = __shfl(wc, p);
          wv[u] = p < n ? wi : 0.f;
          v[u] = *reinterpret_cast<const uint4 *>(src + ci * a.src_row_bytes);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float f[EPL];
          Vec<T>::to_f32(v[u], f);
#pragma unroll
          for (int j = 0; j < EPL; ++j) acc[j] = fmaf(wv[u], f[j], acc[j]);
        }
      }
    }
#pragma unroll
    for (int m = LPR; m < 64; m <<= 1) {
#pragma unroll
      for (int j = 0; j < EPL; ++j) acc[j] += __shfl_xor(acc[j], m);
    }
  }

  if (slot >= 0) {  // a segment of a long row: the unscaled partial sum
    if (grp == 0) {
      float *p = a.partial + static_cast<int64_t>(slot) * D + sub * EPL;
#pragma unroll
      for (int q = 0; q < EPL / 4; ++q)
        reinterpret_cast<float4 *>(p)[q] = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
    }
    return;
  }
  if (grp == 0) gp_finish<D, EPL>(a, row, sub * EPL, acc);
  gp_zero_pad<D>(a, row, lane);
}

// second pass: one wave per long row, lane = column; the row's partials in slot order
template <int D>
__global__ __launch_bounds__(GP_THREADS) void graph_prop_long_kernel(const GpArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * GP_WAVES + (threadIdx.x >> 6);
  if (i >= a.n_long) return;
  const int row = uniform(a.long_row[i]);
  const int s0 = uniform(a.long_ptr[i]), s1 = uniform(a.long_ptr[i + 1]);
  if (lane < D) {
    const float *p = a.partial + lane;
    float t[1] = {0.f};
    int s = s0;
    for (; s + 4 <= s1; s += 4) {
      const float v0 = p[static_cast<int64_t>(s) * D], v1 = p[static_cast<int64_t>(s + 1) * D];
      const float v2 = p[static_cast<int64_t>(s + 2) * D], v3 = p[static_cast<int64_t>(s + 3) * D];
      t[0] = (((t[0] + v0) + v1) + v2) + v3;
    }
    for (; s < s1; ++s) t[0] += p[static_cast<int64_t>(s) * D];
    gp_finish<D, 1>(a, row, lane, t);
  }
  gp_zero_pad<D>(a, row, lane);
}

template <int D>
static void gp_launch(const GpArgs &a, bool src_bf16, hipStream_t st) {
  const unsigned blocks = static_cast<unsigned>((a.n_work + GP_WAVES - 1) / GP_WAVES);
  if (src_bf16)
    graph_prop_kernel<D, true><<<blocks, GP_THREADS, 0, st>>>(a);
  else
    graph_prop_kernel<D, false><<<blocks, GP_THREADS, 0, st>>>(a);
  if (a.n_long > 0) {
    const unsigned lb = static_cast<unsigned>((a.n_long + GP_WAVES - 1) / GP_WAVES);
    graph_prop_long_kernel<D><<<lb, GP_THREADS, 0, st>>>(a);
  }
}

}  // namespace mrec

using namespace mrec;

extern "C" {

int32_t mrec_graph_long_row(void) { return GP_LONG_ROW; }

int32_t mrec_graph_prop_supported(int32_t dim, mrec_dtype src_dtype, mrec_dtype next_dtype) {
  const bool d = dim == 8 || dim == 16 || dim == 32 || dim == 64;
  const bool s = src_dtype == MREC_F32 || src_dtype == MREC_BF16;
  const bool n = next_dtype == MREC_F32 || next_dtype == MREC_BF16;
  return d && s && n;
}

mrec_status mrec_graph_prop(const mrec_graph_prop_args *g, mrec_stream stream) {
  MREC_CHECK_ARG(g, "NULL args");
  MREC_CHECK_ARG(mrec_graph_prop_supported(g->dim, g->src_dtype, g->next_dtype),
                 "unsupported shape: dim must be 8, 16, 32 or 64, the layers fp32 or bf16");
  MREC_CHECK_ARG(g->n_rows >= 0 && g->n_rows < (int64_t{1} << 31), "bad row count");
  if (g->n_rows == 0) return MREC_OK;
  MREC_CHECK_ARG(g->n_work >= 1 && g->n_work < (int64_t{1} << 33) && g->n_long >= 0 &&
                     g->n_long <= g->n_work,
                 "bad work list");
  MREC_CHECK_ARG(g->col && g->dinv && g->work && g->work_beg && g->src && g->acc_in && g->acc_out,
                 "NULL pointer");
  MREC_CHECK_ARG(g->n_long == 0 || (g->long_row && g->long_ptr && g->partial),
                 "long rows without their row list, slot list or partial buffer");
  const int es = g->src_dtype == MREC_BF16 ? 2 : 4;
  MREC_CHECK_ARG(g->ld_src >= g->dim && (g->ld_src * es) % 16 == 0 &&
                     (reinterpret_cast<uintptr_t>(g->src) & 15) == 0,
                 "src rows must be 16-byte aligned and at least dim wide");
  MREC_CHECK_ARG(g->ld_acc_in >= g->dim && g->ld_acc_in % 4 == 0 && g->ld_acc_out >= g->dim &&
                     g->ld_acc_out % 4 == 0 &&
                     ((reinterpret_cast<uintptr_t>(g->acc_in) | reinterpret_cast<uintptr_t>(g->acc_out) |
                       reinterpret_cast<uintptr_t>(g->partial) | reinterpret_cast<uintptr_t>(g->next) |
                       reinterpret_cast<uintptr_t>(g->work)) & 15) == 0,
                 "acc_in / acc_out / next / partial / work must be 16-byte aligned, their rows too");
  MREC_CHECK_ARG(!(g->divide < 0.f), "divide < 0");
  GpArgs a;
  a.n_work = g->n_work, a.n_long = g->n_long;
  a.col = g->col, a.dinv = g->dinv;
  a.work = reinterpret_cast<const int4 *>(g->work), a.work_beg = g->work_beg;
  a.long_row = g->long_row, a.long_ptr = g->long_ptr, a.partial = g->partial;
  a.src = static_cast<const char *>(g->src), a.src_row_bytes = g->ld_src * es;
  a.next = g->next, a.next_bf16 = g->next_dtype == MREC_BF16;
  a.acc_in = g->acc_in, a.ld_acc_in = g->ld_acc_in;
  a.acc_out = g->acc_out, a.ld_acc_out = g->ld_acc_out;
  a.divide = g->divide, a.zero_pad = g->zero_pad && g->ld_acc_out > g->dim;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool sb = g->src_dtype == MREC_BF16;
  switch (g->dim) {
    case 8: gp_launch<8>(a, sb, st); break;
    case 16: gp_launch<16>(a, sb, st); break;
    case 32: gp_launch<32>(a, sb, st); break;
    default: gp_launch<64>(a, sb, st); break;
  }
  return launch_status("mrec_graph_prop");
}

}  // extern "C"
