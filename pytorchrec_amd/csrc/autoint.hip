// AutoInt interacting layer: multi-head self-attention over the fields (mrec.h "AutoInt",
// ABI 40).
//
//   Q = X Wq^T, K = X Wk^T, V = X Wv^T      S_h = scale Q_h K_h^T      P_h = softmax_keys(S_h)
//   Y = relu([P_1 V_1 | .. ] + X Wres^T)
//
// One wave per sample; a workgroup of W waves walks the batch W samples at a time.  m <= 32,
// so the sample's fields are ONE 32-row tile (rows >= m are zero rows) and every product is
// v_mfma_f32_32x32x16_bf16.  Operand map: lane (r = lane & 31, h = lane >> 5) holds
// A[row r][k = 8 h + j] and B[k = 8 h + j][col r]; the accumulator has its column on the lane
// and row (e & 3) + 8 (e >> 2) + 4 h in register e.  Every operand a product reads lies in the
// wave's LDS with the k index contiguous (one 16-byte read per fragment) or comes as such rows
// of the bf16 weight images from memory (32 KB at most: they stay in L2).  An accumulator
// leaves for LDS in the layout its consumer sums over: row-major (2-byte stores, consecutive
// lanes) or transposed (register quads e = 4 g .. 4 g + 3 are 4 consecutive rows: one packed
// 8-byte store).
//
//   forward   the projections run over the image rows [res | q | k | v]; the res tile stays in
//             the accumulators as O's initial value, Q and K go row-major and V transposed to
//             LDS.  Per head S^T = K_h Q_h^T, so a query's keys lie in the lane's 16 registers
//             and those of lane ^ 32: max and sum are in-register plus one exchange.  Keys >= m
//             are excluded (-inf), not merely zero.  P^T's registers are then the A operand of
//             O_h += P_h V_h with no lane movement (the k order of a step is row 16 s + 8 (j >>
//             2) + 4 h + (j & 3); V^T is read in that order).
//   backward  recomputes Q, K, V, S, P; dP^T = V_h dZ_h^T in S^T's layout, dS^T in registers;
//             dQ_h = dS_h K_h from the registers as above, dK_h = dS_h^T Q_h and dV_h = P_h^T
//             dZ_h through 32 x 32 LDS images of dS^T and P^T.  G = [dZ | dQ | dK | dV] is kept
//             row-major in LDS for dX = G [Wres; Wq; Wk; Wv], and goes transposed ([4 A][32]
//             per sample, bf16) to the workspace.
//   dW        a second launch: a workgroup owns a contiguous range of samples, its four waves
//             the 32-row tiles of G^T X (A operand straight from the workspace, X through
//             LDS); the per-workgroup fp32 partials are summed in workgroup order by a third,
//             tiny launch.  No atomics anywhere.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int AI_THREADS = 256;        // 4 waves at most
constexpr int AI_TP = 40;              // row pitch of the 32-column (transposed) images
constexpr int AI_LDS_BUDGET = 152 * 1024;
constexpr int AI_DW_MAX_PARTS = 256;

struct AiArgs {
  MatIn x, dy, yin;
  MatOut y, dx;
  const uint16_t *wf, *wb;  // images [4 A][ld_wf], [d_in][ld_wb]
  int64_t ld_wf, ld_wb;
  uint16_t *gt;             // workspace: G^T [B][4 A][32] bf16
  float *part;              // workspace: dW partials [parts][4 A][d_in]
  float *dw;
  int64_t B, groups;
  int32_t m, d_in, dpad, px, wave_elems, has_res, per, parts;
  float scale;
};

__device__ __forceinline__ int ai_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 ai_zero() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}

__device__ __forceinline__ bf16x8 ai_ld16(const uint16_t *p) {
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(p));
}

// the permuted-k fragment that pairs with accumulator registers 8 s .. 8 s + 7 used as an
// operand: elements [16 s + 4 h, + 4) and [16 s + 8 + 4 h, + 4) of a 32-element row
__device__ __forceinline__ bf16x8 ai_ld_perm(const uint16_t *row, int s, int h) {
  const uint2 lo = *reinterpret_cast<const uint2 *>(row + 16 * s + 4 * h);
  const uint2 hi = *reinterpret_cast<const uint2 *>(row + 16 * s + 8 + 4 * h);
  return __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
}

// accumulator -> dst[row][col] (row-major, this lane's column)
__device__ __forceinline__ void ai_store_rm(const f32x16 &acc, uint16_t *dst, int ld, int col, int h) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[ai_row(e, h) * ld + col] = f32_to_bf16_rne(acc[e]);
}

// accumulator -> dst[col][row] (transposed; dst points at this lane's 32-element row)
__device__ __forceinline__ void ai_store_tr(const f32x16 &acc, uint16_t *dst_row, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<uint2 *>(dst_row + 8 * g + 4 * h) =
        make_uint2(pack_bf16x2(acc[4 * g], acc[4 * g + 1]), pack_bf16x2(acc[4 * g + 2], acc[4 * g + 3]));
}

// the sample's X tile as bf16 [32][px]: rows >= m and columns >= d_in are zeros
__device__ __forceinline__ void ai_stage_x(const AiArgs &p, int64_t b, bool live, int lane, int first, int step,
                                           uint16_t *Xs) {
  const int ch = p.dpad >> 3;
  for (int idx = first; idx < 32 * ch; idx += step) {
    const int i = idx / ch, c0 = 8 * (idx - i * ch);
    bf16x8 v = frag_zero8();
    if (live && i < p.m && c0 < p.d_in) v = mat_load8(p.x, b, i * p.d_in + c0);
    *reinterpret_cast<uint4 *>(Xs + i * p.px + c0) = __builtin_bit_cast(uint4, v);
  }
}

// one 32-column tile of X [res | q | k | v]^T: image rows 32 t .. 32 t + 31
__device__ __forceinline__ f32x16 ai_project(const AiArgs &p, const uint16_t *Xs, int t, int r, int h) {
  f32x16 acc = ai_zero();
  const uint16_t *wrow = p.wf + static_cast<int64_t>(32 * t + r) * p.ld_wf;
  const int ks = p.dpad >> 4;
  for (int s = 0; s < ks; ++s) {
    const int c0 = 16 * s + 8 * h;
    const bf16x8 a = ai_ld16(Xs + r * p.px + c0);
    bf16x8 w = frag_zero8();
    if (c0 < p.d_in) w = ai_ld16(wrow + c0);
    acc = mfma_32x32x16(a, w, acc);
  }
  return acc;
}

// S^T = K_h Q_h^T over the head's columns, then the softmax over the keys (the registers and
// lane ^ 32) into prob[]: keys >= m get probability 0 and take no part in the maximum
template <int HD>
__device__ __forceinline__ void ai_scores(const uint16_t *Qs, const uint16_t *Ks, int PA, int hh, int r, int h,
                                          int m, float scale, float (&prob)[16]) {
  f32x16 S = ai_zero();
#pragma unroll
  for (int s = 0; s < (HD <= 16 ? 1 : 2); ++s) {
    const int c = 16 * s + 8 * h;
    bf16x8 a = frag_zero8(), q = frag_zero8();
    if (c < HD) {
      a = ai_ld16(Ks + r * PA + hh * HD + c);
      q = ai_ld16(Qs + r * PA + hh * HD + c);
    }
    S = mfma_32x32x16(a, q, S);
  }
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    prob[e] = ai_row(e, h) < m ? scale * S[e] : -INFINITY;
    mx = fmaxf(mx, prob[e]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    prob[e] = ai_row(e, h) < m ? expf(prob[e] - mx) : 0.f;
    sum += prob[e];
  }
  sum += __shfl_xor(sum, 32);
#pragma unroll
  for (int e = 0; e < 16; ++e) prob[e] = prob[e] / sum;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int A, int HD>
__global__ __launch_bounds__(AI_THREADS) void autoint_fwd_kernel(AiArgs p) {
  extern __shared__ __attribute__((aligned(16))) char ai_lds[];
  constexpr int NH = A / HD, NT = (A + 31) / 32, PA = A + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t *Xs = reinterpret_cast<uint16_t *>(ai_lds) + static_cast<size_t>(wave) * p.wave_elems;
  uint16_t *Qs = Xs + 32 * p.px;
  uint16_t *Ks = Qs + 32 * PA;
  uint16_t *Vt = Ks + 32 * PA;  // [A][AI_TP]
  const int m = p.m;

  for (int64_t g = blockIdx.x; g < p.groups; g += gridDim.x) {
    const int64_t b = g * W + wave;
    const bool live = b < p.B;
    __syncthreads();
    ai_stage_x(p, b, live, lane, lane, 64, Xs);
    __syncthreads();

    f32x16 O[NT];
#pragma unroll
    for (int t = 0; t < 4 * A / 32; ++t) {
      const f32x16 acc = ai_project(p, Xs, t, r, h);
      const int cg = 32 * t + r, which = cg / A, cc = cg - which * A;
      if (which == 1)
        ai_store_rm(acc, Qs, PA, cc, h);
      else if (which == 2)
        ai_store_rm(acc, Ks, PA, cc, h);
      else if (which == 3)
        ai_store_tr(acc, Vt + cc * AI_TP, h);
      if (t < NT) {
#pragma unroll
        for (int e = 0; e < 16; ++e) O[t][e] = which == 0 ? acc[e] : 0.f;
      }
    }
    __syncthreads();

#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      float prob[16];
      ai_scores<HD>(Qs, Ks, PA, hh, r, h, m, p.scale, prob);
      constexpr int dummy = 0;
      (void)dummy;
      const int t = hh * HD / 32;
      const int cg = 32 * t + r;
      const bool mine = cg < A && cg / HD == hh;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pa = frag_pack8(&prob[8 * s]);
        bf16x8 v = frag_zero8();
        if (mine) v = ai_ld_perm(Vt + cg * AI_TP, s, h);
        O[t] = mfma_32x32x16(pa, v, O[t]);
      }
    }

    if (live) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int cg = 32 * t + r;
        if (cg >= A) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = ai_row(e, h);
          if (i < m) mat_store(p.y, b, i * A + cg, fmaxf(O[t][e], 0.f));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: dx and the transposed G rows
// ---------------------------------------------------------------------------
// dZ = dY (Y > 0) as bf16, row-major into G's first A columns and transposed into dZt
template <int A>
__device__ __forceinline__ void ai_stage_dz(const AiArgs &p, int64_t b, bool live, int lane, uint16_t *G, int PG,
                                            uint16_t *dZt) {
  constexpr int CH = A / 8;
  for (int idx = lane; idx < 32 * CH; idx += 64) {
    const int i = idx / CH, c0 = 8 * (idx - i * CH);
    uint16_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0;
    if (live && i < p.m) {
      const bf16x8 d = mat_load8(p.dy, b, i * A + c0);
      const char *yr = p.yin.p + b * p.yin.ld_bytes;
      if (p.yin.bf16) {
        const uint4 raw = *reinterpret_cast<const uint4 *>(yr + 2 * (i * A + c0));
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t u = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
          v[k] = (u & 0x7fffu) != 0 && !(u & 0x8000u) && (u & 0x7fffu) <= 0x7f80u ? static_cast<uint16_t>(d[k]) : 0;
        }
      } else {
        const float *yf = reinterpret_cast<const float *>(yr) + i * A + c0;
        const float4 y0 = *reinterpret_cast<const float4 *>(yf), y1 = *reinterpret_cast<const float4 *>(yf + 4);
        const float yy[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = yy[k] > 0.f ? static_cast<uint16_t>(d[k]) : 0;
      }
    }
    *reinterpret_cast<uint4 *>(G + i * PG + c0) =
        make_uint4(v[0] | (uint32_t(v[1]) << 16), v[2] | (uint32_t(v[3]) << 16), v[4] | (uint32_t(v[5]) << 16),
                   v[6] | (uint32_t(v[7]) << 16));
#pragma unroll
    for (int k = 0; k < 8; ++k) dZt[(c0 + k) * AI_TP + i] = v[k];
  }
}

template <int A, int HD>
__global__ __launch_bounds__(AI_THREADS) void autoint_bwd_kernel(AiArgs p) {
  extern __shared__ __attribute__((aligned(16))) char ai_lds[];
  constexpr int NH = A / HD, PA = A + 8, PG = 4 * A + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, W = blockDim.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint16_t *Xs = reinterpret_cast<uint16_t *>(ai_lds) + static_cast<size_t>(wave) * p.wave_elems;
  uint16_t *Qs = Xs + 32 * p.px;
  uint16_t *Ks = Qs + 32 * PA;
  uint16_t *Vs = Ks + 32 * PA;
  uint16_t *Qt = Vs + 32 * PA;  // [A][AI_TP]
  uint16_t *Kt = Qt + A * AI_TP;
  uint16_t *dZt = Kt + A * AI_TP;
  uint16_t *Pt = dZt + A * AI_TP;  // P^T [key][query], [32][AI_TP]
  uint16_t *dSt = Pt + 32 * AI_TP;
  uint16_t *G = dSt + 32 * AI_TP;  // [32][PG]: dZ | dQ | dK | dV
  const int m = p.m;

  for (int64_t g = blockIdx.x; g < p.groups; g += gridDim.x) {
    const int64_t b = g * W + wave;
    const bool live = b < p.B;
    uint16_t *gt = p.gt + (live ? b : 0) * (4 * A * 32);
    __syncthreads();
    ai_stage_x(p, b, live, lane, lane, 64, Xs);
    ai_stage_dz<A>(p, b, live, lane, G, PG, dZt);
    __syncthreads();

    // Q, K, V again (the res rows of the image are not needed here)
#pragma unroll
    for (int t = (A >= 32 ? A / 32 : 0); t < 4 * A / 32; ++t) {
      const f32x16 acc = ai_project(p, Xs, t, r, h);
      const int cg = 32 * t + r, which = cg / A, cc = cg - which * A;
      if (which == 1) {
        ai_store_rm(acc, Qs, PA, cc, h);
        ai_store_tr(acc, Qt + cc * AI_TP, h);
      } else if (which == 2) {
        ai_store_rm(acc, Ks, PA, cc, h);
        ai_store_tr(acc, Kt + cc * AI_TP, h);
      } else if (which == 3) {
        ai_store_rm(acc, Vs, PA, cc, h);
      }
    }
    __syncthreads();

#pragma unroll
    for (int hh = 0; hh < NH; ++hh) {
      float prob[16], ds[16];
      ai_scores<HD>(Qs, Ks, PA, hh, r, h, m, p.scale, prob);
      // dP^T = V_h dZ_h^T: rows = keys, this lane's column = the query
      f32x16 dP = ai_zero();
#pragma unroll
      for (int s = 0; s < (HD <= 16 ? 1 : 2); ++s) {
        const int c = 16 * s + 8 * h;
        bf16x8 a = frag_zero8(), z = frag_zero8();
        if (c < HD) {
          a = ai_ld16(Vs + r * PA + hh * HD + c);
          z = ai_ld16(G + r * PG + hh * HD + c);
        }
        dP = mfma_32x32x16(a, z, dP);
      }
      float rs = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) rs += dP[e] * prob[e];
      rs += __shfl_xor(rs, 32);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        ds[e] = p.scale * (prob[e] * (dP[e] - rs));
        const int j = ai_row(e, h);
        Pt[j * AI_TP + r] = f32_to_bf16_rne(prob[e]);
        dSt[j * AI_TP + r] = f32_to_bf16_rne(ds[e]);
      }
      __syncthreads();

      const int t = hh * HD / 32;
      const int cg = 32 * t + r;
      const bool mine = cg < A && cg / HD == hh;
      f32x16 dQ = ai_zero(), dK = ai_zero(), dV = ai_zero();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 dsa = frag_pack8(&ds[8 * s]);
        bf16x8 kt = frag_zero8(), qt = frag_zero8(), zt = frag_zero8();
        if (mine) {
          kt = ai_ld_perm(Kt + cg * AI_TP, s, h);
          qt = ai_ld16(Qt + cg * AI_TP + 16 * s + 8 * h);
          zt = ai_ld16(dZt + cg * AI_TP + 16 * s + 8 * h);
        }
        dQ = mfma_32x32x16(dsa, kt, dQ);
        dK = mfma_32x32x16(ai_ld16(dSt + r * AI_TP + 16 * s + 8 * h), qt, dK);
        dV = mfma_32x32x16(ai_ld16(Pt + r * AI_TP + 16 * s + 8 * h), zt, dV);
      }
      if (mine) {
        ai_store_rm(dQ, G, PG, A + cg, h);
        ai_store_rm(dK, G, PG, 2 * A + cg, h);
        ai_store_rm(dV, G, PG, 3 * A + cg, h);
        if (live) {
          ai_store_tr(dQ, gt + (A + cg) * 32, h);
          ai_store_tr(dK, gt + (2 * A + cg) * 32, h);
          ai_store_tr(dV, gt + (3 * A + cg) * 32, h);
        }
      }
      __syncthreads();
    }

    // dX = G [Wres; Wq; Wk; Wv]: rows = fields, this lane's column = d
    for (int dt = 0; 32 * dt < p.d_in; ++dt) {
      const int d = 32 * dt + r;
      f32x16 acc = ai_zero();
      const uint16_t *wrow = p.wb + static_cast<int64_t>(d < p.d_in ? d : 0) * p.ld_wb;
#pragma unroll
      for (int s = 0; s < 4 * A / 16; ++s) {
        const int c0 = 16 * s + 8 * h;
        bf16x8 w = frag_zero8();
        if (d < p.d_in) w = ai_ld16(wrow + c0);
        acc = mfma_32x32x16(ai_ld16(G + r * PG + c0), w, acc);
      }
      if (live && d < p.d_in) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = ai_row(e, h);
          if (i < m) mat_store(p.dx, b, i * p.d_in + d, acc[e]);
        }
      }
    }
    // dZ^T rows of the workspace
    if (live)
      for (int idx = lane; idx < A * 4; idx += 64) {
        const int c = idx >> 2, q = idx & 3;
        *reinterpret_cast<uint4 *>(gt + c * 32 + 8 * q) = *reinterpret_cast<const uint4 *>(dZt + c * AI_TP + 8 * q);
      }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: per-workgroup partials of G^T X, then their sum in workgroup order
// ---------------------------------------------------------------------------
template <int A>
__global__ __launch_bounds__(AI_THREADS) void autoint_dw_kernel(AiArgs p) {
  constexpr int MT = 4 * A / 32;            // 32-row tiles of G^T
  constexpr int NU = MT >= 4 ? MT / 4 : 1;  // tiles per wave
  __shared__ __attribute__((aligned(16))) uint16_t Xs[32 * 72];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * p.per;
  const int64_t b1 = b0 + p.per < p.B ? b0 + p.per : p.B;
  f32x16 acc[NU][2];
#pragma unroll
  for (int u = 0; u < NU; ++u) acc[u][0] = acc[u][1] = ai_zero();

  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();
    ai_stage_x(p, b, true, lane, tid, AI_THREADS, Xs);
    __syncthreads();
    const uint16_t *gt = p.gt + b * (4 * A * 32);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 xb[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int d = 32 * dt + r;
        xb[dt] = frag_zero8();
        if (d < p.dpad) {
#pragma unroll
          for (int k = 0; k < 8; ++k) xb[dt][k] = static_cast<short>(Xs[(16 * s + 8 * h + k) * p.px + d]);
        }
      }
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int t = wave + 4 * u;
        if (t >= MT) continue;
        const bf16x8 a = ai_ld16(gt + (32 * t + r) * 32 + 16 * s + 8 * h);
        acc[u][0] = mfma_32x32x16(a, xb[0], acc[u][0]);
        if (p.d_in > 32) acc[u][1] = mfma_32x32x16(a, xb[1], acc[u][1]);
      }
    }
  }
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * (4 * A) * p.d_in;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int t = wave + 4 * u;
    if (t >= MT) continue;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int d = 32 * dt + r;
      if (d >= p.d_in) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) part[(32 * t + ai_row(e, h)) * p.d_in + d] = acc[u][dt][e];
    }
  }
}

// dw [q | k | v | res][A][d_in] from the partials' [res | q | k | v] blocks
__global__ __launch_bounds__(AI_THREADS) void autoint_dw_sum_kernel(AiArgs p, int A) {
  const int n = (p.has_res ? 4 : 3) * A * p.d_in;
  const int idx = blockIdx.x * AI_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int blk = idx / (A * p.d_in), rem = idx - blk * (A * p.d_in);
  const int src = ((blk + 1) & 3) * A * p.d_in + rem;
  float s = 0.f;
  for (int q = 0; q < p.parts; ++q) s += p.part[static_cast<int64_t>(q) * (4 * A) * p.d_in + src];
  p.dw[idx] = s;
}

}  // namespace mrec

using namespace mrec;

namespace {

bool ai_shape_ok(int32_t m, int32_t d_in, int32_t heads, int32_t hd, int32_t A) {
  return m >= 2 && m <= 32 && (d_in == 8 || d_in == 16 || d_in == 32 || d_in == 64) &&
         (A == 16 || A == 32 || A == 64) && (hd == 8 || hd == 16 || hd == 32) && heads >= 1 &&
         static_cast<int64_t>(heads) * hd == A;
}

int ai_dpad(int d_in) { return d_in < 16 ? 16 : d_in; }
int64_t ai_fwd_wave_elems(int d_in, int A) { return 32 * (ai_dpad(d_in) + 8) + 2 * 32 * (A + 8) + A * AI_TP; }
int64_t ai_bwd_wave_elems(int d_in, int A) {
  return 32 * (ai_dpad(d_in) + 8) + 3 * 32 * (A + 8) + 3 * A * AI_TP + 2 * 32 * AI_TP + 32 * (4 * A + 8);
}
int64_t ai_parts(int64_t B) {
  const int64_t want = (B + 3) / 4;
  return want < 1 ? 1 : want > AI_DW_MAX_PARTS ? AI_DW_MAX_PARTS : want;
}
int64_t ai_gt_bytes(int64_t B, int A) { return B * 4 * A * 32 * 2; }
int64_t ai_ws_bytes(int64_t B, int d_in, int A) {
  return ai_gt_bytes(B, A) + ai_parts(B) * 4 * A * d_in * 4;
}

mrec_status ai_check(const mrec_autoint_args *a, bool bwd, AiArgs &p) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(is_float_dtype(a->x_dtype) && is_float_dtype(a->y_dtype) &&
                     (!bwd || (is_float_dtype(a->dy_dtype) && is_float_dtype(a->dx_dtype))),
                 "unknown dtype: x, y, dy and dx must each be MREC_F32 or MREC_BF16");
  MREC_CHECK_ARG(static_cast<int64_t>(a->heads) * a->head_dim == a->A, "heads * head_dim must equal A");
  MREC_CHECK_ARG(ai_shape_ok(a->n_fields, a->d_in, a->heads, a->head_dim, a->A),
                 "unsupported shape (mrec_autoint_supported: 2 <= n_fields <= 32, d_in in {8, 16, 32, 64}, A in "
                 "{16, 32, 64}, head_dim in {8, 16, 32} dividing A)");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  const int64_t wx = static_cast<int64_t>(a->n_fields) * a->d_in, wy = static_cast<int64_t>(a->n_fields) * a->A;
  if (a->batch > 0) {
    MREC_CHECK_ARG(rows16_ok(a->x, a->ld_x, wx, a->x_dtype),
                   "x needs 16-byte aligned rows of at least n_fields * d_in elements");
    MREC_CHECK_ARG(rows16_ok(a->y, a->ld_y, wy, a->y_dtype),
                   "y needs 16-byte aligned rows of at least n_fields * A elements");
    MREC_CHECK_ARG(rows16_ok(a->w_fwd, a->ld_w_fwd, a->d_in, MREC_BF16),
                   "w_fwd needs 16-byte aligned rows of at least d_in elements");
    if (bwd) {
      MREC_CHECK_ARG(rows16_ok(a->w_bwd, a->ld_w_bwd, 4 * a->A, MREC_BF16),
                     "w_bwd needs 16-byte aligned rows of at least 4 * A elements");
      MREC_CHECK_ARG(rows16_ok(a->dy, a->ld_dy, wy, a->dy_dtype),
                     "dy needs 16-byte aligned rows of at least n_fields * A elements");
      MREC_CHECK_ARG(rows16_ok(a->dx, a->ld_dx, wx, a->dx_dtype),
                     "dx needs 16-byte aligned rows of at least n_fields * d_in elements");
      MREC_CHECK_ARG(a->dw, "dw is NULL");
      MREC_CHECK_ARG(a->workspace && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0,
                     "workspace is NULL or not 16-byte aligned");
      MREC_CHECK_ARG(a->workspace_bytes >= ai_ws_bytes(a->batch, a->d_in, a->A),
                     "workspace smaller than mrec_autoint_bwd_workspace_size");
    }
  }
  p.x = mat_in(a->x, a->ld_x, a->x_dtype);
  p.dy = mat_in(a->dy, a->ld_dy, a->dy_dtype);
  p.yin = mat_in(a->y, a->ld_y, a->y_dtype);
  p.y = mat_out(a->y, a->ld_y, a->y_dtype);
  p.dx = mat_out(a->dx, a->ld_dx, a->dx_dtype);
  p.wf = static_cast<const uint16_t *>(a->w_fwd);
  p.wb = static_cast<const uint16_t *>(a->w_bwd);
  p.ld_wf = a->ld_w_fwd;
  p.ld_wb = a->ld_w_bwd;
  p.gt = static_cast<uint16_t *>(a->workspace);
  p.part = a->workspace ? reinterpret_cast<float *>(static_cast<char *>(a->workspace) + ai_gt_bytes(a->batch, a->A))
                        : nullptr;
  p.dw = a->dw;
  p.B = a->batch;
  p.m = a->n_fields;
  p.d_in = a->d_in;
  p.dpad = ai_dpad(a->d_in);
  p.px = p.dpad + 8;
  p.has_res = a->has_res != 0;
  p.scale = a->scale;
  return MREC_OK;
}

template <int A, int HD>
void ai_launch(const AiArgs &p, bool bwd, unsigned grid, unsigned threads, size_t lds, hipStream_t s) {
  if (bwd) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(autoint_bwd_kernel<A, HD>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, AI_LDS_BUDGET);
    autoint_bwd_kernel<A, HD><<<grid, threads, lds, s>>>(p);
  } else {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(autoint_fwd_kernel<A, HD>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, AI_LDS_BUDGET);
    autoint_fwd_kernel<A, HD><<<grid, threads, lds, s>>>(p);
  }
}

template <int A>
void ai_launch_hd(const AiArgs &p, int hd, bool bwd, unsigned grid, unsigned threads, size_t lds, hipStream_t s) {
  if (hd == 8) ai_launch<A, 8>(p, bwd, grid, threads, lds, s);
  if constexpr (A >= 16)
    if (hd == 16) ai_launch<A, 16>(p, bwd, grid, threads, lds, s);
  if constexpr (A >= 32)
    if (hd == 32) ai_launch<A, 32>(p, bwd, grid, threads, lds, s);
}

mrec_status ai_run(const mrec_autoint_args *a, bool bwd, mrec_stream stream, const char *what) {
  AiArgs p{};
  const mrec_status st = ai_check(a, bwd, p);
  if (st != MREC_OK) return st;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t we = bwd ? ai_bwd_wave_elems(a->d_in, a->A) : ai_fwd_wave_elems(a->d_in, a->A);
  int W = 4;
  while (W > 1 && W * we * 2 > AI_LDS_BUDGET) --W;
  p.wave_elems = static_cast<int32_t>(we);
  p.groups = (a->batch + W - 1) / W;
  const int64_t cap = 8LL * device_cus();
  const unsigned grid = static_cast<unsigned>(p.groups < cap ? p.groups : cap);
  const size_t lds = static_cast<size_t>(W) * we * 2;
  switch (a->A) {
    case 16: ai_launch_hd<16>(p, a->head_dim, bwd, grid, 64 * W, lds, s); break;
    case 32: ai_launch_hd<32>(p, a->head_dim, bwd, grid, 64 * W, lds, s); break;
    default: ai_launch_hd<64>(p, a->head_dim, bwd, grid, 64 * W, lds, s); break;
  }
  if (bwd) {
    p.parts = static_cast<int32_t>(ai_parts(a->batch));
    p.per = static_cast<int32_t>((a->batch + p.parts - 1) / p.parts);
    p.parts = static_cast<int32_t>((a->batch + p.per - 1) / p.per);
    switch (a->A) {
      case 16: autoint_dw_kernel<16><<<p.parts, AI_THREADS, 0, s>>>(p); break;
      case 32: autoint_dw_kernel<32><<<p.parts, AI_THREADS, 0, s>>>(p); break;
      default: autoint_dw_kernel<64><<<p.parts, AI_THREADS, 0, s>>>(p); break;
    }
    const int n = (p.has_res ? 4 : 3) * a->A * a->d_in;
    autoint_dw_sum_kernel<<<(n + AI_THREADS - 1) / AI_THREADS, AI_THREADS, 0, s>>>(p, a->A);
  }
  return launch_status(what);
}

}  // namespace

extern "C" {

int32_t mrec_autoint_supported(int32_t n_fields, int32_t d_in, int32_t heads, int32_t head_dim, mrec_dtype x_dtype,
                               mrec_dtype y_dtype) {
  const int64_t A = static_cast<int64_t>(heads) * head_dim;
  return A <= 64 && ai_shape_ok(n_fields, d_in, heads, head_dim, static_cast<int32_t>(A)) &&
         is_float_dtype(x_dtype) && is_float_dtype(y_dtype);
}

int32_t mrec_autoint_image_rows(int32_t A) { return 4 * A; }

int64_t mrec_autoint_bwd_workspace_size(int64_t batch, int32_t d_in, int32_t A) {
  if (batch <= 0 || d_in <= 0 || A <= 0) return 0;
  return ai_ws_bytes(batch, d_in, A);
}

mrec_status mrec_autoint_fwd(const mrec_autoint_args *a, mrec_stream stream) {
  return ai_run(a, false, stream, "mrec_autoint_fwd");
}

mrec_status mrec_autoint_bwd(const mrec_autoint_args *a, mrec_stream stream) {
  return ai_run(a, true, stream, "mrec_autoint_bwd");
}

}  // extern "C"
