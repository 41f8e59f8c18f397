// Shared-negative list-wise losses: every query of a batch ranked against its own positive
// and one pool of S negatives shared by the batch (mrec.h "Shared negatives", ABI 37).
//
//   s[b, j] = sum_d bf16(q[b, d]) bf16(neg[j, d]) (+ neg_bias[j])      j in [0, S)
//   s+[b]   = sum_d bf16(q[b, d]) bf16(pos[b, d]) (+ pos_bias[b])
//   L_b     = softmax / bpr / top1 over the candidates j with neg_id[j] != pos_id[b]
//
// The [B, S] score matrix never exists, neither way.  Every pass tiles it 32 x 32 with
// v_mfma_f32_32x32x16_bf16: a workgroup of four waves HOLDS 32 rows of one side as the B
// operand (column = held row, so a lane's 16 accumulator registers are 16 streamed rows
// against ONE held row) and STREAMS the other side 128 rows at a time, wave w taking rows
// 32 w .. 32 w + 31 of the step as the A operand, each lane loading its own fragment -- 8
// consecutive elements of its row -- straight from memory.
//
//   forward           holds queries, streams the pool: per lane an online log-sum-exp
//                     (running maximum) or a running sum, combined per query in a fixed
//                     order; saves 4 floats per query (s+, the maximum, the sum, n_b).
//   backward, query-major      holds queries, streams the pool:      dq, dpos
//   backward, candidate-major  holds candidates, streams the queries: dneg
//
// The two backward passes are ONE kernel with the roles swapped.  A step recomputes its
// score tile, turns it into the coefficients a[b, j] in registers, splits each into two bf16
// values hi + lo (2^-16 relative) and uses them -- still in registers, the accumulator-as-
// operand layout -- as the A operands of the second product, out[held, :] += a^T x streamed rows, whose B operand is the streamed
// tile transposed through a wave-private LDS image.  A streamed row that no held row of
// the tile uses (coefficient zero for all 32) enters that image as zeros, so a candidate
// masked for every query contributes exactly nothing whatever its row holds.
//
// Determinism: a wave's partial product is one MFMA chain over SH_CHUNK = 1024 streamed
// rows; the four waves' partials are summed in wave order per chunk, and the chunks in
// chunk order.  Splitting the candidate-major pass over the batch only moves whole chunks
// to other workgroups (their partials go through the workspace and are summed in the same
// order), so the bits do not depend on the split count, the grid or the run.  No atomics.
#include <algorithm>

#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int SH_T = 32;            // held rows per workgroup
constexpr int SH_W = 4;             // waves per workgroup
constexpr int SH_TS = 32 * SH_W;    // streamed rows per step
constexpr int SH_CHUNK = 1024;      // streamed rows per canonical partial sum
constexpr int SH_THREADS = 64 * SH_W;
constexpr int SH_MAX_SPLITS = 64;
constexpr int SH_TLD = 36;          // row pitch of the transposed image (bf16 elements, 8-B rows)
constexpr int SH_RT = 1024;         // threads of the loss reduction

struct ShArgs {
  MatIn q, pos, neg;
  int64_t B, S;
  const void *pos_id, *neg_id;
  int32_t id64;
  const float *pos_bias, *neg_bias;
  int32_t kind, reduction;
  float *stats;   // [B][4]: s+, maximum, sum (softmax), n_b
  float *loss_b;  // [B]
  const float *g;
  MatOut dq, dpos, dneg;
  float *ws;  // candidate-major partials [chunks][S][D], splits > 1 only
  int32_t splits, chunks_per_split;
};

__device__ __forceinline__ long long sh_id(const void *ids, int id64, int64_t i) {
  return id64 ? static_cast<long long>(static_cast<const int64_t *>(ids)[i])
              : static_cast<long long>(static_cast<const int32_t *>(ids)[i]);
}

// the upstream gradient of query b
__device__ __forceinline__ float sh_upstream(const ShArgs &p, int64_t b) {
  if (p.reduction == MREC_REDUCE_NONE) return p.g[b];
  const float g = p.g[0];
  return p.reduction == MREC_REDUCE_MEAN ? g / static_cast<float>(p.B) : g;
}

// c_b: the factor every coefficient of query b carries.  softmax: g_b / sum; bpr, top1:
// g_b / n_b (0 when n_b = 0)
__device__ __forceinline__ float sh_scale(int kind, float g, float sum, float n) {
  if (kind == MREC_SHNEG_SOFTMAX) return g / sum;
  return n > 0.f ? g / n : 0.f;
}

// a[b, j] = c_b dL_b/ds[b, j] (before c_b: per unit of g_b / sum or g_b / n_b), and `pp`,
// the part of it that is -dL_b/ds+[b] (bpr, top1)
__device__ __forceinline__ float sh_coef(int kind, float s, float sp, float mx, float c, float &pp) {
  if (kind == MREC_SHNEG_SOFTMAX) {
    pp = 0.f;
    return expf(s - mx) * c;
  }
  const float x = s - sp;
  if (kind == MREC_SHNEG_BPR) {
    pp = (x > 20.f ? 1.f : sigmoid_stable(x)) * c;  // softplus' under torch's threshold
    return pp;
  }
  const float d = dsigmoid_stable(x);
  pp = d * c;
  return (d + 2.f * s * dsigmoid_stable(s * s)) * c;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SH_THREADS) void shneg_fwd_kernel(ShArgs p) {
  constexpr int KS = D <= 16 ? 1 : D / 16;
  __shared__ float spart[SH_T][8];
  __shared__ float row_bias[SH_W][32];
  __shared__ long long row_id[SH_W][32];
  __shared__ float part_m[SH_W * 2][SH_T], part_l[SH_W * 2][SH_T];
  __shared__ int part_n[SH_W * 2][SH_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * SH_T;
  const int64_t qrow = q0 + r;
  const bool qlive = qrow < p.B;
  const bool klive = 8 * h < D;
  const bool has_id = p.pos_id != nullptr;

  // s+ of the tile's queries: 8 threads per query, D / 8 elements each, summed in order
  {
    const int qi = tid >> 3, part = tid & 7;
    float s = 0.f;
    if (q0 + qi < p.B) {
#pragma unroll
      for (int k = 0; k < D / 8; ++k) {
        const int d = part * (D / 8) + k;
        s = fmaf(mat_elem_bf16(p.q, q0 + qi, d), mat_elem_bf16(p.pos, q0 + qi, d), s);
      }
    }
    spart[qi][part] = s;
  }
  bf16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = qlive && klive ? mat_load8(p.q, qrow, 16 * s + 8 * h) : frag_zero8();
  const long long qid = has_id && qlive ? sh_id(p.pos_id, p.id64, qrow) : 0;
  __syncthreads();
  float sp = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) sp += spart[r][k];
  if (p.pos_bias && qlive) sp += p.pos_bias[qrow];

  float m = -INFINITY, l = 0.f;
  int n = 0;
  const int64_t n_steps = (p.S + SH_TS - 1) / SH_TS;
  for (int64_t step = 0; step < n_steps; ++step) {
    const int64_t row0 = step * SH_TS + 32 * wave;
    const bool rlive = row0 + r < p.S;
    if (h == 0) {
      row_bias[wave][r] = rlive && p.neg_bias ? p.neg_bias[row0 + r] : 0.f;
      row_id[wave][r] = rlive && has_id ? sh_id(p.neg_id, p.id64, row0 + r) : 0;
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const bf16x8 af = rlive && klive ? mat_load8(p.neg, row0 + r, 16 * s + 8 * h) : frag_zero8();
      acc = mfma_32x32x16(af, qf[s], acc);
    }
    __syncthreads();
    float sc[16];
    bool ok[16];
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;
      sc[e] = acc[e] + row_bias[wave][rr];
      ok[e] = qlive && row0 + rr < p.S && !(has_id && row_id[wave][rr] == qid);
      if (ok[e]) {
        ++n;
        tmax = fmaxf(tmax, sc[e]);
      }
    }
    if (p.kind == MREC_SHNEG_SOFTMAX) {
      if (tmax > m) {  // (m = -inf: l is 0 and exp(-inf) is 0)
        l *= expf(m - tmax);
        m = tmax;
      }
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (ok[e] && sc[e] != -INFINITY) l += expf(sc[e] - m);
    } else if (p.kind == MREC_SHNEG_BPR) {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (ok[e]) {
          const float x = sc[e] - sp;
          l += x > 20.f ? x : log1pf(expf(x));  // torch's softplus
        }
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (ok[e]) l += sigmoid_stable(sc[e] - sp) + sigmoid_stable(sc[e] * sc[e]);
    }
    __syncthreads();
  }
  part_m[2 * wave + h][r] = m;
  part_l[2 * wave + h][r] = l;
  part_n[2 * wave + h][r] = n;
  __syncthreads();
  if (tid < SH_T && q0 + tid < p.B) {
    // (thread tid holds query tid's s+ only when tid == r of its own lane: lanes 0 .. 31 of wave 0)
    int nb = 0;
#pragma unroll
    for (int k = 0; k < 2 * SH_W; ++k) nb += part_n[k][tid];
    float mx = sp, sum = 0.f, loss;
    if (p.kind == MREC_SHNEG_SOFTMAX) {
#pragma unroll
      for (int k = 0; k < 2 * SH_W; ++k) mx = fmaxf(mx, part_m[k][tid]);
      sum = expf(sp - mx);
#pragma unroll
      for (int k = 0; k < 2 * SH_W; ++k)
        if (part_m[k][tid] != -INFINITY) sum += part_l[k][tid] * expf(part_m[k][tid] - mx);
      loss = logf(sum) + (mx - sp);
    } else {
#pragma unroll
      for (int k = 0; k < 2 * SH_W; ++k) sum += part_l[k][tid];
      loss = nb > 0 ? sum / static_cast<float>(nb) : 0.f;
    }
    float *st = p.stats + 4 * (q0 + tid);
    st[0] = sp;
    st[1] = mx;
    st[2] = sum;
    st[3] = static_cast<float>(nb);
    p.loss_b[q0 + tid] = loss;
  }
}

// mean / sum of the per-query losses: ONE workgroup; thread t sums rows t, t + 1024, .. in
// order, then the wave butterfly, then the 16 wave partials in order (pair_loss_fwd_kernel's
// reduction): bitwise reproducible
__global__ __launch_bounds__(SH_RT) void shneg_reduce_kernel(const float *__restrict__ loss_b, int64_t B,
                                                             int reduction, float *__restrict__ out) {
  __shared__ float red[SH_RT / 64];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < B; i += SH_RT) acc += loss_b[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < SH_RT / 64; ++i) s += red[i];
    if (reduction == MREC_REDUCE_MEAN) s = B > 0 ? s / static_cast<float>(B) : 0.f;
    out[0] = s;
  }
}

// ---------------------------------------------------------------------------
// backward: QM (query-major) holds queries and streams the pool -> dq, dpos;
//           !QM (candidate-major) holds candidates and streams the queries -> dneg
// ---------------------------------------------------------------------------
template <int D, bool QM>
__global__ __launch_bounds__(SH_THREADS) void shneg_bwd_kernel(ShArgs p) {
  constexpr int KS = D <= 16 ? 1 : D / 16;
  constexpr int NCB = D == 64 ? 2 : 1;            // 32-column blocks of the output
  constexpr int EPT = SH_T * D / SH_THREADS;      // output elements per thread
  __shared__ __attribute__((aligned(16))) uint16_t timg[SH_W][D][SH_TLD];
  __shared__ float red[SH_W][SH_T * D];
  __shared__ float4 row_par[SH_W][32];            // streamed row: QM (bias, live, -, -); else (s+, max, c, -)
  __shared__ long long row_id[SH_W][32];
  __shared__ float4 held_par[SH_T];               // QM: (s+, max, c, g) of the held queries
  __shared__ float psum_s[SH_W * 2][SH_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const MatIn &held = QM ? p.q : p.neg;
  const MatIn &strm = QM ? p.neg : p.q;
  const int64_t NH = QM ? p.B : p.S, NS = QM ? p.S : p.B;
  const int64_t h0 = static_cast<int64_t>(blockIdx.x) * SH_T;
  const int64_t hrow = h0 + r;
  const bool hlive = hrow < NH;
  const bool klive = 8 * h < D;
  const bool has_id = p.pos_id != nullptr;

  bf16x8 hf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) hf[s] = hlive && klive ? mat_load8(held, hrow, 16 * s + 8 * h) : frag_zero8();
  long long hid = 0;
  float h_sp = 0.f, h_mx = 0.f, h_c = 0.f, h_bias = 0.f;
  if (hlive) {
    if (has_id) hid = sh_id(QM ? p.pos_id : p.neg_id, p.id64, hrow);
    if (QM) {
      const float *st = p.stats + 4 * hrow;
      const float g = sh_upstream(p, hrow);
      h_sp = st[0];
      h_mx = st[1];
      h_c = sh_scale(p.kind, g, st[2], st[3]);
      if (wave == 0 && h == 0) held_par[r] = make_float4(h_sp, h_mx, h_c, g);
    } else if (p.neg_bias) {
      h_bias = p.neg_bias[hrow];
    }
  }

  const int64_t n_chunks = (NS + SH_CHUNK - 1) / SH_CHUNK;
  const int64_t c0 = static_cast<int64_t>(blockIdx.y) * p.chunks_per_split;
  const int64_t c1 = c0 + p.chunks_per_split < n_chunks ? c0 + p.chunks_per_split : n_chunks;
  float tot[EPT];
#pragma unroll
  for (int i = 0; i < EPT; ++i) tot[i] = 0.f;
  float psum = 0.f;

  for (int64_t chunk = c0; chunk < c1; ++chunk) {
    f32x16 Z[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int e = 0; e < 16; ++e) Z[cb][e] = 0.f;
    for (int step = 0; step < SH_CHUNK / SH_TS; ++step) {
      const int64_t base = chunk * SH_CHUNK + static_cast<int64_t>(step) * SH_TS;
      if (base >= NS) break;  // (uniform over the workgroup)
      const int64_t row0 = base + 32 * wave;
      const bool rlive = row0 + r < NS;
      if (h == 0) {
        float4 par = make_float4(0.f, 0.f, 0.f, 0.f);
        long long id = 0;
        if (rlive) {
          if (has_id) id = sh_id(QM ? p.neg_id : p.pos_id, p.id64, row0 + r);
          if (QM) {
            par.x = p.neg_bias ? p.neg_bias[row0 + r] : 0.f;
          } else {
            const float *st = p.stats + 4 * (row0 + r);
            par = make_float4(st[0], st[1], sh_scale(p.kind, sh_upstream(p, row0 + r), st[2], st[3]), 0.f);
          }
        }
        row_par[wave][r] = par;
        row_id[wave][r] = id;
      }
      bf16x8 af[KS];
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        af[s] = rlive && klive ? mat_load8(strm, row0 + r, 16 * s + 8 * h) : frag_zero8();
        acc = mfma_32x32x16(af[s], hf[s], acc);
      }
      __syncthreads();
      // the coefficients of this lane's held row against its 16 streamed rows
      float w[16];
      unsigned used = 0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;
        const float4 par = row_par[wave][rr];
        const bool ok = hlive && row0 + rr < NS && !(has_id && row_id[wave][rr] == hid);
        float pp = 0.f, a = 0.f;
        if (QM)
          a = sh_coef(p.kind, acc[e] + par.x, h_sp, h_mx, h_c, pp);
        else
          a = sh_coef(p.kind, acc[e] + h_bias, par.x, par.y, par.z, pp);
        w[e] = ok ? a : 0.f;
        if (QM && ok) psum += pp;
        const unsigned long long bal = __ballot(w[e] != 0.f);
        const int rr0 = (e & 3) + 8 * (e >> 2);
        if (bal & 0xffffffffull) used |= 1u << rr0;
        if (bal >> 32) used |= 1u << (rr0 + 4);
      }
      // the streamed tile transposed, [d][streamed row]; an unused row enters as zeros
      if (klive) {
        const bool keep = (used >> r) & 1u;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            timg[wave][16 * s + 8 * h + j][r] = keep ? static_cast<uint16_t>(af[s][j]) : uint16_t(0);
      }
      __syncthreads();
      // out[held, :] += a^T x streamed rows: the coefficient registers are the A operand
      // (element j of lane half h of K-step s2 is streamed row 16 s2 + 8 (j >> 2) + 4 h + (j & 3))
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        // each coefficient as hi + lo, two bf16 values (w - hi is exact in fp32): 2^-16 relative
        uint32_t ch[4], cl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float w0 = w[8 * s2 + 2 * k], w1 = w[8 * s2 + 2 * k + 1];
          ch[k] = pack_bf16x2(w0, w1);
          cl[k] = pack_bf16x2(w0 - __uint_as_float(ch[k] << 16), w1 - __uint_as_float(ch[k] & 0xffff0000u));
        }
        const bf16x8 cf_hi = __builtin_bit_cast(bf16x8, make_uint4(ch[0], ch[1], ch[2], ch[3]));
        const bf16x8 cf_lo = __builtin_bit_cast(bf16x8, make_uint4(cl[0], cl[1], cl[2], cl[3]));
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int d = 32 * cb + r;
          uint2 lo = make_uint2(0, 0), hi = make_uint2(0, 0);
          if (d < D) {
            lo = *reinterpret_cast<const uint2 *>(&timg[wave][d][16 * s2 + 4 * h]);
            hi = *reinterpret_cast<const uint2 *>(&timg[wave][d][16 * s2 + 8 + 4 * h]);
          }
          const bf16x8 bf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
          Z[cb] = mfma_32x32x16(cf_hi, bf, Z[cb]);
          Z[cb] = mfma_32x32x16(cf_lo, bf, Z[cb]);
        }
      }
    }
    // the chunk's partial: the four waves' products summed in wave order
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int d = 32 * cb + r;
      if (d < D) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red[wave][((e & 3) + 8 * (e >> 2) + 4 * h) * D + d] = Z[cb][e];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + SH_THREADS * i;
      const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
      if (QM || p.splits == 1) {
        tot[i] += v;
      } else if (h0 + e / D < NH) {
        p.ws[(chunk * NH + h0 + e / D) * D + e % D] = v;
      }
    }
    __syncthreads();
  }

  if (QM) {
    psum_s[2 * wave + h][r] = psum;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + SH_THREADS * i;
      const int row = e / D, d = e % D;
      if (h0 + row >= NH) continue;
      const float4 hp = held_par[row];
      float ap;  // a[b, +] = g_b dL_b/ds+[b]
      if (p.kind == MREC_SHNEG_SOFTMAX) {
        ap = expf(hp.x - hp.y) * hp.z - hp.w;
      } else {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * SH_W; ++k) s += psum_s[k][row];
        ap = -s;
      }
      const float pv = ap == 0.f ? 0.f : ap * mat_elem_bf16(p.pos, h0 + row, d);
      const float qv = ap == 0.f ? 0.f : ap * mat_elem_bf16(p.q, h0 + row, d);
      mat_store(p.dq, h0 + row, d, tot[i] + pv);
      mat_store(p.dpos, h0 + row, d, qv);
    }
  } else if (p.splits == 1) {
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const int e = tid + SH_THREADS * i;
      if (h0 + e / D < NH) mat_store(p.dneg, h0 + e / D, e % D, tot[i]);
    }
  }
}

// dneg from the per-chunk partials, in chunk order (the order a single split sums them in)
__global__ __launch_bounds__(256) void shneg_ws_reduce_kernel(const float *__restrict__ ws, int64_t S, int D,
                                                              int64_t n_chunks, MatOut dneg) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= S * D) return;
  float tot = 0.f;
  for (int64_t c = 0; c < n_chunks; ++c) tot += ws[c * S * D + i];
  mat_store(dneg, i / D, static_cast<int>(i % D), tot);
}

// the device functions the losses call, one per element (the tolerance probe of the tests)
__global__ __launch_bounds__(256) void shneg_math_kernel(int fn, const float *__restrict__ x, int64_t n,
                                                         float *__restrict__ y) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i];
  float o;
  switch (fn) {
    case 0: o = expf(v); break;
    case 1: o = logf(v); break;
    case 2: o = v > 20.f ? v : log1pf(expf(v)); break;
    case 3: o = sigmoid_stable(v); break;
    default: o = dsigmoid_stable(v); break;
  }
  y[i] = o;
}

}  // namespace mrec

using namespace mrec;

namespace {

bool sh_dim_ok(int32_t D) { return D == 8 || D == 16 || D == 32 || D == 64; }

int64_t sh_chunks(int64_t batch) { return (batch + SH_CHUNK - 1) / SH_CHUNK; }

// an output: rows of at least D elements, element aligned (weaker than rows16_ok)
bool sh_out_ok(const void *p, int64_t ld, int32_t D, mrec_dtype t) {
  const uintptr_t eb = t == MREC_F32 ? 4 : 2;
  return p && ld >= D && (reinterpret_cast<uintptr_t>(p) & (eb - 1)) == 0;
}

mrec_status sh_check(const mrec_shneg_args *a, bool bwd, ShArgs &p) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(mrec_shneg_supported(a->D, a->q_dtype, a->row_dtype),
                 "unsupported shape (mrec_shneg_supported: D in {8, 16, 32, 64}, q and rows F32 or BF16)");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX && a->n_neg >= 0 && a->n_neg <= INT32_MAX,
                 "batch and n_neg must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->kind == MREC_SHNEG_SOFTMAX || a->kind == MREC_SHNEG_BPR || a->kind == MREC_SHNEG_TOP1,
                 "kind must be MREC_SHNEG_SOFTMAX, _BPR or _TOP1");
  MREC_CHECK_ARG(a->reduction == MREC_REDUCE_NONE || a->reduction == MREC_REDUCE_MEAN ||
                     a->reduction == MREC_REDUCE_SUM,
                 "reduction must be none, mean or sum");
  MREC_CHECK_ARG((a->pos_id == nullptr) == (a->neg_id == nullptr), "pos_id and neg_id go together");
  MREC_CHECK_ARG(!a->pos_id || a->id_dtype == MREC_I32 || a->id_dtype == MREC_I64, "ids must be int32 or int64");
  MREC_CHECK_ARG(a->splits >= 0 && a->splits <= SH_MAX_SPLITS, "splits must be in 0 .. 64 (0: the default)");
  if (a->batch > 0) {
    MREC_CHECK_ARG(rows16_ok(a->q, a->ldq, a->D, a->q_dtype) && rows16_ok(a->pos, a->ld_pos, a->D, a->row_dtype),
                   "q and pos need 16-byte aligned rows of at least D elements");
    MREC_CHECK_ARG(a->n_neg == 0 || rows16_ok(a->neg, a->ld_neg, a->D, a->row_dtype),
                   "neg needs 16-byte aligned rows of at least D elements");
    MREC_CHECK_ARG(a->stats != nullptr, "NULL stats");
    if (!bwd) {
      MREC_CHECK_ARG(a->loss != nullptr, "NULL loss");
    } else {
      MREC_CHECK_ARG(a->g != nullptr, "NULL upstream gradient");
      MREC_CHECK_ARG(sh_out_ok(a->dq, a->ld_dq, a->D, a->q_dtype) && sh_out_ok(a->dpos, a->ld_dpos, a->D, a->row_dtype),
                     "dq and dpos need rows of at least D elements");
      MREC_CHECK_ARG(a->n_neg == 0 || sh_out_ok(a->dneg, a->ld_dneg, a->D, a->row_dtype),
                     "dneg needs rows of at least D elements");
    }
    const int32_t splits = a->splits ? a->splits : mrec_shneg_splits(a->batch, a->n_neg);
    // the forward's per-query losses (mean, sum), the candidate-major pass's chunk partials
    const size_t need = bwd ? static_cast<size_t>(sh_chunks(a->batch)) * a->n_neg * a->D * 4
                            : static_cast<size_t>(a->batch) * 4;
    const bool uses = bwd ? (splits > 1 && a->n_neg > 0) : a->reduction != MREC_REDUCE_NONE;
    if (uses) {
      MREC_CHECK_ARG(a->workspace != nullptr && a->workspace_bytes >= need,
                     "workspace smaller than mrec_shneg_workspace_size");
      MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, "workspace not 16-byte aligned");
    }
    p.splits = splits;
  }
  p.q = mat_in(a->q, a->ldq, a->q_dtype);
  p.pos = mat_in(a->pos, a->ld_pos, a->row_dtype);
  p.neg = mat_in(a->neg, a->ld_neg, a->row_dtype);
  p.B = a->batch;
  p.S = a->n_neg;
  p.pos_id = a->pos_id;
  p.neg_id = a->neg_id;
  p.id64 = a->id_dtype == MREC_I64;
  p.pos_bias = a->pos_bias;
  p.neg_bias = a->neg_bias;
  p.kind = a->kind;
  p.reduction = a->reduction;
  p.stats = a->stats;
  p.g = a->g;
  p.dq = mat_out(a->dq, a->ld_dq, a->q_dtype);
  p.dpos = mat_out(a->dpos, a->ld_dpos, a->row_dtype);
  p.dneg = mat_out(a->dneg, a->ld_dneg, a->row_dtype);
  p.ws = static_cast<float *>(a->workspace);
  return MREC_OK;
}

template <int D>
void sh_launch(const ShArgs &p, int pass, dim3 grid, hipStream_t s) {
  if (pass == 0)
    shneg_fwd_kernel<D><<<grid, SH_THREADS, 0, s>>>(p);
  else if (pass == 1)
    shneg_bwd_kernel<D, true><<<grid, SH_THREADS, 0, s>>>(p);
  else
    shneg_bwd_kernel<D, false><<<grid, SH_THREADS, 0, s>>>(p);
}

void sh_launch_dim(int D, const ShArgs &p, int pass, dim3 grid, hipStream_t s) {
  switch (D) {
    case 8: sh_launch<8>(p, pass, grid, s); break;
    case 16: sh_launch<16>(p, pass, grid, s); break;
    case 32: sh_launch<32>(p, pass, grid, s); break;
    default: sh_launch<64>(p, pass, grid, s); break;
  }
}

}  // namespace

extern "C" {

int32_t mrec_shneg_supported(int32_t D, mrec_dtype q_dtype, mrec_dtype row_dtype) {
  return sh_dim_ok(D) && is_float_dtype(q_dtype) && is_float_dtype(row_dtype);
}

int32_t mrec_shneg_tile_queries(void) { return SH_T; }
int32_t mrec_shneg_tile_candidates(void) { return SH_T; }

int32_t mrec_shneg_splits(int64_t batch, int64_t n_neg) {
  if (batch <= 0 || n_neg <= 0) return 1;
  const int64_t ct = (n_neg + SH_T - 1) / SH_T;
  // fill the CUs twice over when the pool is small; whole chunks of the batch only
  int64_t s = (2 * device_cus() + ct - 1) / ct;
  s = std::min<int64_t>(s, sh_chunks(batch));
  s = std::min<int64_t>(s, SH_MAX_SPLITS);
  return static_cast<int32_t>(s < 1 ? 1 : s);
}

size_t mrec_shneg_workspace_size(int64_t batch, int64_t n_neg, int32_t D, int32_t splits) {
  if (batch <= 0 || D <= 0) return 0;
  const size_t fwd = static_cast<size_t>(batch) * 4;
  if (splits == 0) splits = SH_MAX_SPLITS;  // (sizes for any default)
  size_t bwd = 0;
  if (splits > 1 && n_neg > 0)
    bwd = static_cast<size_t>(sh_chunks(batch)) * static_cast<size_t>(n_neg) * static_cast<size_t>(D) * 4;
  return std::max(fwd, bwd);
}

mrec_status mrec_shneg_loss_fwd(const mrec_shneg_args *a, mrec_stream stream) {
  ShArgs p{};
  const mrec_status st0 = sh_check(a, false, p);
  if (st0 != MREC_OK) return st0;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool none = a->reduction == MREC_REDUCE_NONE;
  p.loss_b = none ? a->loss : static_cast<float *>(a->workspace);
  const dim3 grid(static_cast<unsigned>((a->batch + SH_T - 1) / SH_T));
  sh_launch_dim(a->D, p, 0, grid, s);
  mrec_status st = launch_status("mrec_shneg_loss_fwd");
  if (st != MREC_OK || none) return st;
  shneg_reduce_kernel<<<1, SH_RT, 0, s>>>(p.loss_b, a->batch, a->reduction, a->loss);
  return launch_status("mrec_shneg_loss_fwd");
}

mrec_status mrec_shneg_loss_bwd(const mrec_shneg_args *a, mrec_stream stream) {
  ShArgs p{};
  const mrec_status st0 = sh_check(a, true, p);
  if (st0 != MREC_OK) return st0;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // query-major: dq, dpos (never split)
  const int32_t splits = p.splits;
  p.splits = 1;
  p.chunks_per_split = static_cast<int32_t>(std::max<int64_t>(sh_chunks(a->n_neg), 1));
  sh_launch_dim(a->D, p, 1, dim3(static_cast<unsigned>((a->batch + SH_T - 1) / SH_T)), s);
  mrec_status st = launch_status("mrec_shneg_loss_bwd");
  if (st != MREC_OK || a->n_neg == 0) return st;
  // candidate-major: dneg
  const int64_t chunks = sh_chunks(a->batch);
  const int64_t cps = (chunks + splits - 1) / splits;
  const int64_t ny = (chunks + cps - 1) / cps;
  p.splits = ny > 1 ? static_cast<int32_t>(ny) : 1;
  p.chunks_per_split = static_cast<int32_t>(cps);
  sh_launch_dim(a->D, p, 2, dim3(static_cast<unsigned>((a->n_neg + SH_T - 1) / SH_T), static_cast<unsigned>(ny)), s);
  st = launch_status("mrec_shneg_loss_bwd");
  if (st != MREC_OK || ny == 1) return st;
  const int64_t total = a->n_neg * a->D;
  shneg_ws_reduce_kernel<<<static_cast<unsigned>((total + 255) / 256), 256, 0, s>>>(p.ws, a->n_neg, a->D, chunks,
                                                                                     p.dneg);
  return launch_status("mrec_shneg_loss_bwd");
}

mrec_status mrec_shneg_math_probe(int32_t fn, const float *x, int64_t n, float *y, mrec_stream stream) {
  MREC_CHECK_ARG(fn >= 0 && fn <= 4, "fn must be 0 (exp), 1 (log), 2 (softplus), 3 (sigmoid) or 4 (sigmoid')");
  MREC_CHECK_ARG(n >= 0 && (n == 0 || (x && y)), "NULL pointer");
  if (n == 0) return MREC_OK;
  shneg_math_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(fn, x, n, y);
  return launch_status("mrec_shneg_math_probe");
}

}  // extern "C"
