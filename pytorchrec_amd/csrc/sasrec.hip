// SASRec encoder fused per sample (torchrec/model/SASRec.py:83-110).
//
// One workgroup (8 waves) per sample at a time, persistent over samples.  The four
// shared weight matrices are staged once per workgroup as bf16; the sample's X, Q, K,
// scores, probabilities, context and FFN activations live in LDS only.  One launch
// runs every layer:
//
//   X0 = rows[b, j] + pos[(his_len - j) valid_j]        (bf16; invalid rows are zero)
//   per layer   Q = X Wq^T, K = X Wk^T                  (bf16)
//               S = D^-0.5 Q K^T, A = softmax over valid keys, shifted by the row's own
//               maximum (fp32; the reference shifts by the global maximum, the same
//               softmax on paper)
//               C = A K, F = relu(C W1^T + b1), G = F W2^T + b2
//               X <- bf16(LayerNorm(X + G))             (fp32 statistics)
//   v[b] = sum_{valid j} X_j / his_len
//
// Invalid history rows (his == 0 past position 0) are masked as keys and dropped from
// v, so nothing they hold reaches a valid row: the kernels load them as zero rows,
// whatever the gathered row holds, and their gradient is exactly zero.
//
// All GEMMs are v_mfma_f32_16x16x32_bf16 with fp32 accumulation on [64][72] bf16 LDS
// tiles (L padded to 64 rows, D-wide operands zero-padded to the 32-wide k step): lane
// l holds A[m = l % 16][k = 8 (l / 16) .. + 8] and B[n = l % 16][k ..], read as one
// 16-B vector from a tile stored "row = output index, k contiguous" or as two
// transposing 8-B reads (ds_read_b64_tr_b16) from a tile stored the other way round
// (sr_frag<true>): the backward's transposed products read the forward's tiles in place.
//
// Saved between forward and backward: the layer outputs hs [num_layers, B, L, D] bf16
// (num_layers * L * D * 2 bytes per sample: 12.5 KiB at L = 50, D = 64, 2 layers) and
// nothing else: the backward recomputes a layer's Q, K, A, C, F and LayerNorm
// statistics from that layer's input (the gathered rows for layer 0, hs[l - 1] after).
//
// Backward, per layer from the last: LayerNorm, residual, FFN, A K, softmax, Q K^T,
// with every gradient operand rounded to bf16 and fp32 accumulation.  The weight
// gradients stay in MFMA accumulators over the workgroup's samples and layers, the
// bias / LayerNorm gradients in per-thread registers, the position-table gradient in
// the workgroup's own partial; one fp32 partial per workgroup, summed in workgroup
// order by sasrec_wgrad_kernel (bit-reproducible).
//
// LDS: 12 bf16 tiles (X Q K P C F + two gradient tiles + four weights) 108 KiB, three
// fp32 [64][64] buffers 48 KiB, vectors 2 KiB: 158 KiB, one workgroup per CU.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int SR_ROWS = 64;  // history positions per sample, padded
constexpr int SR_THREADS = 512;
constexpr int SR_WAVES = SR_THREADS / 64;
constexpr int SR_LD = 72;  // bf16 elements per tile row (144 B: 16-B aligned rows)
constexpr int SR_TILE = SR_ROWS * SR_LD;
constexpr int SR_F32 = SR_ROWS * 64;  // an fp32 [64][64] buffer

struct SasrecArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const int32_t *his_len;
  const float *pos;  // position table [pos_rows, D] fp32
  int64_t ld_pos;
  int pos_rows;
  const float *wq, *wk, *w1, *w2;  // fp32 masters, nn.Linear layout [out, in]
  int64_t ldq, ldk, ld1, ld2;
  const float *b1, *b2, *gamma, *beta;
  float eps;
  int num_layers;
  int64_t batch;
  int L;
  uint16_t *hs;  // [num_layers, batch, L, D] bf16 layer outputs
  float *v;      // [batch, D]
  int32_t *oob;  // set to 1 on a position id outside the table (NULL: not reported)
  const float *dv;
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][P]
  int64_t P;
};

enum { SR_X = 0, SR_Q, SR_K, SR_P, SR_C, SR_F, SR_GA, SR_GB, SR_WQ, SR_WK, SR_W1, SR_W2, SR_NTILES };

template <int D>
struct SrShape {
  static_assert(D == 16 || D == 32 || D == 64, "compiled widths");
  static constexpr int NT = D / 16;         // column tiles of a D-wide output
  static constexpr int KS = (D + 31) / 32;  // k steps over a D-wide operand
  static constexpr int CH = D / 8;          // 16-B chunks per row
  static constexpr int G = SR_THREADS / D;  // row groups of the column passes
  static constexpr size_t f32_off = static_cast<size_t>(SR_NTILES) * SR_TILE * 2;
  static constexpr size_t bytes = f32_off + 3 * SR_F32 * 4 + 8 * 64 * 4;
  static constexpr float scale = D == 16 ? 0.25f : (D == 64 ? 0.125f : 0.17677669529663687f);
};

struct SrLds {
  uint16_t *t;          // SR_NTILES bf16 tiles
  float *S, *Z, *G;     // fp32 [64][64]: scores / probabilities; X + G, later dP; dY -> dz -> dX
  float *b1, *b2, *gam, *bet, *mu, *rstd;
  int *valid, *pos;
  __device__ uint16_t *tile(int i) const { return t + i * SR_TILE; }
};

template <int D>
__device__ __forceinline__ SrLds sr_lds(char *base) {
  SrLds m;
  m.t = reinterpret_cast<uint16_t *>(base);
  m.S = reinterpret_cast<float *>(base + SrShape<D>::f32_off);
  m.Z = m.S + SR_F32;
  m.G = m.Z + SR_F32;
  m.b1 = m.G + SR_F32;
  m.b2 = m.b1 + 64;
  m.gam = m.b2 + 64;
  m.bet = m.gam + 64;
  m.mu = m.bet + 64;
  m.rstd = m.mu + 64;
  m.valid = reinterpret_cast<int *>(m.rstd + 64);
  m.pos = m.valid + 64;
  return m;
}

// operand fragment of rows r0 .. r0 + 15, k0 .. k0 + 31: element (r, k) is
// base[r][k], or base[k][r] with TR (the tile holds the operand transposed)
template <bool TR>
__device__ __forceinline__ bf16x8 sr_frag(const uint16_t *base, int r0, int k0, int lane) {
  const int r = r0 + (lane & 15), k = k0 + 8 * (lane >> 4);
  if constexpr (!TR) {
    return *reinterpret_cast<const bf16x8 *>(base + r * SR_LD + k);
  } else {
    // two transposing reads (frag.h): tile rows k .. + 3 and k + 4 .. + 7 are the lane's
    // 8 k values; every address lies inside the tile
    const int li = lane & 15;
    const uint16_t *p = base + (k + (li >> 2)) * SR_LD + r0 + 4 * (li & 3);
    return lds_tr16_pair(p, 4 * SR_LD);
  }
}

// An [16 MT, 16 NT] product's tiles t = wave, wave + 8, ... (tile t: rows 16 (t / NT),
// columns 16 (t % NT)); acc[i] += A[rows, :] . B[columns, :] over KS k steps.
template <int MT, int NT>
struct SrAcc {
  static constexpr int N = (MT * NT + SR_WAVES - 1) / SR_WAVES;
  f32x4 a[N];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
};

template <int MT, int NT, int KS, bool TA, bool TB>
__device__ __forceinline__ void sr_mma(const uint16_t *A, const uint16_t *B, int wave, int lane,
                                       SrAcc<MT, NT> &acc) {
#pragma unroll
  for (int i = 0; i < SrAcc<MT, NT>::N; ++i) {
    const int t = wave + SR_WAVES * i;
    if (t < MT * NT) {
      const int mt = t / NT, nt = t % NT;
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc.a[i] = mfma_16x16x32(sr_frag<TA>(A, 16 * mt, 32 * s, lane),
                                 sr_frag<TB>(B, 16 * nt, 32 * s, lane), acc.a[i]);
    }
  }
}

// f(row, column, value) for every element this lane holds
template <int MT, int NT, class F>
__device__ __forceinline__ void sr_each(const SrAcc<MT, NT> &acc, int wave, int lane, F f) {
#pragma unroll
  for (int i = 0; i < SrAcc<MT, NT>::N; ++i) {
    const int t = wave + SR_WAVES * i;
    if (t < MT * NT) {
      const int mt = t / NT, nt = t % NT;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        f(16 * mt + 4 * (lane >> 4) + e, 16 * nt + (lane & 15), acc.a[i][e]);
    }
  }
}

// sum / max over the 8 lanes of a row pass (lanes 8 q .. 8 q + 7), every lane gets it
__device__ __forceinline__ float sr_sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}
__device__ __forceinline__ float sr_max8(float v) {
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  return fmaxf(v, __shfl_xor(v, 4));
}

// zero the LDS, then the weights as bf16 tiles and the vectors (once per workgroup)
template <int D>
__device__ void sr_stage(const SasrecArgs &p, const SrLds &m, char *base, int tid) {
  for (size_t o = static_cast<size_t>(tid) * 16; o < SrShape<D>::bytes; o += SR_THREADS * 16)
    *reinterpret_cast<uint4 *>(base + o) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  for (int i = tid; i < D * D; i += SR_THREADS) {
    const int n = i / D, k = i % D;
    m.tile(SR_WQ)[n * SR_LD + k] = f32_to_bf16_rne(p.wq[n * p.ldq + k]);
    m.tile(SR_WK)[n * SR_LD + k] = f32_to_bf16_rne(p.wk[n * p.ldk + k]);
    m.tile(SR_W1)[n * SR_LD + k] = f32_to_bf16_rne(p.w1[n * p.ld1 + k]);
    m.tile(SR_W2)[n * SR_LD + k] = f32_to_bf16_rne(p.w2[n * p.ld2 + k]);
  }
  if (tid < D) {
    m.b1[tid] = p.b1[tid];
    m.b2[tid] = p.b2[tid];
    m.gam[tid] = p.gamma[tid];
    m.bet[tid] = p.beta[tid];
  }
  __syncthreads();
}

// validity and position id of every history position of sample b (pos < 0: no row)
__device__ __forceinline__ void sr_meta(const SasrecArgs &p, int64_t b, const SrLds &m, int tid) {
  if (tid < SR_ROWS) {
    const int j = tid;
    const bool ok = j < p.L && (j == 0 || p.his[b * p.ld_his + j] > 0);
    int pos = -1;
    if (ok) {
      pos = p.his_len[b] - j;
      if (pos < 0 || pos >= p.pos_rows) {
        pos = -1;
        if (p.oob) *p.oob = 1;
      }
    }
    m.valid[j] = ok ? 1 : 0;
    m.pos[j] = pos;
  }
  __syncthreads();
}

// X tile <- layer 0's input: bf16(item row + position row) at valid positions, else 0
template <int D>
__device__ __forceinline__ void sr_load_x0(const SasrecArgs &p, int64_t b, const SrLds &m, int tid) {
  constexpr int CH = SrShape<D>::CH;
  for (int t = tid; t < SR_ROWS * CH; t += SR_THREADS) {
    const int j = t / CH, c = (t % CH) * 8;
    uint4 out = make_uint4(0, 0, 0, 0);
    if (m.valid[j]) {
      const uint4 raw = *reinterpret_cast<const uint4 *>(p.rows + (b * p.L + j) * p.ld_rows + c);
      float x[8];
      Vec<uint16_t>::to_f32(raw, x);
      const int pos = m.pos[j];
      if (pos >= 0) {
        const float *pr = p.pos + pos * p.ld_pos + c;
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] += pr[i];
      }
      out = make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]),
                       pack_bf16x2(x[6], x[7]));
    }
    *reinterpret_cast<uint4 *>(m.tile(SR_X) + j * SR_LD + c) = out;
  }
}

// X tile <- a saved layer output (rows j < L; the others zero)
template <int D>
__device__ __forceinline__ void sr_load_hs(const uint16_t *src, int L, const SrLds &m, int tid) {
  constexpr int CH = SrShape<D>::CH;
  for (int t = tid; t < SR_ROWS * CH; t += SR_THREADS) {
    const int j = t / CH, c = (t % CH) * 8;
    uint4 out = make_uint4(0, 0, 0, 0);
    if (j < L) out = *reinterpret_cast<const uint4 *>(src + j * D + c);
    *reinterpret_cast<uint4 *>(m.tile(SR_X) + j * SR_LD + c) = out;
  }
}

// One layer's forward on the X tile: fills Q, K, S (probabilities, fp32), P (bf16), C,
// F, Z = X + G and the LayerNorm statistics.  With WRITE_X the X tile becomes the
// layer's output bf16(LayerNorm(Z)).  Starts and ends at a barrier.
template <int D, bool WRITE_X>
__device__ __forceinline__ void sr_layer(const SasrecArgs &p, const SrLds &m, int tid) {
  using S = SrShape<D>;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 3, sub = tid & 7;  // the row passes: 8 lanes per row
  {  // Q = X Wq^T, K = X Wk^T
    SrAcc<4, S::NT> q, k;
    q.zero();
    k.zero();
    sr_mma<4, S::NT, S::KS, false, false>(m.tile(SR_X), m.tile(SR_WQ), wave, lane, q);
    sr_mma<4, S::NT, S::KS, false, false>(m.tile(SR_X), m.tile(SR_WK), wave, lane, k);
    uint16_t *tq = m.tile(SR_Q), *tk = m.tile(SR_K);
    sr_each<4, S::NT>(q, wave, lane, [&](int i, int c, float x) { tq[i * SR_LD + c] = f32_to_bf16_rne(x); });
    sr_each<4, S::NT>(k, wave, lane, [&](int i, int c, float x) { tk[i * SR_LD + c] = f32_to_bf16_rne(x); });
  }
  __syncthreads();
  {  // S = D^-0.5 Q K^T
    SrAcc<4, 4> s;
    s.zero();
    sr_mma<4, 4, S::KS, false, false>(m.tile(SR_Q), m.tile(SR_K), wave, lane, s);
    float *ss = m.S;
    sr_each<4, 4>(s, wave, lane, [&](int i, int c, float x) { ss[i * 64 + c] = x * S::scale; });
  }
  __syncthreads();
  {  // A = softmax over the valid keys of row r (key 0 is always valid)
    float e[8];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = sub + 8 * i;
      e[i] = m.valid[c] ? m.S[r * 64 + c] : -INFINITY;
      mx = fmaxf(mx, e[i]);
    }
    mx = sr_max8(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      e[i] = m.valid[sub + 8 * i] ? expf(e[i] - mx) : 0.f;
      sum += e[i];
    }
    const float inv = 1.f / sr_sum8(sum);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = sub + 8 * i;
      const float a = e[i] * inv;
      m.S[r * 64 + c] = a;
      m.tile(SR_P)[r * SR_LD + c] = f32_to_bf16_rne(a);
    }
  }
  __syncthreads();
  {  // C = A K
    SrAcc<4, S::NT> c;
    c.zero();
    sr_mma<4, S::NT, 2, false, true>(m.tile(SR_P), m.tile(SR_K), wave, lane, c);
    uint16_t *tc = m.tile(SR_C);
    sr_each<4, S::NT>(c, wave, lane, [&](int i, int j, float x) { tc[i * SR_LD + j] = f32_to_bf16_rne(x); });
  }
  __syncthreads();
  {  // F = relu(C W1^T + b1)
    SrAcc<4, S::NT> f;
    f.zero();
    sr_mma<4, S::NT, S::KS, false, false>(m.tile(SR_C), m.tile(SR_W1), wave, lane, f);
    uint16_t *tf = m.tile(SR_F);
    const float *b1 = m.b1;
    sr_each<4, S::NT>(f, wave, lane, [&](int i, int j, float x) {
      tf[i * SR_LD + j] = f32_to_bf16_rne(fmaxf(x + b1[j], 0.f));
    });
  }
  __syncthreads();
  {  // Z = X + F W2^T + b2
    SrAcc<4, S::NT> g;
    g.zero();
    sr_mma<4, S::NT, S::KS, false, false>(m.tile(SR_F), m.tile(SR_W2), wave, lane, g);
    const uint16_t *tx = m.tile(SR_X);
    const float *b2 = m.b2;
    float *z = m.Z;
    sr_each<4, S::NT>(g, wave, lane, [&](int i, int j, float x) {
      z[i * 64 + j] = bf16_to_f32(tx[i * SR_LD + j]) + (x + b2[j]);
    });
  }
  __syncthreads();
  {  // LayerNorm statistics of row r (biased variance), and the output row
    float z[S::CH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) {
      z[i] = m.Z[r * 64 + sub + 8 * i];
      s += z[i];
    }
    const float mu = sr_sum8(s) * (1.f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) q += (z[i] - mu) * (z[i] - mu);
    const float rstd = rsqrtf(sr_sum8(q) * (1.f / D) + p.eps);
    if (sub == 0) {
      m.mu[r] = mu;
      m.rstd[r] = rstd;
    }
    if constexpr (WRITE_X) {
#pragma unroll
      for (int i = 0; i < S::CH; ++i) {
        const int c = sub + 8 * i;
        m.tile(SR_X)[r * SR_LD + c] = f32_to_bf16_rne((z[i] - mu) * rstd * m.gam[c] + m.bet[c]);
      }
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SR_THREADS, 1) void sasrec_fwd_kernel(SasrecArgs p) {
  using S = SrShape<D>;
  extern __shared__ __attribute__((aligned(16))) char sr_smem[];
  const SrLds m = sr_lds<D>(sr_smem);
  const int tid = threadIdx.x;
  sr_stage<D>(p, m, sr_smem, tid);
  for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
    sr_meta(p, b, m, tid);
    sr_load_x0<D>(p, b, m, tid);
    __syncthreads();
    for (int l = 0; l < p.num_layers; ++l) {
      sr_layer<D, true>(p, m, tid);
      uint16_t *dst = p.hs + ((static_cast<int64_t>(l) * p.batch + b) * p.L) * D;
      for (int t = tid; t < p.L * S::CH; t += SR_THREADS) {
        const int j = t / S::CH, c = (t % S::CH) * 8;
        *reinterpret_cast<uint4 *>(dst + j * D + c) =
            *reinterpret_cast<const uint4 *>(m.tile(SR_X) + j * SR_LD + c);
      }
    }
    // v = sum over valid rows / his_len: row group g sums rows g, g + G, ...; the
    // groups are added in group order
    {
      const int d = tid % D, g = tid / D;
      float s = 0.f;
      for (int j = g; j < p.L; j += S::G)
        if (m.valid[j]) s += bf16_to_f32(m.tile(SR_X)[j * SR_LD + d]);
      m.Z[g * D + d] = s;
    }
    __syncthreads();
    if (tid < D) {
      float s = 0.f;
      for (int g = 0; g < S::G; ++g) s += m.Z[g * D + tid];
      p.v[b * D + tid] = s / static_cast<float>(p.his_len[b]);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(SR_THREADS, 1) void sasrec_bwd_kernel(SasrecArgs p) {
  using S = SrShape<D>;
  constexpr int NT = S::NT, KS = S::KS;
  extern __shared__ __attribute__((aligned(16))) char sr_smem[];
  const SrLds m = sr_lds<D>(sr_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 3, sub = tid & 7;  // row passes
  const int cd = tid % D, cg = tid / D;   // column passes: column cd, rows cg, cg + G, ...
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * p.P;
  float *part_pos = part + 4 * D * D + 4 * D;
  sr_stage<D>(p, m, sr_smem, tid);
  for (int i = tid; i < p.pos_rows * D; i += SR_THREADS) part_pos[i] = 0.f;
  SrAcc<NT, NT> gwq, gwk, gw1, gw2;
  gwq.zero();
  gwk.zero();
  gw1.zero();
  gw2.zero();
  float gb1 = 0.f, gb2 = 0.f, ggam = 0.f, gbet = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
    sr_meta(p, b, m, tid);
    {  // dY of the last layer: dv / his_len at the valid rows
      const float inv = 1.f / static_cast<float>(p.his_len[b]);
      for (int i = tid; i < SR_ROWS * D; i += SR_THREADS) {
        const int j = i / D, d = i % D;
        m.G[j * 64 + d] = m.valid[j] ? p.dv[b * D + d] * inv : 0.f;
      }
    }
    for (int l = p.num_layers - 1; l >= 0; --l) {
      if (l == 0)
        sr_load_x0<D>(p, b, m, tid);
      else
        sr_load_hs<D>(p.hs + ((static_cast<int64_t>(l - 1) * p.batch + b) * p.L) * D, p.L, m, tid);
      __syncthreads();
      sr_layer<D, false>(p, m, tid);
      // LayerNorm: dgamma, dbeta from dY (column pass), then dz in place (row pass)
      for (int j = cg; j < SR_ROWS; j += S::G) {
        const float dy = m.G[j * 64 + cd];
        ggam = fmaf(dy, (m.Z[j * 64 + cd] - m.mu[j]) * m.rstd[j], ggam);
        gbet += dy;
      }
      __syncthreads();
      {
        const float mu = m.mu[r], rs = m.rstd[r];
        float g[S::CH], xh[S::CH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < S::CH; ++i) {
          const int c = sub + 8 * i;
          g[i] = m.G[r * 64 + c] * m.gam[c];
          xh[i] = (m.Z[r * 64 + c] - mu) * rs;
          s1 += g[i];
          s2 = fmaf(g[i], xh[i], s2);
        }
        s1 = sr_sum8(s1) * (1.f / D);
        s2 = sr_sum8(s2) * (1.f / D);
#pragma unroll
        for (int i = 0; i < S::CH; ++i) {
          const int c = sub + 8 * i;
          const float dz = rs * (g[i] - s1 - xh[i] * s2);
          m.G[r * 64 + c] = dz;
          m.tile(SR_GA)[r * SR_LD + c] = f32_to_bf16_rne(dz);
        }
      }
      __syncthreads();
      // FFN layer 2: db2, dW2 += dG^T F, dF = (dG W2) masked by F > 0  -> GB
      for (int j = cg; j < SR_ROWS; j += S::G) gb2 += m.G[j * 64 + cd];
      sr_mma<NT, NT, 2, true, true>(m.tile(SR_GA), m.tile(SR_F), wave, lane, gw2);
      {
        SrAcc<4, NT> a;
        a.zero();
        sr_mma<4, NT, KS, false, true>(m.tile(SR_GA), m.tile(SR_W2), wave, lane, a);
        const uint16_t *tf = m.tile(SR_F);
        uint16_t *tb = m.tile(SR_GB);
        sr_each<4, NT>(a, wave, lane, [&](int i, int c, float x) {
          tb[i * SR_LD + c] = (tf[i * SR_LD + c] & 0x7fff) ? f32_to_bf16_rne(x) : uint16_t(0);
        });
      }
      __syncthreads();
      // FFN layer 1: db1, dW1 += dF^T C, dC = dF W1  -> GA
      for (int j = cg; j < SR_ROWS; j += S::G) gb1 += bf16_to_f32(m.tile(SR_GB)[j * SR_LD + cd]);
      sr_mma<NT, NT, 2, true, true>(m.tile(SR_GB), m.tile(SR_C), wave, lane, gw1);
      {
        SrAcc<4, NT> a;
        a.zero();
        sr_mma<4, NT, KS, false, true>(m.tile(SR_GB), m.tile(SR_W1), wave, lane, a);
        uint16_t *ta = m.tile(SR_GA);
        sr_each<4, NT>(a, wave, lane, [&](int i, int c, float x) { ta[i * SR_LD + c] = f32_to_bf16_rne(x); });
      }
      __syncthreads();
      // C = A K: dA = dC K^T -> Z (fp32); dK = A^T dC (kept in registers)
      SrAcc<4, NT> dk;
      dk.zero();
      {
        SrAcc<4, 4> a;
        a.zero();
        sr_mma<4, 4, KS, false, false>(m.tile(SR_GA), m.tile(SR_K), wave, lane, a);
        float *z = m.Z;
        sr_each<4, 4>(a, wave, lane, [&](int i, int c, float x) { z[i * 64 + c] = x; });
      }
      sr_mma<4, NT, 2, true, true>(m.tile(SR_P), m.tile(SR_GA), wave, lane, dk);
      __syncthreads();
      {  // softmax: dS = D^-0.5 A (dA - sum_k A dA)  -> P (bf16)
        float a[8], da[8];
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int c = sub + 8 * i;
          a[i] = m.S[r * 64 + c];
          da[i] = m.Z[r * 64 + c];
          t = fmaf(a[i], da[i], t);
        }
        t = sr_sum8(t);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          m.tile(SR_P)[r * SR_LD + sub + 8 * i] = f32_to_bf16_rne(a[i] * (da[i] - t) * S::scale);
      }
      __syncthreads();
      // S = Q K^T: dQ = dS K -> C tile; dK += dS^T Q -> F tile
      {
        SrAcc<4, NT> a;
        a.zero();
        sr_mma<4, NT, 2, false, true>(m.tile(SR_P), m.tile(SR_K), wave, lane, a);
        uint16_t *tc = m.tile(SR_C);
        sr_each<4, NT>(a, wave, lane, [&](int i, int c, float x) { tc[i * SR_LD + c] = f32_to_bf16_rne(x); });
      }
      sr_mma<4, NT, 2, true, true>(m.tile(SR_P), m.tile(SR_Q), wave, lane, dk);
      {
        uint16_t *tf = m.tile(SR_F);
        sr_each<4, NT>(dk, wave, lane, [&](int i, int c, float x) { tf[i * SR_LD + c] = f32_to_bf16_rne(x); });
      }
      __syncthreads();
      // dWq += dQ^T X, dWk += dK^T X, dX = dz + dQ Wq + dK Wk (in place in G)
      sr_mma<NT, NT, 2, true, true>(m.tile(SR_C), m.tile(SR_X), wave, lane, gwq);
      sr_mma<NT, NT, 2, true, true>(m.tile(SR_F), m.tile(SR_X), wave, lane, gwk);
      {
        SrAcc<4, NT> a;
        a.zero();
        sr_mma<4, NT, KS, false, true>(m.tile(SR_C), m.tile(SR_WQ), wave, lane, a);
        sr_mma<4, NT, KS, false, true>(m.tile(SR_F), m.tile(SR_WK), wave, lane, a);
        float *g = m.G;
        sr_each<4, NT>(a, wave, lane, [&](int i, int c, float x) { g[i * 64 + c] += x; });
      }
      __syncthreads();
    }
    // layer 0's dX: the rows' gradient (zero at invalid positions) and the position
    // rows' (a sample's valid positions have distinct ids: no two threads meet)
    for (int t = tid; t < p.L * S::CH; t += SR_THREADS) {
      const int j = t / S::CH, c = (t % S::CH) * 8;
      uint4 out = make_uint4(0, 0, 0, 0);
      if (m.valid[j]) {
        const float *g = m.G + j * 64 + c;
        out = make_uint4(pack_bf16x2(g[0], g[1]), pack_bf16x2(g[2], g[3]), pack_bf16x2(g[4], g[5]),
                         pack_bf16x2(g[6], g[7]));
        const int pos = m.pos[j];
        if (pos >= 0) {
          float *pp = part_pos + pos * D + c;
#pragma unroll
          for (int i = 0; i < 8; ++i) pp[i] += g[i];
        }
      }
      *reinterpret_cast<uint4 *>(p.drows + (b * p.L + j) * p.ld_drows + c) = out;
    }
    __syncthreads();
  }
  // the workgroup's partial: [dWq | dWk | dW1 | dW2 | db1 | db2 | dgamma | dbeta | dpos]
  {
    float *o = part;
    sr_each<NT, NT>(gwq, wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
    o += D * D;
    sr_each<NT, NT>(gwk, wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
    o += D * D;
    sr_each<NT, NT>(gw1, wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
    o += D * D;
    sr_each<NT, NT>(gw2, wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
  }
  // the column passes' row groups, added in group order
  m.S[0 * SR_THREADS + tid] = gb1;
  m.S[1 * SR_THREADS + tid] = gb2;
  m.S[2 * SR_THREADS + tid] = ggam;
  m.S[3 * SR_THREADS + tid] = gbet;
  __syncthreads();
  if (tid < 4 * D) {
    const int k = tid / D, d = tid % D;
    float s = 0.f;
    for (int g = 0; g < S::G; ++g) s += m.S[k * SR_THREADS + g * D + d];
    part[4 * D * D + k * D + d] = s;
  }
}

// grads[i] = sum over the partials in workgroup order
__global__ __launch_bounds__(256) void sasrec_wgrad_kernel(const float *__restrict__ part, int parts,
                                                           int64_t P, float *__restrict__ grads) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= P) return;
  // eight loads in flight, added in workgroup order (the same sum, bit for bit, as one
  // load per addition: that chain of dependent round trips took 61 us over 256 partials)
  float s = 0.f;
  int g = 0;
  for (; g + 8 <= parts; g += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = part[(g + k) * P + i];
#pragma unroll
    for (int k = 0; k < 8; ++k) s += v[k];
  }
  for (; g < parts; ++g) s += part[g * P + i];
  grads[i] = s;
}

}  // namespace mrec

using namespace mrec;

namespace {

template <int D>
void sr_set_attrs() {
  for (const void *k : {reinterpret_cast<const void *>(sasrec_fwd_kernel<D>),
                        reinterpret_cast<const void *>(sasrec_bwd_kernel<D>)})
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(SrShape<D>::bytes));
  (void)hipGetLastError();
}

bool sr_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

mrec_status sr_check(const mrec_sasrec_args *a, SasrecArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his && a->his_len && a->pos && a->wq && a->wk && a->w1 && a->b1 &&
                     a->w2 && a->b2 && a->gamma && a->beta && a->hs,
                 "NULL pointer");
  MREC_CHECK_ARG(a->D == 16 || a->D == 32 || a->D == 64, "D must be 16, 32 or 64");
  MREC_CHECK_ARG(a->L >= 1 && a->L <= SR_ROWS, "need 1 <= L <= 64");
  MREC_CHECK_ARG(a->batch >= 0, "negative batch");
  MREC_CHECK_ARG(a->num_layers >= 1, "num_layers < 1");
  MREC_CHECK_ARG(a->pos_rows >= 1, "pos_rows < 1");
  MREC_CHECK_ARG(a->ld_rows >= a->D && a->ld_his >= a->L && a->ld_pos >= a->D &&
                     a->ld_wq >= a->D && a->ld_wk >= a->D && a->ld_w1 >= a->D && a->ld_w2 >= a->D,
                 "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(sr_aligned(a->rows) && a->ld_rows % 8 == 0 && sr_aligned(a->hs),
                 "rows and hs must be 16-byte aligned bf16 rows (ld_rows a multiple of 8)");
  SasrecArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his = a->his;
  p.ld_his = a->ld_his;
  p.his_len = a->his_len;
  p.pos = a->pos;
  p.ld_pos = a->ld_pos;
  p.pos_rows = a->pos_rows;
  p.wq = a->wq, p.wk = a->wk, p.w1 = a->w1, p.w2 = a->w2;
  p.ldq = a->ld_wq, p.ldk = a->ld_wk, p.ld1 = a->ld_w1, p.ld2 = a->ld_w2;
  p.b1 = a->b1, p.b2 = a->b2, p.gamma = a->gamma, p.beta = a->beta;
  p.eps = a->eps;
  p.num_layers = a->num_layers;
  p.batch = a->batch;
  p.L = a->L;
  p.hs = static_cast<uint16_t *>(a->hs);
  p.v = a->v;
  p.oob = a->d_oob_flag;
  p.dv = a->dv;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  p.P = mrec_sasrec_param_count(a->D, a->pos_rows);
  *out = p;
  return MREC_OK;
}

}  // namespace

extern "C" {

int32_t mrec_sasrec_supported(int32_t D, int32_t L) {
  return (D == 16 || D == 32 || D == 64) && L >= 1 && L <= SR_ROWS ? 1 : 0;
}

int64_t mrec_sasrec_parts(int64_t batch) {
  const int64_t g = device_cus();
  return batch < g ? (batch > 0 ? batch : 1) : g;
}

int64_t mrec_sasrec_param_count(int32_t D, int32_t pos_rows) {
  return 4 * static_cast<int64_t>(D) * D + 4 * static_cast<int64_t>(D) +
         static_cast<int64_t>(pos_rows) * D;
}

mrec_status mrec_sasrec_fwd(const mrec_sasrec_args *a, mrec_stream stream) {
  SasrecArgs p;
  const mrec_status st = sr_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(mrec_sasrec_parts(p.batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
#define X(d)                                                                         \
  if (a->D == d) {                                                                   \
    static const int once = (sr_set_attrs<d>(), 1);                                  \
    (void)once;                                                                      \
    sasrec_fwd_kernel<d><<<dim3(grid), SR_THREADS, SrShape<d>::bytes, s>>>(p);       \
    return launch_status("mrec_sasrec_fwd");                                         \
  }
  X(16) X(32) X(64)
#undef X
  return MREC_EINVAL;
}

mrec_status mrec_sasrec_bwd(const mrec_sasrec_args *a, mrec_stream stream) {
  SasrecArgs p;
  const mrec_status st = sr_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->dv && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= a->D && a->ld_drows % 8 == 0 && sr_aligned(a->d_rows),
                 "d_rows must be 16-byte aligned bf16 rows (ld_drows a multiple of 8, >= D)");
  MREC_CHECK_ARG(a->parts == mrec_sasrec_parts(a->batch), "parts must be mrec_sasrec_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define X(d)                                                                         \
  if (a->D == d) {                                                                   \
    static const int once = (sr_set_attrs<d>(), 1);                                  \
    (void)once;                                                                      \
    sasrec_bwd_kernel<d><<<dim3(grid), SR_THREADS, SrShape<d>::bytes, s>>>(p);       \
    return launch_status("mrec_sasrec_bwd");                                         \
  }
  X(16) X(32) X(64)
#undef X
  return MREC_EINVAL;
}

mrec_status mrec_sasrec_wgrad(const float *part, int64_t parts, int64_t count, float *grads,
                              mrec_stream stream) {
  MREC_CHECK_ARG(part && grads, "NULL pointer");
  MREC_CHECK_ARG(parts >= 1 && parts <= (1 << 20) && count >= 1, "no partials / no parameters");
  sasrec_wgrad_kernel<<<dim3(static_cast<unsigned>((count + 255) / 256)), 256, 0,
                        static_cast<hipStream_t>(stream)>>>(part, static_cast<int>(parts), count,
                                                            grads);
  return launch_status("mrec_sasrec_wgrad");
}

}  // extern "C"
