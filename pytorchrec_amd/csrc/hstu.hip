// HSTU encoder (Zhai et al., "Actions Speak Louder than Words", ICML 2024): causal
// multi-head pointwise SiLU attention with a learned relative-position bias and a gating
// branch, every layer with its own weights, fused per sample.
//
//   X0 = bf16(rows[b, j] + pos[(his_len - j) valid_j])        (invalid rows are zero rows)
//   per layer l   N         = bf16(LayerNorm(X; g1, be1))              (fp32 statistics)
//                 [U|V|Q|K] = bf16(SiLU(N W^T + b))                    W [4D, D]
//                 per head  S = Q_h K_h^T + rab[h, i - j]              (fp32)
//                           A = bf16(SiLU(S) att_scale) for j <= i and valid_j, else 0
//                           C_h = bf16(A V_h)
//                 G         = bf16(LayerNorm(C; g2, be2) U)
//                 X        <- bf16(X + G Wo^T + bo) at valid rows, zero rows elsewhere
//   v[b] = X[b, t_b], t_b the largest valid j
//
// Work split: layer-major per workgroup.  A persistent workgroup (8 waves) owns samples
// blockIdx.x, + gridDim.x, ...; per layer it stages that layer's five weight tiles once
// and runs all of its samples through the layer, reading hs[l - 1] (its own earlier
// stores; layer 0 reads the rows) and writing hs[l].  The weights are staged `layers`
// times per workgroup, not layers x samples times: four layers of 5 D^2 bf16 do not fit
// in LDS beside the activations at D = 64, and hs is saved for the backward anyway.
//
// All GEMMs are v_mfma_f32_16x16x32_bf16 on [64][72] bf16 LDS tiles (frag.h; L padded to
// 64 rows, D-wide operands zero-padded to the 32-wide k step).  A head's operands are
// column windows of the Q, K, V, C tiles; for dh = 16 the upper half of the k step is
// zero in the fragment (hs_frag<false, 16>).  Heads run one after another through the
// same probability tile.  The transposed products read tiles in place (lds_tr16_pair).
//
// Backward, layers in reverse, recomputing a layer from its saved input (nothing but hs
// is saved).  A sample's dX travels between layers in a per-sample fp32 scratch row
// block (`carry`); only the final d_rows is bf16.  Gradient tiles overwrite the forward
// tiles they make dead: dU over U, dC over C (same thread, same element), a head's
// dV / dQ / dK over that head's V / Q / K columns, the probabilities over G, dS over dY.
// SiLU' of the projection needs the pre-activation, which is one more N W^T into the
// same accumulator layout, multiplied lane-locally.  dW and dWo stay in MFMA
// accumulators over the workgroup's samples (80 16x16 tiles over 8 waves at D = 64: 40
// registers per lane), bias / LayerNorm gradients and d rab in per-thread registers; one
// fp32 partial per workgroup per layer, kind-major so that it splits into the stacked
// parameters: [dW | dWo | db | dbo | dg1 | dbe1 | dg2 | dbe2 | drab] x layers, then dpos.
// d rab[h, delta] is a fixed-order diagonal sum of the fp32 dS in LDS, one thread per
// delta.  No atomics: two runs give equal bits; a sample's v and d_rows depend on that
// sample alone; d_rows is bitwise zero at invalid positions.
//
// LDS (of the CU's 160 KiB), the same map both ways: 14 bf16 tiles (X N U V Q K C G/P
// dY/dS + five weights) 126 KiB, one fp32 [64][64] buffer 16 KiB, vectors 4.8 KiB:
// 146.8 KiB, one workgroup per CU.  The dX carry stays out of LDS: with it (16 KiB more)
// the backward would not fit at D = 64.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int HS_ROWS = 64;  // history positions per sample, padded
constexpr int HS_THREADS = 512;
constexpr int HS_WAVES = HS_THREADS / 64;
constexpr int HS_LD = 72;  // bf16 elements per tile row (144 B: 16-B aligned rows)
constexpr int HS_TILE = HS_ROWS * HS_LD;
constexpr int HS_F32 = HS_ROWS * 64;  // an fp32 [64][64] buffer
constexpr int HS_MAX_LAYERS = 4;

struct HstuArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const int32_t *his_len;
  const float *pos;  // position table [pos_rows, D] fp32
  int64_t ld_pos;
  int pos_rows;
  // fp32 masters, stacked per kind and contiguous: [layers, ...]
  const float *g1, *be1, *w, *b, *rab, *g2, *be2, *wo, *bo;
  int rab_cols;
  float eps, att_scale;
  int layers, H;
  int64_t batch;
  int L;
  uint16_t *hs;  // [layers, batch, L, D] bf16 layer outputs
  float *v;      // [batch, D]
  int32_t *oob;  // set to 1 on a position id outside the table (NULL: not reported)
  const float *dv;
  float *carry;  // [batch, L, D] fp32: a sample's dX between layers
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][P]
  int64_t P;
};

// tiles; U V Q K and their weights are consecutive (HS_U + part, HS_W + part)
enum { HS_X = 0, HS_N, HS_U, HS_V, HS_Q, HS_K, HS_C, HS_GP, HS_DY, HS_W, HS_WO = HS_W + 4, HS_NTILES };

// offsets of the kinds in a workgroup's partial (kind-major: kind k of layer l starts at
// off[k] + l * size[k])
struct HsPart {
  int64_t w, wo, b, bo, g1, be1, g2, be2, rab, pos, total;
  int64_t nrab;  // H * rab_cols
};
__host__ __device__ inline HsPart hs_part(int D, int H, int rab_cols, int layers, int pos_rows) {
  HsPart o;
  const int64_t n = layers;
  o.nrab = static_cast<int64_t>(H) * rab_cols;
  o.w = 0;
  o.wo = o.w + n * 4 * D * D;
  o.b = o.wo + n * D * D;
  o.bo = o.b + n * 4 * D;
  o.g1 = o.bo + n * D;
  o.be1 = o.g1 + n * D;
  o.g2 = o.be1 + n * D;
  o.be2 = o.g2 + n * D;
  o.rab = o.be2 + n * D;
  o.pos = o.rab + n * o.nrab;
  o.total = o.pos + static_cast<int64_t>(pos_rows) * D;
  return o;
}

template <int D>
struct HsShape {
  static_assert(D == 16 || D == 32 || D == 64, "compiled widths");
  static constexpr int NT = D / 16;         // column tiles of a D-wide output
  static constexpr int KS = (D + 31) / 32;  // k steps over a D-wide operand
  static constexpr int CH = D / 8;          // 16-B chunks per row; columns per lane of a row pass
  static constexpr int G = HS_THREADS / D;  // row groups of the column passes
  static constexpr size_t f32_off = static_cast<size_t>(HS_NTILES) * HS_TILE * 2;
  static constexpr int NVEC = 256 + 64 + 4 * 64 + 4 * 64 + 256;  // b bo | g1 be1 g2 be2 | stats | rab
  static constexpr size_t bytes = f32_off + HS_F32 * 4 + NVEC * 4 + (64 + 64 + 4) * 4;
};

struct HsLds {
  uint16_t *t;  // HS_NTILES bf16 tiles
  float *Z;     // fp32 [64][64]: dG, then a head's dS, then dN
  float *b, *bo, *g1, *be1, *g2, *be2, *mu1, *rstd1, *mu2, *rstd2, *rab;
  int *valid, *pos, *tb;
  __device__ uint16_t *tile(int i) const { return t + i * HS_TILE; }
};

template <int D>
__device__ __forceinline__ HsLds hs_lds(char *base) {
  HsLds m;
  m.t = reinterpret_cast<uint16_t *>(base);
  m.Z = reinterpret_cast<float *>(base + HsShape<D>::f32_off);
  m.b = m.Z + HS_F32;
  m.bo = m.b + 256;
  m.g1 = m.bo + 64;
  m.be1 = m.g1 + 64;
  m.g2 = m.be1 + 64;
  m.be2 = m.g2 + 64;
  m.mu1 = m.be2 + 64;
  m.rstd1 = m.mu1 + 64;
  m.mu2 = m.rstd1 + 64;
  m.rstd2 = m.mu2 + 64;
  m.rab = m.rstd2 + 64;
  m.valid = reinterpret_cast<int *>(m.rab + 256);
  m.pos = m.valid + 64;
  m.tb = m.pos + 64;
  return m;
}

// operand fragment of rows r0 .. r0 + 15, k0 .. k0 + 31: element (r, k) is base[r][k], or
// base[k][r] with TR (the tile holds the operand transposed).  KW = 16: a 16-wide
// operand, the upper half of the k step is zero.
template <bool TR, int KW = 32>
__device__ __forceinline__ bf16x8 hs_frag(const uint16_t *base, int r0, int k0, int lane) {
  const int r = r0 + (lane & 15), k = k0 + 8 * (lane >> 4);
  if constexpr (!TR) {
    if (KW == 16 && (lane >> 4) >= 2) return frag_zero8();
    return *reinterpret_cast<const bf16x8 *>(base + r * HS_LD + k);
  } else {
    static_assert(KW == 32, "transposed operands run over the 64 rows");
    // two transposing reads (frag.h): tile rows k .. + 3 and k + 4 .. + 7 are the lane's
    // 8 k values; every address lies inside the tile
    const int li = lane & 15;
    const uint16_t *p = base + (k + (li >> 2)) * HS_LD + r0 + 4 * (li & 3);
    return lds_tr16_pair(p, 4 * HS_LD);
  }
}

// An [16 MT, 16 NT] product's tiles t = wave, wave + 8, ... (tile t: rows 16 (t / NT),
// columns 16 (t % NT)); acc[i] += A[rows, :] . B[columns, :] over KS k steps.
template <int MT, int NT>
struct HsAcc {
  static constexpr int N = (MT * NT + HS_WAVES - 1) / HS_WAVES;
  f32x4 a[N];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
};

// LOWER: only the tiles on and below the diagonal (the causal scores)
template <int MT, int NT, int KS, bool TA, bool TB, int KW = 32, bool LOWER = false>
__device__ __forceinline__ void hs_mma(const uint16_t *A, const uint16_t *B, int wave, int lane,
                                       HsAcc<MT, NT> &acc) {
#pragma unroll
  for (int i = 0; i < HsAcc<MT, NT>::N; ++i) {
    const int t = wave + HS_WAVES * i;
    if (t < MT * NT) {
      const int mt = t / NT, nt = t % NT;
      if (LOWER && nt > mt) continue;
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc.a[i] = mfma_16x16x32(hs_frag<TA, KW>(A, 16 * mt, 32 * s, lane),
                                 hs_frag<TB, KW>(B, 16 * nt, 32 * s, lane), acc.a[i]);
    }
  }
}

// f(row, column, value) for every element this lane holds
template <int MT, int NT, class F>
__device__ __forceinline__ void hs_each(const HsAcc<MT, NT> &acc, int wave, int lane, F f) {
#pragma unroll
  for (int i = 0; i < HsAcc<MT, NT>::N; ++i) {
    const int t = wave + HS_WAVES * i;
    if (t < MT * NT) {
      const int mt = t / NT, nt = t % NT;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        f(16 * mt + 4 * (lane >> 4) + e, 16 * nt + (lane & 15), acc.a[i][e]);
    }
  }
}

// sum over the 8 lanes of a row pass (lanes 8 q .. 8 q + 7), every lane gets it
__device__ __forceinline__ float hs_sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}

__device__ __forceinline__ float hs_silu(float x) { return x * sigmoid_stable(x); }
// SiLU'(x) = s + x s (1 - s)
__device__ __forceinline__ float hs_dsilu(float x) { return sigmoid_stable(x) + x * dsigmoid_stable(x); }


// zero the whole LDS (once per workgroup): tile rows and columns no pass writes stay zero
template <int D>
__device__ void hs_clear(char *base, int tid) {
  for (size_t o = static_cast<size_t>(tid) * 16; o < HsShape<D>::bytes; o += HS_THREADS * 16)
    *reinterpret_cast<uint4 *>(base + o) = make_uint4(0, 0, 0, 0);
  __syncthreads();
}

// layer l's five weight matrices as bf16 tiles and its vectors (once per workgroup and
// layer).  Starts and ends at a barrier.
template <int D>
__device__ void hs_stage(const HstuArgs &p, const HsLds &m, int l, int tid) {
  __syncthreads();
  const float *w = p.w + static_cast<int64_t>(l) * 4 * D * D;
  const float *wo = p.wo + static_cast<int64_t>(l) * D * D;
  for (int i = tid; i < D * D; i += HS_THREADS) {
    const int n = i / D, k = i % D;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      m.tile(HS_W + q)[n * HS_LD + k] = f32_to_bf16_rne(w[(q * D + n) * D + k]);
    m.tile(HS_WO)[n * HS_LD + k] = f32_to_bf16_rne(wo[i]);
  }
  if (tid < 4 * D) m.b[tid] = p.b[static_cast<int64_t>(l) * 4 * D + tid];
  if (tid < D) {
    const int64_t o = static_cast<int64_t>(l) * D + tid;
    m.bo[tid] = p.bo[o];
    m.g1[tid] = p.g1[o];
    m.be1[tid] = p.be1[o];
    m.g2[tid] = p.g2[o];
    m.be2[tid] = p.be2[o];
  }
  if (tid < 4 * 64) {  // rab[h][delta] for delta < 64 (a sample reads delta <= L - 1)
    const int h = tid >> 6, d = tid & 63;
    m.rab[tid] = h < p.H && d < p.rab_cols
                     ? p.rab[(static_cast<int64_t>(l) * p.H + h) * p.rab_cols + d]
                     : 0.f;
  }
  __syncthreads();
}

// validity and position id of every history position of sample b (pos < 0: no row), and
// t_b, the largest valid position.  Ends at a barrier.
__device__ __forceinline__ void hs_meta(const HstuArgs &p, int64_t b, const HsLds &m, int tid) {
  if (tid < HS_ROWS) {
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
    const unsigned long long mk = __ballot(ok);  // wave 0, all 64 lanes; bit 0 is always set
    if (j == 0) m.tb[0] = 63 - __clzll(static_cast<long long>(mk));
  }
  __syncthreads();
}

// X tile <- layer 0's input: bf16(item row + position row) at valid positions, else 0
template <int D>
__device__ __forceinline__ void hs_load_x0(const HstuArgs &p, int64_t b, const HsLds &m, int tid) {
  constexpr int CH = HsShape<D>::CH;
  for (int t = tid; t < HS_ROWS * CH; t += HS_THREADS) {
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
    *reinterpret_cast<uint4 *>(m.tile(HS_X) + j * HS_LD + c) = out;
  }
}

// X tile <- a saved layer output (rows j < L; the others zero)
template <int D>
__device__ __forceinline__ void hs_load_hs(const uint16_t *src, int L, const HsLds &m, int tid) {
  constexpr int CH = HsShape<D>::CH;
  for (int t = tid; t < HS_ROWS * CH; t += HS_THREADS) {
    const int j = t / CH, c = (t % CH) * 8;
    uint4 out = make_uint4(0, 0, 0, 0);
    if (j < L) out = *reinterpret_cast<const uint4 *>(src + j * D + c);
    *reinterpret_cast<uint4 *>(m.tile(HS_X) + j * HS_LD + c) = out;
  }
}

template <int D>
__device__ __forceinline__ void hs_load_x(const HstuArgs &p, int64_t b, int l, const HsLds &m, int tid) {
  if (l == 0)
    hs_load_x0<D>(p, b, m, tid);
  else
    hs_load_hs<D>(p.hs + ((static_cast<int64_t>(l - 1) * p.batch + b) * p.L) * D, p.L, m, tid);
  __syncthreads();
}

// One layer's forward on the X tile up to the gated tile: fills N, U, V, Q, K, C, the
// LayerNorm statistics and G (in the G/P tile, which holds each head's probabilities
// before).  Starts and ends at a barrier.
template <int D, int DH>
__device__ __forceinline__ void hs_layer(const HstuArgs &p, const HsLds &m, int tid) {
  using S = HsShape<D>;
  constexpr int NT = S::NT, KS = S::KS, H = D / DH, NTH = DH / 16, KSH = (DH + 31) / 32;
  constexpr int KW = DH == 16 ? 16 : 32;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 3, sub = tid & 7;  // the row passes: 8 lanes per row
  {  // N = LayerNorm(X) (biased variance)
    float x[S::CH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) {
      x[i] = bf16_to_f32(m.tile(HS_X)[r * HS_LD + sub + 8 * i]);
      s += x[i];
    }
    const float mu = hs_sum8(s) * (1.f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) q += (x[i] - mu) * (x[i] - mu);
    const float rstd = rsqrtf(hs_sum8(q) * (1.f / D) + p.eps);
    if (sub == 0) {
      m.mu1[r] = mu;
      m.rstd1[r] = rstd;
    }
#pragma unroll
    for (int i = 0; i < S::CH; ++i) {
      const int c = sub + 8 * i;
      m.tile(HS_N)[r * HS_LD + c] = f32_to_bf16_rne((x[i] - mu) * rstd * m.g1[c] + m.be1[c]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // U, V, Q, K = SiLU(N W_q^T + b_q)
    HsAcc<4, NT> a;
    a.zero();
    hs_mma<4, NT, KS, false, false>(m.tile(HS_N), m.tile(HS_W + q), wave, lane, a);
    uint16_t *t = m.tile(HS_U + q);
    const float *bq = m.b + q * D;
    hs_each<4, NT>(a, wave, lane, [&](int i, int c, float x) {
      t[i * HS_LD + c] = f32_to_bf16_rne(hs_silu(x + bq[c]));
    });
  }
  __syncthreads();
  for (int h = 0; h < H; ++h) {
    {  // A = SiLU(Q_h K_h^T + rab) att_scale at j <= i, valid_j; exactly 0 elsewhere
      HsAcc<4, 4> s;
      s.zero();
      hs_mma<4, 4, KSH, false, false, KW, true>(m.tile(HS_Q) + h * DH, m.tile(HS_K) + h * DH, wave,
                                                lane, s);
      uint16_t *tp = m.tile(HS_GP);
      const float *rab = m.rab + h * 64;
      const float sc = p.att_scale;
      hs_each<4, 4>(s, wave, lane, [&](int i, int j, float x) {
        const bool ok = j <= i && m.valid[j];
        tp[i * HS_LD + j] = ok ? f32_to_bf16_rne(hs_silu(x + rab[i - j]) * sc) : uint16_t(0);
      });
    }
    __syncthreads();
    {  // C_h = A V_h
      HsAcc<4, NTH> c;
      c.zero();
      hs_mma<4, NTH, 2, false, true>(m.tile(HS_GP), m.tile(HS_V) + h * DH, wave, lane, c);
      uint16_t *tc = m.tile(HS_C) + h * DH;
      hs_each<4, NTH>(c, wave, lane, [&](int i, int j, float x) { tc[i * HS_LD + j] = f32_to_bf16_rne(x); });
    }
    __syncthreads();
  }
  {  // G = LayerNorm(C) U
    float x[S::CH];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) {
      x[i] = bf16_to_f32(m.tile(HS_C)[r * HS_LD + sub + 8 * i]);
      s += x[i];
    }
    const float mu = hs_sum8(s) * (1.f / D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < S::CH; ++i) q += (x[i] - mu) * (x[i] - mu);
    const float rstd = rsqrtf(hs_sum8(q) * (1.f / D) + p.eps);
    if (sub == 0) {
      m.mu2[r] = mu;
      m.rstd2[r] = rstd;
    }
#pragma unroll
    for (int i = 0; i < S::CH; ++i) {
      const int c = sub + 8 * i;
      const float u = bf16_to_f32(m.tile(HS_U)[r * HS_LD + c]);
      m.tile(HS_GP)[r * HS_LD + c] = f32_to_bf16_rne(((x[i] - mu) * rstd * m.g2[c] + m.be2[c]) * u);
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D, int DH>
__global__ __launch_bounds__(HS_THREADS, 1) void hstu_fwd_kernel(HstuArgs p) {
  using S = HsShape<D>;
  extern __shared__ __attribute__((aligned(16))) char hs_smem[];
  const HsLds m = hs_lds<D>(hs_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  hs_clear<D>(hs_smem, tid);
  for (int l = 0; l < p.layers; ++l) {
    hs_stage<D>(p, m, l, tid);
    for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
      hs_meta(p, b, m, tid);
      hs_load_x<D>(p, b, l, m, tid);
      hs_layer<D, DH>(p, m, tid);
      {  // X <- X + G Wo^T + bo at valid rows, zero rows elsewhere (each lane its own elements)
        HsAcc<4, S::NT> y;
        y.zero();
        hs_mma<4, S::NT, S::KS, false, false>(m.tile(HS_GP), m.tile(HS_WO), wave, lane, y);
        uint16_t *tx = m.tile(HS_X);
        hs_each<4, S::NT>(y, wave, lane, [&](int i, int c, float x) {
          tx[i * HS_LD + c] =
              m.valid[i] ? f32_to_bf16_rne(bf16_to_f32(tx[i * HS_LD + c]) + (x + m.bo[c])) : uint16_t(0);
        });
      }
      __syncthreads();
      uint16_t *dst = p.hs + ((static_cast<int64_t>(l) * p.batch + b) * p.L) * D;
      for (int t = tid; t < p.L * S::CH; t += HS_THREADS) {
        const int j = t / S::CH, c = (t % S::CH) * 8;
        *reinterpret_cast<uint4 *>(dst + j * D + c) =
            *reinterpret_cast<const uint4 *>(m.tile(HS_X) + j * HS_LD + c);
      }
      if (l == p.layers - 1 && tid < D)
        p.v[b * D + tid] = bf16_to_f32(m.tile(HS_X)[m.tb[0] * HS_LD + tid]);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int D, int DH>
__global__ __launch_bounds__(HS_THREADS, 1) void hstu_bwd_kernel(HstuArgs p) {
  using S = HsShape<D>;
  constexpr int NT = S::NT, KS = S::KS, H = D / DH, NTH = DH / 16, KSH = (DH + 31) / 32;
  constexpr int KW = DH == 16 ? 16 : 32;
  extern __shared__ __attribute__((aligned(16))) char hs_smem[];
  const HsLds m = hs_lds<D>(hs_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 3, sub = tid & 7;  // row passes
  const int cd = tid % D, cg = tid / D;   // column passes: column cd, rows cg, cg + G, ...
  const HsPart off = hs_part(D, H, p.rab_cols, p.layers, p.pos_rows);
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * p.P;
  float *part_pos = part + off.pos;
  hs_clear<D>(hs_smem, tid);
  for (int i = tid; i < p.pos_rows * D; i += HS_THREADS) part_pos[i] = 0.f;
  for (int l = p.layers - 1; l >= 0; --l) {
    const bool last = l == p.layers - 1;
    hs_stage<D>(p, m, l, tid);
    HsAcc<NT, NT> gw[4], gwo;
#pragma unroll
    for (int q = 0; q < 4; ++q) gw[q].zero();
    gwo.zero();
    float gb[4] = {0.f, 0.f, 0.f, 0.f};
    float gbo = 0.f, gg1 = 0.f, gbe1 = 0.f, gg2 = 0.f, gbe2 = 0.f, grab = 0.f;
    for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
      hs_meta(p, b, m, tid);
      hs_load_x<D>(p, b, l, m, tid);
      hs_layer<D, DH>(p, m, tid);
      // dY, the gradient of this layer's output: dv at row t_b for the last layer, the
      // carry below it; zero at rows j >= L (invalid rows of the carry are stored as zero)
      const float *cy = p.carry + b * p.L * D;
      const int tb = m.tb[0];
      auto dy = [&](int j, int c) -> float {
        if (j >= p.L) return 0.f;
        if (last) return j == tb ? p.dv[b * D + c] : 0.f;
        return cy[j * D + c];
      };
      // dbo, and dY as a bf16 tile
      for (int j = cg; j < HS_ROWS; j += S::G) {
        const float g = dy(j, cd);
        gbo += g;
        m.tile(HS_DY)[j * HS_LD + cd] = f32_to_bf16_rne(g);
      }
      __syncthreads();
      // Y = X + G Wo^T + bo: dWo += dY^T G, dG = dY Wo -> Z
      hs_mma<NT, NT, 2, true, true>(m.tile(HS_DY), m.tile(HS_GP), wave, lane, gwo);
      {
        HsAcc<4, NT> a;
        a.zero();
        hs_mma<4, NT, KS, false, true>(m.tile(HS_DY), m.tile(HS_WO), wave, lane, a);
        float *z = m.Z;
        hs_each<4, NT>(a, wave, lane, [&](int i, int c, float x) { z[i * 64 + c] = x; });
      }
      __syncthreads();
      // G = LayerNorm(C) U: dg2, dbe2 (column pass), then dU over U and dC over C (row pass)
      for (int j = cg; j < HS_ROWS; j += S::G) {
        const float d = m.Z[j * 64 + cd] * bf16_to_f32(m.tile(HS_U)[j * HS_LD + cd]);
        gg2 = fmaf(d, (bf16_to_f32(m.tile(HS_C)[j * HS_LD + cd]) - m.mu2[j]) * m.rstd2[j], gg2);
        gbe2 += d;
      }
      __syncthreads();
      {
        const float mu = m.mu2[r], rs = m.rstd2[r];
        float g[S::CH], xh[S::CH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < S::CH; ++i) {
          const int c = sub + 8 * i;
          const float dg = m.Z[r * 64 + c];
          const float u = bf16_to_f32(m.tile(HS_U)[r * HS_LD + c]);
          xh[i] = (bf16_to_f32(m.tile(HS_C)[r * HS_LD + c]) - mu) * rs;
          m.tile(HS_U)[r * HS_LD + c] = f32_to_bf16_rne(dg * (xh[i] * m.g2[c] + m.be2[c]));
          g[i] = dg * u * m.g2[c];
          s1 += g[i];
          s2 = fmaf(g[i], xh[i], s2);
        }
        s1 = hs_sum8(s1) * (1.f / D);
        s2 = hs_sum8(s2) * (1.f / D);
#pragma unroll
        for (int i = 0; i < S::CH; ++i)
          m.tile(HS_C)[r * HS_LD + sub + 8 * i] = f32_to_bf16_rne(rs * (g[i] - s1 - xh[i] * s2));
      }
      __syncthreads();
      for (int h = 0; h < H; ++h) {
        {  // the head's scores again and dA = dC_h V_h^T: A -> P, dS -> dY tile and Z (fp32)
          HsAcc<4, 4> s, da;
          s.zero();
          da.zero();
          hs_mma<4, 4, KSH, false, false, KW, true>(m.tile(HS_Q) + h * DH, m.tile(HS_K) + h * DH,
                                                    wave, lane, s);
          hs_mma<4, 4, KSH, false, false, KW, true>(m.tile(HS_C) + h * DH, m.tile(HS_V) + h * DH,
                                                    wave, lane, da);
          const float *rab = m.rab + h * 64;
          const float sc = p.att_scale;
#pragma unroll
          for (int i = 0; i < HsAcc<4, 4>::N; ++i) {
            const int t = wave + HS_WAVES * i, mt = t / 4, nt = t % 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int row = 16 * mt + 4 * (lane >> 4) + e, col = 16 * nt + (lane & 15);
              const bool ok = col <= row && m.valid[col];
              float a = 0.f, ds = 0.f;
              if (ok) {
                const float x = s.a[i][e] + rab[row - col];
                a = hs_silu(x) * sc;
                ds = da.a[i][e] * sc * hs_dsilu(x);
              }
              m.tile(HS_GP)[row * HS_LD + col] = f32_to_bf16_rne(a);
              m.tile(HS_DY)[row * HS_LD + col] = f32_to_bf16_rne(ds);
              m.Z[row * 64 + col] = ds;
            }
          }
        }
        __syncthreads();
        // dV_h = A^T dC_h, dQ_h = dS K_h, dK_h = dS^T Q_h (registers), d rab (diagonal sums)
        HsAcc<4, NTH> dvh, dqh, dkh;
        dvh.zero();
        dqh.zero();
        dkh.zero();
        hs_mma<4, NTH, 2, true, true>(m.tile(HS_GP), m.tile(HS_C) + h * DH, wave, lane, dvh);
        hs_mma<4, NTH, 2, false, true>(m.tile(HS_DY), m.tile(HS_K) + h * DH, wave, lane, dqh);
        hs_mma<4, NTH, 2, true, true>(m.tile(HS_DY), m.tile(HS_Q) + h * DH, wave, lane, dkh);
        if ((tid >> 6) == h) {  // one thread per delta, rows in order
          const int delta = tid & 63;
          float s = 0.f;
          for (int i = delta; i < HS_ROWS; ++i) s += m.Z[i * 64 + i - delta];
          grab += s;
        }
        __syncthreads();
        {  // over the head's V, Q, K columns, which nothing reads any more
          uint16_t *tv = m.tile(HS_V) + h * DH, *tq = m.tile(HS_Q) + h * DH, *tk = m.tile(HS_K) + h * DH;
          hs_each<4, NTH>(dvh, wave, lane, [&](int i, int c, float x) { tv[i * HS_LD + c] = f32_to_bf16_rne(x); });
          hs_each<4, NTH>(dqh, wave, lane, [&](int i, int c, float x) { tq[i * HS_LD + c] = f32_to_bf16_rne(x); });
          hs_each<4, NTH>(dkh, wave, lane, [&](int i, int c, float x) { tk[i * HS_LD + c] = f32_to_bf16_rne(x); });
        }
      }
      __syncthreads();
      // SiLU of the projection: the pre-activation again, dZ_q = dP_q SiLU'(z) in place
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        HsAcc<4, NT> a;
        a.zero();
        hs_mma<4, NT, KS, false, false>(m.tile(HS_N), m.tile(HS_W + q), wave, lane, a);
        uint16_t *t = m.tile(HS_U + q);
        const float *bq = m.b + q * D;
        hs_each<4, NT>(a, wave, lane, [&](int i, int c, float x) {
          t[i * HS_LD + c] = f32_to_bf16_rne(bf16_to_f32(t[i * HS_LD + c]) * hs_dsilu(x + bq[c]));
        });
      }
      __syncthreads();
      // db, dW_q += dZ_q^T N, dN = sum_q dZ_q W_q -> Z
#pragma unroll
      for (int q = 0; q < 4; ++q)
        for (int j = cg; j < HS_ROWS; j += S::G) gb[q] += bf16_to_f32(m.tile(HS_U + q)[j * HS_LD + cd]);
      {
        HsAcc<4, NT> a;
        a.zero();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          hs_mma<NT, NT, 2, true, true>(m.tile(HS_U + q), m.tile(HS_N), wave, lane, gw[q]);
          hs_mma<4, NT, KS, false, true>(m.tile(HS_U + q), m.tile(HS_W + q), wave, lane, a);
        }
        float *z = m.Z;
        hs_each<4, NT>(a, wave, lane, [&](int i, int c, float x) { z[i * 64 + c] = x; });
      }
      __syncthreads();
      // N = LayerNorm(X): dg1, dbe1 (column pass), dX = dY + the LayerNorm's input gradient
      for (int j = cg; j < HS_ROWS; j += S::G) {
        const float d = m.Z[j * 64 + cd];
        gg1 = fmaf(d, (bf16_to_f32(m.tile(HS_X)[j * HS_LD + cd]) - m.mu1[j]) * m.rstd1[j], gg1);
        gbe1 += d;
      }
      {
        const float mu = m.mu1[r], rs = m.rstd1[r];
        const bool ok = m.valid[r] != 0;  // (false at rows >= L)
        const int pos = m.pos[r];
        float g[S::CH], xh[S::CH];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < S::CH; ++i) {
          const int c = sub + 8 * i;
          g[i] = m.Z[r * 64 + c] * m.g1[c];
          xh[i] = (bf16_to_f32(m.tile(HS_X)[r * HS_LD + c]) - mu) * rs;
          s1 += g[i];
          s2 = fmaf(g[i], xh[i], s2);
        }
        s1 = hs_sum8(s1) * (1.f / D);
        s2 = hs_sum8(s2) * (1.f / D);
        if (r < p.L) {
#pragma unroll
          for (int i = 0; i < S::CH; ++i) {
            const int c = sub + 8 * i;
            // invalid rows are zero rows whatever came before: no gradient passes them
            const float dx = ok ? dy(r, c) + rs * (g[i] - s1 - xh[i] * s2) : 0.f;
            if (l > 0) {
              p.carry[(b * p.L + r) * D + c] = dx;
            } else {
              // layer 0: the rows' gradient and the position rows' (a sample's valid
              // positions have distinct ids: no two threads meet)
              p.drows[(b * p.L + r) * p.ld_drows + c] = ok ? f32_to_bf16_rne(dx) : uint16_t(0);
              if (ok && pos >= 0) part_pos[pos * D + c] += dx;
            }
          }
        }
      }
      __syncthreads();
    }
    // the layer's share of the workgroup's partial
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float *o = part + off.w + (static_cast<int64_t>(l) * 4 + q) * D * D;
      hs_each<NT, NT>(gw[q], wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
    }
    {
      float *o = part + off.wo + static_cast<int64_t>(l) * D * D;
      hs_each<NT, NT>(gwo, wave, lane, [&](int i, int c, float x) { o[i * D + c] = x; });
    }
    // the column passes' row groups, added in group order (Z holds one register of every
    // thread at a time)
    auto cols = [&](float x, float *dst) {
      m.Z[tid] = x;
      __syncthreads();
      if (tid < D) {
        float s = 0.f;
        for (int g = 0; g < S::G; ++g) s += m.Z[g * D + tid];
        dst[tid] = s;
      }
      __syncthreads();
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) cols(gb[q], part + off.b + (static_cast<int64_t>(l) * 4 + q) * D);
    cols(gbo, part + off.bo + static_cast<int64_t>(l) * D);
    cols(gg1, part + off.g1 + static_cast<int64_t>(l) * D);
    cols(gbe1, part + off.be1 + static_cast<int64_t>(l) * D);
    cols(gg2, part + off.g2 + static_cast<int64_t>(l) * D);
    cols(gbe2, part + off.be2 + static_cast<int64_t>(l) * D);
    // d rab[h][delta]: thread 64 h + delta holds it; columns past 63 were never read
    m.Z[tid] = grab;
    __syncthreads();
    for (int i = tid; i < H * p.rab_cols; i += HS_THREADS) {
      const int h = i / p.rab_cols, d = i % p.rab_cols;
      part[off.rab + static_cast<int64_t>(l) * off.nrab + i] = d < 64 ? m.Z[h * 64 + d] : 0.f;
    }
  }
}

}  // namespace mrec

using namespace mrec;

namespace {

template <int D, int DH>
void hs_set_attrs() {
  for (const void *k : {reinterpret_cast<const void *>(hstu_fwd_kernel<D, DH>),
                        reinterpret_cast<const void *>(hstu_bwd_kernel<D, DH>)})
    (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize,
                              static_cast<int>(HsShape<D>::bytes));
  (void)hipGetLastError();
}

bool hs_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

mrec_status hs_check(const mrec_hstu_args *a, HstuArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his && a->his_len && a->pos && a->norm1_w && a->norm1_b && a->w &&
                     a->b && a->rab && a->norm2_w && a->norm2_b && a->wo && a->bo && a->hs,
                 "NULL pointer");
  MREC_CHECK_ARG(mrec_hstu_supported(a->D, a->H, a->L, a->num_layers),
                 "need D in {16, 32, 64}, D / H in {16, 32, 64}, 1 <= L <= 64, 1 <= num_layers <= 4");
  MREC_CHECK_ARG(a->batch >= 0, "negative batch");
  MREC_CHECK_ARG(a->pos_rows >= 1, "pos_rows < 1");
  MREC_CHECK_ARG(a->rab_cols >= a->L, "rab_cols is smaller than L");
  MREC_CHECK_ARG(a->ld_rows >= a->D && a->ld_his >= a->L && a->ld_pos >= a->D,
                 "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(hs_aligned(a->rows) && a->ld_rows % 8 == 0 && hs_aligned(a->hs),
                 "rows and hs must be 16-byte aligned bf16 rows (ld_rows a multiple of 8)");
  HstuArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his = a->his;
  p.ld_his = a->ld_his;
  p.his_len = a->his_len;
  p.pos = a->pos;
  p.ld_pos = a->ld_pos;
  p.pos_rows = a->pos_rows;
  p.g1 = a->norm1_w, p.be1 = a->norm1_b, p.w = a->w, p.b = a->b, p.rab = a->rab;
  p.g2 = a->norm2_w, p.be2 = a->norm2_b, p.wo = a->wo, p.bo = a->bo;
  p.rab_cols = a->rab_cols;
  p.eps = a->eps;
  p.att_scale = a->att_scale;
  p.layers = a->num_layers;
  p.H = a->H;
  p.batch = a->batch;
  p.L = a->L;
  p.hs = static_cast<uint16_t *>(a->hs);
  p.v = a->v;
  p.oob = a->d_oob_flag;
  p.dv = a->dv;
  p.carry = a->carry;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  p.P = mrec_hstu_param_count(a->D, a->H, a->num_layers, a->rab_cols, a->pos_rows);
  *out = p;
  return MREC_OK;
}

// f(D, dh) as integral constants for a supported (D, H)
template <typename Fn>
bool hs_dispatch(int D, int H, Fn &&f) {
  const int dh = D / H;
#define X(d, e)                                                                          \
  if (D == d && dh == e) {                                                               \
    f(std::integral_constant<int, d>{}, std::integral_constant<int, e>{});               \
    return true;                                                                         \
  }
  X(16, 16) X(32, 16) X(32, 32) X(64, 16) X(64, 32) X(64, 64)
#undef X
  return false;
}

}  // namespace

extern "C" {

int32_t mrec_hstu_supported(int32_t D, int32_t H, int32_t L, int32_t num_layers) {
  if (!(D == 16 || D == 32 || D == 64) || H < 1 || D % H != 0) return 0;
  const int dh = D / H;
  return (dh == 16 || dh == 32 || dh == 64) && L >= 1 && L <= HS_ROWS && num_layers >= 1 &&
                 num_layers <= HS_MAX_LAYERS
             ? 1
             : 0;
}

int64_t mrec_hstu_parts(int64_t batch) {
  const int64_t g = device_cus();
  return batch < g ? (batch > 0 ? batch : 1) : g;
}

int64_t mrec_hstu_param_count(int32_t D, int32_t H, int32_t num_layers, int32_t rab_cols,
                              int32_t pos_rows) {
  return hs_part(D, H, rab_cols, num_layers, pos_rows).total;
}

mrec_status mrec_hstu_fwd(const mrec_hstu_args *a, mrec_stream stream) {
  HstuArgs p;
  const mrec_status st = hs_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(mrec_hstu_parts(p.batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hs_dispatch(a->D, a->H, [&](auto d, auto e) {
    constexpr int D = decltype(d)::value, DH = decltype(e)::value;
    static const int once = (hs_set_attrs<D, DH>(), 1);
    (void)once;
    hstu_fwd_kernel<D, DH><<<dim3(grid), HS_THREADS, HsShape<D>::bytes, s>>>(p);
  });
  return launch_status("mrec_hstu_fwd");
}

mrec_status mrec_hstu_bwd(const mrec_hstu_args *a, mrec_stream stream) {
  HstuArgs p;
  const mrec_status st = hs_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->dv && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->carry || a->num_layers == 1, "NULL pointer (carry)");
  MREC_CHECK_ARG(a->ld_drows >= a->D && a->ld_drows % 8 == 0 && hs_aligned(a->d_rows),
                 "d_rows must be 16-byte aligned bf16 rows (ld_drows a multiple of 8, >= D)");
  MREC_CHECK_ARG(a->parts == mrec_hstu_parts(a->batch), "parts must be mrec_hstu_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hs_dispatch(a->D, a->H, [&](auto d, auto e) {
    constexpr int D = decltype(d)::value, DH = decltype(e)::value;
    static const int once = (hs_set_attrs<D, DH>(), 1);
    (void)once;
    hstu_bwd_kernel<D, DH><<<dim3(grid), HS_THREADS, HsShape<D>::bytes, s>>>(p);
  });
  return launch_status("mrec_hstu_bwd");
}

}  // extern "C"
