// DIEN interest evolution (Zhou et al., AAAI 2019): an interest-extractor GRU, a softmax
// attention over its states and an attention-gated GRU (AUGRU), one launch each way.
//
//   per sample, t = 0 .. his_len - 1, h1_-1 = h2_-1 = 0:
//   layer 1   h1_t = GRU1(x_t, h1_{t-1})                       (gru.hip's equations)
//   scores    s_t = h1_t . p,  a = softmax_t(s) over t < his_len (fp32, own maximum)
//   layer 2   r, z, n as a GRU on (bf16(h1_t), h2_{t-1});  u_t = a_t (1 - z_t)
//             h2_t = h2_{t-1} + u_t (n_t - h2_{t-1});          v = h2_{his_len - 1}
//
// Work split: gru.hip's.  A workgroup takes a tile of 16 samples (the rows of
// v_mfma_f32_16x16x32_bf16), its H / 16 waves each own 16 hidden units of all three
// gates, the fp32 state and the wave's bf16 weight slices stay in registers over the
// sequence, bf16(h_t) goes through a double-buffered LDS tile with one barrier per step.
// Both layers are ONE recurrence body (au_recur_fwd / au_recur_bwd), instantiated twice
// per kernel: <E, H, false> reads bf16 rows, <H, H, true> reads the fp32 hidden sequence
// of layer 1 and gates the update with a_t.  The two instances run one after the other,
// so their weight registers (and, backward, their accumulators) take turns.
//
// A tile's samples never meet another tile's, so the three stages need no grid-wide
// dependency: a workgroup reads back only what it wrote itself (hs1 forward, the
// workspace backward), after a barrier, which at workgroup scope also orders its global
// stores before its loads (one CU, one vector L1, write-through).
//
// Forward, per tile:
//   1. layer 1 over t: hs1 (live positions; dead ones are written as zero once).  The
//      partial score of a wave's 16 units is a DPP sum inside the 16-lane row -> LDS
//      s_sc[wave][16][t]; the waves' partials are added in wave order in phase 2.
//   2. softmax in LDS by wave 0: 4 lanes per sample, 16 positions per lane -> s_att, a.
//   3. layer 2 over t: A fragments are the fp32 hs1 rows, two 16-B loads per k step
//      issued one step ahead and rounded at use; a_t from LDS; hs2 saved; v.
// Backward, per tile:
//   1. layer 2 from the longest length - 1 down, gates recomputed from hs2[t - 1] and
//      hs1[t] with the forward's MFMAs; dGx2 W_ih2 -> workspace [B, L, H] fp32;
//      da_t = sum_units dh2 (1 - z)(n - h2_{t-1}): DPP row sums -> LDS s_red[wave][16][t].
//   2. ds_t = a_t (da_t - sum a da) in LDS (wave 0); dp = sum_t ds_t h1_t (every thread:
//      one sample's four units).
//   3. layer 1, with workspace[t] + ds_t p + d_hs1[t] added to the carried dh at every
//      step (loaded one step ahead).
//   Each instance adds its accumulators to the workgroup's own partial when it ends
//   (first tile: stores), so at E = H = 64 the 96 weight + 96 accumulator VGPRs of one
//   layer never coexist with the other's.  Partial [parts][P]: layer 1's
//   [dW_ih | dW_hh | db_ih | db_hh], then layer 2's; summed in workgroup order by
//   mrec_sasrec_wgrad.  No atomics: every output has equal bits from run to run.
//
// `order`, his_len outside 1..L, the out-of-bounds flag: as mrec_gru.
#include <type_traits>

#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int AU_TILE = 16;  // samples per workgroup tile (the MFMA's rows)
constexpr int AU_MAXL = 64;
constexpr int AU_LS = 68;    // floats per sample row of the [16][L] LDS arrays (68 mod 32 = 4:
                             // the softmax's 4-lanes-per-sample reads are 2-way at worst)

struct AuLayer {
  const float *w_ih, *w_hh;  // fp32 masters [3H, in], [3H, H] (gates r, z, n)
  int64_t ld_ih, ld_hh;
  const float *b_ih, *b_hh;
};

struct AuArgs {
  const uint16_t *rows;  // x [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his_len;
  const int32_t *order;  // tile slot -> sample, or NULL
  const float *pq;       // attention query [batch, H]
  int64_t ld_p;
  AuLayer l1, l2;
  int L;
  int64_t batch, tiles;
  float *hs1, *hs2;  // [batch, L, H] fp32
  float *att;        // [batch, L]
  float *v;          // [batch, H]
  int32_t *oob;
  const float *dv, *d_hs1;
  float *ws;  // [batch, L, H]: layer 2's input gradient
  uint16_t *drows;
  int64_t ld_drows;
  float *dp;
  int64_t ld_dp;
  float *part;  // [gridDim.x][P]
  int64_t P;
};

template <int EI, int H>
struct AuShape {
  static_assert((EI == 16 || EI == 32 || EI == 64) && (H == 16 || H == 32 || H == 64), "compiled widths");
  static constexpr int NW = H / 16;            // waves: 16 hidden units each
  static constexpr int NT = 64 * NW;           // threads
  static constexpr int KSE = (EI + 31) / 32;   // k steps over the input
  static constexpr int KSH = (H + 31) / 32;    // k steps over h
  static constexpr int KG = (3 * H + 31) / 32 * 32;  // dG columns, padded to the k step
  static constexpr int KSG = KG / 32;
  static constexpr int CT = EI / 16;                 // column tiles of dx / dW_ih
  static constexpr int CTW = (CT + NW - 1) / NW;     // dx column tiles per wave
  static constexpr int LDX = EI + 8, LDH = H + 8, LDG = KG + 8;  // bf16 elements per LDS row
  static constexpr int CHX = EI / 8;                 // 8-element chunks of an input row
  static constexpr int XI = (AU_TILE * CHX + NT - 1) / NT;  // input chunks a thread stages
  static constexpr int64_t PL = 3 * static_cast<int64_t>(H) * (EI + H + 2);  // a layer's partial
};

// gru.hip's forms (v_exp_f32, v_rcp_f32): both go to their limits without inf / inf, and
// forward and backward share them, so the backward recomputes the forward's bits
constexpr float AU_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float au_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-AU_LOG2E * x));
}

// sum over the 16 lanes of this lane's DPP row (every lane gets it; a fixed tree)
__device__ __forceinline__ float au_row_sum(float v) {
  v = sum_quad(v);
  v += dpp_f32<0x124>(v);  // row_ror:4
  return v + dpp_f32<0x128>(v);  // row_ror:8
}
__device__ __forceinline__ float au_quad_max(float v) {
  v = fmaxf(v, dpp_f32<0xb1>(v));  // quad_perm [1, 0, 3, 2]
  return fmaxf(v, dpp_f32<0x4e>(v));  // quad_perm [2, 3, 0, 1]
}

// fragment of W[n0 + (lane & 15)][k0 + 8 (lane >> 4) .. + 8] (zero past `cols`)
__device__ __forceinline__ bf16x8 au_wfrag(const float *w, int64_t ld, int n0, int k0, int cols,
                                           int lane) {
  const int k = k0 + 8 * (lane >> 4);
  if (k >= cols) return frag_zero8();
  const float *p = w + (n0 + (lane & 15)) * ld + k;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = p[i];
  return frag_pack8(f);
}
// fragment of W^T: element i is W[k0 + 8 (lane >> 4) + i][n0 + (lane & 15)] (zero past `rows`)
__device__ __forceinline__ bf16x8 au_wfrag_t(const float *w, int64_t ld, int n0, int k0, int rows,
                                             int lane) {
  const int k = k0 + 8 * (lane >> 4);
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = k + i < rows ? w[(k + i) * ld + n0 + (lane & 15)] : 0.f;
  return frag_pack8(f);
}
// A fragment of rows 0..15, k0 .. k0 + 31 of a bf16 [16][ld] LDS tile `cols` wide
__device__ __forceinline__ bf16x8 au_afrag(const uint16_t *tile, int ld, int k0, int cols, int lane) {
  const int k = k0 + 8 * (lane >> 4);
  if (k >= cols) return frag_zero8();
  return *reinterpret_cast<const bf16x8 *>(tile + (lane & 15) * ld + k);
}

// The two layers' weight registers take turns: the weights do not depend on the tile, and
// without this the compiler computes both layers' loads and their 64-bit addresses once,
// above the tile loop, where together with the accumulators they no longer fit.  An empty
// statement that the loads and the address arithmetic (through ld) cannot cross.
__device__ __forceinline__ void au_take_turns(AuLayer &w, int &tid) {
  asm volatile("" : "+s"(w.w_ih), "+s"(w.w_hh), "+s"(w.b_ih), "+s"(w.b_hh), "+s"(w.ld_ih), "+s"(w.ld_hh));
  asm volatile("" : "+v"(tid));  // nor the thread's LDS addresses of the other layer
}

// sample and clamped length of the tile's 16 slots -> LDS (slot past the batch: -1, 0);
// returns the tile's longest length.  Starts and ends at a barrier.
__device__ __forceinline__ int au_meta(const AuArgs &p, int64_t tile, int *s_b, int *s_len, int tid) {
  __syncthreads();
  if (tid < AU_TILE) {
    const int64_t slot = tile * AU_TILE + tid;
    int b = -1, len = 0;
    if (slot < p.batch) {
      const int64_t s = p.order ? static_cast<int64_t>(p.order[slot]) : slot;
      if (s < 0 || s >= p.batch) {
        if (p.oob) *p.oob = 1;
      } else {
        b = static_cast<int>(s);
        len = p.his_len[s];
        if (len < 1 || len > p.L) {
          if (p.oob) *p.oob = 1;
          len = len < 1 ? 0 : p.L;
        }
      }
    }
    s_b[tid] = b;
    s_len[tid] = len;
  }
  __syncthreads();
  int tmax = 0;
#pragma unroll
  for (int i = 0; i < AU_TILE; ++i) tmax = max(tmax, s_len[i]);
  return __builtin_amdgcn_readfirstlane(tmax);
}

// ---------------------------------------------------------------------------
// forward: one layer's recurrence over a tile.  ATT = false: layer 1 (bf16 rows in, hs1
// and the partial scores out).  ATT = true: layer 2 (fp32 hs1 in, a_t from s_att, hs2 and
// v out).  s_h: two [16][H + 8] bf16 tiles.  Starts and ends at a barrier.
// ---------------------------------------------------------------------------
template <int EI, int H, bool ATT>
__device__ __forceinline__ void au_recur_fwd(const AuArgs &p, AuLayer w, uint16_t *s_h,
                                             float *s_sc, const float *s_att, const int *s_b,
                                             const int *s_len, int tmax, int tid) {
  using S = AuShape<EI, H>;
  using TIn = std::conditional_t<ATT, float, uint16_t>;
  constexpr int RPF = ATT ? 2 : 1;  // 16-byte loads per fragment
  au_take_turns(w, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  const int u = 16 * wave + a;  // this lane's hidden unit
  bf16x8 wi[3][S::KSE], wh[3][S::KSH];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) wi[g][s] = au_wfrag(w.w_ih, w.ld_ih, g * H + 16 * wave, 32 * s, EI, lane);
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) wh[g][s] = au_wfrag(w.w_hh, w.ld_hh, g * H + 16 * wave, 32 * s, H, lane);
  }
  const float br = w.b_ih[u] + w.b_hh[u], bz = w.b_ih[H + u] + w.b_hh[H + u];
  const float bnx = w.b_ih[2 * H + u], bnh = w.b_hh[2 * H + u];
  float *hs_out = ATT ? p.hs2 : p.hs1;
  if constexpr (!ATT) {
    // dead positions of hs1 read as zero
    for (int i = tid; i < AU_TILE * p.L * (H / 4); i += S::NT) {
      const int row = i / (p.L * (H / 4)), rem = i % (p.L * (H / 4));
      const int t = rem / (H / 4), c = rem % (H / 4);
      const int b = s_b[row];
      if (b >= 0 && t >= s_len[row])
        *reinterpret_cast<float4 *>(p.hs1 + (static_cast<int64_t>(b) * p.L + t) * H + 4 * c) =
            make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const int lenA = s_len[a];
  const int64_t posA = static_cast<int64_t>(max(s_b[a], 0)) * p.L;  // b L of this lane's A row
  // 16-byte units: the lane's 8 input elements of k step 0, position 0
  const uint4 *xrow = ATT ? reinterpret_cast<const uint4 *>(p.hs1 + posA * H + 8 * q)
                          : reinterpret_cast<const uint4 *>(p.rows + posA * p.ld_rows + 8 * q);
  const int64_t xstep = ATT ? H / 4 : p.ld_rows / 8;  // 16-byte units per position
  int lenC[4];
  float *hsC[4];
  float h[4], pc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = max(s_b[4 * q + e], 0);
    lenC[e] = s_len[4 * q + e];
    hsC[e] = hs_out + (static_cast<int64_t>(b) * p.L) * H + u;
    h[e] = 0.f;
    pc[e] = ATT ? 0.f : p.pq[static_cast<int64_t>(b) * p.ld_p + u];
  }
  for (int i = tid; i < AU_TILE * S::LDH / 8; i += S::NT)
    reinterpret_cast<uint4 *>(s_h)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  auto load_x = [&](int t, uint4 *raw) {
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) {
#pragma unroll
      for (int k = 0; k < RPF; ++k) raw[RPF * s + k] = make_uint4(0, 0, 0, 0);
      if (32 * s + 8 * q < EI && t < lenA) {
        const uint4 *src = xrow + t * xstep + 4 * RPF * s;
#pragma unroll
        for (int k = 0; k < RPF; ++k) raw[RPF * s + k] = src[k];
      }
    }
  };
  uint4 xf[RPF * S::KSE], xn[RPF * S::KSE];
  load_x(0, xf);
  for (int t = 0; t < tmax; ++t) {
    load_x(t + 1, xn);  // (t + 1 >= lenA: no load)
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, anx = ar, anh = ar;
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) {
      const bf16x8 x8 = frag_from_raw<TIn>(xf, s);
      ar = mfma_16x16x32(x8, wi[0][s], ar);
      az = mfma_16x16x32(x8, wi[1][s], az);
      anx = mfma_16x16x32(x8, wi[2][s], anx);
    }
    const uint16_t *hc = s_h + (t & 1) * (AU_TILE * S::LDH);
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) {
      const bf16x8 hf = au_afrag(hc, S::LDH, 32 * s, H, lane);
      ar = mfma_16x16x32(hf, wh[0][s], ar);
      az = mfma_16x16x32(hf, wh[1][s], az);
      anh = mfma_16x16x32(hf, wh[2][s], anh);
    }
    uint16_t *hn = s_h + ((t + 1) & 1) * (AU_TILE * S::LDH);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float r = au_sigmoid(ar[e] + br), z = au_sigmoid(az[e] + bz);
      const float n = tanh_rcp(anx[e] + bnx + r * (anh[e] + bnh));
      const bool live = t < lenC[e];
      if constexpr (ATT) {
        const float ug = s_att[(4 * q + e) * AU_LS + t] * (1.f - z);
        h[e] = live ? h[e] + ug * (n - h[e]) : h[e];
      } else {
        h[e] = live ? (1.f - z) * n + z * h[e] : h[e];
        const float sc = au_row_sum(live ? h[e] * pc[e] : 0.f);
        if (a == 0) s_sc[(wave * AU_TILE + 4 * q + e) * AU_LS + t] = sc;
      }
      if (live) hsC[e][static_cast<int64_t>(t) * H] = h[e];
      hn[(4 * q + e) * S::LDH + u] = f32_to_bf16_rne(h[e]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RPF * S::KSE; ++s) xf[s] = xn[s];
  }
  if constexpr (ATT) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = s_b[4 * q + e];
      if (b >= 0) p.v[static_cast<int64_t>(b) * H + u] = h[e];
    }
  }
}

template <int E, int H>
__global__ __launch_bounds__(64 * (H / 16)) void interest_fwd_kernel(AuArgs p) {
  using S = AuShape<E, H>;
  __shared__ __attribute__((aligned(16))) uint16_t s_h[2 * AU_TILE * S::LDH];
  __shared__ float s_sc[S::NW * AU_TILE * AU_LS];  // partial scores [wave][sample][t]
  __shared__ float s_att[AU_TILE * AU_LS];         // a [sample][t]
  __shared__ int s_b[AU_TILE], s_len[AU_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int tmax = au_meta(p, tile, s_b, s_len, tid);
    au_recur_fwd<E, H, false>(p, p.l1, s_h, s_sc, s_att, s_b, s_len, tmax, tid);
    // masked softmax over t: 4 lanes per sample, positions j, j + 4, ...
    if (wave == 0) {
      const int s = lane >> 2, j = lane & 3, len = s_len[s], b = s_b[s];
      float x[16], m = -INFINITY, sum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = j + 4 * i;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < S::NW; ++k) acc += s_sc[(k * AU_TILE + s) * AU_LS + t];
        x[i] = t < len ? acc : -INFINITY;
        m = fmaxf(m, x[i]);
      }
      m = au_quad_max(m);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        x[i] = j + 4 * i < len ? __builtin_amdgcn_exp2f(AU_LOG2E * (x[i] - m)) : 0.f;
        sum += x[i];
      }
      sum = sum_quad(sum);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = j + 4 * i;
        const float av = t < len ? x[i] / sum : 0.f;
        s_att[s * AU_LS + t] = av;
        if (b >= 0 && t < p.L) p.att[static_cast<int64_t>(b) * p.L + t] = av;
      }
    }
    __threadfence_block();  // hs1 of this tile, stored above, is what layer 2 loads
    __syncthreads();
    au_recur_fwd<H, H, true>(p, p.l2, s_h, s_sc, s_att, s_b, s_len, tmax, tid);
  }
}

// ---------------------------------------------------------------------------
// backward: one layer's recurrence over a tile, t from tmax - 1 down.  ATT = true: layer
// 2 (dh starts at dv; input gradient -> workspace fp32; da partials -> s_red).  ATT =
// false: layer 1 (dh starts at 0 and takes workspace + ds p + d_hs1 at every step; input
// gradient -> d_rows bf16).  The layer's dW / db go to `part` when the tile ends.
// ---------------------------------------------------------------------------
template <int EI, int H, bool ATT>
__device__ __forceinline__ void au_recur_bwd(const AuArgs &p, AuLayer w, float *part, bool first,
                                             uint16_t *s_x, int xbuf, uint16_t *s_h, uint16_t *s_gx,
                                             uint16_t *s_gh, const float *s_att, const float *s_ds,
                                             float *s_red, const int *s_b, const int *s_len, int tmax,
                                             int tid) {
  using S = AuShape<EI, H>;
  constexpr int RPF = ATT ? 2 : 1;  // 16-byte loads per staged 8-element chunk
  au_take_turns(w, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  const int u = 16 * wave + a;
  const float *hs = ATT ? p.hs2 : p.hs1;  // this layer's own hidden sequence
  // the weights in both orientations
  bf16x8 wi[3][S::KSE], wh[3][S::KSH], wiT[S::CTW][S::KSG], whT[S::KSG];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) wi[g][s] = au_wfrag(w.w_ih, w.ld_ih, g * H + 16 * wave, 32 * s, EI, lane);
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) wh[g][s] = au_wfrag(w.w_hh, w.ld_hh, g * H + 16 * wave, 32 * s, H, lane);
  }
#pragma unroll
  for (int s = 0; s < S::KSG; ++s) {
    whT[s] = au_wfrag_t(w.w_hh, w.ld_hh, 16 * wave, 32 * s, 3 * H, lane);
#pragma unroll
    for (int ci = 0; ci < S::CTW; ++ci) {
      const int c = wave + S::NW * ci;
      wiT[ci][s] = c < S::CT ? au_wfrag_t(w.w_ih, w.ld_ih, 16 * c, 32 * s, 3 * H, lane) : frag_zero8();
    }
  }
  const float br = w.b_ih[u] + w.b_hh[u], bz = w.b_ih[H + u] + w.b_hh[H + u];
  const float bnx = w.b_ih[2 * H + u], bnh = w.b_hh[2 * H + u];
  f32x4 dwi[3][S::CT], dwh[3][S::NW];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int c = 0; c < S::CT; ++c) dwi[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < S::NW; ++c) dwh[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float db[4] = {0.f, 0.f, 0.f, 0.f};  // sums of da_r, da_z, da_n, da_n r over this lane's rows
  const int hrow = tid / (H / 4), hcol = 4 * (tid % (H / 4));  // this thread's 4 staged h values
  if constexpr (!ATT) {
    // dead positions of d_rows: bitwise zero
    for (int i = tid; i < AU_TILE * p.L * S::CHX; i += S::NT) {
      const int row = i / (p.L * S::CHX), rem = i % (p.L * S::CHX);
      const int t = rem / S::CHX, c = rem % S::CHX;
      const int b = s_b[row];
      if (b >= 0 && t >= s_len[row])
        *reinterpret_cast<uint4 *>(p.drows + (static_cast<int64_t>(b) * p.L + t) * p.ld_drows + 8 * c) =
            make_uint4(0, 0, 0, 0);
    }
  }
  int lenC[4];
  int64_t baseC[4];  // b L of this lane's four samples
  float dh[4], pc[4], ex[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int b = s_b[4 * q + e];
    lenC[e] = s_len[4 * q + e];
    baseC[e] = static_cast<int64_t>(max(b, 0)) * p.L;
    dh[e] = ATT && b >= 0 ? p.dv[static_cast<int64_t>(b) * H + u] : 0.f;
    pc[e] = ATT ? 0.f : p.pq[static_cast<int64_t>(max(b, 0)) * p.ld_p + u];
    ex[e] = 0.f;
  }
  // layer 1: what step t's h receives from above, workspace[t] + ds_t p + d_hs1[t]
  auto load_ex = [&](int t) {
    if constexpr (!ATT) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ex[e] = 0.f;
        if (t >= 0 && t < lenC[e]) {
          const int64_t i = (baseC[e] + t) * H + u;
          float v = p.ws[i] + s_ds[(4 * q + e) * AU_LS + t] * pc[e];
          if (p.d_hs1) v += p.d_hs1[i];
          ex[e] = v;
        }
      }
    }
  };
  // staging of step t: the input x_t and bf16(h_{t-1}) of live samples, zero rows otherwise
  uint4 stx[RPF * S::XI];
  float4 sth;
  auto stage_load = [&](int t) {
#pragma unroll
    for (int k = 0; k < S::XI; ++k) {
      const int i = tid + S::NT * k;
      const int row = (i / S::CHX) & (AU_TILE - 1), c = i % S::CHX;
#pragma unroll
      for (int r = 0; r < RPF; ++r) stx[RPF * k + r] = make_uint4(0, 0, 0, 0);
      if (i < AU_TILE * S::CHX && t < s_len[row]) {
        const int64_t pos = static_cast<int64_t>(s_b[row]) * p.L + t;
        const uint4 *src = ATT ? reinterpret_cast<const uint4 *>(p.hs1 + pos * H + 8 * c)
                               : reinterpret_cast<const uint4 *>(p.rows + pos * p.ld_rows + 8 * c);
#pragma unroll
        for (int r = 0; r < RPF; ++r) stx[RPF * k + r] = src[r];
      }
    }
    sth = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 1 && t < s_len[hrow])
      sth = *reinterpret_cast<const float4 *>(hs + (static_cast<int64_t>(s_b[hrow]) * p.L + t - 1) * H + hcol);
  };
  auto stage_store = [&](int buf) {
#pragma unroll
    for (int k = 0; k < S::XI; ++k) {
      const int i = tid + S::NT * k;
      if (i < AU_TILE * S::CHX) {
        uint4 v = stx[RPF * k];
        if constexpr (ATT) v = __builtin_bit_cast(uint4, frag_from_f32(stx[2 * k], stx[2 * k + 1]));
        *reinterpret_cast<uint4 *>(s_x + buf * xbuf + (i / S::CHX) * S::LDX + 8 * (i % S::CHX)) = v;
      }
    }
    *reinterpret_cast<uint2 *>(s_h + buf * (AU_TILE * S::LDH) + hrow * S::LDH + hcol) =
        make_uint2(pack_bf16x2(sth.x, sth.y), pack_bf16x2(sth.z, sth.w));
  };
  __syncthreads();  // the stage before this one is done with the staged tiles
  int buf = 0;
  if (tmax > 0) {
    stage_load(tmax - 1);
    stage_store(0);
    load_ex(tmax - 1);
  }
  for (int t = tmax - 1; t >= 0; --t) {
    __syncthreads();  // step t's staged tiles are visible; the dG tiles are free
    const uint16_t *cx = s_x + buf * xbuf, *ch = s_h + buf * (AU_TILE * S::LDH);
    // the forward's gates, recomputed
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, anx = ar, anh = ar;
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) {
      const bf16x8 xf = au_afrag(cx, S::LDX, 32 * s, EI, lane);
      ar = mfma_16x16x32(xf, wi[0][s], ar);
      az = mfma_16x16x32(xf, wi[1][s], az);
      anx = mfma_16x16x32(xf, wi[2][s], anx);
    }
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) {
      const bf16x8 hf = au_afrag(ch, S::LDH, 32 * s, H, lane);
      ar = mfma_16x16x32(hf, wh[0][s], ar);
      az = mfma_16x16x32(hf, wh[1][s], az);
      anh = mfma_16x16x32(hf, wh[2][s], anh);
    }
    float keep[4], dcur[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool live = t < lenC[e];
      const float hp = live && t > 0 ? hs[(baseC[e] + t - 1) * H + u] : 0.f;
      const float r = au_sigmoid(ar[e] + br), z = au_sigmoid(az[e] + bz);
      const float hn = anh[e] + bnh;
      const float n = tanh_rcp(anx[e] + bnx + r * hn);
      const float d = live ? dh[e] + ex[e] : 0.f;
      // h_t = h_{t-1} + gn (n - h_{t-1}):  gn = 1 - z (GRU), a_t (1 - z) (AUGRU)
      const float at = ATT ? s_att[(4 * q + e) * AU_LS + t] : 1.f;
      const float gn = ATT ? at * (1.f - z) : 1.f - z;
      const float dan = d * gn * (1.f - n * n);
      const float dar = dan * hn * r * (1.f - r);
      const float daz = ATT ? d * (hp - n) * at * z * (1.f - z) : d * (hp - n) * z * (1.f - z);
      const float danr = dan * r;
      keep[e] = ATT ? 1.f - gn : z;
      dcur[e] = d;
      if constexpr (ATT) {
        const float da = au_row_sum(d * (n - hp) * (1.f - z));
        if (a == 0) s_red[(wave * AU_TILE + 4 * q + e) * AU_LS + t] = da;
      }
      db[0] += dar;
      db[1] += daz;
      db[2] += dan;
      db[3] += danr;
      uint16_t *gx = s_gx + (4 * q + e) * S::LDG + u, *gh = s_gh + (4 * q + e) * S::LDG + u;
      const uint16_t wr = f32_to_bf16_rne(dar), wz = f32_to_bf16_rne(daz);
      gx[0] = wr, gx[H] = wz, gx[2 * H] = f32_to_bf16_rne(dan);
      gh[0] = wr, gh[H] = wz, gh[2 * H] = f32_to_bf16_rne(danr);
    }
    if (t > 0) stage_load(t - 1);  // in flight over the products below
    load_ex(t - 1);
    __syncthreads();
    // dh <- d keep + dGh W_hh
    f32x4 adh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S::KSG; ++s)
      adh = mfma_16x16x32(au_afrag(s_gh, S::LDG, 32 * s, S::KG, lane), whT[s], adh);
#pragma unroll
    for (int e = 0; e < 4; ++e) dh[e] = t < lenC[e] ? dcur[e] * keep[e] + adh[e] : dh[e];
    // the input gradient dGx W_ih
#pragma unroll
    for (int ci = 0; ci < S::CTW; ++ci) {
      const int c = wave + S::NW * ci;
      if (c < S::CT) {
        f32x4 adx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < S::KSG; ++s)
          adx = mfma_16x16x32(au_afrag(s_gx, S::LDG, 32 * s, S::KG, lane), wiT[ci][s], adx);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (t < lenC[e]) {
            if constexpr (ATT)
              p.ws[(baseC[e] + t) * H + 16 * c + a] = adx[e];
            else
              p.drows[(baseC[e] + t) * p.ld_drows + 16 * c + a] = f32_to_bf16_rne(adx[e]);
          }
      }
    }
    // dW_ih += dGx^T x_t, dW_hh += dGh^T h_{t-1} (h_-1 = 0: nothing at t = 0)
    bf16x4 xT[S::CT], hT[S::NW];
#pragma unroll
    for (int c = 0; c < S::CT; ++c) xT[c] = lds_tr16x4(cx, S::LDX, 16 * c, lane);
    if (t > 0) {
#pragma unroll
      for (int c = 0; c < S::NW; ++c) hT[c] = lds_tr16x4(ch, S::LDH, 16 * c, lane);
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const bf16x4 gxT = lds_tr16x4(s_gx, S::LDG, g * H + 16 * wave, lane);
#pragma unroll
      for (int c = 0; c < S::CT; ++c) dwi[g][c] = mfma_16x16x16(gxT, xT[c], dwi[g][c]);
      if (t > 0) {
        const bf16x4 ghT = lds_tr16x4(s_gh, S::LDG, g * H + 16 * wave, lane);
#pragma unroll
        for (int c = 0; c < S::NW; ++c) dwh[g][c] = mfma_16x16x16(ghT, hT[c], dwh[g][c]);
      }
    }
    if (t > 0) stage_store(buf ^ 1);
    buf ^= 1;
  }
  // into the workgroup's partial of this layer: [dW_ih | dW_hh | db_ih | db_hh].  A thread
  // meets its own earlier values only.
  asm volatile("" : "+s"(part));  // the addresses below are formed here, not above the tile loop
  auto flush = [&](float *dst, float v) { *dst = first ? v : *dst + v; };
  float *pi = part + (16 * wave + 4 * q) * EI + a, *ph = part + 3 * H * EI + (16 * wave + 4 * q) * H + a;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
      for (int c = 0; c < S::CT; ++c) flush(pi + (g * H + e) * EI + 16 * c, dwi[g][c][e]);
#pragma unroll
      for (int c = 0; c < S::NW; ++c) flush(ph + (g * H + e) * H + 16 * c, dwh[g][c][e]);
    }
  }
  // a unit's four row groups (lanes a, a + 16, a + 32, a + 48), added in a fixed order
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    db[k] += __shfl_xor(db[k], 16);
    db[k] += __shfl_xor(db[k], 32);
  }
  if (q == 0) {
    float *bi = part + 3 * H * (EI + H), *bh = bi + 3 * H;
    flush(bi + u, db[0]), flush(bi + H + u, db[1]), flush(bi + 2 * H + u, db[2]);
    flush(bh + u, db[0]), flush(bh + H + u, db[1]), flush(bh + 2 * H + u, db[3]);
  }
}

template <int E, int H>
__global__ __launch_bounds__(64 * (H / 16)) void interest_bwd_kernel(AuArgs p) {
  using S = AuShape<E, H>;
  constexpr int LDXM = (E > H ? E : H) + 8, XBUF = AU_TILE * LDXM;
  __shared__ __attribute__((aligned(16))) uint16_t s_x[2 * XBUF];               // the input of step t
  __shared__ __attribute__((aligned(16))) uint16_t s_h[2 * AU_TILE * S::LDH];   // bf16(h_{t-1})
  __shared__ __attribute__((aligned(16))) uint16_t s_gx[AU_TILE * S::LDG];      // dGx
  __shared__ __attribute__((aligned(16))) uint16_t s_gh[AU_TILE * S::LDG];      // dGh
  __shared__ float s_att[AU_TILE * AU_LS], s_ds[AU_TILE * AU_LS];
  __shared__ float s_red[S::NW * AU_TILE * AU_LS];  // da partials [wave][sample][t]
  __shared__ int s_b[AU_TILE], s_len[AU_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the dG tiles' padding columns (3H .. KG) stay zero
  for (int i = tid; i < AU_TILE * S::LDG / 8; i += S::NT) {
    reinterpret_cast<uint4 *>(s_gx)[i] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4 *>(s_gh)[i] = make_uint4(0, 0, 0, 0);
  }
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * p.P;
  const int hrow = tid / (H / 4), hcol = 4 * (tid % (H / 4));
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const bool first = tile == blockIdx.x;
    const int tmax = au_meta(p, tile, s_b, s_len, tid);
    for (int i = tid; i < AU_TILE * AU_MAXL; i += S::NT) {
      const int s = i / AU_MAXL, t = i % AU_MAXL, b = s_b[s];
      s_att[s * AU_LS + t] = b >= 0 && t < s_len[s] ? p.att[static_cast<int64_t>(b) * p.L + t] : 0.f;
    }
    au_recur_bwd<H, H, true>(p, p.l2, part + AuShape<E, H>::PL, first, s_x, XBUF, s_h, s_gx, s_gh, s_att,
                             s_ds, s_red, s_b, s_len, tmax, tid);
    __threadfence_block();  // the workspace of this tile, stored above, is what layer 1 loads
    __syncthreads();
    // ds_t = a_t (da_t - sum_t' a_t' da_t'): 4 lanes per sample, positions j, j + 4, ...
    if (wave == 0) {
      const int s = lane >> 2, j = lane & 3, len = s_len[s];
      float da[16], dot = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = j + 4 * i;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < S::NW; ++k) acc += s_red[(k * AU_TILE + s) * AU_LS + t];
        da[i] = t < len ? acc : 0.f;
        dot += s_att[s * AU_LS + t] * da[i];
      }
      dot = sum_quad(dot);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int t = j + 4 * i;
        s_ds[s * AU_LS + t] = t < len ? s_att[s * AU_LS + t] * (da[i] - dot) : 0.f;
      }
    }
    __syncthreads();
    // dp = sum_t ds_t h1_t: this thread's sample and four units
    {
      const int b = s_b[hrow], len = s_len[hrow];
      if (b >= 0) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        const float *h1 = p.hs1 + static_cast<int64_t>(b) * p.L * H + hcol;
        for (int t = 0; t < len; ++t) {
          const float4 hv = *reinterpret_cast<const float4 *>(h1 + static_cast<int64_t>(t) * H);
          const float ds = s_ds[hrow * AU_LS + t];
          acc.x += ds * hv.x, acc.y += ds * hv.y, acc.z += ds * hv.z, acc.w += ds * hv.w;
        }
        float *dst = p.dp + static_cast<int64_t>(b) * p.ld_dp + hcol;
        dst[0] = acc.x, dst[1] = acc.y, dst[2] = acc.z, dst[3] = acc.w;
      }
    }
    au_recur_bwd<E, H, false>(p, p.l1, part, first, s_x, XBUF, s_h, s_gx, s_gh, s_att, s_ds, s_red, s_b,
                              s_len, tmax, tid);
  }
}

}  // namespace mrec

using namespace mrec;

namespace {

bool au_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool au_width(int32_t w) { return w == 16 || w == 32 || w == 64; }

mrec_status au_check(const mrec_interest_args *a, AuArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->x && a->his_len && a->p && a->w_ih1 && a->w_hh1 && a->b_ih1 && a->b_hh1 &&
                     a->w_ih2 && a->w_hh2 && a->b_ih2 && a->b_hh2 && a->hs1 && a->hs2 && a->att,
                 "NULL pointer");
  MREC_CHECK_ARG(au_width(a->E) && au_width(a->H), "E and H must be 16, 32 or 64");
  MREC_CHECK_ARG(a->L >= 1 && a->L <= AU_MAXL, "need 1 <= L <= 64");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->ld_x >= a->E && a->ld_p >= a->H && a->ld_ih1 >= a->E && a->ld_hh1 >= a->H &&
                     a->ld_ih2 >= a->H && a->ld_hh2 >= a->H,
                 "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(au_aligned(a->x) && a->ld_x % 8 == 0 && au_aligned(a->hs1) && au_aligned(a->hs2),
                 "x, hs1 and hs2 must be 16-byte aligned (ld_x a multiple of 8 bf16 elements)");
  AuArgs p{};
  p.rows = static_cast<const uint16_t *>(a->x);
  p.ld_rows = a->ld_x;
  p.his_len = a->his_len;
  p.order = a->order;
  p.pq = a->p;
  p.ld_p = a->ld_p;
  p.l1 = AuLayer{a->w_ih1, a->w_hh1, a->ld_ih1, a->ld_hh1, a->b_ih1, a->b_hh1};
  p.l2 = AuLayer{a->w_ih2, a->w_hh2, a->ld_ih2, a->ld_hh2, a->b_ih2, a->b_hh2};
  p.L = a->L;
  p.batch = a->batch;
  p.tiles = (a->batch + AU_TILE - 1) / AU_TILE;
  p.hs1 = a->hs1, p.hs2 = a->hs2, p.att = a->att, p.v = a->v;
  p.oob = a->d_oob_flag;
  p.dv = a->dv, p.d_hs1 = a->d_hs1;
  p.ws = a->workspace;
  p.drows = static_cast<uint16_t *>(a->dx);
  p.ld_drows = a->ld_dx;
  p.dp = a->dp;
  p.ld_dp = a->ld_dp;
  p.part = a->part;
  p.P = mrec_interest_param_count(a->E, a->H);
  *out = p;
  return MREC_OK;
}

}  // namespace

extern "C" {

int32_t mrec_interest_supported(int32_t E, int32_t H, int32_t L) {
  return au_width(E) && au_width(H) && L >= 1 && L <= AU_MAXL ? 1 : 0;
}

int32_t mrec_interest_tile(void) { return AU_TILE; }

int64_t mrec_interest_parts(int64_t batch) {
  const int64_t g = device_cus(), tiles = (batch + AU_TILE - 1) / AU_TILE;
  return tiles < g ? (tiles > 0 ? tiles : 1) : g;
}

int64_t mrec_interest_param_count(int32_t E, int32_t H) {
  return 3 * static_cast<int64_t>(H) * (static_cast<int64_t>(E) + H + 2) +
         3 * static_cast<int64_t>(H) * (2 * static_cast<int64_t>(H) + 2);
}

#define AU_DISPATCH(kernel, what)                                                     \
  X(16, 16, kernel, what) X(16, 32, kernel, what) X(16, 64, kernel, what)             \
  X(32, 16, kernel, what) X(32, 32, kernel, what) X(32, 64, kernel, what)             \
  X(64, 16, kernel, what) X(64, 32, kernel, what) X(64, 64, kernel, what)
#define X(e, h, kernel, what)                                                         \
  if (a->E == e && a->H == h) {                                                       \
    kernel<e, h><<<dim3(grid), AuShape<e, h>::NT, 0, s>>>(p);                         \
    return launch_status(what);                                                       \
  }

mrec_status mrec_interest_fwd(const mrec_interest_args *a, mrec_stream stream) {
  AuArgs p;
  const mrec_status st = au_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(mrec_interest_parts(p.batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  AU_DISPATCH(interest_fwd_kernel, "mrec_interest_fwd")
  return MREC_EINVAL;
}

mrec_status mrec_interest_bwd(const mrec_interest_args *a, mrec_stream stream) {
  AuArgs p;
  const mrec_status st = au_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->dv && a->workspace && a->dx && a->dp && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_dx >= a->E && a->ld_dx % 8 == 0 && au_aligned(a->dx),
                 "dx must be 16-byte aligned bf16 rows (ld_dx a multiple of 8, >= E)");
  MREC_CHECK_ARG(a->ld_dp >= a->H, "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(a->parts == mrec_interest_parts(a->batch), "parts must be mrec_interest_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  AU_DISPATCH(interest_bwd_kernel, "mrec_interest_bwd")
  return MREC_EINVAL;
}

#undef X
#undef AU_DISPATCH

}  // extern "C"
