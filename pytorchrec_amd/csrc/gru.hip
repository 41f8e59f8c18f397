// GRU4Rec session encoder, the whole recurrence in one launch each way
// (torchrec/model/GRU4Rec.py:51-56: nn.GRU over the packed history).
//
//   x_t = rows[b, t]                                   t = 0 .. his_len[b] - 1, h_-1 = 0
//   r_t = sigmoid(W_ir x_t + b_ir + W_hr h_{t-1} + b_hr)
//   z_t = sigmoid(W_iz x_t + b_iz + W_hz h_{t-1} + b_hz)
//   n_t = tanh   (W_in x_t + b_in + r_t (W_hn h_{t-1} + b_hn))
//   h_t = (1 - z_t) n_t + z_t h_{t-1}                  h_last[b] = h_{his_len[b] - 1}
//
// Work split.  A workgroup takes a tile of 16 samples: the 16 rows of
// v_mfma_f32_16x16x32_bf16.  Its H / 16 waves each own 16 hidden units of all three
// gates, with four accumulators: r and z (input + hidden products summed), and n's input
// and hidden products apart, because r multiplies only the latter.  With the C/D mapping
// col = lane & 15, row = 4 (lane >> 4) + reg the four accumulators of a lane address the
// same (sample, unit), so the gate math and the fp32 h it carries stay in registers over
// the whole sequence.  A wave's slices of W_ih and W_hh are constant over the sequence:
// loaded once from the fp32 masters, rounded to bf16, kept in registers (<= 48 VGPRs).
//
// Forward, per step: the x_t fragments come straight from the gathered rows (a 16-B load
// per lane, issued one step ahead: they do not depend on h); bf16(h_t) goes to a
// double-buffered [16][H + 8] LDS tile, one barrier, and every wave reads the whole tile
// as the next step's A operand.  The step loop runs to the tile's longest sample; a
// sample past its own length keeps h by a select and neither reads its row nor writes hs.
//
// Saved: hs [batch, L, H] fp32, the hidden sequence as the forward carried it, at live
// positions only.  The backward recomputes r, z, n and W_hn h + b_hn from hs[t - 1] and
// x_t with the forward's MFMAs, so it sees the forward's bits.
//
// Backward, t from the tile's longest length - 1 down, dh carried in registers in the
// same layout:
//   dn = dh (1 - z), dz = dh (h_{t-1} - n), da_n = dn (1 - n^2),
//   da_r = da_n (W_hn h + b_hn) r (1 - r), da_z = dz z (1 - z)
//   dGx = [da_r, da_z, da_n], dGh = [da_r, da_z, da_n r]   -> LDS, bf16 [16][3H]
//   dx_t = dGx W_ih (bf16 -> d_rows),  dh <- dh z + dGh W_hh
//   dW_ih += dGx^T x_t, dW_hh += dGh^T h_{t-1}: v_mfma_f32_16x16x16_bf16 (k = the 16
//   samples) on transposing LDS reads (ds_read_b64_tr_b16), accumulated in registers over
//   the workgroup's tiles and steps; db_ih / db_hh in per-thread registers (fp32 values).
// Both orientations of the weights stay in registers (96 VGPRs at E = H = 64) next to
// the 96 accumulator registers; one wave per SIMD has 512.  One fp32 partial per
// workgroup [dW_ih | dW_hh | db_ih | db_hh], summed in workgroup order by
// mrec_sasrec_wgrad (bit-reproducible).  d_rows at t >= his_len is written as zero.
//
// `order` (optional) maps tile slot -> sample, to put samples of similar length in one
// tile; samples are independent MFMA rows, so it changes speed only, never a sample's
// bits.  his_len outside 1..L (or an order entry outside the batch) sets *d_oob_flag and
// is clamped: nothing is read or written out of bounds, length 0 gives h_last = 0.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int GR_TILE = 16;  // samples per workgroup tile (the MFMA's rows)
constexpr int GR_MAXL = 64;

struct GruArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his_len;
  const int32_t *order;  // tile slot -> sample, or NULL
  const float *w_ih, *w_hh;  // fp32 masters [3H, E], [3H, H] (gates r, z, n)
  int64_t ld_ih, ld_hh;
  const float *b_ih, *b_hh;
  int L;
  int64_t batch, tiles;
  float *hs;      // [batch, L, H] fp32
  float *h_last;  // [batch, H]
  int32_t *oob;
  const float *dh_last;
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][P]
  int64_t P;
};

template <int E, int H>
struct GrShape {
  static_assert((E == 16 || E == 32 || E == 64) && (H == 16 || H == 32 || H == 64), "compiled widths");
  static constexpr int NW = H / 16;           // waves: 16 hidden units each
  static constexpr int NT = 64 * NW;          // threads
  static constexpr int KSE = (E + 31) / 32;   // k steps over x
  static constexpr int KSH = (H + 31) / 32;   // k steps over h
  static constexpr int KG = (3 * H + 31) / 32 * 32;  // dG columns, padded to the k step
  static constexpr int KSG = KG / 32;
  static constexpr int CT = E / 16;                  // column tiles of dx / dW_ih
  static constexpr int CTW = (CT + NW - 1) / NW;     // dx column tiles per wave
  static constexpr int LDX = E + 8, LDH = H + 8, LDG = KG + 8;  // bf16 elements per LDS row
  static constexpr int CHX = E / 8;                  // 16-B chunks of an x row
  static constexpr int XI = (GR_TILE * CHX + NT - 1) / NT;  // x chunks a thread stages
};

// sigmoid = 1 / (1 + exp(-x)), tanh = 1 - 2 / (1 + exp(2x)): both forms go to their limits
// without inf / inf for large |x| (exp -> inf gives rcp -> 0).  v_exp_f32 and v_rcp_f32
// (1 ulp each): the gate math is the step's VALU work, 12 activations per lane, and libm's
// expf and the IEEE division were ~2000 of a step's cycles (the forward kernel took 83 us
// with them at B = 4096, L = 50, E = H = 64).  Forward and backward share these, so the
// backward recomputes the forward's bits.
constexpr float GR_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float gr_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-GR_LOG2E * x));
}
__device__ __forceinline__ float gr_tanh(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(2.f * GR_LOG2E * x));
}

// fragment of W[n0 + (lane & 15)][k0 + 8 (lane >> 4) .. + 8] (zero past `cols`): the B
// operand of a product over W's columns, from the fp32 master
__device__ __forceinline__ bf16x8 gr_wfrag(const float *w, int64_t ld, int n0, int k0, int cols,
                                           int lane) {
  const int k = k0 + 8 * (lane >> 4);
  if (k >= cols) return frag_zero8();
  const float *p = w + (n0 + (lane & 15)) * ld + k;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = p[i];
  return frag_pack8(f);
}

// fragment of W^T: element i is W[k0 + 8 (lane >> 4) + i][n0 + (lane & 15)] (zero past
// `rows`): the B operand of a product over W's rows
__device__ __forceinline__ bf16x8 gr_wfrag_t(const float *w, int64_t ld, int n0, int k0, int rows,
                                             int lane) {
  const int k = k0 + 8 * (lane >> 4);
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = k + i < rows ? w[(k + i) * ld + n0 + (lane & 15)] : 0.f;
  return frag_pack8(f);
}

// A fragment of rows 0..15, k0 .. k0 + 31 of a bf16 [16][ld] LDS tile `cols` wide
__device__ __forceinline__ bf16x8 gr_afrag(const uint16_t *tile, int ld, int k0, int cols, int lane) {
  const int k = k0 + 8 * (lane >> 4);
  if (k >= cols) return frag_zero8();
  return *reinterpret_cast<const bf16x8 *>(tile + (lane & 15) * ld + k);
}

// sample and clamped length of the tile's 16 slots -> LDS (slot past the batch: -1, 0);
// returns the tile's longest length.  Starts and ends at a barrier.
__device__ __forceinline__ int gr_meta(const GruArgs &p, int64_t tile, int *s_b, int *s_len, int tid) {
  __syncthreads();
  if (tid < GR_TILE) {
    const int64_t slot = tile * GR_TILE + tid;
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
  for (int i = 0; i < GR_TILE; ++i) tmax = max(tmax, s_len[i]);
  return __builtin_amdgcn_readfirstlane(tmax);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int E, int H>
__global__ __launch_bounds__(64 * (H / 16)) void gru_fwd_kernel(GruArgs p) {
  using S = GrShape<E, H>;
  __shared__ __attribute__((aligned(16))) uint16_t s_h[2][GR_TILE * S::LDH];
  __shared__ int s_b[GR_TILE], s_len[GR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  const int u = 16 * wave + a;  // this lane's hidden unit
  bf16x8 wi[3][S::KSE], wh[3][S::KSH];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) wi[g][s] = gr_wfrag(p.w_ih, p.ld_ih, g * H + 16 * wave, 32 * s, E, lane);
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) wh[g][s] = gr_wfrag(p.w_hh, p.ld_hh, g * H + 16 * wave, 32 * s, H, lane);
  }
  const float br = p.b_ih[u] + p.b_hh[u], bz = p.b_ih[H + u] + p.b_hh[H + u];
  const float bnx = p.b_ih[2 * H + u], bnh = p.b_hh[2 * H + u];
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int tmax = gr_meta(p, tile, s_b, s_len, tid);
    const int lenA = s_len[a];
    const uint16_t *xrow = p.rows + (static_cast<int64_t>(max(s_b[a], 0)) * p.L) * p.ld_rows + 8 * q;
    int lenC[4];
    float *hsC[4];
    float h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lenC[e] = s_len[4 * q + e];
      hsC[e] = p.hs + (static_cast<int64_t>(max(s_b[4 * q + e], 0)) * p.L) * H + u;
      h[e] = 0.f;
    }
    for (int i = tid; i < GR_TILE * S::LDH / 8; i += S::NT)
      reinterpret_cast<uint4 *>(s_h[0])[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    auto load_x = [&](int t, bf16x8 *xf) {
#pragma unroll
      for (int s = 0; s < S::KSE; ++s) {
        xf[s] = frag_zero8();
        if (32 * s + 8 * q < E && t < lenA)
          xf[s] = *reinterpret_cast<const bf16x8 *>(xrow + t * p.ld_rows + 32 * s);
      }
    };
    bf16x8 xf[S::KSE], xn[S::KSE];
    load_x(0, xf);
    for (int t = 0; t < tmax; ++t) {
      load_x(t + 1, xn);  // (t + 1 >= lenA: no load)
      f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, anx = ar, anh = ar;
#pragma unroll
      for (int s = 0; s < S::KSE; ++s) {
        ar = mfma_16x16x32(xf[s], wi[0][s], ar);
        az = mfma_16x16x32(xf[s], wi[1][s], az);
        anx = mfma_16x16x32(xf[s], wi[2][s], anx);
      }
      const uint16_t *hc = s_h[t & 1];
#pragma unroll
      for (int s = 0; s < S::KSH; ++s) {
        const bf16x8 hf = gr_afrag(hc, S::LDH, 32 * s, H, lane);
        ar = mfma_16x16x32(hf, wh[0][s], ar);
        az = mfma_16x16x32(hf, wh[1][s], az);
        anh = mfma_16x16x32(hf, wh[2][s], anh);
      }
      uint16_t *hn = s_h[(t + 1) & 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float r = gr_sigmoid(ar[e] + br), z = gr_sigmoid(az[e] + bz);
        const float n = gr_tanh(anx[e] + bnx + r * (anh[e] + bnh));
        const bool live = t < lenC[e];
        h[e] = live ? (1.f - z) * n + z * h[e] : h[e];
        if (live) hsC[e][static_cast<int64_t>(t) * H] = h[e];
        hn[(4 * q + e) * S::LDH + u] = f32_to_bf16_rne(h[e]);
      }
      __syncthreads();
#pragma unroll
      for (int s = 0; s < S::KSE; ++s) xf[s] = xn[s];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = s_b[4 * q + e];
      if (b >= 0) p.h_last[static_cast<int64_t>(b) * H + u] = h[e];
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int E, int H>
__global__ __launch_bounds__(64 * (H / 16)) void gru_bwd_kernel(GruArgs p) {
  using S = GrShape<E, H>;
  __shared__ __attribute__((aligned(16))) uint16_t s_x[2][GR_TILE * S::LDX];  // x_t
  __shared__ __attribute__((aligned(16))) uint16_t s_h[2][GR_TILE * S::LDH];  // bf16(h_{t-1})
  __shared__ __attribute__((aligned(16))) uint16_t s_gx[GR_TILE * S::LDG];    // dGx
  __shared__ __attribute__((aligned(16))) uint16_t s_gh[GR_TILE * S::LDG];    // dGh
  __shared__ int s_b[GR_TILE], s_len[GR_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  const int u = 16 * wave + a;
  // the weights in both orientations
  bf16x8 wi[3][S::KSE], wh[3][S::KSH], wiT[S::CTW][S::KSG], whT[S::KSG];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int s = 0; s < S::KSE; ++s) wi[g][s] = gr_wfrag(p.w_ih, p.ld_ih, g * H + 16 * wave, 32 * s, E, lane);
#pragma unroll
    for (int s = 0; s < S::KSH; ++s) wh[g][s] = gr_wfrag(p.w_hh, p.ld_hh, g * H + 16 * wave, 32 * s, H, lane);
  }
#pragma unroll
  for (int s = 0; s < S::KSG; ++s) {
    whT[s] = gr_wfrag_t(p.w_hh, p.ld_hh, 16 * wave, 32 * s, 3 * H, lane);
#pragma unroll
    for (int ci = 0; ci < S::CTW; ++ci) {
      const int c = wave + S::NW * ci;
      wiT[ci][s] = c < S::CT ? gr_wfrag_t(p.w_ih, p.ld_ih, 16 * c, 32 * s, 3 * H, lane) : frag_zero8();
    }
  }
  const float br = p.b_ih[u] + p.b_hh[u], bz = p.b_ih[H + u] + p.b_hh[H + u];
  const float bnx = p.b_ih[2 * H + u], bnh = p.b_hh[2 * H + u];
  f32x4 dwi[3][S::CT], dwh[3][S::NW];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int c = 0; c < S::CT; ++c) dwi[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < S::NW; ++c) dwh[g][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float db[4] = {0.f, 0.f, 0.f, 0.f};  // sums of da_r, da_z, da_n, da_n r over this lane's rows
  // the dG tiles' padding columns (3H .. KG) stay zero
  for (int i = tid; i < GR_TILE * S::LDG / 8; i += S::NT) {
    reinterpret_cast<uint4 *>(s_gx)[i] = make_uint4(0, 0, 0, 0);
    reinterpret_cast<uint4 *>(s_gh)[i] = make_uint4(0, 0, 0, 0);
  }
  const int hrow = tid / (H / 4), hcol = 4 * (tid % (H / 4));  // this thread's 4 staged h values
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int tmax = gr_meta(p, tile, s_b, s_len, tid);
    // dead positions of d_rows: bitwise zero
    for (int i = tid; i < GR_TILE * p.L * S::CHX; i += S::NT) {
      const int row = i / (p.L * S::CHX), rem = i % (p.L * S::CHX);
      const int t = rem / S::CHX, c = rem % S::CHX;
      const int b = s_b[row];
      if (b >= 0 && t >= s_len[row])
        *reinterpret_cast<uint4 *>(p.drows + (static_cast<int64_t>(b) * p.L + t) * p.ld_drows + 8 * c) =
            make_uint4(0, 0, 0, 0);
    }
    int lenC[4];
    int64_t baseC[4];  // b L of this lane's four samples
    float dh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int b = s_b[4 * q + e];
      lenC[e] = s_len[4 * q + e];
      baseC[e] = static_cast<int64_t>(max(b, 0)) * p.L;
      dh[e] = b >= 0 ? p.dh_last[static_cast<int64_t>(b) * H + u] : 0.f;
    }
    // staging of step t: x_t and bf16(h_{t-1}) of live samples, zero rows otherwise
    uint4 stx[S::XI];
    float4 sth;
    auto stage_load = [&](int t) {
#pragma unroll
      for (int k = 0; k < S::XI; ++k) {
        const int i = tid + S::NT * k;
        const int row = (i / S::CHX) & (GR_TILE - 1), c = i % S::CHX;
        stx[k] = make_uint4(0, 0, 0, 0);
        if (i < GR_TILE * S::CHX && t < s_len[row])
          stx[k] = *reinterpret_cast<const uint4 *>(
              p.rows + (static_cast<int64_t>(s_b[row]) * p.L + t) * p.ld_rows + 8 * c);
      }
      sth = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t >= 1 && t < s_len[hrow])
        sth = *reinterpret_cast<const float4 *>(
            p.hs + (static_cast<int64_t>(s_b[hrow]) * p.L + t - 1) * H + hcol);
    };
    auto stage_store = [&](int buf) {
#pragma unroll
      for (int k = 0; k < S::XI; ++k) {
        const int i = tid + S::NT * k;
        if (i < GR_TILE * S::CHX)
          *reinterpret_cast<uint4 *>(s_x[buf] + (i / S::CHX) * S::LDX + 8 * (i % S::CHX)) = stx[k];
      }
      *reinterpret_cast<uint2 *>(s_h[buf] + hrow * S::LDH + hcol) =
          make_uint2(pack_bf16x2(sth.x, sth.y), pack_bf16x2(sth.z, sth.w));
    };
    int buf = 0;
    if (tmax > 0) {
      stage_load(tmax - 1);
      stage_store(0);
    }
    for (int t = tmax - 1; t >= 0; --t) {
      __syncthreads();  // step t's staged tiles are visible; the dG tiles are free
      // the forward's gates, recomputed
      f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, anx = ar, anh = ar;
#pragma unroll
      for (int s = 0; s < S::KSE; ++s) {
        const bf16x8 xf = gr_afrag(s_x[buf], S::LDX, 32 * s, E, lane);
        ar = mfma_16x16x32(xf, wi[0][s], ar);
        az = mfma_16x16x32(xf, wi[1][s], az);
        anx = mfma_16x16x32(xf, wi[2][s], anx);
      }
#pragma unroll
      for (int s = 0; s < S::KSH; ++s) {
        const bf16x8 hf = gr_afrag(s_h[buf], S::LDH, 32 * s, H, lane);
        ar = mfma_16x16x32(hf, wh[0][s], ar);
        az = mfma_16x16x32(hf, wh[1][s], az);
        anh = mfma_16x16x32(hf, wh[2][s], anh);
      }
      float zk[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool live = t < lenC[e];
        const float hp = live && t > 0 ? p.hs[(baseC[e] + t - 1) * H + u] : 0.f;
        const float r = gr_sigmoid(ar[e] + br), z = gr_sigmoid(az[e] + bz);
        const float hn = anh[e] + bnh;
        const float n = gr_tanh(anx[e] + bnx + r * hn);
        const float d = live ? dh[e] : 0.f;
        const float dan = d * (1.f - z) * (1.f - n * n);
        const float dar = dan * hn * r * (1.f - r);
        const float daz = d * (hp - n) * z * (1.f - z);
        const float danr = dan * r;
        zk[e] = z;
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
      __syncthreads();
      // dh <- dh z + dGh W_hh
      f32x4 adh = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < S::KSG; ++s)
        adh = mfma_16x16x32(gr_afrag(s_gh, S::LDG, 32 * s, S::KG, lane), whT[s], adh);
#pragma unroll
      for (int e = 0; e < 4; ++e) dh[e] = t < lenC[e] ? dh[e] * zk[e] + adh[e] : dh[e];
      // dx_t = dGx W_ih
#pragma unroll
      for (int ci = 0; ci < S::CTW; ++ci) {
        const int c = wave + S::NW * ci;
        if (c < S::CT) {
          f32x4 adx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < S::KSG; ++s)
            adx = mfma_16x16x32(gr_afrag(s_gx, S::LDG, 32 * s, S::KG, lane), wiT[ci][s], adx);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (t < lenC[e])
              p.drows[(baseC[e] + t) * p.ld_drows + 16 * c + a] = f32_to_bf16_rne(adx[e]);
        }
      }
      // dW_ih += dGx^T x_t, dW_hh += dGh^T h_{t-1} (h_-1 = 0: nothing at t = 0)
      bf16x4 xT[S::CT], hT[S::NW];
#pragma unroll
      for (int c = 0; c < S::CT; ++c) xT[c] = lds_tr16x4(s_x[buf], S::LDX, 16 * c, lane);
      if (t > 0) {
#pragma unroll
        for (int c = 0; c < S::NW; ++c) hT[c] = lds_tr16x4(s_h[buf], S::LDH, 16 * c, lane);
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
  }
  // the workgroup's partial: [dW_ih | dW_hh | db_ih | db_hh]
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * p.P;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = g * H + 16 * wave + 4 * q + e;
#pragma unroll
      for (int c = 0; c < S::CT; ++c) part[j * E + 16 * c + a] = dwi[g][c][e];
#pragma unroll
      for (int c = 0; c < S::NW; ++c) part[3 * H * E + j * H + 16 * c + a] = dwh[g][c][e];
    }
  }
  // a unit's four row groups (lanes a, a + 16, a + 32, a + 48), added in a fixed order
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    db[k] += __shfl_xor(db[k], 16);
    db[k] += __shfl_xor(db[k], 32);
  }
  if (q == 0) {
    float *bi = part + 3 * H * (E + H), *bh = bi + 3 * H;
    bi[u] = db[0], bi[H + u] = db[1], bi[2 * H + u] = db[2];
    bh[u] = db[0], bh[H + u] = db[1], bh[2 * H + u] = db[3];
  }
}

}  // namespace mrec

using namespace mrec;

namespace {

bool gr_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

mrec_status gr_check(const mrec_gru_args *a, GruArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his_len && a->w_ih && a->w_hh && a->b_ih && a->b_hh && a->hs,
                 "NULL pointer");
  MREC_CHECK_ARG((a->E == 16 || a->E == 32 || a->E == 64) && (a->H == 16 || a->H == 32 || a->H == 64),
                 "E and H must be 16, 32 or 64");
  MREC_CHECK_ARG(a->L >= 1 && a->L <= GR_MAXL, "need 1 <= L <= 64");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->ld_rows >= a->E && a->ld_ih >= a->E && a->ld_hh >= a->H,
                 "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(gr_aligned(a->rows) && a->ld_rows % 8 == 0 && gr_aligned(a->hs),
                 "rows and hs must be 16-byte aligned (ld_rows a multiple of 8 bf16 elements)");
  GruArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his_len = a->his_len;
  p.order = a->order;
  p.w_ih = a->w_ih, p.w_hh = a->w_hh;
  p.ld_ih = a->ld_ih, p.ld_hh = a->ld_hh;
  p.b_ih = a->b_ih, p.b_hh = a->b_hh;
  p.L = a->L;
  p.batch = a->batch;
  p.tiles = (a->batch + GR_TILE - 1) / GR_TILE;
  p.hs = static_cast<float *>(a->hs);
  p.h_last = a->h_last;
  p.oob = a->d_oob_flag;
  p.dh_last = a->dh_last;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  p.P = mrec_gru_param_count(a->E, a->H);
  *out = p;
  return MREC_OK;
}

}  // namespace

extern "C" {

int32_t mrec_gru_supported(int32_t E, int32_t H, int32_t L) {
  return (E == 16 || E == 32 || E == 64) && (H == 16 || H == 32 || H == 64) && L >= 1 && L <= GR_MAXL
             ? 1
             : 0;
}

int32_t mrec_gru_tile(void) { return GR_TILE; }

int64_t mrec_gru_parts(int64_t batch) {
  const int64_t g = device_cus(), tiles = (batch + GR_TILE - 1) / GR_TILE;
  return tiles < g ? (tiles > 0 ? tiles : 1) : g;
}

int64_t mrec_gru_param_count(int32_t E, int32_t H) {
  return 3 * static_cast<int64_t>(H) * (static_cast<int64_t>(E) + H + 2);
}

#define GR_DISPATCH(kernel, what)                                                     \
  X(16, 16, kernel, what) X(16, 32, kernel, what) X(16, 64, kernel, what)             \
  X(32, 16, kernel, what) X(32, 32, kernel, what) X(32, 64, kernel, what)             \
  X(64, 16, kernel, what) X(64, 32, kernel, what) X(64, 64, kernel, what)
#define X(e, h, kernel, what)                                                         \
  if (a->E == e && a->H == h) {                                                       \
    kernel<e, h><<<dim3(grid), GrShape<e, h>::NT, 0, s>>>(p);                         \
    return launch_status(what);                                                       \
  }

mrec_status mrec_gru_fwd(const mrec_gru_args *a, mrec_stream stream) {
  GruArgs p;
  const mrec_status st = gr_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->h_last, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(mrec_gru_parts(p.batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  GR_DISPATCH(gru_fwd_kernel, "mrec_gru_fwd")
  return MREC_EINVAL;
}

mrec_status mrec_gru_bwd(const mrec_gru_args *a, mrec_stream stream) {
  GruArgs p;
  const mrec_status st = gr_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->dh_last && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= a->E && a->ld_drows % 8 == 0 && gr_aligned(a->d_rows),
                 "d_rows must be 16-byte aligned bf16 rows (ld_drows a multiple of 8, >= E)");
  MREC_CHECK_ARG(a->parts == mrec_gru_parts(a->batch), "parts must be mrec_gru_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  GR_DISPATCH(gru_bwd_kernel, "mrec_gru_bwd")
  return MREC_EINVAL;
}

#undef X
#undef GR_DISPATCH

}  // extern "C"
