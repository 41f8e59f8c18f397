// SR-GNN session encoder (Wu et al., AAAI 2019): the session graph, every gated-GNN step and
// the attention readout of one sample in one workgroup, one launch each way for the batch
// (the forward first; the backward's design is above its kernel).
//
//   valid_j = his_j > 0 or j == 0;  alias(j) = the first valid position with the id of j
//   edge a -> b when two consecutive valid positions have aliases a, b (binary, self-loops too)
//   H^0_a = X_a at representative positions (alias(a) == a); the other rows start as zero
//   rows and are unused: no edge touches them, cnt is 0 there and h_last is a representative
//   steps x:  E_in = bf16(H W_ein^T + b_ein),  E_out = bf16(H W_eout^T + b_eout)
//             M_in_b  = bf16(1 / indeg(b)  sum_{a->b} E_in_a  + b_iah)
//             M_out_a = bf16(1 / outdeg(a) sum_{a->b} E_out_b + b_oah)
//             gi = [M_in | M_out] W_ih^T + b_ih,  gh = H W_hh^T + b_hh
//             r = s(gi_r + gh_r), z = s(gi_z + gh_z), c = tanh(gi_c + r gh_c)
//             H <- bf16(c + z (H - c))
//   readout:  beta_a = q . s(W1 h_last + c1 + W2 H_a),  g = sum_a cnt_a beta_a H_a
//             (cnt_a valid positions have alias a: a sum over positions),
//             v = Wt [g | h_last] + bt
//
// Everything stays in position space: a sample is a [64][D] tile whose rows at duplicate and
// invalid positions take no part (no edge touches them and cnt is 0 there), so there is no
// unique, sort or compaction, on the host or here.
//
// Work split: a persistent grid of 8-wave workgroups, one sample at a time per workgroup.
// Graph: every wave holds position j's id in lane j and finds alias, successor and cnt with
// lane broadcasts and one ballot; wave 0 sets the edges in the binary bf16 tile Adj [64][72],
// waves 0 and 1 count its rows and columns into the fp32 1 / deg vectors.  The transposed
// product A_in reads Adj through the transposing LDS reads; there is no second tile.
// Weights: every product's B operand lives in registers for the workgroup's life.  A wave
// owns one 16-column tile of each product: of [E_in | E_out] and [M_in | M_out] (2 D / 16
// column tiles, the wave's row tiles strided), of the three gates at one 16-wide slice of D
// (so r, z, c and the update of an element are lane-local), and of [W1 | W2] in the readout.
// At D = 64 that is 2 + 18 + 2 fragments, 88 VGPRs, and 16 more for the wave's slice of Wt.
// Activations: H, E_in, E_out [64][72] bf16 (the new H is written over E_in and the three
// rotate), M [64][136] bf16 (the readout's fp32 [64][68] scores reuse it), Adj: 53 KiB with
// the small vectors.  Three workgroup barriers per step; nothing is written to global memory
// but v.  No atomics, and a sample's tiles are written in full before they are read: a
// sample's bits do not depend on its place in the batch.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int SG_ROWS = 64;  // positions per sample, padded
constexpr int SG_LD = 72;    // bf16 elements per [64][D] tile row (144 B)
constexpr int SG_LDM = 136;  // bf16 elements per [64][2 D] tile row (272 B)
constexpr int SG_LDY = 68;   // fp32 elements per readout score row (the same 272 B)
constexpr int SG_WAVES = 8;
constexpr int SG_THREADS = 64 * SG_WAVES;
constexpr int SG_TILE_B = SG_ROWS * SG_LD * 2;
constexpr int SG_M_B = SG_ROWS * SG_LDM * 2;
// fp32 vectors: 1 / indeg, 1 / outdeg, cnt, the node weights, t1 [64] each, g partials
// [8][64], the readout input [g | h_last] [128]
constexpr int SG_VEC_F = 5 * 64 + 8 * 64 + 128;
constexpr int SG_LDS_B = 4 * SG_TILE_B + SG_M_B + SG_VEC_F * 4;
constexpr int SG_MAX_STEPS = 4;
constexpr uint16_t SG_ONE = 0x3F80;  // bf16 1.0

struct SrgnnArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const float *w_ein, *w_eout, *w_ih, *w_hh, *w1, *w2, *wt;  // contiguous fp32
  const float *b_ein, *b_eout, *b_iah, *b_oah, *b_ih, *b_hh, *c1, *q, *bt;
  int64_t batch;
  int L, steps;
  float *v;  // [batch, D]
  uint16_t *hs;  // [steps][batch][L][D] bf16: H after each step (may be NULL in the forward)
  const float *dv;
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][15 D D + 13 D]
};

// rows i0 .. i0 + 15 of a row-major LDS tile as an MFMA operand: element (i0 + (lane & 15),
// k0 + 8 (lane >> 4) + e)
__device__ __forceinline__ bf16x8 sg_frag_row(const uint16_t *t, int ld, int i0, int k0, int lane) {
  return *reinterpret_cast<const bf16x8 *>(t + (i0 + (lane & 15)) * ld + k0 + 8 * (lane >> 4));
}
// columns i0 .. i0 + 15 through the transposing reads: element (i, k) is t[k0 + k][i0 + i];
// every address lies inside the 64-row tile
__device__ __forceinline__ bf16x8 sg_frag_tr(const uint16_t *t, int ld, int i0, int k0, int lane) {
  const int li = lane & 15;
  return lds_tr16_pair(t + (k0 + 8 * (lane >> 4) + (li >> 2)) * ld + i0 + 4 * (li & 3), 4 * ld);
}
// rows n0 .. n0 + 15 of an fp32 weight [., K] as the B operand (column n of the product is
// row n of the weight); zero past K
__device__ __forceinline__ bf16x8 sg_wfrag(const float *w, int K, int n0, int k0, int lane) {
  const int k = k0 + 8 * (lane >> 4);
  if (k >= K) return frag_zero8();
  const float *p = w + static_cast<int64_t>(n0 + (lane & 15)) * K + k;
  return frag_from_f32(*reinterpret_cast<const uint4 *>(p), *reinterpret_cast<const uint4 *>(p + 4));
}
// sum over the 8 lanes 8 i .. 8 i + 7, every lane gets it
__device__ __forceinline__ float sg_sum8(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
}

// the session graph of one sample in a wave's registers (lane j: position j)
struct SgGraph {
  bool ok;                             // the position is valid
  unsigned long long repmask, later;   // representatives; the valid positions after this lane
  int alias, nalias, cnt, last;        // alias, the successor's alias, positions with alias ==
};                                     // lane, the last valid position's alias
__device__ __forceinline__ SgGraph sg_graph(const int32_t *his, int L, int lane) {
  SgGraph G;
  const int id = lane < L ? his[lane] : 0;
  G.ok = lane < L && (lane == 0 || id > 0);
  const unsigned long long mask = __ballot(G.ok);
  int alias = lane;
  for (int i = L - 1; i >= 0; --i) {
    const int idi = __shfl(id, i);
    if (((mask >> i) & 1) && idi == id) alias = i;
  }
  if (!G.ok) alias = -1;
  G.alias = alias;
  G.repmask = __ballot(G.ok && alias == lane);
  int cnt = 0;
  for (int i = 0; i < L; ++i) cnt += __shfl(alias, i) == lane ? 1 : 0;
  G.cnt = cnt;
  G.later = lane >= 63 ? 0ull : mask & ~((2ull << lane) - 1ull);
  G.nalias = __shfl(alias, G.later ? __builtin_ctzll(G.later) : 0);
  G.last = __shfl(alias, 63 - __builtin_clzll(mask));  // (bit 0 is always set)
  return G;
}
// the binary adjacency tile and the fp32 1 / deg and cnt vectors; every thread calls it, and
// what the caller wrote to LDS before is visible after
__device__ __forceinline__ void sg_adjacency(const SgGraph &G, uint16_t *Adj, float *sIn, float *sOut,
                                             float *cntS, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int o = tid * 16; o < SG_TILE_B; o += SG_THREADS * 16)
    *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(Adj) + o) = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (wave == 0 && G.ok && G.later) Adj[G.alias * SG_LD + G.nalias] = SG_ONE;
  __syncthreads();
  if (wave == 0) {  // out-degree: row `lane`
    int n = 0;  // (an entry is 0 or 0x3F80: bit 7 of each half word counts it)
    for (int c = 0; c < SG_ROWS; c += 8) {
      const uint4 x = *reinterpret_cast<const uint4 *>(Adj + lane * SG_LD + c);
      n += __popc(x.x & 0x00800080u) + __popc(x.y & 0x00800080u) + __popc(x.z & 0x00800080u) +
           __popc(x.w & 0x00800080u);
    }
    sOut[lane] = 1.f / static_cast<float>(n > 0 ? n : 1);
  } else if (wave == 1) {  // in-degree: column `lane`
    int n = 0;
    for (int r = 0; r < SG_ROWS; ++r) n += Adj[r * SG_LD + lane] ? 1 : 0;
    sIn[lane] = 1.f / static_cast<float>(n > 0 ? n : 1);
  } else if (wave == 2) {
    cntS[lane] = static_cast<float>(G.cnt);
  }
  __syncthreads();
}

template <int D>
__global__ __launch_bounds__(SG_THREADS, 1) void srgnn_fwd_kernel(SrgnnArgs p) {
  constexpr int NT = D / 16;          // column tiles of a [., D] product
  constexpr int NC = 2 * NT;          // column tiles of a [., 2 D] product
  constexpr int KS = (D + 31) / 32;   // k steps over D
  constexpr int KS2 = (2 * D) / 32;   // k steps over 2 D
  constexpr int CH = D / 8;           // 16-byte chunks per row
  constexpr int SUB = D / 8;          // elements of D per lane of an 8-lane group
  extern __shared__ __attribute__((aligned(16))) char sg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  uint16_t *Adj = reinterpret_cast<uint16_t *>(sg_smem);
  uint16_t *T = Adj + SG_ROWS * SG_LD;  // three [64][72] tiles
  uint16_t *Ms = T + 3 * SG_ROWS * SG_LD;
  float *Ys = reinterpret_cast<float *>(Ms);
  float *sIn = reinterpret_cast<float *>(sg_smem + 4 * SG_TILE_B + SG_M_B);
  float *sOut = sIn + 64, *cntS = sIn + 128, *wnode = sIn + 192, *t1 = sIn + 256;
  float *gpart = sIn + 320, *gin = sIn + 320 + 512;
  for (int o = tid * 16; o < SG_LDS_B; o += SG_THREADS * 16)
    *reinterpret_cast<uint4 *>(sg_smem + o) = make_uint4(0, 0, 0, 0);

  const int L = p.L, MT = (L + 15) / 16, JS = (L + 31) / 32;
  // the wave's tiles: column tile ct of the 2 D-wide products, slice dt of the gates
  const int ct = wave % NC, mt0c = wave / NC, dmtc = SG_WAVES / NC;
  const int dt = wave % NT, mt0d = wave / NT, dmtd = SG_WAVES / NT;
  const bool second = ct >= NT;  // E_out / M_out / W2 half
  const int cc = 16 * (ct % NT) + li;  // the lane's column inside its half
  bf16x8 we[KS], wr[KS], wi[3][KS2], wh[3][KS];
  float be, bm, bc1;
  {
    const float *W = second ? p.w_eout : p.w_ein, *R = second ? p.w2 : p.w1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      we[s] = sg_wfrag(W, D, 16 * (ct % NT), 32 * s, lane);
      wr[s] = sg_wfrag(R, D, 16 * (ct % NT), 32 * s, lane);
    }
    be = (second ? p.b_eout : p.b_ein)[cc];
    bm = (second ? p.b_oah : p.b_iah)[cc];
    bc1 = p.c1[cc];
  }
  float brz[2], bci, bch;
#pragma unroll
  for (int gt = 0; gt < 3; ++gt) {
#pragma unroll
    for (int s = 0; s < KS2; ++s) wi[gt][s] = sg_wfrag(p.w_ih, 2 * D, gt * D + 16 * dt, 32 * s, lane);
#pragma unroll
    for (int s = 0; s < KS; ++s) wh[gt][s] = sg_wfrag(p.w_hh, D, gt * D + 16 * dt, 32 * s, lane);
  }
  brz[0] = p.b_ih[16 * dt + li] + p.b_hh[16 * dt + li];
  brz[1] = p.b_ih[D + 16 * dt + li] + p.b_hh[D + 16 * dt + li];
  bci = p.b_ih[2 * D + 16 * dt + li];
  bch = p.b_hh[2 * D + 16 * dt + li];
  // the readout's last product: thread (d = tid >> 3, sub = tid & 7) owns 2 D / 8 inputs
  const int rd = tid >> 3, rs = tid & 7;
  float wtr[2 * SUB], qv[SUB];
#pragma unroll
  for (int i = 0; i < 2 * SUB; ++i) wtr[i] = rd < D ? p.wt[rd * 2 * D + rs * 2 * SUB + i] : 0.f;
#pragma unroll
  for (int i = 0; i < SUB; ++i) qv[i] = p.q[rs * SUB + i];
  const float btv = rd < D ? p.bt[rd] : 0.f;
  __syncthreads();

  for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
    const SgGraph G = sg_graph(p.his + b * p.ld_his, L, lane);
    const unsigned long long repmask = G.repmask;
    const int last = G.last;

    uint16_t *H = T, *Ei = T + SG_ROWS * SG_LD, *Eo = T + 2 * SG_ROWS * SG_LD;
    for (int t = tid; t < 16 * MT * CH; t += SG_THREADS) {
      const int j = t / CH, c = (t % CH) * 8;
      uint4 x = make_uint4(0, 0, 0, 0);
      if ((repmask >> j) & 1) x = *reinterpret_cast<const uint4 *>(p.rows + (b * L + j) * p.ld_rows + c);
      *reinterpret_cast<uint4 *>(H + j * SG_LD + c) = x;
    }
    sg_adjacency(G, Adj, sIn, sOut, cntS, tid);

    for (int step = 0; step < p.steps; ++step) {
      // [E_in | E_out] = H [W_ein; W_eout]^T + b
      uint16_t *E = second ? Eo : Ei;
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma_16x16x32(sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane), we[s], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) E[(16 * mt + 4 * g + e) * SG_LD + cc] = f32_to_bf16_rne(acc[e] + be);
      }
      __syncthreads();
      // M_in = A_in E_in + b_iah (Adj transposed), M_out = A_out E_out + b_oah
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < JS; ++s) {
          const bf16x8 a = second ? sg_frag_row(Adj, SG_LD, 16 * mt, 32 * s, lane)
                                  : sg_frag_tr(Adj, SG_LD, 16 * mt, 32 * s, lane);
          acc = mfma_16x16x32(a, sg_frag_tr(E, SG_LD, 16 * (ct % NT), 32 * s, lane), acc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * mt + 4 * g + e;
          const float sc = second ? sOut[row] : sIn[row];
          Ms[row * SG_LDM + 16 * ct + li] = f32_to_bf16_rne(fmaf(acc[e], sc, bm));
        }
      }
      __syncthreads();
      // the gates of slice dt and the update, lane-local; the new H goes over E_in
      for (int mt = mt0d; mt < MT; mt += dmtd) {
        f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, ai = ar, ah = ar;
#pragma unroll
        for (int s = 0; s < KS2; ++s) {
          const bf16x8 a = sg_frag_row(Ms, SG_LDM, 16 * mt, 32 * s, lane);
          ar = mfma_16x16x32(a, wi[0][s], ar);
          az = mfma_16x16x32(a, wi[1][s], az);
          ai = mfma_16x16x32(a, wi[2][s], ai);
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const bf16x8 a = sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane);
          ar = mfma_16x16x32(a, wh[0][s], ar);
          az = mfma_16x16x32(a, wh[1][s], az);
          ah = mfma_16x16x32(a, wh[2][s], ah);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = (16 * mt + 4 * g + e) * SG_LD + 16 * dt + li;
          const float r = sigmoid_stable(ar[e] + brz[0]), z = sigmoid_stable(az[e] + brz[1]);
          const float c = tanh_rcp(ai[e] + bci + r * (ah[e] + bch));
          const uint16_t hn = f32_to_bf16_rne(fmaf(z, bf16_to_f32(H[o]) - c, c));
          Ei[o] = hn;
          const int row = 16 * mt + 4 * g + e;
          if (p.hs && row < L) p.hs[((step * p.batch + b) * L + row) * D + 16 * dt + li] = hn;
        }
      }
      __syncthreads();
      uint16_t *old = H;
      H = Ei;
      Ei = old;
    }

    // ---- readout ----
    // t1 = W1 h_last + c1 (the row tile of `last` only), Y = H W2^T (fp32, over M)
    for (int mt = mt0c; mt < MT; mt += dmtc) {
      if (!second && mt != (last >> 4)) continue;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = mfma_16x16x32(sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane), wr[s], acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * mt + 4 * g + e;
        if (second)
          Ys[row * SG_LDY + cc] = acc[e];
        else if (row == last)
          t1[cc] = acc[e] + bc1;
      }
    }
    __syncthreads();
    {  // node weights cnt_a beta_a: 8 lanes per node
      const int a = rd;
      float s = 0.f;
      if (a < 16 * MT) {
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          const int d = rs * SUB + i;
          s = fmaf(qv[i], sigmoid_stable(t1[d] + Ys[a * SG_LDY + d]), s);
        }
      }
      s = sg_sum8(s);
      if (rs == 0) wnode[a] = cntS[a] > 0.f ? cntS[a] * s : 0.f;
    }
    __syncthreads();
    if (lane < D) {  // g partials: wave w sums nodes 8 w .. 8 w + 7 in order
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(wnode[8 * wave + i], bf16_to_f32(H[(8 * wave + i) * SG_LD + lane]), s);
      gpart[wave * 64 + lane] = s;
    }
    __syncthreads();
    if (tid < D) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < SG_WAVES; ++w) s += gpart[w * 64 + tid];
      gin[tid] = s;
    } else if (tid < 2 * D) {
      gin[tid] = bf16_to_f32(H[last * SG_LD + tid - D]);
    }
    __syncthreads();
    {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 2 * SUB; ++i) s = fmaf(wtr[i], gin[rs * 2 * SUB + i], s);
      s = sg_sum8(s);
      if (rs == 0 && rd < D) p.v[b * D + rd] = s + btv;
    }
    // (the next sample writes Adj, H and the vectors only after barriers of its own, and
    // gin again after several more)
  }
}

// ---------------------------------------------------------------------------
// backward: per sample the readout's gradient from the saved H^S, then every step from the
// last, each recomputed from its saved input (H^0 from the rows).  dH [64][D] stays in the
// accumulator layout of the wave that owns the gate slice; dG_i, dG_h [64][200], dM and dE
// go through LDS as bf16 tiles.  The weights of the recompute and of the transposed products
// come from global memory (L2) at use.  Dense gradients: the seven matrices' products dG^T X
// (both operands through the transposing reads, contraction over the positions) stay in MFMA
// accumulators over the workgroup's samples, W1 and Wt (rank one per sample) and the vectors
// in fp32 registers; the workgroup writes one partial.  No atomics.
// ---------------------------------------------------------------------------
constexpr int SG_LDG = 200;  // bf16 elements per [64][3 D] tile row (400 B)
constexpr int SG_G_B = SG_ROWS * SG_LDG * 2;
constexpr int SG_BVEC_F = SG_VEC_F + 128 + 64 + 64;  // + d[g | h_last], d beta, d t1
constexpr int SG_BWD_LDS_B = 4 * SG_TILE_B + SG_M_B + 2 * SG_G_B + SG_BVEC_F * 4;

// B operand of a product with a weight's transpose: element (column n0 + (lane & 15), k) is
// w[k0 + k][n0 + ..] of an fp32 [K, ld] matrix; zero past K
__device__ __forceinline__ bf16x8 sg_wfrag_t(const float *w, int K, int ld, int n0, int k0, int lane) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + 8 * (lane >> 4) + i;
    f[i] = k < K ? w[static_cast<int64_t>(k) * ld + n0 + (lane & 15)] : 0.f;
  }
  return frag_pack8(f);
}
// the same over the stacked [w0; w1], each [D, D]
__device__ __forceinline__ bf16x8 sg_wfrag_t2(const float *w0, const float *w1, int D, int n0, int k0, int lane) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + 8 * (lane >> 4) + i;
    f[i] = k < D ? w0[k * D + n0 + (lane & 15)] : w1[(k - D) * D + n0 + (lane & 15)];
  }
  return frag_pack8(f);
}
// per-lane column sums (column 16 (wave % nown) + (lane & 15)) added over the lanes and waves
// that own the column, in a fixed order -> out[0 .. 16 nown)
__device__ __forceinline__ void sg_reduce_cols(float v, int nown, float *red, float *out, int tid) {
  red[tid] = v;
  __syncthreads();
  if (tid < 16 * nown) {
    float s = 0.f;
    for (int w = tid >> 4; w < SG_WAVES; w += nown)
#pragma unroll
      for (int g = 0; g < 4; ++g) s += red[w * 64 + 16 * g + (tid & 15)];
    out[tid] = s;
  }
  __syncthreads();
}

template <int D>
__global__ __launch_bounds__(SG_THREADS, 1) void srgnn_bwd_kernel(SrgnnArgs p) {
  constexpr int NT = D / 16, NC = 2 * NT, KS = (D + 31) / 32, KS2 = (2 * D) / 32, KS3 = (3 * D + 31) / 32;
  constexpr int CH = D / 8, SUB = D / 8, NR = (4 * NT + 7) / 8;
  constexpr int T_IH = 3 * NT * NC, T_HH = 3 * NT * NT, T_E = NC * NT, T_W2 = NT * NT;
  constexpr int A_IH = (T_IH + 7) / 8, A_HH = (T_HH + 7) / 8, A_E = (T_E + 7) / 8, A_W2 = (T_W2 + 7) / 8;
  constexpr int DD = D * D;
  extern __shared__ __attribute__((aligned(16))) char sg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  uint16_t *Adj = reinterpret_cast<uint16_t *>(sg_smem);
  uint16_t *H = Adj + SG_ROWS * SG_LD, *Ei = H + SG_ROWS * SG_LD, *Eo = Ei + SG_ROWS * SG_LD;
  uint16_t *Ms = Eo + SG_ROWS * SG_LD;
  uint16_t *Gi = Ms + SG_ROWS * SG_LDM, *Gh = Gi + SG_ROWS * SG_LDG;
  uint16_t *Dp = Gi;  // the readout's d pre [64][72], before the steps
  float *Ys = reinterpret_cast<float *>(Ms);
  float *sIn = reinterpret_cast<float *>(sg_smem + 4 * SG_TILE_B + SG_M_B + 2 * SG_G_B);
  float *sOut = sIn + 64, *cntS = sIn + 128, *wnode = sIn + 192, *t1 = sIn + 256;
  float *gpart = sIn + 320, *gin = sIn + 832, *dgin = sIn + 960, *dbeta = sIn + 1088, *dt1 = sIn + 1152;
  for (int o = tid * 16; o < SG_BWD_LDS_B; o += SG_THREADS * 16)
    *reinterpret_cast<uint4 *>(sg_smem + o) = make_uint4(0, 0, 0, 0);

  const int L = p.L, MT = (L + 15) / 16, JS = (L + 31) / 32;
  const int ct = wave % NC, mt0c = wave / NC, dmtc = SG_WAVES / NC;
  const int dt = wave % NT, mt0d = wave / NT, dmtd = SG_WAVES / NT;
  const bool second = ct >= NT;
  const int cc = 16 * (ct % NT) + li;
  bf16x8 we[KS], wr[KS];
  const float *Wr = second ? p.w2 : p.w1;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    we[s] = sg_wfrag(second ? p.w_eout : p.w_ein, D, 16 * (ct % NT), 32 * s, lane);
    wr[s] = sg_wfrag(Wr, D, 16 * (ct % NT), 32 * s, lane);
  }
  const float be = (second ? p.b_eout : p.b_ein)[cc], bm = (second ? p.b_oah : p.b_iah)[cc], bc1 = p.c1[cc];
  const float brz0 = p.b_ih[16 * dt + li] + p.b_hh[16 * dt + li];
  const float brz1 = p.b_ih[D + 16 * dt + li] + p.b_hh[D + 16 * dt + li];
  const float bci = p.b_ih[2 * D + 16 * dt + li], bch = p.b_hh[2 * D + 16 * dt + li];
  const int rd = tid >> 3, rs = tid & 7;
  float qv[SUB];
#pragma unroll
  for (int i = 0; i < SUB; ++i) qv[i] = p.q[rs * SUB + i];
  const float qd = tid < D ? p.q[tid] : 0.f;

  // the workgroup's dense-gradient partial
  f32x4 a_ih[A_IH], a_hh[A_HH], a_e[A_E], a_w2[A_W2];
#pragma unroll
  for (int i = 0; i < A_IH; ++i) a_ih[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < A_HH; ++i) a_hh[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < A_E; ++i) a_e[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < A_W2; ++i) a_w2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dwt[2 * SUB], dw1[SUB];
#pragma unroll
  for (int i = 0; i < 2 * SUB; ++i) dwt[i] = 0.f;
#pragma unroll
  for (int i = 0; i < SUB; ++i) dw1[i] = 0.f;
  float dbe = 0.f, dbm = 0.f, dbi0 = 0.f, dbi1 = 0.f, dbi2 = 0.f, dbh2 = 0.f;  // per-lane column sums
  float dq = 0.f, dc1 = 0.f, dbt = 0.f;                                          // thread d < D
  __syncthreads();

  for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
    const SgGraph G = sg_graph(p.his + b * p.ld_his, L, lane);
    const int last = G.last;
    {  // H^S
      const uint16_t *hs = p.hs + ((p.steps - 1) * p.batch + b) * L * D;
      for (int t = tid; t < 16 * MT * CH; t += SG_THREADS) {
        const int j = t / CH, c = (t % CH) * 8;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (j < L) x = *reinterpret_cast<const uint4 *>(hs + j * D + c);
        *reinterpret_cast<uint4 *>(H + j * SG_LD + c) = x;
      }
    }
    sg_adjacency(G, Adj, sIn, sOut, cntS, tid);

    // ---- the readout again: t1, Y, the node weights, [g | h_last] ----
    for (int mt = mt0c; mt < MT; mt += dmtc) {
      if (!second && mt != (last >> 4)) continue;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = mfma_16x16x32(sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane), wr[s], acc);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * mt + 4 * g + e;
        if (second)
          Ys[row * SG_LDY + cc] = acc[e];
        else if (row == last)
          t1[cc] = acc[e] + bc1;
      }
    }
    __syncthreads();
    {
      float s = 0.f;
      if (rd < 16 * MT) {
#pragma unroll
        for (int i = 0; i < SUB; ++i) {
          const int d = rs * SUB + i;
          s = fmaf(qv[i], sigmoid_stable(t1[d] + Ys[rd * SG_LDY + d]), s);
        }
      }
      s = sg_sum8(s);
      if (rs == 0) wnode[rd] = cntS[rd] > 0.f ? cntS[rd] * s : 0.f;
    }
    __syncthreads();
    if (lane < D) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s = fmaf(wnode[8 * wave + i], bf16_to_f32(H[(8 * wave + i) * SG_LD + lane]), s);
      gpart[wave * 64 + lane] = s;
    }
    __syncthreads();
    if (tid < D) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < SG_WAVES; ++w) s += gpart[w * 64 + tid];
      gin[tid] = s;
    } else if (tid < 2 * D) {
      gin[tid] = bf16_to_f32(H[last * SG_LD + tid - D]);
    }
    __syncthreads();
    // ---- the readout's gradient ----
    const float *dv = p.dv + b * D;
    {  // v = Wt [g | h_last] + bt
      const float dvr = rd < D ? dv[rd] : 0.f;
#pragma unroll
      for (int i = 0; i < 2 * SUB; ++i) dwt[i] = fmaf(dvr, gin[rs * 2 * SUB + i], dwt[i]);
      if (tid < D) dbt += dv[tid];
      if (tid < 2 * D) {
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(p.wt[d * 2 * D + tid], dv[d], s);
        dgin[tid] = s;
      }
    }
    __syncthreads();
    {  // d beta_a = cnt_a dg . H_a
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < SUB; ++i) s = fmaf(dgin[rs * SUB + i], bf16_to_f32(H[rd * SG_LD + rs * SUB + i]), s);
      s = sg_sum8(s);
      if (rs == 0) dbeta[rd] = cntS[rd] > 0.f ? cntS[rd] * s : 0.f;
    }
    __syncthreads();
    {  // d pre = d beta q s (1 - s): the tile for the products, its column sums for c1 and t1
      const float db = dbeta[rd];
#pragma unroll
      for (int i = 0; i < SUB; ++i) {
        const int d = rs * SUB + i;
        float v = 0.f;
        if (rd < 16 * MT) {
          const float sg = sigmoid_stable(t1[d] + Ys[rd * SG_LDY + d]);
          v = db * qv[i] * sg * (1.f - sg);
        }
        Dp[rd * SG_LD + d] = f32_to_bf16_rne(v);
      }
      if (tid < D) {
        float s = 0.f;
        for (int a = 0; a < 16 * MT; ++a) {
          const float sg = sigmoid_stable(t1[tid] + Ys[a * SG_LDY + tid]);
          dq = fmaf(dbeta[a], sg, dq);
          s = fmaf(dbeta[a] * qd, sg * (1.f - sg), s);
        }
        dt1[tid] = s;
        dc1 += s;
      }
    }
    __syncthreads();
    f32x4 dH[NR];
    {
      if (rd < D) {
#pragma unroll
        for (int i = 0; i < SUB; ++i) dw1[i] = fmaf(dt1[rd], gin[D + rs * SUB + i], dw1[i]);
      }
      if (tid < D) {  // d h_last += W1^T d t1
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(bf16_to_f32(f32_to_bf16_rne(p.w1[d * D + tid])), dt1[d], s);
        dgin[D + tid] += s;
      }
#pragma unroll
      for (int i = 0; i < A_W2; ++i) {
        const int t = wave + 8 * i;
        if (t < T_W2)
          for (int s = 0; s < JS; ++s)
            a_w2[i] = mfma_16x16x32(sg_frag_tr(Dp, SG_LD, 16 * (t / NT), 32 * s, lane),
                                    sg_frag_tr(H, SG_LD, 16 * (t % NT), 32 * s, lane), a_w2[i]);
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        dH[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int mt = mt0d + r * dmtd;
        if (mt < MT) {
#pragma unroll
          for (int s = 0; s < KS; ++s)
            dH[r] = mfma_16x16x32(sg_frag_row(Dp, SG_LD, 16 * mt, 32 * s, lane),
                                  sg_wfrag_t(p.w2, D, D, 16 * dt, 32 * s, lane), dH[r]);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int mt = mt0d + r * dmtd;
      if (mt < MT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * mt + 4 * g + e, col = 16 * dt + li;
          dH[r][e] += wnode[row] * dgin[col] + (row == last ? dgin[D + col] : 0.f);
        }
      }
    }
    __syncthreads();  // H^S, Dp and the vectors are dead

    // ---- the steps, from the last ----
    for (int step = p.steps; step >= 1; --step) {
      {  // the step's input: H^(step - 1)
        const uint16_t *hs = step > 1 ? p.hs + ((step - 2) * p.batch + b) * L * D : nullptr;
        for (int t = tid; t < 16 * MT * CH; t += SG_THREADS) {
          const int j = t / CH, c = (t % CH) * 8;
          uint4 x = make_uint4(0, 0, 0, 0);
          if (hs) {
            if (j < L) x = *reinterpret_cast<const uint4 *>(hs + j * D + c);
          } else if ((G.repmask >> j) & 1) {
            x = *reinterpret_cast<const uint4 *>(p.rows + (b * L + j) * p.ld_rows + c);
          }
          *reinterpret_cast<uint4 *>(H + j * SG_LD + c) = x;
        }
        // (Gi and Gh columns are rewritten in full below; Dp's leftovers lie inside them)
      }
      __syncthreads();
      uint16_t *E = second ? Eo : Ei;
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma_16x16x32(sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane), we[s], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) E[(16 * mt + 4 * g + e) * SG_LD + cc] = f32_to_bf16_rne(acc[e] + be);
      }
      __syncthreads();
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < JS; ++s) {
          const bf16x8 a = second ? sg_frag_row(Adj, SG_LD, 16 * mt, 32 * s, lane)
                                  : sg_frag_tr(Adj, SG_LD, 16 * mt, 32 * s, lane);
          acc = mfma_16x16x32(a, sg_frag_tr(E, SG_LD, 16 * (ct % NT), 32 * s, lane), acc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * mt + 4 * g + e;
          Ms[row * SG_LDM + 16 * ct + li] = f32_to_bf16_rne(fmaf(acc[e], second ? sOut[row] : sIn[row], bm));
        }
      }
      __syncthreads();
      // the gates again and their gradients: d G_i, d G_h, dH z
      f32x4 dHc[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        dHc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int mt = mt0d + r * dmtd;
        if (mt < MT) {
          f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, ai = ar, ah = ar;
#pragma unroll
          for (int s = 0; s < KS2; ++s) {
            const bf16x8 a = sg_frag_row(Ms, SG_LDM, 16 * mt, 32 * s, lane);
            ar = mfma_16x16x32(a, sg_wfrag(p.w_ih, 2 * D, 16 * dt, 32 * s, lane), ar);
            az = mfma_16x16x32(a, sg_wfrag(p.w_ih, 2 * D, D + 16 * dt, 32 * s, lane), az);
            ai = mfma_16x16x32(a, sg_wfrag(p.w_ih, 2 * D, 2 * D + 16 * dt, 32 * s, lane), ai);
          }
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const bf16x8 a = sg_frag_row(H, SG_LD, 16 * mt, 32 * s, lane);
            ar = mfma_16x16x32(a, sg_wfrag(p.w_hh, D, 16 * dt, 32 * s, lane), ar);
            az = mfma_16x16x32(a, sg_wfrag(p.w_hh, D, D + 16 * dt, 32 * s, lane), az);
            ah = mfma_16x16x32(a, sg_wfrag(p.w_hh, D, 2 * D + 16 * dt, 32 * s, lane), ah);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int row = 16 * mt + 4 * g + e, col = 16 * dt + li;
            const float r_ = sigmoid_stable(ar[e] + brz0), z = sigmoid_stable(az[e] + brz1);
            const float ghc = ah[e] + bch, c = tanh_rcp(ai[e] + bci + r_ * ghc);
            const float h = bf16_to_f32(H[row * SG_LD + col]), gd = dH[r][e];
            const float dcp = gd * (1.f - z) * (1.f - c * c), dzp = gd * (h - c) * z * (1.f - z);
            const float drp = dcp * ghc * r_ * (1.f - r_), dch = dcp * r_;
            uint16_t *gi = Gi + row * SG_LDG + col, *gh = Gh + row * SG_LDG + col;
            gi[0] = gh[0] = f32_to_bf16_rne(drp);
            gi[D] = gh[D] = f32_to_bf16_rne(dzp);
            gi[2 * D] = f32_to_bf16_rne(dcp);
            gh[2 * D] = f32_to_bf16_rne(dch);
            dbi0 += drp, dbi1 += dzp, dbi2 += dcp, dbh2 += dch;
            dHc[r][e] = gd * z;
          }
        }
      }
      __syncthreads();
      // dM = dG_i W_ih, scaled by 1 / deg into the E tiles; dH += dG_h W_hh; dW_ih, dW_hh
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS3; ++s)
          acc = mfma_16x16x32(sg_frag_row(Gi, SG_LDG, 16 * mt, 32 * s, lane),
                              sg_wfrag_t(p.w_ih, 3 * D, 2 * D, 16 * ct, 32 * s, lane), acc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * mt + 4 * g + e;
          dbm += acc[e];
          E[row * SG_LD + cc] = f32_to_bf16_rne(acc[e] * (second ? sOut[row] : sIn[row]));
        }
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int mt = mt0d + r * dmtd;
        if (mt < MT) {
#pragma unroll
          for (int s = 0; s < KS3; ++s)
            dHc[r] = mfma_16x16x32(sg_frag_row(Gh, SG_LDG, 16 * mt, 32 * s, lane),
                                   sg_wfrag_t(p.w_hh, 3 * D, D, 16 * dt, 32 * s, lane), dHc[r]);
        }
      }
#pragma unroll
      for (int i = 0; i < A_IH; ++i) {
        const int t = wave + 8 * i;
        if (t < T_IH)
          for (int s = 0; s < JS; ++s)
            a_ih[i] = mfma_16x16x32(sg_frag_tr(Gi, SG_LDG, 16 * (t / NC), 32 * s, lane),
                                    sg_frag_tr(Ms, SG_LDM, 16 * (t % NC), 32 * s, lane), a_ih[i]);
      }
#pragma unroll
      for (int i = 0; i < A_HH; ++i) {
        const int t = wave + 8 * i;
        if (t < T_HH)
          for (int s = 0; s < JS; ++s)
            a_hh[i] = mfma_16x16x32(sg_frag_tr(Gh, SG_LDG, 16 * (t / NT), 32 * s, lane),
                                    sg_frag_tr(H, SG_LD, 16 * (t % NT), 32 * s, lane), a_hh[i]);
      }
      __syncthreads();
      // dE_in = Adj (s_in dM_in), dE_out = Adj^T (s_out dM_out), over M
      for (int mt = mt0c; mt < MT; mt += dmtc) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < JS; ++s) {
          const bf16x8 a = second ? sg_frag_tr(Adj, SG_LD, 16 * mt, 32 * s, lane)
                                  : sg_frag_row(Adj, SG_LD, 16 * mt, 32 * s, lane);
          acc = mfma_16x16x32(a, sg_frag_tr(E, SG_LD, 16 * (ct % NT), 32 * s, lane), acc);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dbe += acc[e];
          Ms[(16 * mt + 4 * g + e) * SG_LDM + 16 * ct + li] = f32_to_bf16_rne(acc[e]);
        }
      }
      __syncthreads();
      // dH += dE [W_ein; W_eout]; d[W_ein; W_eout] += dE^T H
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int mt = mt0d + r * dmtd;
        if (mt < MT) {
#pragma unroll
          for (int s = 0; s < KS2; ++s)
            dHc[r] = mfma_16x16x32(sg_frag_row(Ms, SG_LDM, 16 * mt, 32 * s, lane),
                                   sg_wfrag_t2(p.w_ein, p.w_eout, D, 16 * dt, 32 * s, lane), dHc[r]);
        }
        dH[r] = dHc[r];
      }
#pragma unroll
      for (int i = 0; i < A_E; ++i) {
        const int t = wave + 8 * i;
        if (t < T_E)
          for (int s = 0; s < JS; ++s)
            a_e[i] = mfma_16x16x32(sg_frag_tr(Ms, SG_LDM, 16 * (t / NT), 32 * s, lane),
                                   sg_frag_tr(H, SG_LD, 16 * (t % NT), 32 * s, lane), a_e[i]);
      }
      __syncthreads();
    }
    // the rows' gradient: a node's on its representative position, zero bits elsewhere
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int mt = mt0d + r * dmtd;
      if (mt < MT) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int row = 16 * mt + 4 * g + e;
          if (row < L)
            p.drows[(b * L + row) * p.ld_drows + 16 * dt + li] =
                ((G.repmask >> row) & 1) ? f32_to_bf16_rne(dH[r][e]) : uint16_t(0);
        }
      }
    }
  }

  // ---- the workgroup's partial: [W_ein, W_eout, W_ih, W_hh, W1, W2, Wt, b_ein, b_eout, b_iah,
  // b_oah, b_ih, b_hh, c1, q, bt] ----
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * (15 * DD + 13 * D);
#pragma unroll
  for (int i = 0; i < A_E; ++i) {
    const int t = wave + 8 * i;
    if (t < T_E)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[(16 * (t / NT) + 4 * g + e) * D + 16 * (t % NT) + li] = a_e[i][e];
  }
#pragma unroll
  for (int i = 0; i < A_IH; ++i) {
    const int t = wave + 8 * i;
    if (t < T_IH)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        part[2 * DD + (16 * (t / NC) + 4 * g + e) * 2 * D + 16 * (t % NC) + li] = a_ih[i][e];
  }
#pragma unroll
  for (int i = 0; i < A_HH; ++i) {
    const int t = wave + 8 * i;
    if (t < T_HH)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[8 * DD + (16 * (t / NT) + 4 * g + e) * D + 16 * (t % NT) + li] = a_hh[i][e];
  }
#pragma unroll
  for (int i = 0; i < A_W2; ++i) {
    const int t = wave + 8 * i;
    if (t < T_W2)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[12 * DD + (16 * (t / NT) + 4 * g + e) * D + 16 * (t % NT) + li] = a_w2[i][e];
  }
  if (rd < D) {
#pragma unroll
    for (int i = 0; i < SUB; ++i) part[11 * DD + rd * D + rs * SUB + i] = dw1[i];
#pragma unroll
    for (int i = 0; i < 2 * SUB; ++i) part[13 * DD + rd * 2 * D + rs * 2 * SUB + i] = dwt[i];
  }
  float *pb = part + 15 * DD;
  if (tid < D) {
    pb[10 * D + tid] = dc1;
    pb[11 * D + tid] = dq;
    pb[12 * D + tid] = dbt;
  }
  float *red = reinterpret_cast<float *>(Gi);
  __syncthreads();
  sg_reduce_cols(dbe, NC, red, pb, tid);
  sg_reduce_cols(dbm, NC, red, pb + 2 * D, tid);
  sg_reduce_cols(dbi0, NT, red, pb + 4 * D, tid);
  sg_reduce_cols(dbi1, NT, red, pb + 5 * D, tid);
  sg_reduce_cols(dbi2, NT, red, pb + 6 * D, tid);
  if (tid < 2 * D) pb[7 * D + tid] = pb[4 * D + tid];  // b_hh's r and z: the sums of b_ih's
  sg_reduce_cols(dbh2, NT, red, pb + 9 * D, tid);
}

}  // namespace mrec

using namespace mrec;

namespace {

bool sg_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

mrec_status sg_check(const mrec_srgnn_args *a, SrgnnArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his, "NULL pointer");
  MREC_CHECK_ARG(a->w_ein && a->w_eout && a->w_ih && a->w_hh && a->w1 && a->w2 && a->wt && a->b_ein &&
                     a->b_eout && a->b_iah && a->b_oah && a->b_ih && a->b_hh && a->c1 && a->q && a->bt,
                 "NULL parameter");
  MREC_CHECK_ARG(mrec_srgnn_supported(a->D, a->L, a->steps),
                 "need D in {16, 32, 64}, 1 <= L <= 64, 1 <= steps <= 4");
  MREC_CHECK_ARG(a->batch >= 0, "negative batch");
  MREC_CHECK_ARG(a->ld_rows >= a->D && a->ld_his >= a->L, "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(sg_aligned(a->rows) && a->ld_rows % 8 == 0,
                 "rows must be 16-byte aligned bf16 rows (ld_rows a multiple of 8)");
  MREC_CHECK_ARG(sg_aligned(a->w_ein) && sg_aligned(a->w_eout) && sg_aligned(a->w_ih) &&
                     sg_aligned(a->w_hh) && sg_aligned(a->w1) && sg_aligned(a->w2),
                 "the weight matrices must be 16-byte aligned");
  MREC_CHECK_ARG(sg_aligned(a->hs), "hs must be 16-byte aligned");
  SrgnnArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his = a->his;
  p.ld_his = a->ld_his;
  p.w_ein = a->w_ein, p.w_eout = a->w_eout, p.w_ih = a->w_ih, p.w_hh = a->w_hh;
  p.w1 = a->w1, p.w2 = a->w2, p.wt = a->wt;
  p.b_ein = a->b_ein, p.b_eout = a->b_eout, p.b_iah = a->b_iah, p.b_oah = a->b_oah;
  p.b_ih = a->b_ih, p.b_hh = a->b_hh, p.c1 = a->c1, p.q = a->q, p.bt = a->bt;
  p.batch = a->batch;
  p.L = a->L;
  p.steps = a->steps;
  p.v = a->v;
  p.hs = static_cast<uint16_t *>(a->hs);
  p.dv = a->dv;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  *out = p;
  return MREC_OK;
}

template <typename Fn>
void sg_dispatch(int D, Fn &&f) {
  if (D == 16)
    f(std::integral_constant<int, 16>{});
  else if (D == 32)
    f(std::integral_constant<int, 32>{});
  else
    f(std::integral_constant<int, 64>{});
}

// workgroups of the forward kernel that run at once (its registers decide per D), found once
template <int D>
int64_t sg_fwd_slots() {
  static const int64_t slots = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(srgnn_fwd_kernel<D>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, SG_LDS_B);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, srgnn_fwd_kernel<D>, SG_THREADS, SG_LDS_B) !=
            hipSuccess || per_cu < 1)
      per_cu = 1;
    (void)hipGetLastError();
    return static_cast<int64_t>(per_cu) * device_cus();
  }();
  return slots;
}

}  // namespace

extern "C" {

int32_t mrec_srgnn_supported(int32_t D, int32_t L, int32_t steps) {
  return (D == 16 || D == 32 || D == 64) && L >= 1 && L <= SG_ROWS && steps >= 1 && steps <= SG_MAX_STEPS ? 1 : 0;
}

int64_t mrec_srgnn_parts(int64_t batch) {
  const int64_t g = device_cus();
  return batch < g ? (batch > 0 ? batch : 1) : g;
}

int64_t mrec_srgnn_param_count(int32_t D) { return 15 * static_cast<int64_t>(D) * D + 13 * D; }

mrec_status mrec_srgnn_fwd(const mrec_srgnn_args *a, mrec_stream stream) {
  SrgnnArgs p;
  const mrec_status st = sg_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  sg_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    const int64_t slots = sg_fwd_slots<D>();
    const unsigned grid = static_cast<unsigned>(p.batch < slots ? p.batch : slots);
    srgnn_fwd_kernel<D><<<dim3(grid), SG_THREADS, SG_LDS_B, s>>>(p);
  });
  return launch_status("mrec_srgnn_fwd");
}

mrec_status mrec_srgnn_bwd(const mrec_srgnn_args *a, mrec_stream stream) {
  SrgnnArgs p;
  const mrec_status st = sg_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->hs && a->dv && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= a->D, "ld_drows is smaller than a row");
  MREC_CHECK_ARG(a->parts == mrec_srgnn_parts(a->batch), "parts must be mrec_srgnn_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  sg_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    static const int once = ((void)hipFuncSetAttribute(reinterpret_cast<const void *>(srgnn_bwd_kernel<D>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, SG_BWD_LDS_B),
                             (void)hipGetLastError(), 1);
    (void)once;
    srgnn_bwd_kernel<D><<<dim3(grid), SG_THREADS, SG_BWD_LDS_B, s>>>(p);
  });
  return launch_status("mrec_srgnn_bwd");
}

}  // extern "C"
