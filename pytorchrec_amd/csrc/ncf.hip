// NCF / NeuMF pair scoring, the whole scorer in one launch each way
// (torchrec/model/NCF.py:53-79).
//
//   rows[p] = [mf_u | mf_i | mlp_u | mlp_i]              bf16, 4E per (user, candidate) pair
//   g       = mf_u * mf_i                                 [E]
//   h_0     = [mlp_u | mlp_i]                             [2E], contiguous in the row
//   h_{l+1} = relu(W_l h_l + b_l)                         l = 0 .. k - 1
//   pred[p] = wp . [g | h_k]
//
// Work split.  Workgroups of four waves are persistent: each loops over tiles of 64
// pairs, four row blocks of 16 (the rows of v_mfma_f32_16x16x32_bf16).  In a layer wave w
// owns the output tiles w and w + 4 (16 units each) for all four row blocks: per k step
// four A fragments and up to two B fragments feed eight independent MFMAs.  A layer's
// output tile (C/D mapping col = lane & 15 -> output unit, row = 4 (lane >> 4) + reg ->
// pair) goes through bias and ReLU in registers and to the next layer's operand columns
// in LDS, rounded to bf16 there and only there; a barrier ends the layer.  The last
// layer's output stays fp32 for the dot with wp.  The forward fetches the next tile's
// rows into registers before the MLP of the current one.
//
// LDS (dynamic: the largest shape needs ~135 KB; the plan is computed on the host and
// travels in the argument block):
//   W images   per layer [pad16(N)][pad32(K) + 8] bf16, "row = output index, contiguous
//              along k", rounded from the fp32 masters once per workgroup, zero padded;
//   H arena    [64][sum pad32(K_l) + 8] bf16: h_l of every layer side by side (the
//              padding columns are zeroed once and never written);
//   Z arena    [64][sum pad16(N_l) + 8] bf16 (backward): dz_l of every layer side by side;
//   fp32       biases, wp, the tile's MLP dots, the final cross-wave sums, the dW tile table.
//
// Backward.  The forward is recomputed with the same MFMAs (the same device function),
// so it sees the forward's bits.  With dz_l = dh_{l+1} [h_{l+1} > 0]:
//   dh_k = dpred wp[E:],  dh_l = dz_l W_l (each wave its own 16 pairs):
//   v_mfma_f32_16x16x16_bf16 whose B operand is a transposing read (ds_read_b64_tr_b16)
//   of the same W image;  dh_0 -> d_rows[:, 2E:];
//   d mf_u = dpred wp[:E] mf_i, d mf_i = dpred wp[:E] mf_u -> d_rows[:, :2E] (VALU);
//   dW_l += dz_l^T h_l: once per tile over all 64 pairs, both operands transposing reads
//   of the arenas, the 16 x 16 tiles of every layer dealt round-robin to the four waves
//   and accumulated in registers over the workgroup's tiles; db, dwp in registers too.
// One fp32 partial per workgroup [dW_0 | .. | db_0 | .. | dwp], summed in workgroup order
// by mrec_sasrec_wgrad.  No atomics; a pair's bits do not depend on its tile or row.
#include "common.h"
#include "ncf_common.h"

namespace mrec {

// h_0 of the tile's pairs -> the H arena (zero rows past `pairs`).  Between barriers of
// the caller.
__device__ __forceinline__ void nc_load_tile(const NcfArgs &p, uint16_t *sm, int64_t tile, int tid) {
  const int ch = p.E / 4;  // 16-B chunks of [mlp_u | mlp_i]
  for (int i = tid; i < NC_TILE * ch; i += NC_THREADS) {
    const int row = i / ch, c = i % ch;
    const int64_t pair = tile * NC_TILE + row;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (pair < p.pairs) v = *reinterpret_cast<const uint4 *>(p.rows + pair * p.ld_rows + 2 * p.E + 8 * c);
    *reinterpret_cast<uint4 *>(sm + p.hbase + row * p.lda + p.hoff[0] + 8 * c) = v;
  }
}

// The same copy in two halves, for the forward's prefetch: a tile's chunks into registers
// (tiles past the end and pairs past `pairs` give zeros), and from there into the arena.
constexpr int NC_PF = NC_TILE * (2 * 64 / 8) / NC_THREADS;  // chunks per thread at E = 64
__device__ __forceinline__ void nc_tile_fetch(const NcfArgs &p, int64_t tile, int tid, uint4 (&st)[NC_PF]) {
  const int ch = p.E / 4;
#pragma unroll
  for (int k = 0; k < NC_PF; ++k) {
    const int i = tid + NC_THREADS * k;
    const int row = i / ch, c = i % ch;
    const int64_t pair = tile * NC_TILE + row;
    st[k] = make_uint4(0, 0, 0, 0);
    if (i < NC_TILE * ch && tile < p.tiles && pair < p.pairs)
      st[k] = *reinterpret_cast<const uint4 *>(p.rows + pair * p.ld_rows + 2 * p.E + 8 * c);
  }
}
__device__ __forceinline__ void nc_tile_put(const NcfArgs &p, uint16_t *sm, int tid, const uint4 (&st)[NC_PF]) {
  const int ch = p.E / 4;
#pragma unroll
  for (int k = 0; k < NC_PF; ++k) {
    const int i = tid + NC_THREADS * k;
    if (i < NC_TILE * ch)
      *reinterpret_cast<uint4 *>(sm + p.hbase + (i / ch) * p.lda + p.hoff[0] + 8 * (i % ch)) = st[k];
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NC_THREADS) void ncf_fwd_kernel(NcfArgs p) {
  extern __shared__ __attribute__((aligned(16))) char nc_lds[];
  uint16_t *sm = reinterpret_cast<uint16_t *>(nc_lds);
  float *sf = reinterpret_cast<float *>(nc_lds + p.fbase);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  nc_stage(p, sm, sf, tid, false);
  float dbl[2], dwph[2];  // (backward only)
  float dp[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dp[rb][e] = 0.f;
  }
  const int chunks = p.E / 8;
  // the next tile's rows travel from HBM while this tile's MLP runs: h_0 in st, the MF
  // halves in mu / mv
  uint4 st[NC_PF], mu[2], mv[2];
  auto fetch_mf = [&](int64_t tile) {
    const int64_t pair = tile * NC_TILE + 16 * wave + a;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = q + 4 * i;
      mu[i] = mv[i] = make_uint4(0, 0, 0, 0);
      if (c < chunks && tile < p.tiles && pair < p.pairs) {
        const uint16_t *r = p.rows + pair * p.ld_rows + 8 * c;
        mu[i] = *reinterpret_cast<const uint4 *>(r);
        mv[i] = *reinterpret_cast<const uint4 *>(r + p.E);
      }
    }
  };
  nc_tile_fetch(p, blockIdx.x, tid, st);
  fetch_mf(blockIdx.x);
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    __syncthreads();
    nc_tile_put(p, sm, tid, st);
    // g . wp[:E]: lane (a, q) takes 8-element chunks q and q + 4 of pair 16 wave + a (zero
    // chunks where there is none)
    const int64_t pair = tile * NC_TILE + 16 * wave + a;
    float gs = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = q + 4 * i;
      if (c < chunks) {
        float u[8], v[8];
        nc_unpack8(mu[i], u);
        nc_unpack8(mv[i], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) gs += sf[p.wpoff + 8 * c + j] * (u[j] * v[j]);
      }
    }
    gs += __shfl_xor(gs, 16);
    gs += __shfl_xor(gs, 32);
    nc_tile_fetch(p, tile + gridDim.x, tid, st);
    fetch_mf(tile + gridDim.x);
    __syncthreads();
    nc_mlp<false>(p, sm, sf, wave, lane, dp, dbl, dwph);
    if (q == 0 && pair < p.pairs) {
      const float *sd = sf + p.dotoff + 16 * wave + a;  // the four waves' parts, in order
      p.pred[pair] = gs + (((sd[0] + sd[NC_TILE]) + sd[2 * NC_TILE]) + sd[3 * NC_TILE]);
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(NC_THREADS) void ncf_bwd_kernel(NcfArgs p) {
  extern __shared__ __attribute__((aligned(16))) char nc_lds[];
  uint16_t *sm = reinterpret_cast<uint16_t *>(nc_lds);
  float *sf = reinterpret_cast<float *>(nc_lds + p.fbase);
  const int *tab = reinterpret_cast<const int *>(sf + p.taboff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int a = lane & 15, q = lane >> 4;
  nc_stage(p, sm, sf, tid, true);
  f32x4 dw[NC_MAXT];
#pragma unroll
  for (int t = 0; t < NC_MAXT; ++t) dw[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  // db of the layers below the last (this wave's 16 pairs, every unit), the last layer's
  // db and dwp[E:] (this wave's units, all 64 pairs), dwp[:E] (this wave's 16 pairs)
  float db[NC_MAXL][NC_MAXNT], dbl[2] = {0.f, 0.f}, dwph[2] = {0.f, 0.f}, dwpg[2][8];
#pragma unroll
  for (int l = 0; l < NC_MAXL; ++l) {
#pragma unroll
    for (int nt = 0; nt < NC_MAXNT; ++nt) db[l][nt] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 8; ++j) dwpg[i][j] = 0.f;
  }
  const int chunks = p.E / 8;
  uint16_t *H = sm + p.hbase + 16 * wave * p.lda;
  uint16_t *Z = sm + p.zbase + 16 * wave * p.ldz;
  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    __syncthreads();  // the previous tile's dW products are done with the arenas
    nc_load_tile(p, sm, tile, tid);
    const int64_t base = tile * NC_TILE + 16 * wave;
    float dp[4][4];  // dpred of this lane's C/D rows in the four row blocks; 0 past the end
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t pr = tile * NC_TILE + 16 * rb + 4 * q + e;
        dp[rb][e] = pr < p.pairs ? p.dpred[pr] : 0.f;
      }
    }
    __syncthreads();
    nc_mlp<true>(p, sm, sf, wave, lane, dp, dbl, dwph);
    // the MF half: d mf_u = dpred wp mf_i, d mf_i = dpred wp mf_u, dwp[:E] += dpred g
    {
      const int64_t pair = base + a;
      const bool live = pair < p.pairs;
      const float d = live ? p.dpred[pair] : 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = q + 4 * i;
        if (c < chunks && live) {
          const uint16_t *r = p.rows + pair * p.ld_rows + 8 * c;
          uint16_t *o = p.drows + pair * p.ld_drows + 8 * c;
          float u[8], v[8], du[8], dv[8];
          nc_unpack8(*reinterpret_cast<const uint4 *>(r), u);
          nc_unpack8(*reinterpret_cast<const uint4 *>(r + p.E), v);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float s = d * sf[p.wpoff + 8 * c + j];
            du[j] = s * v[j];
            dv[j] = s * u[j];
            dwpg[i][j] += d * (u[j] * v[j]);
          }
          *reinterpret_cast<uint4 *>(o) = make_uint4(pack_bf16x2(du[0], du[1]), pack_bf16x2(du[2], du[3]),
                                                     pack_bf16x2(du[4], du[5]), pack_bf16x2(du[6], du[7]));
          *reinterpret_cast<uint4 *>(o + p.E) =
              make_uint4(pack_bf16x2(dv[0], dv[1]), pack_bf16x2(dv[2], dv[3]), pack_bf16x2(dv[4], dv[5]),
                         pack_bf16x2(dv[6], dv[7]));
        }
      }
    }
    // dh_l = dz_l W_l, from the last layer down; dz_{l-1} = dh_l [h_l > 0]
#pragma unroll
    for (int li = 0; li < NC_MAXL; ++li) {
      const int l = NC_MAXL - 1 - li;
      if (l < p.nl) {
        const uint16_t *W = sm + p.wimg[l];
        const int ldw = p.ldw[l];
        const uint16_t *zin = Z + a * p.ldz + p.zoff[l] + 4 * q;
#pragma unroll
        for (int ct = 0; ct < NC_MAXNT; ++ct) {
          if (ct < p.CT[l]) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int nt = 0; nt < p.NT[l]; ++nt)
              acc = mfma_16x16x16(*reinterpret_cast<const bf16x4 *>(zin + 16 * nt),
                                  lds_tr16x4(W + 16 * nt * ldw, ldw, 16 * ct, lane), acc);
            const int col = 16 * ct + a;
            if (l > 0) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const uint16_t h = H[(4 * q + e) * p.lda + p.hoff[l] + col];
                const float dz = (h & 0x7fffu) ? acc[e] : 0.f;
                db[l > 0 ? l - 1 : 0][ct] += dz;
                Z[(4 * q + e) * p.ldz + p.zoff[l > 0 ? l - 1 : 0] + col] = f32_to_bf16_rne(dz);
              }
            } else if (col < 2 * p.E) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int64_t pair = base + 4 * q + e;
                if (pair < p.pairs) p.drows[pair * p.ld_drows + 2 * p.E + col] = f32_to_bf16_rne(acc[e]);
              }
            }
          }
        }
        __syncthreads();
      }
    }
    // dW_l += dz_l^T h_l over the tile's 64 pairs: tile g = 4 t + wave of the flat list
    const uint16_t *Ha = sm + p.hbase, *Za = sm + p.zbase;
#pragma unroll
    for (int t = 0; t < NC_MAXT; ++t) {
      int g = 4 * t + wave;
      // (opaque: the table reads and the addresses built from them stay inside the tile
      // loop; hoisted out of it, 32 tiles' worth of them cost registers the accumulators
      // need: 97 spilled registers with them hoisted, 86 without)
      asm volatile("" : "+v"(g));
      if (g < p.ntile) {
        const int zc = tab[5 * g], hc = tab[5 * g + 1];
#pragma unroll
        for (int blk = 0; blk < NC_TILE / 16; ++blk)
          dw[t] = mfma_16x16x16(lds_tr16x4(Za + 16 * blk * p.ldz, p.ldz, zc, lane),
                                lds_tr16x4(Ha + 16 * blk * p.lda, p.lda, hc, lane), dw[t]);
      }
    }
  }
  // the workgroup's partial: [dW_0 | .. | db_0 | .. | dwp]
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * p.P;
#pragma unroll
  for (int t = 0; t < NC_MAXT; ++t) {
    const int g = 4 * t + wave;
    if (g < p.ntile) {
      const int l = tab[5 * g + 2], nt = tab[5 * g + 3], ct = tab[5 * g + 4];
      const int col = 16 * ct + a;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * nt + 4 * q + e;
        if (row < p.N[l] && col < p.K[l]) part[p.woff[l] + row * p.K[l] + col] = dw[t][e];
      }
    }
  }
  // the last layer's db and dwp[E:]: a unit belongs to one wave; its four row groups
  // (lanes a, a + 16, a + 32, a + 48) in a fixed order
  {
    const int lk = p.nl - 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float vb = dbl[j], vw = dwph[j];
      vb += __shfl_xor(vb, 16);
      vb += __shfl_xor(vb, 32);
      vw += __shfl_xor(vw, 16);
      vw += __shfl_xor(vw, 32);
      const int n = 16 * (wave + 4 * j) + a;
      if (q == 0 && n < p.N[lk]) {
        part[p.dboff[lk] + n] = vb;
        part[p.dwpoff + p.E + n] = vw;
      }
    }
  }
  // db below the last layer and dwp[:E]: a wave's lanes in a fixed order, then the four
  // waves in order
  __syncthreads();
  float *red = sf + p.redoff + wave * p.red;
  {
    int o = 0;
#pragma unroll
    for (int l = 0; l < NC_MAXL - 1; ++l) {
      if (l < p.nl - 1) {
#pragma unroll
        for (int nt = 0; nt < NC_MAXNT; ++nt) {
          if (nt < p.NT[l]) {
            float v = db[l][nt];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (q == 0) red[o + 16 * nt + a] = v;
          }
        }
        o += 16 * p.NT[l];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = q + 4 * i;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = dwpg[i][j];
        v += __shfl_xor(v, 1);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        if (a == 0 && c < chunks) red[p.rg + 8 * c + j] = v;
      }
    }
  }
  __syncthreads();
  const float *r0 = sf + p.redoff;
  auto sum4 = [&](int i) { return ((r0[i] + r0[p.red + i]) + r0[2 * p.red + i]) + r0[3 * p.red + i]; };
  {
    int o = 0;
    for (int l = 0; l < p.nl - 1; ++l) {
      for (int n = tid; n < p.N[l]; n += NC_THREADS) part[p.dboff[l] + n] = sum4(o + n);
      o += 16 * p.NT[l];
    }
  }
  for (int j = tid; j < p.E; j += NC_THREADS) part[p.dwpoff + j] = sum4(p.rg + j);
}

}  // namespace mrec

using namespace mrec;

namespace {

bool nc_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// The shape's plan: layer geometry, the LDS layout and the partial's sections.  False
// when the shape is outside the compiled domain or does not fit the CU's LDS.
bool nc_plan(int32_t E, int32_t nl, const int32_t *widths, NcfArgs *p) {
  if (!(E == 8 || E == 16 || E == 32 || E == 64) || nl < 1 || nl > NC_MAXL || !widths) return false;
  for (int l = 0; l < nl; ++l)
    if (widths[l] < 8 || widths[l] > NC_MAXW || widths[l] % 8) return false;
  p->E = E, p->nl = nl;
  int sm = 0, hcols = 0, zcols = 0, fl = 0, tiles = 0, P = 0;
  for (int l = 0; l < nl; ++l) {
    p->N[l] = widths[l];
    p->K[l] = l ? widths[l - 1] : 2 * E;
    p->NT[l] = pad_to(p->N[l], 16) / 16;
    p->KS[l] = pad_to(p->K[l], 32) / 32;
    p->CT[l] = pad_to(p->K[l], 16) / 16;
    p->ldw[l] = 32 * p->KS[l] + 8;
    p->wimg[l] = sm;
    sm += 16 * p->NT[l] * p->ldw[l];
    p->hoff[l] = hcols, hcols += 32 * p->KS[l];
    p->zoff[l] = zcols, zcols += 16 * p->NT[l];
    p->boff[l] = fl, fl += 16 * p->NT[l];
    tiles += p->NT[l] * p->CT[l];
    p->woff[l] = P, P += p->N[l] * p->K[l];
  }
  for (int l = 0; l < nl; ++l) p->dboff[l] = P, P += p->N[l];
  p->dwpoff = P, P += E + p->N[nl - 1];
  p->P = P;
  p->ntile = tiles;
  if (tiles > 4 * NC_MAXT) return false;
  p->hbase = sm, p->lda = hcols + 8, sm += NC_TILE * p->lda;
  p->fbase = 2 * sm;
  const int nk16 = 16 * p->NT[nl - 1];
  p->red = fl + E + nk16;  // per wave: [db of every layer | dwp[:E] | dwp[E:]]
  p->rg = fl, p->rh = fl + E;
  p->wpoff = fl, fl += E + nk16;
  p->dotoff = fl, fl += 4 * NC_TILE;  // the MLP dots, one part per wave
  p->fwd_bytes = p->fbase + 4 * fl;
  p->redoff = fl, fl += 4 * p->red;
  p->taboff = fl, fl += 5 * tiles;
  fl = pad_to(fl, 4);
  p->zbase = (p->fbase + 4 * fl) / 2, p->ldz = zcols + 8;
  p->bwd_bytes = 2 * (p->zbase + NC_TILE * p->ldz);
  return p->bwd_bytes <= NC_LDS_LIMIT;
}

mrec_status nc_check(const mrec_ncf_args *a, NcfArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  NcfArgs p{};
  MREC_CHECK_ARG(nc_plan(a->E, a->n_layers, a->widths, &p), "unsupported shape (mrec_ncf_supported)");
  MREC_CHECK_ARG(a->rows && a->wp, "NULL pointer");
  for (int l = 0; l < p.nl; ++l) {
    MREC_CHECK_ARG(a->w[l] && a->b[l], "NULL pointer");
    MREC_CHECK_ARG(a->ld_w[l] >= p.K[l], "a leading dimension is smaller than its row");
    p.w[l] = a->w[l], p.ld_w[l] = a->ld_w[l], p.b[l] = a->b[l];
  }
  MREC_CHECK_ARG(a->pairs >= 0 && a->pairs <= INT32_MAX, "pairs must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->ld_rows >= 4 * a->E && a->ld_rows % 8 == 0 && nc_aligned(a->rows),
                 "rows must be 16-byte aligned bf16 rows (ld_rows a multiple of 8, >= 4 E)");
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.pairs = a->pairs;
  p.tiles = (a->pairs + NC_TILE - 1) / NC_TILE;
  p.wp = a->wp;
  p.pred = a->pred;
  p.dpred = a->dpred;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  *out = p;
  return MREC_OK;
}

void nc_set_attrs() {
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ncf_fwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NC_LDS_LIMIT);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ncf_bwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NC_LDS_LIMIT);
    (void)hipGetLastError();
    return 1;
  }();
  (void)once;
}

}  // namespace

extern "C" {

int32_t mrec_ncf_supported(int32_t E, int32_t n_layers, const int32_t *widths) {
  NcfArgs p{};
  return nc_plan(E, n_layers, widths, &p) ? 1 : 0;
}

int32_t mrec_ncf_tile(void) { return NC_TILE; }

int64_t mrec_ncf_parts(int64_t pairs) {
  const int64_t g = device_cus(), tiles = (pairs + NC_TILE - 1) / NC_TILE;
  return tiles < g ? (tiles > 0 ? tiles : 1) : g;
}

int64_t mrec_ncf_param_count(int32_t E, int32_t n_layers, const int32_t *widths) {
  NcfArgs p{};
  return nc_plan(E, n_layers, widths, &p) ? p.P : 0;
}

mrec_status mrec_ncf_fwd(const mrec_ncf_args *a, mrec_stream stream) {
  NcfArgs p;
  const mrec_status st = nc_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->pred, "NULL pointer");
  if (p.pairs == 0) return MREC_OK;
  nc_set_attrs();
  const unsigned grid = static_cast<unsigned>(mrec_ncf_parts(p.pairs));
  ncf_fwd_kernel<<<dim3(grid), NC_THREADS, p.fwd_bytes, static_cast<hipStream_t>(stream)>>>(p);
  return launch_status("mrec_ncf_fwd");
}

mrec_status mrec_ncf_bwd(const mrec_ncf_args *a, mrec_stream stream) {
  NcfArgs p;
  const mrec_status st = nc_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->dpred && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= 4 * a->E && a->ld_drows % 8 == 0 && nc_aligned(a->d_rows),
                 "d_rows must be 16-byte aligned bf16 rows (ld_drows a multiple of 8, >= 4 E)");
  MREC_CHECK_ARG(a->parts == mrec_ncf_parts(a->pairs), "parts must be mrec_ncf_parts(pairs)");
  if (p.pairs == 0) return MREC_OK;
  nc_set_attrs();
  ncf_bwd_kernel<<<dim3(static_cast<unsigned>(a->parts)), NC_THREADS, p.bwd_bytes,
                   static_cast<hipStream_t>(stream)>>>(p);
  return launch_status("mrec_ncf_bwd");
}

}  // extern "C"
