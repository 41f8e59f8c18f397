// The NCF / NeuMF scorer's shared device code: the argument block with its LDS plan, the
// once-per-workgroup staging and the MLP over a tile of 64 pairs (ncf.hip, whose header
// comment describes the layout; ncf_topk.hip runs the same layers over (user, item) pairs
// it forms on chip).
#pragma once

#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int NC_TILE = 64;      // pairs per tile: four row blocks of 16
constexpr int NC_THREADS = 256;
constexpr int NC_MAXL = 3;       // hidden layers
constexpr int NC_MAXW = 128;     // widest layer
constexpr int NC_MAXNT = NC_MAXW / 16;
constexpr int NC_MAXT = 32;      // dW tiles a wave can accumulate (4 registers each)
constexpr int NC_LDS_LIMIT = 160 * 1024;

struct NcfArgs {
  const uint16_t *rows;
  int64_t ld_rows, pairs, tiles;
  int E, nl;
  int N[NC_MAXL + 1], K[NC_MAXL + 1];  // a layer's outputs and inputs
  int NT[NC_MAXL + 1];                 // pad16(N) / 16
  int KS[NC_MAXL + 1];                 // pad32(K) / 32
  int CT[NC_MAXL + 1];                 // pad16(K) / 16
  const float *w[NC_MAXL];
  int64_t ld_w[NC_MAXL];
  const float *b[NC_MAXL];
  const float *wp;
  float *pred;
  const float *dpred;
  uint16_t *drows;
  int64_t ld_drows;
  float *part;
  int64_t P;
  // LDS plan: bf16 element offsets ...
  int wimg[NC_MAXL + 1], ldw[NC_MAXL + 1];
  int hbase, lda, hoff[NC_MAXL + 1];
  int zbase, ldz, zoff[NC_MAXL + 1];
  // ... and fp32 element offsets from fbase (bytes)
  int fbase, boff[NC_MAXL + 1], wpoff, dotoff, redoff, red, rg, rh, taboff, ntile;
  int fwd_bytes, bwd_bytes;
  // the partial's sections
  int woff[NC_MAXL + 1], dboff[NC_MAXL + 1], dwpoff;
};

// Once per workgroup: the weight images (bf16, zero padded), biases, wp, zeroed arenas,
// the dW tile table, by a workgroup of `threads` threads.  Ends at a barrier.
__device__ __forceinline__ void nc_stage(const NcfArgs &p, uint16_t *sm, float *sf, int tid, bool bwd,
                                         int threads = NC_THREADS) {
  for (int l = 0; l < p.nl; ++l) {
    const int k32 = 32 * p.KS[l], n16 = 16 * p.NT[l];
    uint16_t *img = sm + p.wimg[l];
    // 8 consecutive k per thread (K is a multiple of 8: a chunk is all live or all
    // padding): eight independent loads in flight, one 16-B LDS store
    const int kc = k32 / 8;
    for (int i = tid; i < n16 * kc; i += threads) {
      const int n = i / kc, k = 8 * (i % kc);
      uint4 v = make_uint4(0, 0, 0, 0);
      if (n < p.N[l] && k < p.K[l]) {
        const float *src = p.w[l] + n * p.ld_w[l] + k;
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = src[j];
        v = make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]),
                       pack_bf16x2(f[6], f[7]));
      }
      *reinterpret_cast<uint4 *>(img + n * p.ldw[l] + k) = v;
    }
    for (int n = tid; n < n16; n += threads) sf[p.boff[l] + n] = n < p.N[l] ? p.b[l][n] : 0.f;
  }
  const int nk = p.N[p.nl - 1], nk16 = 16 * p.NT[p.nl - 1];
  for (int i = tid; i < p.E + nk16; i += threads) sf[p.wpoff + i] = i < p.E + nk ? p.wp[i] : 0.f;
  for (int i = tid; i < NC_TILE * p.lda / 8; i += threads)
    reinterpret_cast<uint4 *>(sm + p.hbase)[i] = make_uint4(0, 0, 0, 0);
  if (bwd) {
    for (int i = tid; i < NC_TILE * p.ldz / 8; i += threads)
      reinterpret_cast<uint4 *>(sm + p.zbase)[i] = make_uint4(0, 0, 0, 0);
    // dW tile g of the flat list -> {dz column, h column, layer, n tile, k tile}
    int *tab = reinterpret_cast<int *>(sf + p.taboff);
    int g0 = 0;
    for (int l = 0; l < p.nl; ++l) {
      const int cnt = p.NT[l] * p.CT[l];
      for (int i = tid; i < cnt; i += threads) {
        const int nt = i / p.CT[l], ct = i % p.CT[l];
        int *t = tab + 5 * (g0 + i);
        t[0] = p.zoff[l] + 16 * nt, t[1] = p.hoff[l] + 16 * ct, t[2] = l, t[3] = nt, t[4] = ct;
      }
      g0 += cnt;
    }
  }
  __syncthreads();
}

// The MLP over the tile's 64 pairs.  In a layer wave w owns the output tiles w and w + 4
// (16 units each) for all four 16-pair row blocks: per k step four A fragments and up to
// two B fragments feed eight independent MFMAs.  Forward: the wave's part of the dot of
// wp[E:] with h_k -> sdot[wave][pair].  Backward (the same products, so the same bits):
// dz_{k-1} -> the Z arena, and the last layer's db and dwp sums of the wave's units.
// Every layer ends at a barrier.  L0: the first layer to run (the layers below it are the
// caller's: ncf_topk.hip forms h_1 itself).  NRB, rb0: the row blocks this wave takes, rb0 ..
// rb0 + NRB - 1 (all four here; ncf_topk.hip gives each half of the tile to its own four
// waves, `wave` then being the wave's place among them) -- a product's bits are the same.
template <bool BWD, int L0 = 0, int NRB = 4>
__device__ __forceinline__ void nc_mlp(const NcfArgs &p, uint16_t *sm, float *sf, int wave, int lane,
                                       const float (&dp)[4][4], float (&dbl)[2], float (&dwph)[2],
                                       int rb0 = 0) {
  const int a = lane & 15, q = lane >> 4;
  uint16_t *H = sm + p.hbase;
  uint16_t *Z = sm + p.zbase;
#pragma unroll
  for (int l = 0; l < NC_MAXL; ++l) {
    if (l >= L0 && l < p.nl) {
      const bool last = l == p.nl - 1;
      const uint16_t *W = sm + p.wimg[l];
      const int ldw = p.ldw[l];
      const float *bias = sf + p.boff[l];
      const bool has0 = wave < p.NT[l], has1 = wave + 4 < p.NT[l];  // per wave
      float dot[NRB][4];
#pragma unroll
      for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
        for (int e = 0; e < 4; ++e) dot[rb][e] = 0.f;
      }
      if (has0) {
        f32x4 acc[2][NRB];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) acc[j][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const uint16_t *hin = H + a * p.lda + p.hoff[l] + 8 * q;
        const uint16_t *w0 = W + (16 * wave + a) * ldw + 8 * q;
        const uint16_t *w1 = w0 + 64 * ldw;
        for (int ks = 0; ks < p.KS[l]; ++ks) {
          bf16x8 af[NRB];
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb)
            af[rb] = *reinterpret_cast<const bf16x8 *>(hin + 16 * (rb0 + rb) * p.lda + 32 * ks);
          const bf16x8 b0 = *reinterpret_cast<const bf16x8 *>(w0 + 32 * ks);
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) acc[0][rb] = mfma_16x16x32(af[rb], b0, acc[0][rb]);
          if (has1) {
            const bf16x8 b1 = *reinterpret_cast<const bf16x8 *>(w1 + 32 * ks);
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) acc[1][rb] = mfma_16x16x32(af[rb], b1, acc[1][rb]);
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (j == 0 || has1) {
            const int n = 16 * (wave + 4 * j) + a;
            const float bn = bias[n];
            if (!last) {
              uint16_t *hout = H + p.hoff[l + 1] + n;
#pragma unroll
              for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float x = acc[j][rb][e] + bn;
                  hout[(16 * (rb0 + rb) + 4 * q + e) * p.lda] = f32_to_bf16_rne(x > 0.f ? x : 0.f);
                }
              }
            } else {
              const float wpn = sf[p.wpoff + p.E + n];
#pragma unroll
              for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const float x = acc[j][rb][e] + bn;
                  const float v = x > 0.f ? x : 0.f;
                  if constexpr (!BWD) {
                    dot[rb][e] += wpn * v;
                  } else {
                    const float dz = v > 0.f ? dp[rb][e] * wpn : 0.f;
                    dbl[j] += dz;
                    dwph[j] += dp[rb][e] * v;
                    Z[(16 * (rb0 + rb) + 4 * q + e) * p.ldz + p.zoff[l] + n] = f32_to_bf16_rne(dz);
                  }
                }
              }
            }
          }
        }
      }
      if constexpr (!BWD) {
        if (last) {
          // the 16 units of a tile column sit in the 16 lanes of a row: a butterfly,
          // the same tree for every pair; a wave without a tile contributes zero
#pragma unroll
          for (int rb = 0; rb < NRB; ++rb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float d = dot[rb][e];
              d += __shfl_xor(d, 1);
              d += __shfl_xor(d, 2);
              d += __shfl_xor(d, 4);
              d += __shfl_xor(d, 8);
              if (a == 0) sf[p.dotoff + NC_TILE * wave + 16 * (rb0 + rb) + 4 * q + e] = d;
            }
          }
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ void nc_unpack8(const uint4 &r, float *v) { Vec<uint16_t>::to_f32(r, v); }

}  // namespace mrec
