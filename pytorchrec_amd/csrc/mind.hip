// MIND multi-interest extractor (Li et al., CIKM 2019; ComiRec-DR, Cen et al., KDD 2020):
// behaviour-to-interest dynamic routing of a history into K interest capsules, fused per
// sample.
//
//   H^_j = bf16(X_j S^T)                              X_j a zero row at invalid j
//   b_kj = route_init[k, j]
//   for r = 1 .. R:  w_kj = bf16(softmax over k < K' of b_kj) at valid j, exactly 0 elsewhere
//                    z_k  = sum_j w_kj H^_j                                       (fp32)
//                    u_k  = z_k n2 / ((1 + n2) sqrt(n2 + 1e-9)),  n2 = |z_k|^2    (fp32)
//                    if r < R:  b_kj += bf16(u_k) . H^_j
//   U = u of the last iteration; rows k >= K' are exactly zero
//
// Work split: one wave per sample, a persistent grid of 8-wave workgroups whose waves
// stride over the batch.  Nothing is shared between the waves of a workgroup: every wave
// has its own LDS region and the routing loop has no __syncthreads (md_sync orders one
// wave's LDS writes before its reads).  A wave keeps the S operand fragments in registers
// for its whole life (32 VGPRs at D = 64).
//
// Forward, per sample: the rows go from global memory straight into A fragments (16-byte
// row chunks), H^ is (L / 16) x (D / 16) tiles of mfma_16x16x32 written once as bf16 into
// the wave's [64][72] tile.  In the routing loop lane j owns position j: b[0..K)[j] and
// w[0..K)[j] live in its registers and the softmax over the interests is lane-local.
// z = w H^ contracts over the positions: w goes through an [8][72] bf16 LDS tile into the
// A operand (K padded to the 16-row tile, rows 8 .. 15 a zero fragment) and H^ is read
// through the transposing LDS reads as the B operand.  The squash runs in fp32 on the
// accumulators (a 16-lane DPP sum for n2).  The agreement u H^T contracts over D: u goes
// through an [8][72] bf16 tile into the A operand, the rows of H^ are read directly as the B
// operand, and the [8][64] fp32 result goes back through LDS to the lanes that own the
// positions.  Saved for the backward: the last w (the bf16 values its product used) and the
// pre-squash z.
//
// Backward: the routing logits carry no gradient (the last w is a constant), so dU flows
// through the squash and z = w H^ alone, and dH^ is never formed:
//   dz_k = c dU_k + 2 c' (z_k . dU_k) z_k       c(n2) = n2 / ((1 + n2) sqrt(n2 + 1e-9))
//   g_k  = dz_k S,  dX_j = sum_k w_kj g_k;      p_k = sum_j w_kj X_j,  dS += dz_k^T p_k
// dz is computed in the accumulator layout (row k = 4 (lane >> 4) + i, column lane & 15),
// which is the A operand of mfma_16x16x16 for dS; g and p come out of their products in
// that same layout, which is the B operand of mfma_16x16x16 for dX and dS: neither goes
// through LDS.  dS stays in MFMA accumulators over a wave's samples (D x D fp32: 64 VGPRs
// at D = 64); at the end the workgroup's waves add theirs in wave order through LDS and
// the workgroup writes one [D, D] partial, to be summed in workgroup order by
// mrec_sasrec_wgrad.  dX is assembled in the X tile and leaves as 16-byte row chunks,
// bitwise zero at invalid positions.  No atomics: two runs give equal bits.
//
// LDS per wave: forward 13.25 KiB (H^ 9 KiB, w and u 1.125 KiB each, agreement 2 KiB),
// backward 11.25 KiB (X / dX 9 KiB, w and dz 1.125 KiB each); 8 waves: 106 KiB / 90 KiB of
// the CU's 160 KiB, one workgroup (8 waves, 2 per SIMD) per CU.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int MD_ROWS = 64;  // history positions per sample, padded
constexpr int MD_KMAX = 8;   // interests
constexpr int MD_LD = 72;    // bf16 elements per tile row (144 B: 16-B aligned rows)
constexpr int MD_WAVES = 8;
constexpr int MD_THREADS = 64 * MD_WAVES;
constexpr int MD_TILE_B = MD_ROWS * MD_LD * 2;    // the H^ / X tile
constexpr int MD_SMALL_B = MD_KMAX * MD_LD * 2;   // an [8][72] bf16 tile
constexpr int MD_AGREE_B = MD_KMAX * MD_ROWS * 4;  // the [8][64] fp32 agreement
constexpr int MD_FWD_WAVE_B = MD_TILE_B + 2 * MD_SMALL_B + MD_AGREE_B;
constexpr int MD_BWD_WAVE_B = MD_TILE_B + 2 * MD_SMALL_B;
constexpr int MD_MAX_ITERS = 4;

struct MindArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const int32_t *his_len;
  const float *s;  // route_weight [D, D] fp32
  int64_t ld_s;
  const float *init;  // route_init [K, >= L] fp32
  int64_t ld_init;
  int64_t batch;
  int L, K, iters, dynamic_k;
  float *u;     // [batch, K, D]
  uint16_t *w;  // [batch, K, L] bf16: the last iteration's coupling
  float *z;     // [batch, K, D]: the last iteration's pre-squash capsules
  const float *du;
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][D * D]
};

// this wave's LDS writes, then its reads (one wave: no workgroup barrier)
__device__ __forceinline__ void md_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// sum over the 16 lanes of this lane's row (lanes 16 g .. 16 g + 15), every lane gets it
__device__ __forceinline__ float md_sum16(float v) {
  v = sum_quad(v);
  v += dpp_f32<0x124>(v);  // row_ror:4
  return v + dpp_f32<0x128>(v);  // row_ror:8
}

// squash: u = c(n2) z, and c'
__device__ __forceinline__ float md_squash(float n2) { return n2 / ((1.f + n2) * sqrtf(n2 + 1e-9f)); }
__device__ __forceinline__ float md_dsquash(float n2) {
  const float s = sqrtf(n2 + 1e-9f), q = 1.f + n2;
  return (s - n2 * q / (2.f * s)) / (q * q * s * s);  // 1 / s at n2 = 0: finite
}

// valid positions of sample b as a 64-bit mask (bit j: j < L and (his_j > 0 or j == 0))
__device__ __forceinline__ unsigned long long md_valid(const MindArgs &p, int64_t b, int lane) {
  const bool ok = lane < p.L && (lane == 0 || p.his[b * p.ld_his + lane] > 0);
  return __ballot(ok);
}

// active interests of sample b
__device__ __forceinline__ int md_active(const MindArgs &p, int64_t b) {
  if (!p.dynamic_k) return p.K;
  const int len = max(p.his_len[b], 1);
  return max(1, min(p.K, 31 - __clz(len)));
}

// A operand of a [K, 64]-shaped LDS tile (K padded to 16 rows): rows 8 .. 15 are zero, and
// so is the upper half of the k step of a 16-wide operand (KW = 16)
template <int KW = 32>
__device__ __forceinline__ bf16x8 md_small_frag(const uint16_t *t, int k0, int lane) {
  if ((lane & 15) >= MD_KMAX || (KW == 16 && (lane >> 4) >= 2)) return frag_zero8();
  return *reinterpret_cast<const bf16x8 *>(t + (lane & 15) * MD_LD + k0 + 8 * (lane >> 4));
}

// B operand read through the transposing reads: element (column n0 + (lane & 15), k) is
// tile[k0 + k][n0 + ..]; every address lies inside the 64-row tile
__device__ __forceinline__ bf16x8 md_tr_frag(const uint16_t *tile, int n0, int k0, int lane) {
  const int li = lane & 15;
  return lds_tr16_pair(tile + (k0 + 8 * (lane >> 4) + (li >> 2)) * MD_LD + n0 + 4 * (li & 3), 4 * MD_LD);
}

__device__ __forceinline__ bf16x4 md_pack4(f32x4 a) {
  const uint32_t lo = pack_bf16x2(a[0], a[1]), hi = pack_bf16x2(a[2], a[3]);
  return __builtin_bit_cast(bf16x4, make_uint2(lo, hi));
}

__device__ __forceinline__ void md_clear(char *base, int bytes, int lane) {
  for (int o = lane * 16; o < bytes; o += 64 * 16) *reinterpret_cast<uint4 *>(base + o) = make_uint4(0, 0, 0, 0);
  md_sync();
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(MD_THREADS, 1) void mind_fwd_kernel(MindArgs p) {
  constexpr int NT = D / 16, KS = (D + 31) / 32, KW = D == 16 ? 16 : 32;
  extern __shared__ __attribute__((aligned(16))) char md_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  char *base = md_smem + wave * MD_FWD_WAVE_B;
  uint16_t *Hs = reinterpret_cast<uint16_t *>(base);
  uint16_t *Ws = reinterpret_cast<uint16_t *>(base + MD_TILE_B);
  uint16_t *Us = reinterpret_cast<uint16_t *>(base + MD_TILE_B + MD_SMALL_B);
  float *Bs = reinterpret_cast<float *>(base + MD_TILE_B + 2 * MD_SMALL_B);
  md_clear(base, MD_FWD_WAVE_B, lane);
  const int MT = (p.L + 15) / 16, JS = (p.L + 31) / 32;

  // B operand of H^ = X S^T: column n is row n of S
  bf16x8 sb[NT][KS];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = 32 * s + 8 * g;
      if (k < D) {
        const float *sp = p.s + (16 * nt + li) * p.ld_s + k;
        sb[nt][s] = frag_from_f32(*reinterpret_cast<const uint4 *>(sp), *reinterpret_cast<const uint4 *>(sp + 4));
      } else {
        sb[nt][s] = frag_zero8();
      }
    }

  for (int64_t b = static_cast<int64_t>(blockIdx.x) * MD_WAVES + wave; b < p.batch;
       b += static_cast<int64_t>(gridDim.x) * MD_WAVES) {
    const unsigned long long mask = md_valid(p, b, lane);
    const bool ok = (mask >> lane) & 1;
    const int kp = md_active(p, b);
    // H^ tiles: rows j of X straight from global memory (zero rows at invalid j)
    for (int mt = 0; mt < MT; ++mt) {
      const int j = 16 * mt + li;
      bf16x8 xa[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = 32 * s + 8 * g;
        xa[s] = frag_zero8();
        if (((mask >> j) & 1) && k < D)
          xa[s] = *reinterpret_cast<const bf16x8 *>(p.rows + (b * p.L + j) * p.ld_rows + k);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = mfma_16x16x32(xa[s], sb[nt][s], acc);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          Hs[(16 * mt + 4 * g + e) * MD_LD + 16 * nt + li] = f32_to_bf16_rne(acc[e]);
      }
    }
    float bk[MD_KMAX];
#pragma unroll
    for (int k = 0; k < MD_KMAX; ++k) bk[k] = k < p.K && lane < p.L ? p.init[k * p.ld_init + lane] : 0.f;
    md_sync();

    for (int r = 1; r <= p.iters; ++r) {
      // w = softmax over the active interests, lane-local
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < MD_KMAX; ++k)
        if (k < kp) mx = fmaxf(mx, bk[k]);
      float ex[MD_KMAX], sum = 0.f;
#pragma unroll
      for (int k = 0; k < MD_KMAX; ++k) {
        ex[k] = k < kp ? expf(bk[k] - mx) : 0.f;
        sum += ex[k];
      }
      const float inv = 1.f / sum;
      uint16_t wq[MD_KMAX];
#pragma unroll
      for (int k = 0; k < MD_KMAX; ++k) {
        wq[k] = ok ? f32_to_bf16_rne(ex[k] * inv) : uint16_t(0);
        Ws[k * MD_LD + lane] = wq[k];
      }
      md_sync();
      // z = w H^ (rows k = 4 g + e of the 16-row tile; rows 8 .. 15 are zero), squash
      f32x4 z[NT];
      float n2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        z[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < JS; ++s)
          z[nt] = mfma_16x16x32(md_small_frag(Ws, 32 * s, lane), md_tr_frag(Hs, 16 * nt, 32 * s, lane), z[nt]);
#pragma unroll
        for (int e = 0; e < 4; ++e) n2[e] = fmaf(z[nt][e], z[nt][e], n2[e]);
      }
      float c[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) c[e] = md_squash(md_sum16(n2[e]));
      if (r == p.iters) {
        if (g < 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k = 4 * g + e;
            if (k < p.K) {
#pragma unroll
              for (int nt = 0; nt < NT; ++nt) {
                const int64_t o = (b * p.K + k) * D + 16 * nt + li;
                p.u[o] = z[nt][e] * c[e];
                p.z[o] = z[nt][e];
              }
            }
          }
        }
        if (lane < p.L) {
#pragma unroll
          for (int k = 0; k < MD_KMAX; ++k)
            if (k < p.K) p.w[(b * p.K + k) * p.L + lane] = wq[k];
        }
        break;
      }
      if (g < 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            Us[(4 * g + e) * MD_LD + 16 * nt + li] = f32_to_bf16_rne(z[nt][e] * c[e]);
      }
      md_sync();
      // agreement a[k][j] = u_k . H^_j, back to the lanes that own the positions
      for (int jt = 0; jt < MT; ++jt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          bf16x8 hb = frag_zero8();
          if (KW == 32 || g < 2)
            hb = *reinterpret_cast<const bf16x8 *>(Hs + (16 * jt + li) * MD_LD + 32 * s + 8 * g);
          acc = mfma_16x16x32(md_small_frag<KW>(Us, 32 * s, lane), hb, acc);
        }
        if (g < 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) Bs[(4 * g + e) * MD_ROWS + 16 * jt + li] = acc[e];
        }
      }
      md_sync();
#pragma unroll
      for (int k = 0; k < MD_KMAX; ++k)
        if (k < p.K) bk[k] += Bs[k * MD_ROWS + lane];
      md_sync();
    }
    md_sync();
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(MD_THREADS, 1) void mind_bwd_kernel(MindArgs p) {
  constexpr int NT = D / 16, KS = (D + 31) / 32, KW = D == 16 ? 16 : 32, CH = D / 8;
  extern __shared__ __attribute__((aligned(16))) char md_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, li = lane & 15;
  char *base = md_smem + wave * MD_BWD_WAVE_B;
  uint16_t *Xs = reinterpret_cast<uint16_t *>(base);
  uint16_t *Ws = reinterpret_cast<uint16_t *>(base + MD_TILE_B);
  uint16_t *Dz = reinterpret_cast<uint16_t *>(base + MD_TILE_B + MD_SMALL_B);
  md_clear(base, MD_BWD_WAVE_B, lane);
  const int MT = (p.L + 15) / 16, JS = (p.L + 31) / 32;

  // B operand of g = dz S: column e, contraction d: S[d][e]
  bf16x8 st[NT][KS];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      float f[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int d = 32 * s + 8 * g + i;
        f[i] = d < D ? p.s[d * p.ld_s + 16 * nt + li] : 0.f;
      }
      st[nt][s] = frag_pack8(f);
    }
  f32x4 ds[NT][NT];
#pragma unroll
  for (int mt = 0; mt < NT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) ds[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t b = static_cast<int64_t>(blockIdx.x) * MD_WAVES + wave; b < p.batch;
       b += static_cast<int64_t>(gridDim.x) * MD_WAVES) {
    const unsigned long long mask = md_valid(p, b, lane);
    // X tile (zero rows at invalid j and at L <= j < 16 MT), the saved w
    for (int t = lane; t < 16 * MT * CH; t += 64) {
      const int j = t / CH, c = (t % CH) * 8;
      uint4 x = make_uint4(0, 0, 0, 0);
      if ((mask >> j) & 1) x = *reinterpret_cast<const uint4 *>(p.rows + (b * p.L + j) * p.ld_rows + c);
      *reinterpret_cast<uint4 *>(Xs + j * MD_LD + c) = x;
    }
#pragma unroll
    for (int k = 0; k < MD_KMAX; ++k)
      Ws[k * MD_LD + lane] = k < p.K && lane < p.L ? p.w[(b * p.K + k) * p.L + lane] : uint16_t(0);
    // dz = c dU + 2 c' (z . dU) z in the accumulator layout (rows k >= K stay zero)
    f32x4 dz[NT];
    {
      f32x4 zz[NT], du[NT];
      float n2[4] = {0.f, 0.f, 0.f, 0.f}, zd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 4 * g + e;
          const int64_t o = (b * p.K + (k < p.K ? k : 0)) * D + 16 * nt + li;
          const float zv = p.z[o], dv = p.du[o];
          zz[nt][e] = k < p.K ? zv : 0.f;
          du[nt][e] = k < p.K ? dv : 0.f;
          n2[e] = fmaf(zz[nt][e], zz[nt][e], n2[e]);
          zd[e] = fmaf(zz[nt][e], du[nt][e], zd[e]);
        }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float n = md_sum16(n2[e]);
        const float c = md_squash(n), t = 2.f * md_dsquash(n) * md_sum16(zd[e]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) dz[nt][e] = fmaf(t, zz[nt][e], c * du[nt][e]);
      }
    }
    if (g < 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) Dz[(4 * g + e) * MD_LD + 16 * nt + li] = f32_to_bf16_rne(dz[nt][e]);
    }
    md_sync();
    // g = dz S and p = w X, both left in the accumulator layout: the B operands of the
    // k = 16 products below
    bf16x4 gq[NT], pq[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 ga = {0.f, 0.f, 0.f, 0.f}, pa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) ga = mfma_16x16x32(md_small_frag<KW>(Dz, 32 * s, lane), st[nt][s], ga);
      for (int s = 0; s < JS; ++s)
        pa = mfma_16x16x32(md_small_frag(Ws, 32 * s, lane), md_tr_frag(Xs, 16 * nt, 32 * s, lane), pa);
      gq[nt] = md_pack4(ga);
      pq[nt] = md_pack4(pa);
    }
    // dS += dz^T p over this sample's interests
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
      const bf16x4 da = md_pack4(dz[mt]);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) ds[mt][nt] = mfma_16x16x16(da, pq[nt], ds[mt][nt]);
    }
    md_sync();  // X is dead: dX takes its tile
    for (int jt = 0; jt < MT; ++jt) {
      bf16x4 wa = {0, 0, 0, 0};
      if (g < 2) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wa[i] = static_cast<short>(Ws[(4 * g + i) * MD_LD + 16 * jt + li]);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const f32x4 acc = mfma_16x16x16(wa, gq[nt], f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int j = 16 * jt + 4 * g + e;
          Xs[j * MD_LD + 16 * nt + li] = ((mask >> j) & 1) ? f32_to_bf16_rne(acc[e]) : uint16_t(0);
        }
      }
    }
    md_sync();
    for (int t = lane; t < p.L * CH; t += 64) {
      const int j = t / CH, c = (t % CH) * 8;
      *reinterpret_cast<uint4 *>(p.drows + (b * p.L + j) * p.ld_drows + c) =
          *reinterpret_cast<const uint4 *>(Xs + j * MD_LD + c);
    }
    md_sync();
  }

  // the workgroup's dS: its waves' accumulators added in wave order
  float *Z = reinterpret_cast<float *>(md_smem);
  for (int wv = 0; wv < MD_WAVES; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float *q = Z + (16 * mt + 4 * g + e) * D + 16 * nt + li;
            *q = wv == 0 ? ds[mt][nt][e] : *q + ds[mt][nt][e];
          }
    }
  }
  __syncthreads();
  float *part = p.part + static_cast<int64_t>(blockIdx.x) * D * D;
  for (int i = threadIdx.x; i < D * D; i += MD_THREADS) part[i] = Z[i];
}

}  // namespace mrec

using namespace mrec;

namespace {

bool md_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

mrec_status md_check(const mrec_mind_args *a, MindArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his && a->his_len && a->route_w && a->route_init && a->w && a->z,
                 "NULL pointer");
  MREC_CHECK_ARG(mrec_mind_supported(a->D, a->K, a->L, a->iters),
                 "need D in {16, 32, 64}, 1 <= K <= 8, 1 <= L <= 64, 1 <= iters <= 4");
  MREC_CHECK_ARG(a->batch >= 0, "negative batch");
  MREC_CHECK_ARG(a->ld_rows >= a->D && a->ld_his >= a->L && a->ld_w >= a->D && a->ld_init >= a->L,
                 "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(md_aligned(a->rows) && a->ld_rows % 8 == 0,
                 "rows must be 16-byte aligned bf16 rows (ld_rows a multiple of 8)");
  MREC_CHECK_ARG(md_aligned(a->route_w) && a->ld_w % 4 == 0,
                 "route_w must be 16-byte aligned fp32 rows (ld_w a multiple of 4)");
  MindArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his = a->his;
  p.ld_his = a->ld_his;
  p.his_len = a->his_len;
  p.s = a->route_w;
  p.ld_s = a->ld_w;
  p.init = a->route_init;
  p.ld_init = a->ld_init;
  p.batch = a->batch;
  p.L = a->L;
  p.K = a->K;
  p.iters = a->iters;
  p.dynamic_k = a->dynamic_k;
  p.u = a->u;
  p.w = static_cast<uint16_t *>(a->w);
  p.z = a->z;
  p.du = a->du;
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  *out = p;
  return MREC_OK;
}

template <typename Fn>
void md_dispatch(int D, Fn &&f) {
  if (D == 16)
    f(std::integral_constant<int, 16>{});
  else if (D == 32)
    f(std::integral_constant<int, 32>{});
  else
    f(std::integral_constant<int, 64>{});
}

template <int D>
void md_set_attrs() {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mind_fwd_kernel<D>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, MD_WAVES * MD_FWD_WAVE_B);
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(mind_bwd_kernel<D>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, MD_WAVES * MD_BWD_WAVE_B);
  (void)hipGetLastError();
}

}  // namespace

extern "C" {

int32_t mrec_mind_supported(int32_t D, int32_t K, int32_t L, int32_t iters) {
  return (D == 16 || D == 32 || D == 64) && K >= 1 && K <= MD_KMAX && L >= 1 && L <= MD_ROWS &&
                 iters >= 1 && iters <= MD_MAX_ITERS
             ? 1
             : 0;
}

int64_t mrec_mind_parts(int64_t batch) {
  const int64_t g = device_cus(), need = (batch + MD_WAVES - 1) / MD_WAVES;
  return need < g ? (need > 0 ? need : 1) : g;
}

mrec_status mrec_mind_fwd(const mrec_mind_args *a, mrec_stream stream) {
  MindArgs p;
  const mrec_status st = md_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->u, "NULL pointer");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(mrec_mind_parts(p.batch));
  hipStream_t s = static_cast<hipStream_t>(stream);
  md_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    static const int once = (md_set_attrs<D>(), 1);
    (void)once;
    mind_fwd_kernel<D><<<dim3(grid), MD_THREADS, MD_WAVES * MD_FWD_WAVE_B, s>>>(p);
  });
  return launch_status("mrec_mind_fwd");
}

mrec_status mrec_mind_bwd(const mrec_mind_args *a, mrec_stream stream) {
  MindArgs p;
  const mrec_status st = md_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->du && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= a->D && a->ld_drows % 8 == 0 && md_aligned(a->d_rows),
                 "d_rows must be 16-byte aligned bf16 rows (ld_drows a multiple of 8, >= D)");
  MREC_CHECK_ARG(a->parts == mrec_mind_parts(a->batch), "parts must be mrec_mind_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  md_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    static const int once = (md_set_attrs<D>(), 1);
    (void)once;
    mind_bwd_kernel<D><<<dim3(grid), MD_THREADS, MD_WAVES * MD_BWD_WAVE_B, s>>>(p);
  });
  return launch_status("mrec_mind_bwd");
}

}  // extern "C"
