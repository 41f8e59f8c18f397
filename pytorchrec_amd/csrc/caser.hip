// Caser sequence encoder (Tang & Wang, WSDM 2018): the horizontal convolutions with their
// max-over-time pooling, the vertical convolution and the final layer, one launch each way
// for the batch (the forward first; the backward's design is above its kernel).
//
//   valid_j = his_j > 0 or j == 0;  n = 1 + the last valid position;  X = the rows, zero at
//   invalid positions and at and past n
//   pre_h[t, f] = bh_h[f] + sum_{k < h, d} X[t + k, d] Wh_h[f, k, d],  t = 0 .. max(n - h, 0)
//   pick_h[f]   = the lowest t that attains max_t pre_h[t, f];  o_h[f] = relu(pre_h[pick, f])
//   o_v[j, d]   = relu(bv[j] + sum_{t < n} Wv[j, n - 1 - t] X[t, d])
//   z = bf16([o_h ... | o_v]),  v = relu(W1 z + b1)
//
// Work split: a persistent grid of 4-wave workgroups, 16 samples (a group) at a time.  In the
// conv stage a wave owns one sample at a time: its [72][D + 8] bf16 tile of X is private to the
// wave, so the stage has no workgroup barrier.  The tile has 8 zero rows past position 63, and
// invalid rows are written as zeros.
// Horizontal conv: a GEMM whose im2col is never built.  M = windows in tiles of 16, N =
// filters, K = h D; the A fragment of window t, K-slice (k, d0 .. d0 + 7) is the 16-byte LDS
// read at row t + k.  The B fragment is 8 consecutive fp32 elements of Wh_h[f], rounded at use,
// fetched once per K-step and used by every window tile (the weights stream from L2: DESIGN.md
// 3.29).  Bias, the window mask and the maximum with its lowest index are reduced over the
// accumulator's rows in registers, then over the four lane groups with two shuffles.
// Vertical conv: M = filters padded to 16 (A gathered from Wv in reverse, zero past n), B the
// tile through the transposing LDS reads, K = positions.
// Final layer: z of the 16 samples is one [16][Z] bf16 LDS tile; after one barrier W1 z is a
// 16-row MFMA per 16 output columns, one column tile per wave.
// No atomics; a sample's tile and z row are written in full before they are read.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int CS_WAVES = 4;
constexpr int CS_THREADS = 64 * CS_WAVES;
constexpr int CS_GROUP = 16;       // samples per workgroup pass: the final layer's M
constexpr int CS_ROWS = 72;        // positions per tile: 64 + the tallest filter
constexpr int CS_MAX_HEIGHTS = 4;
constexpr int CS_MAX_H = 8;
constexpr int CS_MAX_NV = 8;
constexpr int CS_MAX_Z = 4 * 32 + 8 * 64;  // 640
constexpr int CS_LDZ = CS_MAX_Z + 8;       // bf16 elements per z row (1296 B)
constexpr int CS_LDP = 72;                 // bf16 elements per dpre row
constexpr int CS_MAX_WH = 16384;           // (sum of heights) n_h D: 64 accumulators per lane
constexpr int CS_MAX_F = CS_MAX_HEIGHTS * 32;  // filters over all heights

struct CaserArgs {
  const uint16_t *rows;  // gathered item rows [batch * L] bf16
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const float *wh[CS_MAX_HEIGHTS];  // [n_h][h][D]
  const float *bh[CS_MAX_HEIGHTS];  // [n_h]
  const float *wv, *bv, *w1, *b1;   // [n_v][L], [n_v], [D][Z], [D]
  int64_t batch;
  int L, nH, n_h, n_v, Z, nF;  // nF = nH n_h
  int hts[CS_MAX_HEIGHTS];
  int wh_total;  // elements of all Wh_h
  float *v;        // [batch][D]
  uint16_t *z;     // [batch][Z] bf16 (may be NULL in the forward)
  uint8_t *pick;   // [batch][nF] (may be NULL in the forward)
  const float *dv;
  uint16_t *dpre;  // [batch][D] bf16: dv (v > 0), the dW1 product's operand
  uint16_t *drows;
  int64_t ld_drows;
  float *part;  // [gridDim.x][P]
  int64_t P;
};

// orders a wave's own LDS writes before its reads of them
__device__ __forceinline__ void cs_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// the valid positions of sample b as a bit mask (bit 0 is always set); every lane of a wave
__device__ __forceinline__ unsigned long long cs_valid_mask(const CaserArgs &p, int64_t b, int lane) {
  const int id = lane < p.L ? p.his[b * p.ld_his + lane] : 0;
  return __ballot(lane < p.L && (lane == 0 || id > 0));
}

// sample b's rows into a [CS_ROWS][D + 8] tile by `nt` threads (t of them this one): zeros at
// invalid positions and from L to the tile's end
template <int D>
__device__ __forceinline__ void cs_stage(const CaserArgs &p, int64_t b, unsigned long long mask,
                                         uint16_t *xt, int t, int nt) {
  constexpr int LD = D + 8, CPR = D / 8;
  for (int c = t; c < CS_ROWS * CPR; c += nt) {
    const int r = c / CPR, q = c % CPR;
    uint4 val = make_uint4(0, 0, 0, 0);
    if (r < p.L && ((mask >> r) & 1ull))
      val = *reinterpret_cast<const uint4 *>(p.rows + (b * p.L + r) * p.ld_rows + 8 * q);
    *reinterpret_cast<uint4 *>(xt + r * LD + 8 * q) = val;
  }
}

// 8 fp32 elements `ld` apart, rounded to one fragment; zero from element `lim` on
__device__ __forceinline__ bf16x8 cs_frag_strided(const float *w, int64_t ld, int k0, int lim) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = k0 + e < lim ? w[(k0 + e) * ld] : 0.f;
  return frag_pack8(f);
}

// Wv in reverse as an MFMA operand over positions: element e is Wv[j, n - 1 - (t0 + e)], zero
// for j >= n_v and positions at and past n
__device__ __forceinline__ bf16x8 cs_wv_frag(const CaserArgs &p, int j, int t0, int n) {
  float f[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int t = t0 + e;
    f[e] = j < p.n_v && t < n ? p.wv[j * p.L + (n - 1 - t)] : 0.f;
  }
  return frag_pack8(f);
}

template <int D>
__global__ __launch_bounds__(CS_THREADS) void caser_fwd_kernel(CaserArgs p) {
  constexpr int LD = D + 8;
  extern __shared__ __align__(16) unsigned char cs_smem[];
  uint16_t *zt = reinterpret_cast<uint16_t *>(cs_smem);  // [16][CS_LDZ]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  uint16_t *xt = zt + CS_GROUP * CS_LDZ + wave * CS_ROWS * LD;
  const int Z = p.Z, Zp = (Z + 31) & ~31, nF = p.nF;
  // the final layer's K runs to a multiple of 32: those columns are zero for good
  for (int c = tid; c < CS_GROUP * (Zp - Z); c += CS_THREADS)
    zt[(c / (Zp - Z)) * CS_LDZ + Z + c % (Zp - Z)] = 0;

  const int64_t groups = (p.batch + CS_GROUP - 1) / CS_GROUP;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t b0 = g * CS_GROUP;
    const int cnt = static_cast<int>(p.batch - b0 < CS_GROUP ? p.batch - b0 : CS_GROUP);
    for (int s = wave; s < cnt; s += CS_WAVES) {
      const int64_t b = b0 + s;
      const unsigned long long mask = cs_valid_mask(p, b, lane);
      const int n = 64 - __builtin_clzll(mask);
      cs_wave_sync();  // the previous sample's reads of the tile are done
      cs_stage<D>(p, b, mask, xt, lane, 64);
      cs_wave_sync();
      uint16_t *zrow = zt + s * CS_LDZ;
      // ---- horizontal: windows x filters, pooled in registers ----
      int zoff = 0;
      for (int hi = 0; hi < p.nH; ++hi) {
        const int h = p.hts[hi], hD = h * D;
        const int tmax = n > h ? n - h : 0;
        const int mtiles = tmax / 16 + 1;
        const int ksteps = (hD + 31) / 32;
        for (int nt = 0; nt < p.n_h / 16; ++nt) {
          const int f = 16 * nt + li;
          const float *wrow = p.wh[hi] + static_cast<int64_t>(f) * hD;
          f32x4 acc[4];
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
          for (int ks = 0; ks < ksteps; ++ks) {
            const int kk0 = 32 * ks + 8 * lg;
            const bool in = kk0 < hD;
            bf16x8 bfr = frag_zero8();
            if (in)
              bfr = frag_from_f32(*reinterpret_cast<const uint4 *>(wrow + kk0),
                                  *reinterpret_cast<const uint4 *>(wrow + kk0 + 4));
            const int k = in ? kk0 / D : 0, d = in ? kk0 % D : 0;
            const uint16_t *ap = xt + (li + k) * LD + d;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              if (mt < mtiles)
                acc[mt] = mfma_16x16x32(*reinterpret_cast<const bf16x8 *>(ap + 16 * mt * LD), bfr, acc[mt]);
          }
          const float bias = p.bh[hi][f];
          float best = -INFINITY;
          int bi = 0;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            if (mt < mtiles) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int t = 16 * mt + 4 * lg + i;
                const float pre = acc[mt][i] + bias;
                if (t <= tmax && pre > best) best = pre, bi = t;
              }
            }
#pragma unroll
          for (int off = 16; off <= 32; off <<= 1) {
            const float ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
          }
          if (lane < 16) {
            zrow[zoff + f] = f32_to_bf16_rne(fmaxf(best, 0.f));
            if (p.pick) p.pick[b * nF + zoff + f] = static_cast<uint8_t>(bi);
          }
        }
        zoff += p.n_h;
      }
      // ---- vertical: filters (padded to 16) x D over the positions ----
      const int vks = (n + 31) / 32;
      bf16x8 va[2];
      va[0] = cs_wv_frag(p, li, 8 * lg, n);
      va[1] = vks > 1 ? cs_wv_frag(p, li, 32 + 8 * lg, n) : frag_zero8();
#pragma unroll
      for (int nt = 0; nt < D / 16; ++nt) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          if (ks < vks)
            acc = mfma_16x16x32(va[ks],
                                lds_tr16_pair(xt + (32 * ks + 8 * lg + (li >> 2)) * LD + 16 * nt + 4 * (li & 3), 4 * LD),
                                acc);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = 4 * lg + i;
          if (j < p.n_v) zrow[nF + j * D + 16 * nt + li] = f32_to_bf16_rne(fmaxf(acc[i] + p.bv[j], 0.f));
        }
      }
    }
    __syncthreads();
    // ---- final layer: v = relu(W1 z + b1), 16 samples x 16 columns per wave ----
    for (int nt = wave; nt < D / 16; nt += CS_WAVES) {
      const int dcol = 16 * nt + li;
      const float *wrow = p.w1 + static_cast<int64_t>(dcol) * Z;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int kk0 = 8 * lg; kk0 < Zp; kk0 += 32) {
        bf16x8 bfr = frag_zero8();
        if (kk0 < Z)
          bfr = frag_from_f32(*reinterpret_cast<const uint4 *>(wrow + kk0),
                              *reinterpret_cast<const uint4 *>(wrow + kk0 + 4));
        acc = mfma_16x16x32(*reinterpret_cast<const bf16x8 *>(zt + li * CS_LDZ + kk0), bfr, acc);
      }
      const float bias = p.b1[dcol];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = 4 * lg + i;
        if (s < cnt) p.v[(b0 + s) * D + dcol] = fmaxf(acc[i] + bias, 0.f);
      }
    }
    if (p.z) {
      const int cpr = Z / 8;
      for (int c = tid; c < cnt * cpr; c += CS_THREADS) {
        const int s = c / cpr, q = c % cpr;
        *reinterpret_cast<uint4 *>(p.z + (b0 + s) * Z + 8 * q) =
            *reinterpret_cast<const uint4 *>(zt + s * CS_LDZ + 8 * q);
      }
    }
    __syncthreads();
  }
}

// Backward.  A workgroup takes 16 samples at a time and keeps every dense gradient but W1's in
// registers over all of its samples; one partial per workgroup at the end.
//   dpre = dv (v > 0), rounded to bf16: written out as the dW1 / db1 product's operand (that
//   product, dpre^T [z | 1] over the batch, is the existing GEMM's: [D, Z] per workgroup would
//   be up to 160 more accumulators per lane and 160 KiB per partial) and kept in LDS;
//   G = (dpre W1) (z > 0) for the 16 samples by MFMA (M = samples, N = Z, K = D; the W1
//   fragment is 8 elements of a column, gathered from the fp32 master), fp32 in LDS.
// Then per sample, the whole workgroup on it, two barriers:
//   dWh_h[f, k, :] += G[f] X[pick + k, :] and dbh on the VALU.  The masked dY of a filter has
//   one non-zero, its pick, so a dY^T X product over the windows would spend 64 values of K on
//   it; the direct form is 64 FMAs per lane, the (f, k, d0 .. d0 + 7) chunks of all heights
//   dealt round-robin to the 256 lanes and fixed for the kernel's life;
//   dWv[j, n - 1 - t] += G_v[j, :] . X[t, :] and dbv on the VALU, lane = (j, distance);
//   dX = sum_{h, k} dY_h shifted down by k rows times Wh_h[:, k, :] by MFMA: dY_h [8 + 64][n_h]
//   bf16 tiles in LDS hold G at row 8 + pick (8 zero rows in front: a shift is the A fragment's
//   row address), K = (k, f) over every height, plus one K-step for the vertical term
//   (A = Wv in reverse, B = G_v); M = positions, N = D, a (16 rows, 16 columns) task per wave
//   at a time.  One bf16 store of d_rows follows, zero at invalid positions.
// No atomics: the accumulation order is the sample order.
template <int D>
__global__ __launch_bounds__(CS_THREADS) void caser_bwd_kernel(CaserArgs p) {
  constexpr int LD = D + 8, NCT = D / 16;
  extern __shared__ __align__(16) unsigned char cs_smem[];
  float *gt = reinterpret_cast<float *>(cs_smem);                         // [16][CS_MAX_Z]
  uint16_t *dpt = reinterpret_cast<uint16_t *>(gt + CS_GROUP * CS_MAX_Z);  // [16][CS_LDP]
  uint16_t *xt = dpt + CS_GROUP * CS_LDP;                                 // [CS_ROWS][LD]
  int *pks = reinterpret_cast<int *>(xt + CS_ROWS * (64 + 8));            // [CS_MAX_F]
  uint16_t *dyt = reinterpret_cast<uint16_t *>(pks + CS_MAX_F);           // [nH][CS_ROWS][n_h + 8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int Z = p.Z, nF = p.nF, L = p.L, n_h = p.n_h, LDY = n_h + 8;
  for (int c = tid; c < CS_GROUP * CS_LDP; c += CS_THREADS) dpt[c] = 0;
  for (int c = tid; c < p.nH * CS_ROWS * LDY; c += CS_THREADS) dyt[c] = 0;

  // this lane's chunks of the horizontal weights: 8 consecutive d of one (height, f, k)
  int cf[8], crow[8];  // filter index over all heights (-1: none); k LD + d0, the tile offset
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int e = (tid + CS_THREADS * j) * 8;
    cf[j] = -1, crow[j] = 0;
    if (e < p.wh_total) {
      int hi = 0;
      while (e >= n_h * p.hts[hi] * D) e -= n_h * p.hts[hi] * D, ++hi;
      const int hD = p.hts[hi] * D;
      cf[j] = hi * n_h + e / hD;
      crow[j] = ((e % hD) / D) * LD + e % D;
    }
  }
  float accw[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) accw[j][i] = 0.f;
  float accbh = 0.f, accwv[2] = {0.f, 0.f}, accbv[2] = {0.f, 0.f};

  const int64_t groups = (p.batch + CS_GROUP - 1) / CS_GROUP;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t b0 = g * CS_GROUP;
    const int cnt = static_cast<int>(p.batch - b0 < CS_GROUP ? p.batch - b0 : CS_GROUP);
    __syncthreads();
    for (int c = tid; c < CS_GROUP * D; c += CS_THREADS) {
      const int s = c / D, d = c % D;
      uint16_t r = 0;
      if (s < cnt) {
        const int64_t o = (b0 + s) * D + d;
        r = f32_to_bf16_rne(p.v[o] > 0.f ? p.dv[o] : 0.f);
        p.dpre[o] = r;
      }
      dpt[s * CS_LDP + d] = r;
    }
    __syncthreads();
    // ---- G = (dpre W1) (z > 0) ----
    for (int nt = wave; nt < Z / 16; nt += CS_WAVES) {
      const int zi = 16 * nt + li;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < (D + 31) / 32; ++ks) {
        const int k0 = 32 * ks + 8 * lg;
        acc = mfma_16x16x32(*reinterpret_cast<const bf16x8 *>(dpt + li * CS_LDP + k0),
                            cs_frag_strided(p.w1 + zi, Z, k0, D), acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = 4 * lg + i;
        float gz = 0.f;
        if (s < cnt && static_cast<int16_t>(p.z[(b0 + s) * Z + zi]) > 0) gz = acc[i];
        gt[s * CS_MAX_Z + zi] = gz;
      }
    }
    __syncthreads();
    for (int s = 0; s < cnt; ++s) {
      const int64_t b = b0 + s;
      const float *gs = gt + s * CS_MAX_Z;
      const unsigned long long mask = cs_valid_mask(p, b, lane);
      const int n = 64 - __builtin_clzll(mask);
      cs_stage<D>(p, b, mask, xt, tid, CS_THREADS);
      int dyo = 0;
      if (tid < nF) {
        int pk = p.pick[b * nF + tid];
        pk = pk < 64 ? pk : 63;
        pks[tid] = pk;
        dyo = ((tid / n_h) * CS_ROWS + 8 + pk) * LDY + tid % n_h;
        dyt[dyo] = f32_to_bf16_rne(gs[tid]);
        accbh += gs[tid];
      }
      __syncthreads();
      // ---- dWh on the VALU ----
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (cf[j] >= 0) {
          const float gf = gs[cf[j]];
          const uint4 x = *reinterpret_cast<const uint4 *>(xt + pks[cf[j]] * LD + crow[j]);
          float xf[8];
          Vec<uint16_t>::to_f32(x, xf);
#pragma unroll
          for (int i = 0; i < 8; ++i) accw[j][i] = fmaf(gf, xf[i], accw[j][i]);
        }
      // ---- dWv, dbv on the VALU: lane = (filter j, distance c from the last item) ----
#pragma unroll
      for (int i2 = 0; i2 < 2; ++i2) {
        const int j = (tid + CS_THREADS * i2) >> 6, c = lane;
        if (j < p.n_v && c < n) {
          const float *gv = gs + nF + j * D;
          const uint16_t *xr = xt + (n - 1 - c) * LD;
          float dot = 0.f, sum = 0.f;
#pragma unroll
          for (int q = 0; q < D / 8; ++q) {
            float xf[8];
            Vec<uint16_t>::to_f32(*reinterpret_cast<const uint4 *>(xr + 8 * q), xf);
#pragma unroll
            for (int i = 0; i < 8; ++i) dot = fmaf(gv[8 * q + i], xf[i], dot), sum += gv[8 * q + i];
          }
          accwv[i2] += dot;
          if (c == 0) accbv[i2] += sum;
        }
      }
      // ---- dX by MFMA ----
      for (int task = wave; task < 4 * NCT; task += CS_WAVES) {
        const int ct = task % NCT, rt = task / NCT;
        if (16 * rt >= L) continue;
        const int dcol = 16 * ct + li, r = 16 * rt + li;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int hi = 0; hi < p.nH; ++hi) {
          const int h = p.hts[hi], hF = h * n_h;
          const uint16_t *dy = dyt + hi * CS_ROWS * LDY;
          for (int kk0 = 8 * lg; kk0 < ((hF + 31) & ~31); kk0 += 32) {
            const bool in = kk0 < hF;
            const int k = in ? kk0 / n_h : 0, f0 = in ? kk0 % n_h : 0;
            const bf16x8 bfr = cs_frag_strided(p.wh[hi] + static_cast<int64_t>(f0) * h * D + k * D + dcol,
                                               static_cast<int64_t>(h) * D, 0, in ? 8 : 0);
            acc = mfma_16x16x32(*reinterpret_cast<const bf16x8 *>(dy + (8 + r - k) * LDY + f0), bfr, acc);
          }
        }
        {  // the vertical term: K = the filters, in the first lane group's 8 elements
          float a[8], f[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const bool on = lg == 0 && e < p.n_v;
            f[e] = on ? gs[nF + e * D + dcol] : 0.f;
            a[e] = on && r < n ? p.wv[e * L + (n - 1 - r)] : 0.f;
          }
          acc = mfma_16x16x32(frag_pack8(a), frag_pack8(f), acc);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = 16 * rt + 4 * lg + i;
          if (row < L)
            p.drows[(b * L + row) * p.ld_drows + dcol] =
                (mask >> row) & 1ull ? f32_to_bf16_rne(acc[i]) : static_cast<uint16_t>(0);
        }
      }
      __syncthreads();
      if (tid < nF) dyt[dyo] = 0;
    }
  }
  // ---- the partial: [Wh of every height | bh of every height | Wv | bv] ----
  float *part = p.part + blockIdx.x * p.P;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int e = (tid + CS_THREADS * j) * 8;
    if (e < p.wh_total) {
      *reinterpret_cast<float4 *>(part + e) = make_float4(accw[j][0], accw[j][1], accw[j][2], accw[j][3]);
      *reinterpret_cast<float4 *>(part + e + 4) = make_float4(accw[j][4], accw[j][5], accw[j][6], accw[j][7]);
    }
  }
  if (tid < nF) part[p.wh_total + tid] = accbh;
#pragma unroll
  for (int i2 = 0; i2 < 2; ++i2) {
    const int j = (tid + CS_THREADS * i2) >> 6, c = lane;
    if (j < p.n_v && c < L) part[p.wh_total + nF + j * L + c] = accwv[i2];
    if (j < p.n_v && c == 0) part[p.wh_total + nF + p.n_v * L + j] = accbv[i2];
  }
}

constexpr int CS_FWD_LDS_B = (CS_GROUP * CS_LDZ + CS_WAVES * CS_ROWS * (64 + 8)) * 2;
constexpr int CS_BWD_LDS_B = CS_GROUP * CS_MAX_Z * 4 + CS_GROUP * CS_LDP * 2 + CS_ROWS * (64 + 8) * 2 +
                             CS_MAX_F * 4 + CS_MAX_HEIGHTS * CS_ROWS * (32 + 8) * 2;

}  // namespace mrec

using namespace mrec;

namespace {

bool cs_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int64_t cs_sum_heights(int32_t nH, const int32_t *hts) {
  int64_t s = 0;
  for (int i = 0; i < nH; ++i) s += hts[i];
  return s;
}

mrec_status cs_check(const mrec_caser_args *a, CaserArgs *out) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(a->rows && a->his && a->wv && a->bv && a->w1 && a->b1, "NULL pointer");
  MREC_CHECK_ARG(mrec_caser_supported(a->D, a->L, a->n_heights, a->heights, a->n_h, a->n_v),
                 "need D in {16, 32, 64}, 1 <= L <= 64, 1 to 4 distinct ascending heights in 1..8, n_h 16 or "
                 "32, 1 <= n_v <= 8 and (sum of heights) n_h D <= 16384");
  for (int i = 0; i < a->n_heights; ++i)
    MREC_CHECK_ARG(a->wh[i] && a->bh[i] && cs_aligned(a->wh[i]), "a height's weights are NULL or not 16-byte aligned");
  MREC_CHECK_ARG(a->batch >= 0, "negative batch");
  MREC_CHECK_ARG(a->ld_rows >= a->D && a->ld_his >= a->L, "a leading dimension is smaller than its row");
  MREC_CHECK_ARG(cs_aligned(a->rows) && a->ld_rows % 8 == 0,
                 "rows must be 16-byte aligned bf16 rows (ld_rows a multiple of 8)");
  MREC_CHECK_ARG(cs_aligned(a->w1) && cs_aligned(a->z), "w1 and z must be 16-byte aligned");
  CaserArgs p{};
  p.rows = static_cast<const uint16_t *>(a->rows);
  p.ld_rows = a->ld_rows;
  p.his = a->his;
  p.ld_his = a->ld_his;
  for (int i = 0; i < a->n_heights; ++i) p.wh[i] = a->wh[i], p.bh[i] = a->bh[i], p.hts[i] = a->heights[i];
  p.wv = a->wv, p.bv = a->bv, p.w1 = a->w1, p.b1 = a->b1;
  p.batch = a->batch;
  p.L = a->L, p.nH = a->n_heights, p.n_h = a->n_h, p.n_v = a->n_v;
  p.nF = a->n_heights * a->n_h;
  p.Z = p.nF + a->n_v * a->D;
  p.wh_total = static_cast<int>(cs_sum_heights(a->n_heights, a->heights) * a->n_h * a->D);
  p.v = a->v;
  p.z = static_cast<uint16_t *>(a->z);
  p.pick = a->pick;
  p.dv = a->dv;
  p.dpre = static_cast<uint16_t *>(a->dpre);
  p.drows = static_cast<uint16_t *>(a->d_rows);
  p.ld_drows = a->ld_drows;
  p.part = a->part;
  p.P = mrec_caser_param_count(a->D, a->L, a->n_heights, a->heights, a->n_h, a->n_v);
  *out = p;
  return MREC_OK;
}

template <typename Fn>
void cs_dispatch(int D, Fn &&f) {
  if (D == 16)
    f(std::integral_constant<int, 16>{});
  else if (D == 32)
    f(std::integral_constant<int, 32>{});
  else
    f(std::integral_constant<int, 64>{});
}

}  // namespace

extern "C" {

int32_t mrec_caser_supported(int32_t D, int32_t L, int32_t n_heights, const int32_t *heights, int32_t n_h,
                             int32_t n_v) {
  if (!(D == 16 || D == 32 || D == 64) || L < 1 || L > 64) return 0;
  if (n_heights < 1 || n_heights > CS_MAX_HEIGHTS || !heights) return 0;
  if (!(n_h == 16 || n_h == 32) || n_v < 1 || n_v > CS_MAX_NV) return 0;
  for (int i = 0; i < n_heights; ++i)
    if (heights[i] < 1 || heights[i] > CS_MAX_H || (i && heights[i] <= heights[i - 1])) return 0;
  return cs_sum_heights(n_heights, heights) * n_h * D <= CS_MAX_WH ? 1 : 0;
}

int64_t mrec_caser_parts(int64_t batch) {
  const int64_t groups = (batch + CS_GROUP - 1) / CS_GROUP, g = device_cus();
  return groups < g ? (groups > 0 ? groups : 1) : g;
}

int64_t mrec_caser_param_count(int32_t D, int32_t L, int32_t n_heights, const int32_t *heights, int32_t n_h,
                               int32_t n_v) {
  if (!mrec_caser_supported(D, L, n_heights, heights, n_h, n_v)) return 0;
  return cs_sum_heights(n_heights, heights) * n_h * D + static_cast<int64_t>(n_heights) * n_h +
         static_cast<int64_t>(n_v) * L + n_v;
}

mrec_status mrec_caser_fwd(const mrec_caser_args *a, mrec_stream stream) {
  CaserArgs p;
  const mrec_status st = cs_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v, "NULL pointer");
  MREC_CHECK_ARG((a->z == nullptr) == (a->pick == nullptr), "z and pick are saved together");
  if (p.batch == 0) return MREC_OK;
  const int64_t groups = (p.batch + CS_GROUP - 1) / CS_GROUP, cus = device_cus();
  const unsigned grid = static_cast<unsigned>(groups < cus ? groups : cus);
  hipStream_t s = static_cast<hipStream_t>(stream);
  cs_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    static const int once = ((void)hipFuncSetAttribute(reinterpret_cast<const void *>(caser_fwd_kernel<D>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, CS_FWD_LDS_B),
                             (void)hipGetLastError(), 1);
    (void)once;
    caser_fwd_kernel<D><<<dim3(grid), CS_THREADS, CS_FWD_LDS_B, s>>>(p);
  });
  return launch_status("mrec_caser_fwd");
}

mrec_status mrec_caser_bwd(const mrec_caser_args *a, mrec_stream stream) {
  CaserArgs p;
  const mrec_status st = cs_check(a, &p);
  if (st != MREC_OK) return st;
  MREC_CHECK_ARG(a->v && a->z && a->pick && a->dv && a->dpre && a->d_rows && a->part, "NULL pointer");
  MREC_CHECK_ARG(a->ld_drows >= a->D, "ld_drows is smaller than a row");
  MREC_CHECK_ARG(a->parts == mrec_caser_parts(a->batch), "parts must be mrec_caser_parts(batch)");
  if (p.batch == 0) return MREC_OK;
  const unsigned grid = static_cast<unsigned>(a->parts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  cs_dispatch(a->D, [&](auto d) {
    constexpr int D = decltype(d)::value;
    static const int once = ((void)hipFuncSetAttribute(reinterpret_cast<const void *>(caser_bwd_kernel<D>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, CS_BWD_LDS_B),
                             (void)hipGetLastError(), 1);
    (void)once;
    caser_bwd_kernel<D><<<dim3(grid), CS_THREADS, CS_BWD_LDS_B, s>>>(p);
  });
  return launch_status("mrec_caser_bwd");
}

}  // extern "C"
