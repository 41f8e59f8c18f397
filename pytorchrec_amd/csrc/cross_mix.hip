// DCN-Mix cross stack: low-rank mixture-of-experts cross layers (mrec.h "DCN-Mix", ABI 42).
//
//   t_i = V_i x_l   a_i = bf16(tanh t_i)   c_i = bf16(tanh(C_i a_i))   gamma = softmax(gate x_l)
//   s_i = bf16(gamma_i c_i)   z = U [s_1 | .. | s_K] + b   x_{l+1} = bf16(x0 * z + x_l)
//
// A workgroup of 8 waves owns a tile of 16 samples; every product is v_mfma_f32_16x16x32_bf16
// with the samples as the 16 rows.  Operand map: lane (col = lane & 15, q = lane >> 4) holds
// A[row col][k = 8 q + j] and B[k = 8 q + j][col]; the accumulator has its column on the lane
// and row 4 q + e in register e.  The A operand is always a bf16 tile in LDS with k contiguous
// (one 16-byte read per fragment); the B operand is a row of a bf16 weight image in memory,
// one row per output column with k contiguous (one 16-byte load per fragment: a layer's images
// are < 1 MB and stay in L2).  A product's 16-column output tiles go round the waves.
//
//   forward   one launch for the stack.  x0 and x_l stay in LDS as bf16 from the first layer
//             to the last.  [t | logits] = x_l [V ; gate]^T: the t tiles leave as a (LDS), the
//             gate tile's wave turns its K logits into gamma (fp32, exchanged inside the
//             16-lane group) and leaves them in LDS.  c = a C_i^T per expert (k = r), s leaves
//             for LDS; z = s U^T and the tail are the third product's epilogue, which
//             overwrites x_l in place (a lane reads and writes only its own elements).  In
//             training each layer's input goes to the saved stack; x_L is the only other store.
//   backward  one launch for the stack, top layer first.  Per layer it reloads x_l from the
//             saved stack, recomputes a, c, gamma, s, z with the forward's code (equal bits),
//             then dz = g x0, ds = dz U, du = gamma ds (1 - c^2), dlogit, dt = (du C_i)(1 -
//             a^2) and dx_l = g + [dt | dlogit] [V ; gate], which replaces g in LDS (bf16).
//             sum_l g z and layer 0's dx_l are fp32 accumulators in registers (the z and dx_l
//             products share their tile-to-wave map), stored once as dx0.  dz, s, du, a and
//             [dt | dlogit] go to the workspace in bf16: the operands of the weight-gradient
//             GEMMs, which the caller runs on mrec_gemm.  No atomics: a sample's results depend
//             on that sample alone.
//
// Tile height 16: at B = 4096 that is 256 workgroups, one per CU, each reading every weight
// image once per layer from L2.  32 rows would halve the image reads per sample but leave
// half the CUs idle at that batch, and the latency of a workgroup's own reads, not L2's total
// rate, bounds it here; DESIGN.md 3.24 has the measured cost.
// LDS at d = 512, K r = 256, K = 4: forward 2 x 16,640 (x0, x_l) + 2 x 9,472 (a, s) + 256 =
// 52,480 bytes; backward 4 x 16,640 (x0, x_l, g, dz) + 5 x 9,472 (a, c, s, du, [dt | dlogit]) +
// 16,640 (ds, fp32) + 256 = 130,816 bytes of the 160 KB.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int XM_TM = 16;        // samples per tile
constexpr int XM_THREADS = 512;  // 8 waves
constexpr int XM_WAVES = 8;
constexpr int XM_JT = 4;         // d-wide output tiles per wave: 512 / 16 / 8
constexpr int XM_LDS_BUDGET = 160 * 1024;

struct XmLayer {
  const uint16_t *vg, *vgT, *u, *uT, *c, *cT;
  const float *b;
};

struct XmArgs {
  MatIn x0, dy;
  uint16_t *y, *saved;
  int64_t ld_y, ld_saved, saved_layer;
  float *dx0;
  int64_t ld_dx0;
  uint16_t *w_dz, *w_s, *w_du, *w_a, *w_dtl;  // [layers][B][dp8 | kr | kr | kr | n1]
  XmLayer lay[MREC_CROSS_MIX_MAX_LAYERS];
  int64_t B, tiles;
  int32_t d, K, r, L, train;
  int32_t dp8, dk, kr, krk, n1, n1k, rk, px, pn, pds;
};

// one 16 x 16 output tile: arow = this lane's row of the LDS tile at the product's first k,
// wrow = this lane's image row.  GUARD: fragments at k >= kvalid are zero (r = 16 is half a k
// step); without it every load is unconditional and the steps' loads overlap.
template <bool GUARD>
__device__ __forceinline__ f32x4 xm_tile(const uint16_t *arow, const uint16_t *wrow, int ksteps, int kvalid, int q) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  arow += 8 * q, wrow += 8 * q;
  if constexpr (GUARD) {
    for (int s = 0; s < ksteps; ++s) {
      bf16x8 a = frag_zero8(), w = frag_zero8();
      if (32 * s + 8 * q < kvalid) {
        a = *reinterpret_cast<const bf16x8 *>(arow + 32 * s);
        w = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wrow + 32 * s));
      }
      acc = mfma_16x16x32(a, w, acc);
    }
  } else {
    // two steps at a time into two accumulators: four loads in flight, no MFMA waits on the last
    f32x4 odd = {0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 2 <= ksteps; s += 2) {
      const bf16x8 a0 = *reinterpret_cast<const bf16x8 *>(arow + 32 * s);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8 *>(arow + 32 * s + 32);
      const uint4 w0 = *reinterpret_cast<const uint4 *>(wrow + 32 * s);
      const uint4 w1 = *reinterpret_cast<const uint4 *>(wrow + 32 * s + 32);
      acc = mfma_16x16x32(a0, __builtin_bit_cast(bf16x8, w0), acc);
      odd = mfma_16x16x32(a1, __builtin_bit_cast(bf16x8, w1), odd);
    }
    if (s < ksteps)
      acc = mfma_16x16x32(*reinterpret_cast<const bf16x8 *>(arow + 32 * s),
                          __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wrow + 32 * s)), acc);
    acc += odd;
  }
  return acc;
}

// rows row0 .. row0 + 15 of a bf16 or fp32 matrix as a bf16 [16][px] tile: rows >= B, columns
// >= d (the source's own pad columns among them) and the pitch pad are zeros
__device__ __forceinline__ void xm_stage(const XmArgs &p, const MatIn &m, int64_t row0, int tid, uint16_t *dst,
                                         uint16_t *dst2) {
  const int ch = p.px >> 3;
  for (int idx = tid; idx < XM_TM * ch; idx += XM_THREADS) {
    const int i = idx / ch, c0 = 8 * (idx - i * ch);
    bf16x8 v = frag_zero8();
    if (row0 + i < p.B && c0 < p.d) {
      v = mat_load8(m, row0 + i, c0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j >= p.d) v[j] = 0;
    }
    *reinterpret_cast<bf16x8 *>(dst + i * p.px + c0) = v;
    if (dst2) *reinterpret_cast<bf16x8 *>(dst2 + i * p.px + c0) = v;
  }
}

// a saved layer input (bf16 [B][ld_saved], pad columns zero) as a [16][px] tile
__device__ __forceinline__ void xm_stage_saved(const XmArgs &p, int l, int64_t row0, int tid, uint16_t *dst) {
  const int ch = p.px >> 3;
  const uint16_t *src = p.saved + l * p.saved_layer;
  for (int idx = tid; idx < XM_TM * ch; idx += XM_THREADS) {
    const int i = idx / ch, c0 = 8 * (idx - i * ch);
    bf16x8 v = frag_zero8();
    if (row0 + i < p.B && c0 < p.dp8) v = *reinterpret_cast<const bf16x8 *>(src + (row0 + i) * p.ld_saved + c0);
    *reinterpret_cast<bf16x8 *>(dst + i * p.px + c0) = v;
  }
}

// the first `cols` (a multiple of 8) columns of the live rows of an LDS tile to dst[B][ld]
__device__ __forceinline__ void xm_store_rows(const XmArgs &p, const uint16_t *tile, int pitch, int cols,
                                              int64_t row0, int tid, uint16_t *dst, int64_t ld) {
  const int ch = cols >> 3;
  for (int idx = tid; idx < XM_TM * ch; idx += XM_THREADS) {
    const int i = idx / ch, c0 = 8 * (idx - i * ch);
    if (row0 + i < p.B)
      *reinterpret_cast<uint4 *>(dst + (row0 + i) * ld + c0) = *reinterpret_cast<const uint4 *>(tile + i * pitch + c0);
  }
}

__device__ __forceinline__ void xm_zero(uint16_t *t, int elems, int tid) {
  for (int idx = tid; idx < (elems >> 3); idx += XM_THREADS) *reinterpret_cast<bf16x8 *>(t + 8 * idx) = frag_zero8();
}

// [t | logits] = x_l [V ; gate]^T: a = bf16(tanh t) to As, gamma (fp32 [16][4]) to Gm
__device__ __forceinline__ void xm_experts_in(const XmArgs &p, const XmLayer &w, const uint16_t *XL, uint16_t *As,
                                              float *Gm, int wave, int lane) {
  const int col = lane & 15, q = lane >> 4;
  for (int nt = wave; 16 * nt < p.n1; nt += XM_WAVES) {
    const f32x4 acc = xm_tile<false>(XL + col * p.px, w.vg + static_cast<int64_t>(16 * nt + col) * p.dk, p.dk >> 5, p.dk, q);
    if (16 * nt < p.kr) {
#pragma unroll
      for (int e = 0; e < 4; ++e) As[(4 * q + e) * p.pn + 16 * nt + col] = f32_to_bf16_rne(tanh_rcp(acc[e]));
    } else {  // the gate tile: this row's K logits lie in lanes 0 .. K - 1 of the 16-lane group
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float lg[4], mx = -INFINITY, sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          lg[j] = __shfl(acc[e], (lane & 48) + j);
          if (j < p.K) mx = fmaxf(mx, lg[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < p.K) sum += expf(lg[j] - mx);
        if (col < p.K) Gm[(4 * q + e) * 4 + col] = expf(acc[e] - mx) / sum;
      }
    }
  }
}

// c_i = bf16(tanh(a_i C_i^T)) (to Cs when given), s_i = bf16(gamma_i c_i) to Ss
__device__ __forceinline__ void xm_experts_mid(const XmArgs &p, const XmLayer &w, const uint16_t *As, uint16_t *Cs,
                                               uint16_t *Ss, const float *Gm, int wave, int lane) {
  const int col = lane & 15, q = lane >> 4;
  for (int nt = wave; 16 * nt < p.kr; nt += XM_WAVES) {
    const int i = 16 * nt / p.r;
    const f32x4 acc =
        xm_tile<true>(As + col * p.pn + i * p.r, w.c + static_cast<int64_t>(16 * nt + col) * p.rk, p.rk >> 5, p.r, q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = 4 * q + e;
      const uint16_t cb = f32_to_bf16_rne(tanh_rcp(acc[e]));
      const float g = p.K > 1 ? Gm[row * 4 + i] : 1.f;
      if (Cs) Cs[row * p.pn + 16 * nt + col] = cb;
      Ss[row * p.pn + 16 * nt + col] = f32_to_bf16_rne(g * bf16_to_f32(cb));
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(XM_THREADS) void cross_mix_fwd_kernel(XmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char xm_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  uint16_t *X0 = reinterpret_cast<uint16_t *>(xm_lds);
  uint16_t *XL = X0 + XM_TM * p.px;
  uint16_t *As = XL + XM_TM * p.px;
  uint16_t *Ss = As + XM_TM * p.pn;
  float *Gm = reinterpret_cast<float *>(Ss + XM_TM * p.pn);
  xm_zero(As, 2 * XM_TM * p.pn, tid);  // the k pad of a and s stays zero

  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int64_t row0 = tile * XM_TM;
    __syncthreads();
    xm_stage(p, p.x0, row0, tid, X0, XL);
    __syncthreads();
    for (int l = 0; l < p.L; ++l) {
      const XmLayer &w = p.lay[l];
      if (p.train) xm_store_rows(p, XL, p.px, p.dp8, row0, tid, p.saved + l * p.saved_layer, p.ld_saved);
      xm_experts_in(p, w, XL, As, Gm, wave, lane);
      __syncthreads();
      xm_experts_mid(p, w, As, nullptr, Ss, Gm, wave, lane);
      __syncthreads();
      // z = s U^T + b and the tail, in place on x_l
      for (int nt = wave; 16 * nt < p.d; nt += XM_WAVES) {
        const int n = 16 * nt + col;
        const f32x4 acc = xm_tile<false>(Ss + col * p.pn, w.u + static_cast<int64_t>(n) * p.krk, p.krk >> 5, p.krk, q);
        if (n < p.d) {
          const float bias = w.b[n];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int at = (4 * q + e) * p.px + n;
            XL[at] = f32_to_bf16_rne(bf16_to_f32(X0[at]) * (acc[e] + bias) + bf16_to_f32(XL[at]));
          }
        }
      }
      __syncthreads();
    }
    // x_L: whole 16-byte chunks, then the last partial one by element
    const int ch = p.dp8 >> 3;
    for (int idx = tid; idx < XM_TM * ch; idx += XM_THREADS) {
      const int i = idx / ch, c0 = 8 * (idx - i * ch);
      if (row0 + i >= p.B) continue;
      uint16_t *dst = p.y + (row0 + i) * p.ld_y + c0;
      if (c0 + 8 <= p.d) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(XL + i * p.px + c0);
      } else {
        for (int j = 0; c0 + j < p.d; ++j) dst[j] = XL[i * p.px + c0 + j];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: dx0 and the operands of the weight-gradient GEMMs
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(XM_THREADS) void cross_mix_bwd_kernel(XmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char xm_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, q = lane >> 4;
  uint16_t *X0 = reinterpret_cast<uint16_t *>(xm_lds);
  uint16_t *XL = X0 + XM_TM * p.px;
  uint16_t *G = XL + XM_TM * p.px;
  uint16_t *DZ = G + XM_TM * p.px;
  uint16_t *As = DZ + XM_TM * p.px;
  uint16_t *Cs = As + XM_TM * p.pn;
  uint16_t *Ss = Cs + XM_TM * p.pn;
  uint16_t *DU = Ss + XM_TM * p.pn;
  uint16_t *DTL = DU + XM_TM * p.pn;
  float *DS = reinterpret_cast<float *>(DTL + XM_TM * p.pn);  // [16][pds]
  float *Gm = DS + XM_TM * p.pds;
  xm_zero(DZ, XM_TM * p.px, tid);       // dz's k pad stays zero
  xm_zero(As, 5 * XM_TM * p.pn, tid);   // so does that of the K r wide tiles, the gate tile's among them

  for (int64_t tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int64_t row0 = tile * XM_TM;
    f32x4 acc0[XM_JT];
#pragma unroll
    for (int j = 0; j < XM_JT; ++j) acc0[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    xm_stage_saved(p, 0, row0, tid, X0);
    xm_stage(p, p.dy, row0, tid, G, nullptr);

    for (int l = p.L - 1; l >= 0; --l) {
      const XmLayer &w = p.lay[l];
      const int64_t wrow = static_cast<int64_t>(l) * p.B;
      __syncthreads();  // g of the layer above is complete; its operand tiles are stored
      xm_stage_saved(p, l, row0, tid, XL);
      __syncthreads();
      xm_experts_in(p, w, XL, As, Gm, wave, lane);
      __syncthreads();
      xm_experts_mid(p, w, As, Cs, Ss, Gm, wave, lane);
      __syncthreads();
      // z = s U^T + b: dx0 += g z, dz = bf16(g x0)
#pragma unroll
      for (int j = 0; j < XM_JT; ++j) {
        const int nt = wave + XM_WAVES * j, n = 16 * nt + col;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (16 * nt < p.d) acc = xm_tile<false>(Ss + col * p.pn, w.u + static_cast<int64_t>(n) * p.krk, p.krk >> 5, p.krk, q);
        if (n < p.d) {
          const float bias = w.b[n];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int at = (4 * q + e) * p.px + n;
            const float g = bf16_to_f32(G[at]);
            acc0[j][e] += g * (acc[e] + bias);
            DZ[at] = f32_to_bf16_rne(g * bf16_to_f32(X0[at]));
          }
        }
      }
      __syncthreads();
      // ds = dz U (fp32, to LDS)
      for (int nt = wave; 16 * nt < p.kr; nt += XM_WAVES) {
        const f32x4 acc = xm_tile<false>(DZ + col * p.px, w.uT + static_cast<int64_t>(16 * nt + col) * p.dk, p.dk >> 5, p.dk, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) DS[(4 * q + e) * p.pds + 16 * nt + col] = acc[e];
      }
      __syncthreads();
      // du = bf16(gamma ds (1 - c^2)); wave 0 also: e_i = ds_i . c_i and dlogit
      for (int idx = tid; idx < XM_TM * p.kr; idx += XM_THREADS) {
        const int row = idx & 15, n = idx >> 4, i = n / p.r;
        const float c = bf16_to_f32(Cs[row * p.pn + n]);
        const float g = p.K > 1 ? Gm[row * 4 + i] : 1.f;
        DU[row * p.pn + n] = f32_to_bf16_rne(g * DS[row * p.pds + n] * (1.f - c * c));
      }
      if (wave == 0 && p.K > 1) {
        const int row = lane & 15, i = lane >> 4;
        float ei = 0.f, gi = 0.f;
        if (i < p.K) {
          for (int j = 0; j < p.r; ++j) ei += DS[row * p.pds + i * p.r + j] * bf16_to_f32(Cs[row * p.pn + i * p.r + j]);
          gi = Gm[row * 4 + i];
        }
        float tot = gi * ei;
        tot += __shfl_xor(tot, 16);
        tot += __shfl_xor(tot, 32);
        DTL[row * p.pn + p.kr + i] = i < p.K ? f32_to_bf16_rne(gi * (ei - tot)) : 0;
      }
      __syncthreads();
      // dt = bf16((du C_i)(1 - a^2))
      for (int nt = wave; 16 * nt < p.kr; nt += XM_WAVES) {
        const int i = 16 * nt / p.r;
        const f32x4 acc =
            xm_tile<true>(DU + col * p.pn + i * p.r, w.cT + static_cast<int64_t>(16 * nt + col) * p.rk, p.rk >> 5, p.r, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int at = (4 * q + e) * p.pn + 16 * nt + col;
          const float a = bf16_to_f32(As[at]);
          DTL[at] = f32_to_bf16_rne(acc[e] * (1.f - a * a));
        }
      }
      __syncthreads();
      // dx_l = g + [dt | dlogit] [V ; gate]: the next g, or layer 0's share of dx0
#pragma unroll
      for (int j = 0; j < XM_JT; ++j) {
        const int nt = wave + XM_WAVES * j, n = 16 * nt + col;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (16 * nt < p.d) acc = xm_tile<false>(DTL + col * p.pn, w.vgT + static_cast<int64_t>(n) * p.n1k, p.n1k >> 5, p.n1k, q);
        if (n < p.d) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int at = (4 * q + e) * p.px + n;
            const float v = acc[e] + bf16_to_f32(G[at]);
            if (l > 0)
              G[at] = f32_to_bf16_rne(v);
            else
              acc0[j][e] += v;
          }
        }
      }
      xm_store_rows(p, DZ, p.px, p.dp8, row0, tid, p.w_dz + wrow * p.dp8, p.dp8);
      xm_store_rows(p, Ss, p.pn, p.kr, row0, tid, p.w_s + wrow * p.kr, p.kr);
      xm_store_rows(p, DU, p.pn, p.kr, row0, tid, p.w_du + wrow * p.kr, p.kr);
      xm_store_rows(p, As, p.pn, p.kr, row0, tid, p.w_a + wrow * p.kr, p.kr);
      xm_store_rows(p, DTL, p.pn, p.n1, row0, tid, p.w_dtl + wrow * p.n1, p.n1);
    }
#pragma unroll
    for (int j = 0; j < XM_JT; ++j) {
      const int n = 16 * (wave + XM_WAVES * j) + col;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n < p.d && row0 + 4 * q + e < p.B) p.dx0[(row0 + 4 * q + e) * p.ld_dx0 + n] = acc0[j][e];
    }
  }
}

}  // namespace mrec

using namespace mrec;

namespace {

int r8(int v) { return (v + 7) / 8 * 8; }
int r16(int v) { return (v + 15) / 16 * 16; }
int r32(int v) { return (v + 31) / 32 * 32; }

bool xm_shape_ok(int32_t d, int32_t K, int32_t r, int32_t layers) {
  return d >= 1 && d <= 512 && (r == 16 || r == 32 || r == 64) && K >= 1 && K <= 4 && K * r <= 256 && layers >= 1 &&
         layers <= MREC_CROSS_MIX_MAX_LAYERS;
}

// the derived widths; the images of a layer follow each other as [vg | vgT | u | uT | c | cT]
void xm_dims(XmArgs &p, int d, int K, int r) {
  p.d = d, p.K = K, p.r = r;
  p.dp8 = r8(d), p.dk = r32(d), p.kr = K * r, p.krk = r32(p.kr);
  p.n1 = p.kr + (K > 1 ? 16 : 0), p.n1k = r32(p.n1), p.rk = r < 32 ? 32 : r;
  p.px = p.dk + 8, p.pn = p.n1k + 8, p.pds = p.kr + 4;
}
int64_t xm_image_elems(const XmArgs &p) {
  return static_cast<int64_t>(p.n1) * p.dk + static_cast<int64_t>(r16(p.d)) * p.n1k +
         static_cast<int64_t>(r16(p.d)) * p.krk + static_cast<int64_t>(p.kr) * p.dk + 2LL * p.kr * p.rk;
}
int64_t xm_ws_row_elems(const XmArgs &p) { return p.dp8 + 3LL * p.kr + p.n1; }
size_t xm_lds_bytes(const XmArgs &p, bool bwd) {
  return bwd ? 2u * XM_TM * (4 * p.px + 5 * p.pn) + 4u * XM_TM * p.pds + 256
             : 2u * XM_TM * (2 * p.px + 2 * p.pn) + 256;
}

mrec_status xm_run(const mrec_cross_mix_args *a, bool bwd, mrec_stream stream, const char *what) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(xm_shape_ok(a->d, a->K, a->r, a->layers),
                 "unsupported shape (mrec_cross_mix_supported: 1 <= d <= 512, r in {16, 32, 64}, 1 <= K <= 4 with "
                 "K r <= 256, 1 <= layers <= 4)");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  if (a->batch == 0) return MREC_OK;
  XmArgs p{};
  xm_dims(p, a->d, a->K, a->r);
  p.B = a->batch, p.L = a->layers, p.train = a->train != 0 || bwd;
  p.tiles = (p.B + XM_TM - 1) / XM_TM;
  for (int l = 0; l < p.L; ++l) {
    MREC_CHECK_ARG(a->w_img[l] && (reinterpret_cast<uintptr_t>(a->w_img[l]) & 15) == 0 && a->bias[l],
                   "a layer's image (16-byte aligned) or bias is NULL");
    const uint16_t *w = static_cast<const uint16_t *>(a->w_img[l]);
    XmLayer &y = p.lay[l];
    y.vg = w;
    y.vgT = y.vg + static_cast<int64_t>(p.n1) * p.dk;
    y.u = y.vgT + static_cast<int64_t>(r16(p.d)) * p.n1k;
    y.uT = y.u + static_cast<int64_t>(r16(p.d)) * p.krk;
    y.c = y.uT + static_cast<int64_t>(p.kr) * p.dk;
    y.cT = y.c + static_cast<int64_t>(p.kr) * p.rk;
    y.b = a->bias[l];
  }
  if (p.train) {
    MREC_CHECK_ARG(rows16_ok(a->saved, a->ld_saved, p.dp8, MREC_BF16) && a->saved_layer_stride % 8 == 0 &&
                       a->saved_layer_stride >= (p.B - 1) * a->ld_saved + p.dp8,
                   "saved needs 16-byte aligned rows of round8(d) bf16 elements and layers that do not overlap");
    p.saved = static_cast<uint16_t *>(a->saved), p.ld_saved = a->ld_saved, p.saved_layer = a->saved_layer_stride;
  }
  if (!bwd) {
    MREC_CHECK_ARG(is_float_dtype(a->x0_dtype) && rows16_ok(a->x0, a->ld_x0, p.dp8, a->x0_dtype),
                   "x0 must be MREC_F32 or MREC_BF16 with 16-byte aligned rows of at least round8(d) elements");
    MREC_CHECK_ARG(rows16_ok(a->y, a->ld_y, p.d, MREC_BF16), "y needs 16-byte aligned rows of at least d bf16 elements");
    p.x0 = mat_in(a->x0, a->ld_x0, a->x0_dtype);
    p.y = static_cast<uint16_t *>(a->y), p.ld_y = a->ld_y;
  } else {
    MREC_CHECK_ARG(is_float_dtype(a->dy_dtype) && rows16_ok(a->dy, a->ld_dy, p.dp8, a->dy_dtype),
                   "dy must be MREC_F32 or MREC_BF16 with 16-byte aligned rows of at least round8(d) elements");
    MREC_CHECK_ARG(a->dx0 && a->ld_dx0 >= p.d, "dx0 is NULL or its rows are shorter than d");
    MREC_CHECK_ARG(a->workspace && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0 &&
                       a->workspace_bytes >= 2 * p.L * p.B * xm_ws_row_elems(p),
                   "workspace is NULL, not 16-byte aligned or smaller than mrec_cross_mix_bwd_workspace_size");
    p.dy = mat_in(a->dy, a->ld_dy, a->dy_dtype);
    p.dx0 = a->dx0, p.ld_dx0 = a->ld_dx0;
    const int64_t LB = p.L * p.B;
    p.w_dz = static_cast<uint16_t *>(a->workspace);
    p.w_s = p.w_dz + LB * p.dp8;
    p.w_du = p.w_s + LB * p.kr;
    p.w_a = p.w_du + LB * p.kr;
    p.w_dtl = p.w_a + LB * p.kr;
  }
  const size_t lds = xm_lds_bytes(p, bwd);
  const int64_t cap = (bwd ? 1LL : 2LL) * device_cus();
  const unsigned grid = static_cast<unsigned>(p.tiles < cap ? p.tiles : cap);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (bwd) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cross_mix_bwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, XM_LDS_BUDGET);
    cross_mix_bwd_kernel<<<grid, XM_THREADS, lds, s>>>(p);
  } else {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(cross_mix_fwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, XM_LDS_BUDGET);
    cross_mix_fwd_kernel<<<grid, XM_THREADS, lds, s>>>(p);
  }
  return launch_status(what);
}

}  // namespace

extern "C" {

int32_t mrec_cross_mix_supported(int32_t d, int32_t K, int32_t r, int32_t layers) {
  return xm_shape_ok(d, K, r, layers);
}

int64_t mrec_cross_mix_image_elems(int32_t d, int32_t K, int32_t r) {
  if (!xm_shape_ok(d, K, r, 1)) return 0;
  XmArgs p{};
  xm_dims(p, d, K, r);
  return xm_image_elems(p);
}

int64_t mrec_cross_mix_bwd_workspace_size(int64_t batch, int32_t d, int32_t K, int32_t r, int32_t layers) {
  if (batch <= 0 || !xm_shape_ok(d, K, r, layers)) return 0;
  XmArgs p{};
  xm_dims(p, d, K, r);
  return 2 * layers * batch * xm_ws_row_elems(p);
}

mrec_status mrec_cross_mix_fwd(const mrec_cross_mix_args *a, mrec_stream stream) {
  return xm_run(a, false, stream, "mrec_cross_mix_fwd");
}

mrec_status mrec_cross_mix_bwd(const mrec_cross_mix_args *a, mrec_stream stream) {
  return xm_run(a, true, stream, "mrec_cross_mix_bwd");
}

}  // extern "C"
