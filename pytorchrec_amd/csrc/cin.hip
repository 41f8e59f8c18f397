// xDeepFM's Compressed Interaction Network, one layer per call (mrec.h "CIN", ABI 39).
//
//   X^k[b, h, d] = sum_{i < H_prev} sum_{j < m} W[h, i, j] X^{k-1}[b, i, d] X^0[b, j, d]
//   p[b, h]      = sum_d X^k[b, h, d]
//
// A GEMM whose A operand Z[(b, d), (i, j)] = X^{k-1}[b, i, d] X^0[b, j, d] never exists in
// memory.  Rows are the flattened (b, d), k is (i, j) with j padded to the field pitch MP (16
// for m <= 16, else 32: the zero columns of the weight images cover the pad), columns are h.
// Every product is v_mfma_f32_32x32x16_bf16: lane (r = lane & 31, hh = lane >> 5) holds
// A[row r][k = 8 hh + e], B[k = 8 hh + e][col r], and C[row (e & 3) + 8 (e >> 2) + 4 hh][col r].
//
//   forward   a wave owns 64 rows (two row tiles) and all H columns.  A lane keeps its rows'
//             X^0 values for its 8 j per 16-wide K-step in registers for the whole K loop and
//             forms its A fragment as bf16(X^{k-1}[b, i, d] * X^0[b, j, d]), one scalar of
//             X^{k-1} per i.  The B fragment is 16 bytes of the weight image [h][(i, j)].
//             64 rows hold 64 / D whole samples, so p is summed from the fp32 accumulators
//             in registers and one cross-half shuffle.
//   data      dZ^T = W^T dX^k^T: rows (i, j), columns the wave's 64 data rows, K = h.  The
//   gradient  wave's dX^k tile is built once as B fragments; the A fragment is 16 bytes of the
//             transposed image [(i, j)][h].  A 32-row tile of dZ^T is one i (MP = 32) or two
//             (MP = 16) with j on the registers, so it contracts at once with the lane's X^0
//             values into dX^{k-1} (one shuffle) and, scaled by X^{k-1}, into the lane's
//             fp32 dX^0 registers, added to the dX^0 accumulator at the end: each element is
//             owned by one lane of one workgroup.
//   weight    dW = (dX^k)^T Z: rows h, columns (i, j), K = all B D data rows.  A workgroup owns
//   gradient  a 64 x 64 output tile and walks the whole batch, its four waves taking every
//             fourth K-step; their partial tiles are added in wave order through LDS (48 KB):
//             no partials in memory, no atomics.  Both fragments are 16-byte loads along d;
//             Z is re-formed as in the forward.
//
// Nothing is summed across waves except through that fixed order, so a sample's X^k, p,
// dX^{k-1} and dX^0 depend on that sample alone and dW has the same bits every run.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int CIN_THREADS = 256;     // forward and data gradient: 4 waves of 64 rows
constexpr int CIN_WG_ROWS = 256;
constexpr int CIN_DW_WAVES = 4;      // weight gradient: four waves share one 64 x 64 tile's K-steps
constexpr int CIN_DW_THREADS = 64 * CIN_DW_WAVES;

struct CinArgs {
  MatIn x0, xp, dxk;
  MatOut xk, dxp;
  const uint16_t *wf, *wb;
  int64_t ld_wf, ld_wb;
  float *p;
  const float *dp, *dpp;
  float *dx0, *dw;
  int64_t ld_p, ld_dp, ld_dpp, ld_dx0;
  int64_t B;
  int32_t m, D, dshift, Hp, H;
  int32_t nt0;  // forward: the launch's first 32-column tile of h
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int NT, int NJ>
__global__ __launch_bounds__(CIN_THREADS) void cin_fwd_kernel(CinArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int D = p.D, sh = p.dshift, m = p.m;
  const int64_t rows = p.B << sh;
  const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * 4 + wave) * 64;
  if (row0 >= rows) return;  // (whole wave; nothing below synchronises the workgroup)

  int64_t b[2];
  int d[2];
  bool live[2];
  float x0f[2][NJ][8];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t R = row0 + 32 * rt + r;
    live[rt] = R < rows;
    b[rt] = R >> sh;
    d[rt] = static_cast<int>(R & (D - 1));
#pragma unroll
    for (int s = 0; s < NJ; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = 16 * s + 8 * hh + e;
        x0f[rt][s][e] = (live[rt] && j < m) ? mat_elem_bf16(p.x0, b[rt], j * D + d[rt]) : 0.f;
      }
  }

  f32x16 acc[2][NT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[rt][nt][e] = 0.f;

  const uint16_t *wl = p.wf + static_cast<int64_t>(32 * p.nt0 + r) * p.ld_wf + 8 * hh;
  const int64_t wtile = 32 * p.ld_wf;
#pragma unroll 1
  for (int i = 0; i < p.Hp; ++i) {
    float xs[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) xs[rt] = live[rt] ? mat_elem_bf16(p.xp, b[rt], i * D + d[rt]) : 0.f;
#pragma unroll
    for (int s = 0; s < NJ; ++s) {
      const uint16_t *wk = wl + 16 * (i * NJ + s);
      bf16x8 a[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        float z[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = xs[rt] * x0f[rt][s][e];
        a[rt] = frag_pack8(z);
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf16x8 bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wk + nt * wtile));
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) acc[rt][nt] = mfma_32x32x16(a[rt], bf, acc[rt][nt]);
      }
    }
  }

  // X^k[b, h, d]: register group q of row tile rt holds rows 32 rt + 8 q + 4 hh + (0 .. 3),
  // four consecutive d of one sample; column h = 32 nt + r
  const int64_t s0 = row0 >> sh;  // first sample of the wave (row0 is a multiple of 64 >= D)
  const int ns = 64 >> sh;        // whole samples per wave
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int h = 32 * (p.nt0 + nt) + r;
    float g[8];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x16 &c = acc[rt][nt];
        const int64_t R = row0 + 32 * rt + 8 * q + 4 * hh;
        if (h < p.H && R < rows) {
          char *dst = p.xk.p + (R >> sh) * p.xk.ld_bytes;
          const int64_t col = static_cast<int64_t>(h) * D + (R & (D - 1));
          if (p.xk.bf16)
            *reinterpret_cast<uint2 *>(dst + 2 * col) =
                make_uint2(pack_bf16x2(c[4 * q], c[4 * q + 1]), pack_bf16x2(c[4 * q + 2], c[4 * q + 3]));
          else
            *reinterpret_cast<float4 *>(dst + 4 * col) = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        }
        const float part = (c[4 * q] + c[4 * q + 1]) + (c[4 * q + 2] + c[4 * q + 3]);
        g[4 * rt + q] = part + __shfl_xor(part, 32);  // the 8 rows 32 rt + 8 q .. + 7
      }
    // sums over D rows: D / 8 consecutive groups, a fixed tree
    if (D >= 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) g[q] = g[2 * q] + g[2 * q + 1];
    }
    if (D >= 32) {
#pragma unroll
      for (int q = 0; q < 2; ++q) g[q] = g[2 * q] + g[2 * q + 1];
    }
    if (D >= 64) g[0] = g[0] + g[1];
    if (hh == 0 && h < p.H) {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < ns && s0 + q < p.B) p.p[(s0 + q) * p.ld_p + h] = g[q];
    }
  }
}

// ---------------------------------------------------------------------------
// backward: the data gradient
// ---------------------------------------------------------------------------
template <int KS, int NJ>
__global__ __launch_bounds__(CIN_THREADS) void cin_dgrad_kernel(CinArgs p) {
  constexpr int NI = 2 / NJ;   // i per 32-row tile of (i, j)
  constexpr int NQ = 8 * NJ;   // the lane's j per i: j = (q & 3) + 8 (q >> 2) + 4 hh
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int D = p.D, sh = p.dshift, m = p.m;
  const int64_t rows = p.B << sh;
  const int64_t row0 = (static_cast<int64_t>(blockIdx.x) * 4 + wave) * 64;
  if (row0 >= rows) return;

  int64_t b[2];
  int d[2];
  bool live[2];
  float x0f[2][NQ], dx0a[2][NQ];
  bf16x8 gf[2][KS];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t R = row0 + 32 * rt + r;
    live[rt] = R < rows;
    b[rt] = live[rt] ? R >> sh : p.B - 1;  // (a dead lane loads a valid row and drops it)
    d[rt] = static_cast<int>(R & (D - 1));
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = (q & 3) + 8 * (q >> 2) + 4 * hh;
      const float v = mat_elem_bf16(p.x0, b[rt], min(j, m - 1) * D + d[rt]);
      x0f[rt][q] = (live[rt] && j < m) ? v : 0.f;
      dx0a[rt][q] = 0.f;
    }
    // dX^k for h = 16 t + 8 hh + e: a group of 8 h is whole or absent (H is a multiple of 8).
    // The pointer walks in a vector register so that the unrolled loads share 8 offsets.
    const char *g0 = p.dxk.p ? p.dxk.p + b[rt] * p.dxk.ld_bytes + (p.dxk.bf16 ? 2 : 4) * d[rt]
                             : reinterpret_cast<const char *>(p.dp + b[rt] * p.ld_dp);
    const int64_t ghalf = p.dxk.p ? (p.dxk.bf16 ? 2 : 4) * 8 * D : 4 * 8;
    const int64_t gstep = p.dxk.p ? (p.dxk.bf16 ? 2 : 4) * 16 * D : 4 * 16;
    const int estep = p.dxk.p ? D : 1;
    const bool g16 = p.dxk.p && p.dxk.bf16;
    const char *gp = g0 + hh * ghalf;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      float v[8];
      const bool ok = live[rt] && 16 * t + 8 * hh < p.H;
      const char *gs = ok ? gp : g0;  // (an absent group reads group 0 and is masked to zero)
      uint32_t okm = ok ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(gs), "+v"(okm));
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = g16 ? bf16_to_f32(reinterpret_cast<const uint16_t *>(gs)[e * estep])
                            : bf16_to_f32(f32_to_bf16_rne(reinterpret_cast<const float *>(gs)[e * estep]));
        v[e] = g;
      }
      gp += gstep;
      const uint4 w = __builtin_bit_cast(uint4, frag_pack8(v));  // (exact: the values are bf16 already)
      gf[rt][t] = __builtin_bit_cast(bf16x8, make_uint4(w.x & okm, w.y & okm, w.z & okm, w.w & okm));
    }
  }

  const uint16_t *wl = p.wb + static_cast<int64_t>(r) * p.ld_wb + 8 * hh;
  const int64_t wtile = 32 * p.ld_wb;
  const int ntiles = (p.Hp * 16 * NJ + 31) / 32;
  for (int mt = 0; mt < ntiles; ++mt) {
    f32x16 acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[rt][e] = 0.f;
    const uint16_t *wk = wl + mt * wtile;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(wk + 16 * t));
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) acc[rt] = mfma_32x32x16(a, gf[rt][t], acc[rt]);
    }
#pragma unroll
    for (int u = 0; u < NI; ++u) {
      const int i = mt * NI + u;
      if (i >= p.Hp) continue;  // (uniform: the zero rows that pad the last tile)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const float xpf = live[rt] ? mat_elem_bf16(p.xp, b[rt], i * D + d[rt]) : 0.f;
        float part = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float dz = acc[rt][u * NQ + q];
          part += dz * x0f[rt][q];
          dx0a[rt][q] += dz * xpf;
        }
        const float tot = part + __shfl_xor(part, 32);
        if (hh == 0 && live[rt])
          mat_store(p.dxp, b[rt], i * D + d[rt], tot + (p.dpp ? p.dpp[b[rt] * p.ld_dpp + i] : 0.f));
      }
    }
  }

#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = (q & 3) + 8 * (q >> 2) + 4 * hh;
      if (live[rt] && j < m) p.dx0[b[rt] * p.ld_dx0 + j * D + d[rt]] += dx0a[rt][q];
    }
}

// ---------------------------------------------------------------------------
// backward: the weight gradient
// ---------------------------------------------------------------------------
// 8 consecutive elements as a fragment; BF: the operand is known to be bf16 (no dtype branch
// between the loads of the unrolled K-steps)
template <bool BF>
__device__ __forceinline__ bf16x8 cin_load8(const MatIn &m, int64_t row, int col0) {
  if constexpr (BF)
    return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(m.p + row * m.ld_bytes + 2 * col0));
  else
    return mat_load8(m, row, col0);
}

// MODE 0: any dtypes.  1: x0, xp and dxk are bf16.  2: x0 and xp are bf16, dX^k is dp (no dxk).
template <int NJ, int MODE>
__global__ __launch_bounds__(CIN_DW_THREADS) void cin_wgrad_kernel(CinArgs p, int n_pairs) {
  constexpr bool BF = MODE != 0;
  constexpr int MP = 16 * NJ;
  __shared__ float red[CIN_DW_WAVES - 1][64][64];  // [wave][accumulator register][lane]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int D = p.D, sh = p.dshift;
  const int hp = blockIdx.x / n_pairs, np = blockIdx.x % n_pairs;
  const int64_t rows = p.B << sh;

  // this lane's output row h of each h tile (the A side) and column (i, j) of each n tile;
  // a lane outside the tile loads a valid element and masks it to zero
  int hrow[2], ci[2], cj[2];
  uint32_t hmask[2], cmask[2];
  bool cok[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int h = 64 * hp + 32 * u + r;
    hmask[u] = h < p.H ? 0xffffffffu : 0u;
    hrow[u] = min(h, p.H - 1);
    const int n = 64 * np + 32 * u + r;
    cok[u] = n / MP < p.Hp && n % MP < p.m;
    cmask[u] = cok[u] ? 0xffffffffu : 0u;
    ci[u] = min(n / MP, p.Hp - 1);
    cj[u] = min(n % MP, p.m - 1);
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[u][v][e] = 0.f;

  // wave w takes the K-steps w, w + 4, ...: 16 data rows each, this lane's 8 being one
  // sample's d0 .. d0 + 7
  const int64_t steps = (rows + 15) / 16;
  // (four steps per trip, so that their loads are in flight together; a step past the end
  // is masked like a row past the batch)
  for (int64_t t0 = wave; t0 < steps; t0 += 4 * CIN_DW_WAVES) {
    uint32_t on[4];
    uint4 g[4][2];
    bf16x8 xa[4][2], xb[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // every load of the trip first
      const int64_t R0 = 16 * (t0 + q * CIN_DW_WAVES) + 8 * hh;
      on[q] = R0 < rows ? 0xffffffffu : 0u;
      const int64_t R = R0 < rows ? R0 : rows - 8;
      const int64_t b = R >> sh;
      const int d0 = static_cast<int>(R & (D - 1));
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (MODE == 1 || (MODE == 0 && p.dxk.p)) {  // (uniform)
          g[q][u] = __builtin_bit_cast(uint4, cin_load8<BF>(p.dxk, b, hrow[u] * D + d0));
        } else {
          const uint32_t g1 = f32_to_bf16_rne(p.dp[b * p.ld_dp + hrow[u]]);
          const uint32_t g2 = g1 | (g1 << 16);
          g[q][u] = make_uint4(g2, g2, g2, g2);
        }
        xa[q][u] = cin_load8<BF>(p.xp, b, ci[u] * D + d0);
        xb[q][u] = cin_load8<BF>(p.x0, b, cj[u] * D + d0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bf16x8 a[2], z[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t ma = on[q] & hmask[u];
        a[u] = __builtin_bit_cast(bf16x8, make_uint4(g[q][u].x & ma, g[q][u].y & ma, g[q][u].z & ma, g[q][u].w & ma));
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          f[e] = bf16_to_f32(static_cast<uint16_t>(xa[q][u][e])) * bf16_to_f32(static_cast<uint16_t>(xb[q][u][e]));
        const uint4 zz = __builtin_bit_cast(uint4, frag_pack8(f));
        const uint32_t mz = on[q] & cmask[u];
        z[u] = __builtin_bit_cast(bf16x8, make_uint4(zz.x & mz, zz.y & mz, zz.z & mz, zz.w & mz));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mfma_32x32x16(a[u], z[v], acc[u][v]);
    }
  }

  // the four partial tiles are added in wave order: the same bits every run
  if (wave > 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int e = 0; e < 16; ++e) red[wave - 1][(2 * u + v) * 16 + e][lane] = acc[u][v][e];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      if (!cok[v]) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float s = acc[u][v][e];
#pragma unroll
        for (int w = 0; w < CIN_DW_WAVES - 1; ++w) s += red[w][(2 * u + v) * 16 + e][lane];
        const int h = 64 * hp + 32 * u + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (h < p.H) p.dw[(static_cast<int64_t>(h) * p.Hp + ci[v]) * p.m + cj[v]] = s;
      }
    }
}

}  // namespace mrec

using namespace mrec;

namespace {

int cin_pitch(int32_t m) { return m <= 16 ? 16 : 32; }
int cin_ks(int32_t H) {
  const int need = (H + 15) / 16;
  for (int ks : {1, 2, 4, 8, 13, 16})
    if (ks >= need) return ks;
  return 16;
}
bool cin_shape_ok(int32_t m, int32_t D, int32_t Hp, int32_t H) {
  return m >= 2 && m <= 32 && (D == 8 || D == 16 || D == 32 || D == 64) && H >= 8 && H <= 256 && H % 8 == 0 &&
         (Hp == m || (Hp >= 8 && Hp <= 256 && Hp % 8 == 0));
}

mrec_status cin_check(const mrec_cin_args *a, bool bwd, CinArgs &p) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(is_float_dtype(a->x0_dtype) && is_float_dtype(a->x_dtype),
                 "unknown dtype: x0_dtype and x_dtype must each be MREC_F32 or MREC_BF16");
  MREC_CHECK_ARG(cin_shape_ok(a->n_fields, a->D, a->H_prev, a->H),
                 "unsupported shape (mrec_cin_supported: 2 <= n_fields <= 32, D in {8, 16, 32, 64}, H and H_prev "
                 "multiples of 8 up to 256, or H_prev = n_fields)");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  const int MP = cin_pitch(a->n_fields);
  const int64_t w0 = static_cast<int64_t>(a->n_fields) * a->D, wp = static_cast<int64_t>(a->H_prev) * a->D,
                wk = static_cast<int64_t>(a->H) * a->D;
  if (a->batch > 0) {
    MREC_CHECK_ARG(rows16_ok(a->x0, a->ld_x0, w0, a->x0_dtype),
                   "x0 needs 16-byte aligned rows of at least n_fields * D elements");
    MREC_CHECK_ARG(rows16_ok(a->xp, a->ld_xp, wp, a->xp_dtype) && is_float_dtype(a->xp_dtype),
                   "xp needs 16-byte aligned rows of at least H_prev * D elements, MREC_F32 or MREC_BF16");
    if (!bwd) {
      MREC_CHECK_ARG(rows16_ok(a->w_fwd, a->ld_w_fwd, static_cast<int64_t>(a->H_prev) * MP, MREC_BF16),
                     "w_fwd needs 16-byte aligned rows of at least H_prev * mrec_cin_field_pitch elements");
      MREC_CHECK_ARG(rows16_ok(a->xk, a->ld_xk, wk, a->x_dtype),
                     "xk needs 16-byte aligned rows of at least H * D elements");
      MREC_CHECK_ARG(a->p && a->ld_p >= a->H, "p needs rows of at least H elements");
    } else {
      MREC_CHECK_ARG(rows16_ok(a->w_bwd, a->ld_w_bwd, 16 * cin_ks(a->H), MREC_BF16),
                     "w_bwd needs 16-byte aligned rows of at least mrec_cin_bwd_cols elements");
      if (a->dxk)
        MREC_CHECK_ARG(rows16_ok(a->dxk, a->ld_dxk, wk, a->x_dtype),
                       "dxk needs 16-byte aligned rows of at least H * D elements");
      else
        MREC_CHECK_ARG(a->dp && a->ld_dp >= a->H, "without dxk, dp needs rows of at least H elements");
      MREC_CHECK_ARG(!a->dp_prev || a->ld_dp_prev >= a->H_prev, "dp_prev needs rows of at least H_prev elements");
      MREC_CHECK_ARG(rows16_ok(a->dxp, a->ld_dxp, wp, a->dxp_dtype) && is_float_dtype(a->dxp_dtype),
                     "dxp needs 16-byte aligned rows of at least H_prev * D elements, MREC_F32 or MREC_BF16");
      MREC_CHECK_ARG(a->dx0 && a->ld_dx0 >= w0, "dx0 needs rows of at least n_fields * D elements");
      MREC_CHECK_ARG(a->dw, "dw is NULL");
    }
  }
  p.x0 = mat_in(a->x0, a->ld_x0, a->x0_dtype);
  p.xp = mat_in(a->xp, a->ld_xp, a->xp_dtype);
  p.dxk = mat_in(a->dxk, a->ld_dxk, a->x_dtype);
  p.xk = mat_out(a->xk, a->ld_xk, a->x_dtype);
  p.dxp = mat_out(a->dxp, a->ld_dxp, a->dxp_dtype);
  p.wf = static_cast<const uint16_t *>(a->w_fwd);
  p.wb = static_cast<const uint16_t *>(a->w_bwd);
  p.ld_wf = a->ld_w_fwd;
  p.ld_wb = a->ld_w_bwd;
  p.p = a->p;
  p.dp = a->dp;
  p.dpp = a->dp_prev;
  p.dx0 = a->dx0;
  p.dw = a->dw;
  p.ld_p = a->ld_p;
  p.ld_dp = a->ld_dp;
  p.ld_dpp = a->ld_dp_prev;
  p.ld_dx0 = a->ld_dx0;
  p.B = a->batch;
  p.m = a->n_fields;
  p.D = a->D;
  p.dshift = a->D == 8 ? 3 : a->D == 16 ? 4 : a->D == 32 ? 5 : 6;
  p.Hp = a->H_prev;
  p.H = a->H;
  return MREC_OK;
}

template <int NT>
void cin_fwd_launch(const CinArgs &p, unsigned grid, hipStream_t s) {
  if (p.m <= 16)
    cin_fwd_kernel<NT, 1><<<grid, CIN_THREADS, 0, s>>>(p);
  else
    cin_fwd_kernel<NT, 2><<<grid, CIN_THREADS, 0, s>>>(p);
}

template <int KS>
void cin_dgrad_launch(const CinArgs &p, unsigned grid, hipStream_t s) {
  if (p.m <= 16)
    cin_dgrad_kernel<KS, 1><<<grid, CIN_THREADS, 0, s>>>(p);
  else
    cin_dgrad_kernel<KS, 2><<<grid, CIN_THREADS, 0, s>>>(p);
}

template <int NJ>
void cin_wgrad_launch(const CinArgs &p, int mode, int n_pairs, unsigned tiles, hipStream_t s) {
  if (mode == 1)
    cin_wgrad_kernel<NJ, 1><<<tiles, CIN_DW_THREADS, 0, s>>>(p, n_pairs);
  else if (mode == 2)
    cin_wgrad_kernel<NJ, 2><<<tiles, CIN_DW_THREADS, 0, s>>>(p, n_pairs);
  else
    cin_wgrad_kernel<NJ, 0><<<tiles, CIN_DW_THREADS, 0, s>>>(p, n_pairs);
}

}  // namespace

extern "C" {

int32_t mrec_cin_supported(int32_t n_fields, int32_t D, int32_t H_prev, int32_t H, mrec_dtype x0_dtype,
                           mrec_dtype x_dtype) {
  return cin_shape_ok(n_fields, D, H_prev, H) && is_float_dtype(x0_dtype) && is_float_dtype(x_dtype);
}

int32_t mrec_cin_field_pitch(int32_t n_fields) { return cin_pitch(n_fields); }
int32_t mrec_cin_fwd_rows(int32_t H) { return (H + 31) / 32 * 32; }
int32_t mrec_cin_bwd_cols(int32_t H) { return 16 * cin_ks(H); }

mrec_status mrec_cin_fwd(const mrec_cin_args *a, mrec_stream stream) {
  CinArgs p{};
  const mrec_status st = cin_check(a, false, p);
  if (st != MREC_OK) return st;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(((p.B << p.dshift) + CIN_WG_ROWS - 1) / CIN_WG_ROWS);
  switch ((p.H + 31) / 32) {
    case 1: cin_fwd_launch<1>(p, grid, s); break;
    case 2: cin_fwd_launch<2>(p, grid, s); break;
    case 3: cin_fwd_launch<3>(p, grid, s); break;
    case 4: cin_fwd_launch<4>(p, grid, s); break;
    case 5: cin_fwd_launch<5>(p, grid, s); break;
    case 6: cin_fwd_launch<6>(p, grid, s); break;
    case 7: cin_fwd_launch<7>(p, grid, s); break;
    default:  // 8 column tiles are two launches of 4: 256 accumulator registers leave too few
      cin_fwd_launch<4>(p, grid, s);
      p.nt0 = 4;
      cin_fwd_launch<4>(p, grid, s);
      break;
  }
  return launch_status("mrec_cin_fwd");
}

mrec_status mrec_cin_bwd(const mrec_cin_args *a, mrec_stream stream) {
  CinArgs p{};
  const mrec_status st = cin_check(a, true, p);
  if (st != MREC_OK) return st;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(((p.B << p.dshift) + CIN_WG_ROWS - 1) / CIN_WG_ROWS);
  switch (cin_ks(p.H)) {
    case 1: cin_dgrad_launch<1>(p, grid, s); break;
    case 2: cin_dgrad_launch<2>(p, grid, s); break;
    case 4: cin_dgrad_launch<4>(p, grid, s); break;
    case 8: cin_dgrad_launch<8>(p, grid, s); break;
    case 13: cin_dgrad_launch<13>(p, grid, s); break;
    default: cin_dgrad_launch<16>(p, grid, s); break;
  }
  const int MP = cin_pitch(p.m);
  const int h_pairs = (p.H + 63) / 64, n_pairs = (p.Hp * MP + 63) / 64;
  const bool bf = p.x0.bf16 && p.xp.bf16 && (!p.dxk.p || p.dxk.bf16);
  const int mode = !bf ? 0 : p.dxk.p ? 1 : 2;
  const unsigned tiles = static_cast<unsigned>(h_pairs * n_pairs);
  if (p.m <= 16)
    cin_wgrad_launch<1>(p, mode, n_pairs, tiles, s);
  else
    cin_wgrad_launch<2>(p, mode, n_pairs, tiles, s);
  return launch_status("mrec_cin_bwd");
}

}  // extern "C"
