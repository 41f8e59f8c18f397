// DLRM pairwise dot interaction (mrec.h "DLRM dot interaction", ABI 38).
//
//   t_0 = bot[b], t_i = rows[b, (i-1) D : i D]                 n = F + 1 vectors of D elements
//   x[b] = [ t_0 | z[i, j] = bf16(t_i) . bf16(t_j), 0 <= j < i < n | 0 pad ]
//   G[i, j] = G[j, i] = dx[b, D + p(i, j)],  dt_i = sum_j G[i, j] bf16(t_j),  dbot = dt_0 + dx[b, :D]
//   p(i, j) = i (i - 1) / 2 + j
//
// One wave per sample, four samples per workgroup, one launch each way.  n <= 32, so the
// sample's vectors are ONE 32-row tile T (rows >= n are zeros) and both directions are
// v_mfma_f32_32x32x16_bf16 products over it.
//
//   forward   Z = T T^T.  Lane (r = lane & 31, h = lane >> 5) loads elements
//             [16 s + 8 h, + 8) of row r of K-step s straight from memory.  The A fragment
//             (A[row r][k]) and the B fragment (B[k][col r]) of T T^T are then the SAME
//             registers: acc = mfma(f[s], f[s], acc) over D / 16 steps, no LDS for the
//             operands.  The accumulator map (col = lane & 31, row = (e & 3) + 8 (e >> 2) +
//             4 h) puts row i of the triangle on consecutive lanes, so the pairs scatter
//             conflict-free into an fp32 image of the x row in LDS ([t_0 | pairs]), which the
//             wave then writes as whole 16-byte vectors, the zero pad included.
//   backward  dT = G T, one 32 x 32 tile per 32 columns of D, K = 32 (two K-steps).  The dx
//             row goes through LDS once (coalesced); a lane builds its A fragments, 8
//             consecutive entries of row r of G, by indexed reads of that image, split into
//             hi + lo bf16 when dx is fp32.  The B operand is T transposed through LDS
//             ([d][vector], 80-byte rows: one 16-byte read per fragment).
//
// Nothing is summed across waves and there are no atomics: a sample's bits depend on that
// sample's inputs alone.
#include "common.h"
#include "frag.h"

namespace mrec {

constexpr int DI_W = 4;                 // waves (samples) per workgroup
constexpr int DI_THREADS = 64 * DI_W;
constexpr int DI_MAXP = 32 * 31 / 2;    // pairs of a full tile
constexpr int DI_IMG = 128 + DI_MAXP;   // fp32 image of [t_0 | pairs]
constexpr int DI_TLD = 40;              // row pitch of the transposed T image (bf16 elements)

struct DiArgs {
  MatIn bot, rows, dx;
  MatOut x, dbot, drows;
  int64_t B, x_cols;
  int32_t n;        // vectors per sample (fields + the bottom vector)
  int32_t has_bot;  // vector 0 is bot[b]; else every vector is a row
};

// this lane's fragments of the sample's tile: elements [16 s + 8 h, + 8) of vector r
template <int D, int KS>
__device__ __forceinline__ void di_load_tile(const DiArgs &p, int64_t b, bool live, int r, int h,
                                             bf16x8 (&f)[KS]) {
  const bool on = live && r < p.n && 8 * h < D;
  const bool from_bot = p.has_bot && r == 0;
  const int c0 = from_bot ? 0 : (r - p.has_bot) * D;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (!on)
      f[s] = frag_zero8();
    else if (from_bot)
      f[s] = mat_load8(p.bot, b, 16 * s + 8 * h);
    else
      f[s] = mat_load8(p.rows, b, c0 + 16 * s + 8 * h);
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(DI_THREADS) void dot_interact_fwd_kernel(DiArgs p) {
  constexpr int KS = D <= 16 ? 1 : D / 16;
  __shared__ float img[DI_W][DI_IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * DI_W + wave;
  const bool live = b < p.B;
  const int n = p.n;
  const int Dh = p.has_bot ? D : 0;
  const int filled = Dh + n * (n - 1) / 2;
  float *im = img[wave];

  bf16x8 f[KS];
  di_load_tile<D, KS>(p, b, live, r, h, f);
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = mfma_32x32x16(f[s], f[s], acc);

  if (live) {
    if (p.has_bot)
      for (int d = lane; d < D; d += 64) im[d] = mat_elem(p.bot, b, d);
    // z[i, j], i = the register's row, j = this lane's column
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = (e & 3) + 8 * (e >> 2) + 4 * h;
      if (r < i && i < n) im[Dh + i * (i - 1) / 2 + r] = acc[e];
    }
  }
  __syncthreads();
  if (!live) return;

  // the x row as 16-byte vectors: [t_0 | pairs] from the image, zeros up to x_cols
  char *xr = p.x.p + b * p.x.ld_bytes;
  const int64_t xc = p.x_cols;
  if (p.x.bf16) {
    for (int64_t c0 = 8 * lane; c0 < xc; c0 += 8 * 64) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = c0 + k < filled ? im[c0 + k] : 0.f;
      if (c0 + 8 <= xc) {
        *reinterpret_cast<uint4 *>(xr + 2 * c0) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]),
                                                             pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (c0 + k < xc) reinterpret_cast<uint16_t *>(xr)[c0 + k] = f32_to_bf16_rne(v[k]);
      }
    }
  } else {
    for (int64_t c0 = 4 * lane; c0 < xc; c0 += 4 * 64) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = c0 + k < filled ? im[c0 + k] : 0.f;
      if (c0 + 4 <= xc) {
        *reinterpret_cast<float4 *>(xr + 4 * c0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < xc) reinterpret_cast<float *>(xr)[c0 + k] = v[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(DI_THREADS) void dot_interact_bwd_kernel(DiArgs p) {
  constexpr int KS = D <= 16 ? 1 : D / 16;
  constexpr int NCB = D <= 32 ? 1 : D / 32;  // 32-column blocks of dT
  __shared__ __attribute__((aligned(16))) uint16_t timg[DI_W][D][DI_TLD];
  __shared__ float tri[DI_W][DI_MAXP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * DI_W + wave;
  const bool live = b < p.B;
  const int n = p.n;
  const int Dh = p.has_bot ? D : 0;
  const int P = n * (n - 1) / 2;

  bf16x8 f[KS];
  di_load_tile<D, KS>(p, b, live, r, h, f);
  if (live)
    for (int q = lane; q < P; q += 64) tri[wave][q] = mat_elem(p.dx, b, Dh + q);
  // T transposed, [d][vector]; vectors >= n are zeros
  if (8 * h < D) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k) timg[wave][16 * s + 8 * h + k][r] = static_cast<uint16_t>(f[s][k]);
  }
  __syncthreads();
  if (!live) return;

  f32x16 Z[NCB];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int e = 0; e < 16; ++e) Z[cb][e] = 0.f;
  const bool split = !p.dx.bf16;  // a bf16 dx is its own hi: lo is exactly 0
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    // entries [16 s2 + 8 h, + 8) of row r of G
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = 16 * s2 + 8 * h + k;
      const int hi = r > j ? r : j, lo = r > j ? j : r;
      const bool ok = r != j && hi < n;
      const float v = tri[wave][ok ? hi * (hi - 1) / 2 + lo : 0];
      g[k] = ok ? v : 0.f;
    }
    uint32_t ch[4], cl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ch[k] = pack_bf16x2(g[2 * k], g[2 * k + 1]);
      cl[k] = pack_bf16x2(g[2 * k] - __uint_as_float(ch[k] << 16),
                          g[2 * k + 1] - __uint_as_float(ch[k] & 0xffff0000u));
    }
    const bf16x8 a_hi = __builtin_bit_cast(bf16x8, make_uint4(ch[0], ch[1], ch[2], ch[3]));
    const bf16x8 a_lo = __builtin_bit_cast(bf16x8, make_uint4(cl[0], cl[1], cl[2], cl[3]));
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int d = 32 * cb + r;
      bf16x8 bf = frag_zero8();
      if (d < D) bf = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(&timg[wave][d][16 * s2 + 8 * h]));
      // (the builtin, not mfma_32x32x16: through the wrapper the compiler orders this loop,
      // with its conditional second product, differently)
      Z[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_hi, bf, Z[cb], 0, 0, 0);
      if (split) Z[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_lo, bf, Z[cb], 0, 0, 0);
    }
  }

  // dT[i][d]: i = the register's row, d = this lane's column (consecutive lanes, consecutive d)
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
    const int d = 32 * cb + r;
    if (d >= D) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = (e & 3) + 8 * (e >> 2) + 4 * h;
      if (i >= n) continue;
      if (p.has_bot && i == 0)
        mat_store(p.dbot, b, d, Z[cb][e] + mat_elem(p.dx, b, d));
      else
        mat_store(p.drows, b, (i - p.has_bot) * D + d, Z[cb][e]);
    }
  }
}

}  // namespace mrec

using namespace mrec;

namespace {

bool di_dim_ok(int32_t D) { return D == 8 || D == 16 || D == 32 || D == 64 || D == 128; }

mrec_status di_check(const mrec_dot_interact_args *a, bool bwd, DiArgs &p) {
  MREC_CHECK_ARG(a, "NULL arguments");
  MREC_CHECK_ARG(is_float_dtype(a->bot_dtype) && is_float_dtype(a->rows_dtype) &&
                     is_float_dtype(a->x_dtype) && is_float_dtype(a->dx_dtype),
                 "unknown dtype: bot, rows, x and dx must each be MREC_F32 or MREC_BF16");
  MREC_CHECK_ARG(mrec_dot_interact_supported(a->D, a->n_fields, a->bot_dtype, a->rows_dtype, a->x_dtype, a->dx_dtype),
                 "unsupported shape (mrec_dot_interact_supported: D in {8, 16, 32, 64, 128}, 1 <= n_fields <= 31)");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  const int has_bot = a->bot != nullptr;
  const int n = a->n_fields + has_bot;
  const int64_t Dh = has_bot ? a->D : 0, P = static_cast<int64_t>(n) * (n - 1) / 2;
  if (!bwd) MREC_CHECK_ARG(a->x_cols >= Dh + P, "x_cols smaller than D + P (the bottom vector and the pairs)");
  if (a->batch > 0) {
    MREC_CHECK_ARG(!has_bot || rows16_ok(a->bot, a->ld_bot, a->D, a->bot_dtype),
                   "bot needs 16-byte aligned rows of at least D elements");
    MREC_CHECK_ARG(rows16_ok(a->rows, a->ld_rows, static_cast<int64_t>(a->n_fields) * a->D, a->rows_dtype),
                   "rows needs 16-byte aligned rows of at least n_fields * D elements");
    if (!bwd) {
      MREC_CHECK_ARG(rows16_ok(a->x, a->ld_x, a->x_cols, a->x_dtype),
                     "x needs 16-byte aligned rows of at least x_cols elements");
    } else {
      MREC_CHECK_ARG(rows16_ok(a->dx, a->ld_dx, Dh + P, a->dx_dtype),
                     "dx needs 16-byte aligned rows of at least D + P elements");
      MREC_CHECK_ARG(!has_bot || rows16_ok(a->dbot, a->ld_dbot, a->D, a->bot_dtype),
                     "dbot needs 16-byte aligned rows of at least D elements");
      MREC_CHECK_ARG(rows16_ok(a->drows, a->ld_drows, static_cast<int64_t>(a->n_fields) * a->D, a->rows_dtype),
                     "drows needs 16-byte aligned rows of at least n_fields * D elements");
    }
  }
  p.bot = mat_in(a->bot, a->ld_bot, a->bot_dtype);
  p.rows = mat_in(a->rows, a->ld_rows, a->rows_dtype);
  p.dx = mat_in(a->dx, a->ld_dx, a->dx_dtype);
  p.x = mat_out(a->x, a->ld_x, a->x_dtype);
  p.dbot = mat_out(a->dbot, a->ld_dbot, a->bot_dtype);
  p.drows = mat_out(a->drows, a->ld_drows, a->rows_dtype);
  p.B = a->batch;
  p.x_cols = a->x_cols;
  p.n = n;
  p.has_bot = has_bot;
  return MREC_OK;
}

template <int D>
void di_launch(const DiArgs &p, bool bwd, unsigned grid, hipStream_t s) {
  if (bwd)
    dot_interact_bwd_kernel<D><<<grid, DI_THREADS, 0, s>>>(p);
  else
    dot_interact_fwd_kernel<D><<<grid, DI_THREADS, 0, s>>>(p);
}

mrec_status di_run(const mrec_dot_interact_args *a, bool bwd, mrec_stream stream, const char *what) {
  DiArgs p{};
  const mrec_status st = di_check(a, bwd, p);
  if (st != MREC_OK) return st;
  if (a->batch == 0) return MREC_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>((a->batch + DI_W - 1) / DI_W);
  switch (a->D) {
    case 8: di_launch<8>(p, bwd, grid, s); break;
    case 16: di_launch<16>(p, bwd, grid, s); break;
    case 32: di_launch<32>(p, bwd, grid, s); break;
    case 64: di_launch<64>(p, bwd, grid, s); break;
    default: di_launch<128>(p, bwd, grid, s); break;
  }
  return launch_status(what);
}

}  // namespace

extern "C" {

int32_t mrec_dot_interact_supported(int32_t D, int32_t n_fields, mrec_dtype bot_dtype, mrec_dtype rows_dtype,
                                    mrec_dtype x_dtype, mrec_dtype dx_dtype) {
  return di_dim_ok(D) && n_fields >= 1 && n_fields <= 31 && is_float_dtype(bot_dtype) &&
         is_float_dtype(rows_dtype) && is_float_dtype(x_dtype) && is_float_dtype(dx_dtype);
}

mrec_status mrec_dot_interact_fwd(const mrec_dot_interact_args *a, mrec_stream stream) {
  return di_run(a, false, stream, "mrec_dot_interact_fwd");
}

mrec_status mrec_dot_interact_bwd(const mrec_dot_interact_args *a, mrec_stream stream) {
  return di_run(a, true, stream, "mrec_dot_interact_bwd");
}

}  // extern "C"
