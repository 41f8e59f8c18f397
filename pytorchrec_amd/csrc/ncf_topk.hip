// Full-catalogue top-K retrieval for NCF / NeuMF: every item of [low, high) scored for a
// batch of users with the pair scorer of ncf.hip, fused with the selection of the k best per
// user (mrec.h "NCF retrieval", ABI 36).  No per-pair row and no [B, items] score reaches
// memory.
//
//   a[b, n] = b_0[n] + sum_e W_0[n, e]     mlp_u[u, e]       fp32, once per user
//   c[i, n] =          sum_e W_0[n, E + e] mlp_i[i, e]       fp32, once per item of a tile
//   h_1     = relu(a[b] + c[i])
//   h_{l+1} = relu(W_l h_l + b_l)          l = 1 .. nl - 1   (nc_mlp, ncf_common.h)
//   score   = sum_e wp[e] (mf_u[u, e] mf_i[i, e]) + wp[E:] . h_nl
//
// Layer 0 is the scorer's largest and splits into a user half and an item half: the grid
// is user tiles x item splits, a workgroup of eight waves carries NT_TU = 16 users for the
// whole launch (their a rows and mf_u rows stay in LDS) and streams its split of the item
// tables NT_TI = 64 items at a time.  Per tile: the items' mlp_i rows go to the H arena as
// bf16 and one MFMA layer against the item half of W_0 (staged like any other layer's
// image) leaves c [64, N_0] in LDS as fp32.  Then one pass per carried user over the
// tile's 64 (user, item) pairs, the pair tile of ncf.hip: h_1 is formed on the VALU (add,
// max, one rounding to bf16 where it becomes an MFMA operand), layers 1 .. nl - 1 are
// nc_mlp as it stands -- with the tile's four row blocks dealt to two groups of four waves,
// two each, so that two waves share a SIMD and hide each other's LDS and MFMA latency --
// the MF term is ncf.hip's, and lane (16 wave + a) of the first group holds the score of
// item 16 wave + a of the tile, which it offers to the user's key buffer (topk_select.h).
// A pair's score bits depend on nothing but the pair.
//
// LDS: [W images | H arena] bf16, then fp32 [biases | wp | the MLP dots | a | c | mf_u],
// then the selection state [keys | thresholds | exclusion bounds | counts | user rows |
// the reduction vote]; the kernel has no static LDS, so the plan is the whole budget;
// the plan is computed on the host and travels in the argument block.
#include "common.h"
#include "ncf_common.h"
#include "topk_select.h"

namespace mrec {

constexpr int NT_TU = 16;       // users a workgroup carries
constexpr int NT_TI = NC_TILE;  // items per streamed tile: one pass of pairs per user
constexpr int NT_THREADS = 512;  // eight waves: each half of a pair tile has its own four

struct NcfTopkArgs {
  NcfArgs m;           // the layers (layer 0: the item half of W_0, K = E) and their LDS plan
  const char *tab[4];  // row 0 of the mf_u, mf_i, mlp_u, mlp_i tables
  int64_t row_bytes;
  int64_t n_users;
  int32_t low, high;
  const void *uid;
  int32_t uid64;
  const float *w0;  // W_0's master: the user half is read from it, once per workgroup
  int64_t ld_w0;
  int32_t *oob;
  const int64_t *ex_off;
  const int32_t *ex_items;
  int64_t ex_rows;
  const void *ex_row;
  int32_t ex_row64;
  int32_t cap, lim, P;  // key buffer capacity, reduction trigger, pow2 >= cap
  int32_t tiles_per_split;
  int32_t aoff, lda_a, coff, ldc, muoff;  // fp32 element offsets from m.fbase
  int32_t kbase, bytes;                   // the selection state's byte offset; all of it
  TkOut o;
};

template <typename T>
__global__ __launch_bounds__(NT_THREADS) void ncf_topk_kernel(NcfTopkArgs p) {
  extern __shared__ __attribute__((aligned(16))) char nt_lds[];
  const NcfArgs &m = p.m;
  uint16_t *sm = reinterpret_cast<uint16_t *>(nt_lds);
  float *sf = reinterpret_cast<float *>(nt_lds + m.fbase);
  unsigned long long *buf = reinterpret_cast<unsigned long long *>(nt_lds + p.kbase);  // [NT_TU][cap]
  unsigned long long *thr = buf + NT_TU * p.cap;                                       // [NT_TU]
  int64_t *exlo = reinterpret_cast<int64_t *>(thr + NT_TU), *exhi = exlo + NT_TU;
  int *cnt = reinterpret_cast<int *>(exhi + NT_TU);  // [NT_TU]
  int *urow = cnt + NT_TU;                           // the user's table row, -1: no such user
  int *due = urow + NT_TU;                           // a count passed lim in this tile
  const int tid = threadIdx.x, lane = tid & 63;
  // waves 0 .. 3 take row blocks 0 and 1 of a pair tile, waves 4 .. 7 row blocks 2 and 3; in
  // a layer wave `wave` of either group owns the output tiles wave and wave + 4
  const int wave = (tid >> 6) & 3, rb0 = 2 * (tid >> 8);
  const int a = lane & 15, q = lane >> 4;
  const int E = m.E, n16 = 16 * m.NT[0];
  const int64_t b0 = static_cast<int64_t>(blockIdx.x) * NT_TU;

  nc_stage(m, sm, sf, tid, false, NT_THREADS);
  if (tid < NT_TU) {
    const int64_t b = b0 + tid;
    int64_t u = -1, lo = 0, hi = 0;
    if (b < p.o.batch) {
      u = p.uid64 ? static_cast<const int64_t *>(p.uid)[b]
                  : static_cast<int64_t>(static_cast<const int32_t *>(p.uid)[b]);
      if (u < 0 || u >= p.n_users) {  // never a table index: flagged, its list is all padding
        if (p.oob) *p.oob = 1;
        u = -1;
      } else if (p.ex_off) {
        int64_t er = b;
        if (p.ex_row)
          er = p.ex_row64 ? static_cast<const int64_t *>(p.ex_row)[b]
                          : static_cast<int64_t>(static_cast<const int32_t *>(p.ex_row)[b]);
        if (er >= 0 && er < p.ex_rows) lo = p.ex_off[er], hi = p.ex_off[er + 1];
      }
    }
    urow[tid] = static_cast<int>(u);
    exlo[tid] = lo, exhi[tid] = hi;
    cnt[tid] = 0, thr[tid] = 0;
    if (tid == 0) *due = 0;
  }
  __syncthreads();
  // the users' rows: mf_u stays for the launch, mlp_u only until a is formed (in c's place)
  for (int i = tid; i < NT_TU * E; i += NT_THREADS) {
    const int u = i / E, e = i - u * E;
    const int64_t row = urow[u];
    sf[p.muoff + i] = row >= 0 ? elem_bf16<T>(p.tab[0] + row * p.row_bytes, e) : 0.f;
    sf[p.coff + i] = row >= 0 ? elem_bf16<T>(p.tab[2] + row * p.row_bytes, e) : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < NT_TU * n16; i += NT_THREADS) {
    const int u = i / n16, n = i - u * n16;
    float acc = 0.f;
    if (n < m.N[0]) {
      acc = sf[m.boff[0] + n];
      const float *w = p.w0 + n * p.ld_w0;
      const float *x = sf + p.coff + u * E;
      for (int e = 0; e < E; ++e) acc += bf16_to_f32(f32_to_bf16_rne(w[e])) * x[e];
    }
    sf[p.aoff + u * p.lda_a + n] = acc;
  }
  __syncthreads();

  const int64_t n_items = static_cast<int64_t>(p.high) - p.low;
  const int64_t n_tiles = (n_items + NT_TI - 1) / NT_TI;
  const int64_t t0 = static_cast<int64_t>(blockIdx.y) * p.tiles_per_split;
  const int64_t t1 = t0 + p.tiles_per_split < n_tiles ? t0 + p.tiles_per_split : n_tiles;
  const int chunks = E / 8, eb = static_cast<int>(sizeof(T));
  uint16_t *H = sm + m.hbase;
  float *C = sf + p.coff;
  float dbl[2], dwph[2];  // (nc_mlp's backward arguments)
  float dp[4][4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) dp[rb][e] = 0.f;
  }
  for (int64_t tile = t0; tile < t1; ++tile) {
    const int64_t base = p.low + tile * NT_TI;
    // the tile's mlp_i rows -> the H arena (zero rows past `high`); this lane's part of
    // its item's mf_i row: chunks q and q + 4 of item 16 wave + a, as in ncf.hip (waves
    // 0 .. 3, which finish the scores)
    for (int i = tid; i < NT_TI * chunks; i += NT_THREADS) {
      const int row = i / chunks, c = i - row * chunks;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (base + row < p.high) v = load8_bf16<T>(p.tab[3] + (base + row) * p.row_bytes + 8 * c * eb);
      *reinterpret_cast<uint4 *>(H + row * m.lda + m.hoff[0] + 8 * c) = v;
    }
    const int64_t item = base + 16 * wave + a;
    uint4 mv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int c = q + 4 * i;
      mv[i] = make_uint4(0, 0, 0, 0);
      if (c < chunks && item < p.high && tid < NC_THREADS) mv[i] = load8_bf16<T>(p.tab[1] + item * p.row_bytes + 8 * c * eb);
    }
    __syncthreads();
    // c = mlp_i W_0[:, E:]^T: the wave's output tiles and row blocks as in a layer of
    // nc_mlp; fp32 to LDS, no bias, no ReLU
    if (wave < m.NT[0]) {
      const bool has1 = wave + 4 < m.NT[0];
      f32x4 acc[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[j][rb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      const uint16_t *hin = H + (16 * rb0 + a) * m.lda + m.hoff[0] + 8 * q;
      const uint16_t *w0 = sm + m.wimg[0] + (16 * wave + a) * m.ldw[0] + 8 * q;
      const uint16_t *w1 = w0 + 64 * m.ldw[0];
      for (int ks = 0; ks < m.KS[0]; ++ks) {
        bf16x8 af[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
          af[rb] = *reinterpret_cast<const bf16x8 *>(hin + 16 * rb * m.lda + 32 * ks);
        const bf16x8 f0 = *reinterpret_cast<const bf16x8 *>(w0 + 32 * ks);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) acc[0][rb] = mfma_16x16x32(af[rb], f0, acc[0][rb]);
        if (has1) {
          const bf16x8 f1 = *reinterpret_cast<const bf16x8 *>(w1 + 32 * ks);
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) acc[1][rb] = mfma_16x16x32(af[rb], f1, acc[1][rb]);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j == 0 || has1) {
          const int n = 16 * (wave + 4 * j) + a;
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int e = 0; e < 4; ++e) C[(16 * (rb0 + rb) + 4 * q + e) * p.ldc + n] = acc[j][rb][e];
          }
        }
      }
    }
    __syncthreads();

    int full = 0;
    for (int u = 0; u < NT_TU; ++u) {
      if (urow[u] < 0) continue;  // (the whole workgroup together)
      const float *ua = sf + p.aoff + u * p.lda_a;
      if (m.nl > 1) {
        // h_1 = relu(a + c), rounded to bf16 as layer 1's operand: 8 units per thread
        const int cpr = n16 / 8;
        for (int i = tid; i < NT_TI * cpr; i += NT_THREADS) {
          const int row = i / cpr, c = i - row * cpr;
          const float4 x0 = *reinterpret_cast<const float4 *>(ua + 8 * c);
          const float4 x1 = *reinterpret_cast<const float4 *>(ua + 8 * c + 4);
          const float4 y0 = *reinterpret_cast<const float4 *>(C + row * p.ldc + 8 * c);
          const float4 y1 = *reinterpret_cast<const float4 *>(C + row * p.ldc + 8 * c + 4);
          const float h[8] = {x0.x + y0.x, x0.y + y0.y, x0.z + y0.z, x0.w + y0.w,
                              x1.x + y1.x, x1.y + y1.y, x1.z + y1.z, x1.w + y1.w};
          float r[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = h[j] > 0.f ? h[j] : 0.f;
          *reinterpret_cast<uint4 *>(H + row * m.lda + m.hoff[1] + 8 * c) =
              make_uint4(pack_bf16x2(r[0], r[1]), pack_bf16x2(r[2], r[3]), pack_bf16x2(r[4], r[5]),
                         pack_bf16x2(r[6], r[7]));
        }
        __syncthreads();
        nc_mlp<false, 1, 2>(m, sm, sf, wave, lane, dp, dbl, dwph, rb0);
      }
      if (tid >= NC_THREADS) continue;  // one lane group per item: waves 0 .. 3 finish the score
      // g . wp[:E], ncf.hip's sum: chunks q and q + 4, then the four quarters of the row
      float gs = 0.f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = q + 4 * i;
        if (c < chunks) {
          float v[8];
          nc_unpack8(mv[i], v);
          const float *mu = sf + p.muoff + u * E + 8 * c;
#pragma unroll
          for (int j = 0; j < 8; ++j) gs += sf[m.wpoff + 8 * c + j] * (mu[j] * v[j]);
        }
      }
      gs += __shfl_xor(gs, 16);
      gs += __shfl_xor(gs, 32);
      float score;
      if (m.nl > 1) {
        const float *sd = sf + m.dotoff + 16 * wave + a;  // the four tile owners' parts, in order
        score = gs + (((sd[0] + sd[NC_TILE]) + sd[2 * NC_TILE]) + sd[3 * NC_TILE]);
      } else {
        // one layer: h_1 is the last and stays fp32; its dot with wp[E:] in the MF term's
        // arrangement (unit chunks q, q + 4, .., then the four quarters of the row)
        const float *cr = C + (16 * wave + a) * p.ldc;
        float d = 0.f;
        for (int c = q; 8 * c < n16; c += 4) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float x = ua[8 * c + j] + cr[8 * c + j];
            d += sf[m.wpoff + E + 8 * c + j] * (x > 0.f ? x : 0.f);
          }
        }
        d += __shfl_xor(d, 16);
        d += __shfl_xor(d, 32);
        score = gs + d;
      }
      if (q == 0 && item < p.high) {
        const unsigned long long th = thr[u];
        full |= tk_offer(score, static_cast<int32_t>(item), th, tk_thr_score(th), p.ex_items, exlo[u],
                         exhi[u], buf, cnt, u, p.cap, p.lim);
      }
    }
    // a reduction is due when any lane saw a count pass lim.  The vote goes through a word
    // of the plan, not __syncthreads_or, whose scratch is static LDS outside the plan's
    // budget; the barriers are needed either way (the next tile overwrites the arena and c)
    if (full) *due = 1;
    __syncthreads();
    const int reduce = *due;
    __syncthreads();
    if (tid == 0) *due = 0;
    if (reduce) tk_cut<NT_THREADS>(buf, thr, cnt, NT_TU, p.cap, p.o.k, p.P, tid);
  }
  tk_finish<NT_THREADS>(buf, cnt, NT_TU, p.cap, p.P, b0, blockIdx.y, p.o, tid);
}

}  // namespace mrec

using namespace mrec;

namespace {

int nt_pad(int v, int m) { return (v + m - 1) / m * m; }

// The shape's plan: layer geometry (layer 0 is the item half of W_0) and the LDS layout.
// False when the shape is outside the compiled domain or does not fit the CU's LDS.
bool nt_plan(int32_t E, int32_t nl, const int32_t *widths, int32_t k, NcfTopkArgs *t) {
  if (!(E == 8 || E == 16 || E == 32 || E == 64) || nl < 1 || nl > NC_MAXL || !widths) return false;
  if (k < 1 || k > TK_MAXK) return false;
  for (int l = 0; l < nl; ++l)
    if (widths[l] < 8 || widths[l] > NC_MAXW || widths[l] % 8) return false;
  NcfArgs *p = &t->m;
  p->E = E, p->nl = nl;
  int sm = 0, hcols = 0, fl = 0;
  for (int l = 0; l < nl; ++l) {
    p->N[l] = widths[l];
    p->K[l] = l ? widths[l - 1] : E;
    p->NT[l] = nt_pad(p->N[l], 16) / 16;
    p->KS[l] = nt_pad(p->K[l], 32) / 32;
    p->CT[l] = nt_pad(p->K[l], 16) / 16;
    p->ldw[l] = 32 * p->KS[l] + 8;
    p->wimg[l] = sm;
    sm += 16 * p->NT[l] * p->ldw[l];
    p->hoff[l] = hcols, hcols += 32 * p->KS[l];
    p->boff[l] = fl, fl += 16 * p->NT[l];
  }
  p->hbase = sm, p->lda = hcols + 8, sm += NC_TILE * p->lda;
  p->fbase = 2 * sm;
  const int n16 = 16 * p->NT[0], nk16 = 16 * p->NT[nl - 1];
  p->wpoff = fl, fl += E + nk16;
  p->dotoff = fl, fl += 4 * NC_TILE;
  t->aoff = fl, t->lda_a = n16, fl += NT_TU * n16;
  t->coff = fl, t->ldc = n16 + 4, fl += NT_TI * t->ldc;  // (also the users' mlp_u rows, at the start)
  t->muoff = fl, fl += NT_TU * E;
  // a tile adds at most NT_TI keys to a user: the reduction falls due past lim = cap - NT_TI
  t->lim = 2 * k > 64 ? 2 * k : 64;
  if (t->lim > 192) t->lim = 192;
  t->cap = t->lim + NT_TI;
  t->P = tk_pow2_at_least(t->cap);
  t->kbase = nt_pad(p->fbase + 4 * fl, 8);
  t->bytes = t->kbase + NT_TU * (t->cap * 8 + 8 + 8 + 8 + 4 + 4) + 8;  // (+ the vote word)
  return NT_TU * E <= NT_TI * t->ldc && t->bytes <= NC_LDS_LIMIT;
}

template <typename T>
mrec_status nt_launch(const NcfTopkArgs &p, dim3 grid, hipStream_t s) {
  // the plan is all of the kernel's LDS (static_lds below): a plan within NC_LDS_LIMIT can
  // be placed.  Both facts are checked once, so that the gate and the launch agree.
  static const hipError_t once = [] {
    hipFuncAttributes fa{};
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(ncf_topk_kernel<T>));
    if (e == hipSuccess && fa.sharedSizeBytes != 0) e = hipErrorInvalidValue;
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void *>(ncf_topk_kernel<T>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, NC_LDS_LIMIT);
    (void)hipGetLastError();
    return e;
  }();
  if (once != hipSuccess) {
    set_error("mrec_ncf_topk: the kernel's LDS budget could not be set up");
    return MREC_EHIP;
  }
  ncf_topk_kernel<T><<<grid, NT_THREADS, p.bytes, s>>>(p);
  return launch_status("mrec_ncf_topk");
}

}  // namespace

extern "C" {

int32_t mrec_ncf_topk_supported(int32_t E, int32_t n_layers, const int32_t *widths, int32_t k,
                                mrec_dtype bank_dtype) {
  NcfTopkArgs t{};
  return (bank_dtype == MREC_F32 || bank_dtype == MREC_BF16) && nt_plan(E, n_layers, widths, k, &t);
}

int32_t mrec_ncf_topk_tile_users(void) { return NT_TU; }
int32_t mrec_ncf_topk_tile_items(void) { return NT_TI; }

int32_t mrec_ncf_topk_splits(int64_t batch, int64_t n_items) {
  if (batch <= 0 || n_items <= 0) return 1;
  const int64_t ut = (batch + NT_TU - 1) / NT_TU, it = (n_items + NT_TI - 1) / NT_TI;
  // fill the CUs when the batch is small; c is recomputed per user tile, so no more
  // splits than that takes
  int64_t s = (device_cus() + ut - 1) / ut;
  if (s > it) s = it;
  if (s > TK_MAX_SPLITS) s = TK_MAX_SPLITS;
  return static_cast<int32_t>(s < 1 ? 1 : s);
}

size_t mrec_ncf_topk_workspace_size(int64_t batch, int32_t k, int32_t splits) {
  return tk_workspace_size(batch, k, splits);
}

mrec_status mrec_ncf_topk(const mrec_ncf_topk_args *a, mrec_stream stream) {
  MREC_CHECK_ARG(a, "NULL arguments");
  const mrec_table_bank *bank = a->bank;
  MREC_CHECK_ARG(bank && bank->data && bank->row_offset && bank->rows, "NULL bank pointer");
  MREC_CHECK_ARG(bank->dtype == MREC_F32 || bank->dtype == MREC_BF16, "bank dtype must be F32/BF16");
  NcfTopkArgs p{};
  MREC_CHECK_ARG(nt_plan(bank->dim, a->n_layers, a->widths, a->k, &p),
                 "unsupported shape (mrec_ncf_topk_supported)");
  MREC_CHECK_ARG(bank->n_tables <= MREC_MAX_TABLES, "too many tables");
  const int32_t tabs[4] = {a->table_mf_u, a->table_mf_i, a->table_mlp_u, a->table_mlp_i};
  for (int f = 0; f < 4; ++f)
    MREC_CHECK_ARG(tabs[f] >= 0 && tabs[f] < bank->n_tables, "table index out of range");
  const int eb = bank->dtype == MREC_F32 ? 4 : 2;
  const int64_t row_bytes = static_cast<int64_t>(bank->row_stride) * eb;
  MREC_CHECK_ARG(bank->row_stride >= bank->dim && row_bytes >= 16 && row_bytes <= 256 &&
                     (row_bytes & (row_bytes - 1)) == 0,
                 "row_stride*elem_size must be a power of two in [16, 256] bytes");
  MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(bank->data) & 15) == 0, "bank->data not 16B aligned");
  const int64_t users = bank->rows[tabs[0]], items = bank->rows[tabs[1]];
  MREC_CHECK_ARG(users >= 0 && users <= INT32_MAX && items >= 0 && items <= INT32_MAX,
                 "a table must have 0 .. 2^31 - 1 rows");
  MREC_CHECK_ARG(bank->rows[tabs[2]] == users && bank->rows[tabs[3]] == items,
                 "the mf and mlp tables of a side must have the same rows");
  for (int f = 0; f < 4; ++f) MREC_CHECK_ARG(bank->row_offset[tabs[f]] >= 0, "negative row offset");
  MREC_CHECK_ARG(a->low >= 0 && a->low <= a->high && a->high <= items,
                 "need 0 <= low <= high <= the item tables' rows");
  MREC_CHECK_ARG(a->batch >= 0 && a->batch <= INT32_MAX, "batch must be in 0 .. 2^31 - 1");
  MREC_CHECK_ARG(a->uid_dtype == MREC_I32 || a->uid_dtype == MREC_I64, "uid must be int32 or int64");
  MREC_CHECK_ARG(a->ld_out >= a->k, "ld_out is smaller than k");
  MREC_CHECK_ARG(a->batch == 0 || (a->uid && a->out_ids && a->out_scores), "NULL pointer");
  MREC_CHECK_ARG(a->wp, "NULL pointer");
  for (int l = 0; l < p.m.nl; ++l) {
    MREC_CHECK_ARG(a->w[l] && a->b[l], "NULL pointer");
    MREC_CHECK_ARG(a->ld_w[l] >= (l ? p.m.K[l] : 2 * bank->dim), "a leading dimension is smaller than its row");
  }
  const bool excl = a->excl_offsets != nullptr;
  MREC_CHECK_ARG(!excl || (a->excl_items && a->excl_n_rows >= 0),
                 "an exclusion needs offsets, items and n_rows >= 0");
  MREC_CHECK_ARG(excl || (!a->excl_items && !a->excl_row), "exclusion items or rows without offsets");
  MREC_CHECK_ARG(!a->excl_row || a->excl_row_dtype == MREC_I32 || a->excl_row_dtype == MREC_I64,
                 "excl_row must be int32 or int64");
  MREC_CHECK_ARG(a->splits >= 0 && a->splits <= TK_MAX_SPLITS, "splits must be in 0 .. 64 (0: the default)");
  const int64_t n_items = a->high - a->low;
  const int32_t splits = a->splits ? a->splits : mrec_ncf_topk_splits(a->batch, n_items);
  const size_t need = tk_workspace_size(a->batch, a->k, splits);
  if (need > 0 && a->batch > 0 && n_items > 0) {
    MREC_CHECK_ARG(a->workspace != nullptr && a->workspace_bytes >= need,
                   "workspace smaller than mrec_ncf_topk_workspace_size");
    MREC_CHECK_ARG((reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0, "workspace not 8-byte aligned");
  }
  if (a->batch == 0) return MREC_OK;

  for (int l = 0; l < p.m.nl; ++l) {
    p.m.w[l] = l ? a->w[l] : a->w[0] + bank->dim;  // layer 0's image: the item half
    p.m.ld_w[l] = a->ld_w[l];
    p.m.b[l] = a->b[l];
  }
  p.m.wp = a->wp;
  p.w0 = a->w[0];
  p.ld_w0 = a->ld_w[0];
  for (int f = 0; f < 4; ++f)
    p.tab[f] = static_cast<const char *>(bank->data) + bank->row_offset[tabs[f]] * row_bytes;
  p.row_bytes = row_bytes;
  p.n_users = users;
  p.low = static_cast<int32_t>(a->low);
  p.high = static_cast<int32_t>(a->high);
  p.uid = a->uid;
  p.uid64 = a->uid_dtype == MREC_I64;
  p.oob = a->d_oob_flag;
  p.ex_off = a->excl_offsets;
  p.ex_items = a->excl_items;
  p.ex_rows = a->excl_n_rows;
  p.ex_row = a->excl_row;
  p.ex_row64 = a->excl_row_dtype == MREC_I64;
  p.o.batch = static_cast<int32_t>(a->batch);
  p.o.k = a->k;
  p.o.splits = 1;
  p.o.out_ids = a->out_ids;
  p.o.out_scores = a->out_scores;
  p.o.ld_out = a->ld_out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_items == 0) return tk_launch_fill(p.o, s, "mrec_ncf_topk");
  const int64_t n_tiles = (n_items + NT_TI - 1) / NT_TI;
  p.o.splits = splits;
  p.tiles_per_split = static_cast<int32_t>((n_tiles + splits - 1) / splits);
  p.o.part = static_cast<unsigned long long *>(a->workspace);
  const dim3 grid(static_cast<unsigned>((a->batch + NT_TU - 1) / NT_TU), static_cast<unsigned>(splits));
  const mrec_status st = bank->dtype == MREC_BF16 ? nt_launch<uint16_t>(p, grid, s) : nt_launch<float>(p, grid, s);
  if (st != MREC_OK || splits == 1) return st;
  return tk_launch_merge(p.o, s, "mrec_ncf_topk");
}

}  // extern "C"
