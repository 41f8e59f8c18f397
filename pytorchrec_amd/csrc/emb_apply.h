// Embedding-backward apply helpers: the per-lookup gradient, the row update
// (SGD with RNE / stochastic rounding, or dense-gradient accumulation) and the
// register sort network.  Shared by the batched apply (emb_bwd.hip) and the
// large-batch path (emb_bwd_large.hip).
#pragma once
#include "common.h"

namespace mrec {

struct ApplyArgs {
  const void *dx;
  int64_t dx_ld;
  int dx_bf16;
  const float *dfm;
  const float *fm_sum;
  const void *x0;
  int64_t x0_ld;
  int x0_bf16;
  const float *dw;
  int mode;
  float lr;
  uint64_t seed;
  const uint64_t *d_step;
  void *grad;
  // per-lookup gradient rows given directly (owner side of a sharded table):
  // lookup b of table f -> g_occ[idx * g_ld + e], idx = chunked(b) + f * chunk
  const float *g_occ;
  int64_t g_ld;
  int64_t chunk;
  int64_t chunk_stride;
  // or read straight from the received wire records (ABI 23, owner side of the
  // compact exchange): entry j of part p, table f -> record p * cap_rows +
  // pref[p * F + f] + j (p = b / chunk, j = b % chunk), pitch g_rec_pitch elements
  const void *g_rec;
  int g_rec_bf16;
  int g_rec_pitch;
  const int32_t *g_pref;
  int64_t g_cap_rows;
  int g_F;
  OptArgs opt;
  // DENSE_GRAD straight into wire records (ABI 26, sender side of the compact
  // exchange, mrec_emb_bwd_apply_rec): slot row s = (p * F + f) * cap + j -> record
  // p * cap_rows + o_pref[p * F + f] + j (o_rec_dw dwords); no wire pack launch
  uint32_t *o_rec;
  int o_rec_dw;
  const int32_t *o_pref;
  int o_F, o_cap;
  int64_t o_cap_rows;
  // data-parallel dense SGD tiles riding in this launch (ABI 28,
  // mrec_emb_bwd_apply_wire_sgd): a device-resident SgdArgs (optim_common.h)
  const struct SgdArgs *sgd;
  int sgd_blocks;
  // bag indirection (ABI 30, mrec_emb_bwd_apply_bag / _large_fused_bag): the lookups
  // are the bag_len positions of pooled bags, lookup i of table f belongs to bag
  // bb = i / bag and its gradient is bag_scale[bb * g_F + f] * (dx | dw)[bb]: the
  // bag's gradient row is read through the index, never expanded.  0 = off.
  int bag;
  const float *bag_scale;
};

// One embedding-backward apply as its entry point describes it (host only).  Every
// extern "C" entry fills the members it has, by name, and hands the request on; a new
// gradient source or rider is a member here, not another positional list.
struct BwdRequest {
  const char *who = "";  // the entry point's own name (error text, ws_layout_check)
  // gradients derived per lookup from dx / dfm / dw
  const void *dx = nullptr;
  mrec_dtype dx_dtype = MREC_F32;
  int64_t dx_ld = 0;
  const float *dfm = nullptr;
  const float *fm_sum = nullptr;
  const void *x0 = nullptr;
  mrec_dtype x0_dtype = MREC_F32;
  int64_t x0_ld = 0;
  const float *dw = nullptr;
  // or given as fp32 rows
  const float *g_occ = nullptr;
  int64_t g_ld = 0;
  // or given as wire records (from_wire: the entry takes them, so `wire` must be set)
  bool from_wire = false;
  const void *wire = nullptr;
  mrec_dtype wire_dtype = MREC_F32;
  int32_t rec_bytes = 0;
  const int32_t *pref = nullptr;
  int32_t cap_rows = 0;
  // the exchange-view chunking of both given forms
  int64_t chunk = 0;
  int64_t chunk_stride = 0;
  // bag indirection (bag: the entry takes pooled bags, so bag_len / bag_scale must be set)
  bool bag = false;
  int32_t bag_len = 0;
  const float *bag_scale = nullptr;
  // DENSE_GRAD sums into wire records instead of `grad` (mrec_emb_bwd_apply_rec)
  const mrec_grad_records *rec_out = nullptr;
  // the update
  mrec_bwd_mode mode = MREC_BWD_SGD;
  float lr = 0.f;
  uint64_t seed = 0;
  const uint64_t *d_step = nullptr;
  void *grad = nullptr;
  // what rides along in the launch
  int32_t n_reduce = 0;
  const mrec_gemm_call *reduce = nullptr;
  const void *sgd_table = nullptr;
  int32_t sgd_blocks = 0;

  void set_given(const mrec_given_grads &g) {
    g_occ = g.g_occ, g_ld = g.g_ld;
    from_wire = g.wire != nullptr;
    wire = g.wire, wire_dtype = g.wire_dtype, rec_bytes = g.rec_bytes;
    pref = g.pref, cap_rows = g.cap_rows;
    chunk = g.chunk, chunk_stride = g.chunk_stride;
  }
};

// MREC_CHECK_ARG with the entry point's own name in the error text
#define MREC_CHECK_REQ(req, cond, msg)                          \
  do {                                                          \
    if (!(cond)) {                                              \
      ::mrec::set_error(std::string((req).who) + ": " + (msg)); \
      return MREC_EINVAL;                                       \
    }                                                           \
  } while (0)

// The checked ApplyArgs of a request: every check the batched and the large-batch
// path share, each once.  What only one path requires (its batch bounds, the layout
// rule, record output and SGD tiles, chunk >= 1 on the large path) stays with it.
static inline mrec_status make_apply_args(const mrec_table_bank *bank, const BankArgs &ba,
                                          int64_t batch, const BwdRequest &req, ApplyArgs *out) {
  const auto aligned = [](const void *p, uintptr_t to) {
    return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0;
  };
  const auto f32_or_bf16 = [](mrec_dtype t) { return t == MREC_F32 || t == MREC_BF16; };
  const auto row_bytes = [](int64_t ld, mrec_dtype t) { return ld * (t == MREC_F32 ? 4 : 2); };
  const int F = ba.n_tables, D = ba.dim, row = D + (ba.has_w ? 1 : 0);
  MREC_CHECK_REQ(req, req.mode >= MREC_BWD_DENSE_GRAD && req.mode <= MREC_BWD_ADAM, "bad mode");
  MREC_CHECK_REQ(req, req.mode != MREC_BWD_DENSE_GRAD || req.grad || req.rec_out,
                 "DENSE_GRAD needs grad");
  ApplyArgs a{};
  if (mrec_status st = make_opt_args(bank, req.mode, &a.opt); st != MREC_OK) return st;
  if (req.dx) {
    MREC_CHECK_REQ(req, f32_or_bf16(req.dx_dtype), "dx dtype must be F32/BF16");
    MREC_CHECK_REQ(req, req.dx_ld >= static_cast<int64_t>(F) * D, "dx_ld < F*dim");
    MREC_CHECK_REQ(req, aligned(req.dx, 16) && row_bytes(req.dx_ld, req.dx_dtype) % 16 == 0,
                   "dx must be 16B aligned with 16B-multiple rows");
  }
  if (req.dfm) {
    MREC_CHECK_REQ(req, req.fm_sum != nullptr && req.x0 != nullptr, "dfm needs fm_sum and x0");
    MREC_CHECK_REQ(req, f32_or_bf16(req.x0_dtype), "x0 dtype must be F32/BF16");
    MREC_CHECK_REQ(req, req.x0_ld >= static_cast<int64_t>(F) * D, "x0_ld < F*dim");
    MREC_CHECK_REQ(req, aligned(req.x0, 16) && row_bytes(req.x0_ld, req.x0_dtype) % 16 == 0 &&
                       aligned(req.fm_sum, 16),
                   "x0/fm_sum must be 16B aligned with 16B-multiple rows");
  }
  MREC_CHECK_REQ(req, req.dw == nullptr || ba.has_w, "dw given but bank has no w column");
  if (req.from_wire) {
    MREC_CHECK_REQ(req, !req.dx && !req.dfm && !req.dw && !req.g_occ,
                   "wire gradients exclude dx / dfm / dw / g_occ");
    MREC_CHECK_REQ(req, f32_or_bf16(req.wire_dtype), "wire dtype must be BF16/F32");
    const int es = req.wire_dtype == MREC_BF16 ? 2 : 4;
    MREC_CHECK_REQ(req, req.rec_bytes > 0 && req.rec_bytes % es == 0 && req.rec_bytes % 4 == 0,
                   "bad record bytes");
    MREC_CHECK_REQ(req, req.wire && req.pref && req.cap_rows >= 1,
                   "NULL wire / pref, cap_rows < 1");
    MREC_CHECK_REQ(req, req.rec_bytes / es >= row && aligned(req.wire, 4),
                   "records: pitch >= dim + has_w elements, 4-B aligned");
    MREC_CHECK_REQ(req, req.chunk >= 1, "chunk (entries per exchange part) must be >= 1");
    a.g_rec = req.wire;
    a.g_rec_bf16 = req.wire_dtype == MREC_BF16;
    a.g_rec_pitch = req.rec_bytes / es;
    a.g_pref = req.pref;
    a.g_cap_rows = req.cap_rows;
  }
  if (req.g_occ) {
    MREC_CHECK_REQ(req, !req.dx && !req.dfm && !req.dw, "g_occ excludes dx / dfm / dw");
    MREC_CHECK_REQ(req, req.g_ld >= row && req.g_ld % 4 == 0 && aligned(req.g_occ, 16),
                   "g_occ rows must be 16B aligned, g_ld >= dim + has_w, g_ld % 4 == 0");
    MREC_CHECK_REQ(req, req.chunk >= 0 && (req.chunk == 0 || req.chunk_stride >= F * req.chunk),
                   "chunk < 0, or chunk_stride < n_tables * chunk");
  }
  if (req.bag) {
    MREC_CHECK_REQ(req, req.bag_len >= 1, "bag_len < 1");
    MREC_CHECK_REQ(req, batch >= 0 && batch % req.bag_len == 0, "batch is not a multiple of bag_len");
    MREC_CHECK_REQ(req, req.bag_scale != nullptr, "bag_scale is NULL");
    MREC_CHECK_REQ(req, req.dfm == nullptr, "the FM term is undefined for bags (dfm must be NULL)");
    a.bag = req.bag_len;  // (dx / dw hold batch / bag_len rows: one per bag)
    a.bag_scale = req.bag_scale;
  }
  a.dx = req.dx;
  a.dx_ld = req.dx_ld;
  a.dx_bf16 = req.dx_dtype == MREC_BF16;
  a.dfm = req.dfm;
  a.fm_sum = req.fm_sum;
  a.x0 = req.x0;
  a.x0_ld = req.x0_ld;
  a.x0_bf16 = req.x0_dtype == MREC_BF16;
  a.dw = req.dw;
  a.mode = req.mode;
  a.lr = req.lr;
  a.seed = req.seed;
  a.d_step = req.d_step;
  a.grad = req.grad;
  a.g_occ = req.g_occ;
  a.g_ld = req.g_ld;
  a.chunk = req.chunk;
  a.chunk_stride = req.chunk_stride;
  a.g_F = a.o_F = F;
  a.o_cap = 1;  // (record output, hash layout only: the batched apply fills o_*)
  *out = a;
  return MREC_OK;
}

// lookup i -> its bag (i < 2^31: the entry points check batch), and the bag's scale
__device__ __forceinline__ float bag_index(const ApplyArgs &a, int64_t &b, int f) {
  b = static_cast<int64_t>(static_cast<uint32_t>(b) / static_cast<uint32_t>(a.bag));
  return a.bag_scale[b * a.g_F + f];
}
// one fp32 multiply per element (never contracted into the segment sum's add)
template <int EPL>
__device__ __forceinline__ void bag_scale_grad(float bs, bool v_lane, float *g) {
  if (v_lane) {
#pragma unroll
    for (int j = 0; j < EPL; ++j) g[j] = __fmul_rn(bs, g[j]);
  } else {
    g[0] = __fmul_rn(bs, g[0]);
  }
}

// a given gradient from a wire record (4-B aligned rows: records are not 16-B).
// An entry past its part's cap_rows records had its record clipped by the sender
// (the overflow flag is set): zero gradient -- never another entry's record.
template <int EPL>
__device__ __forceinline__ void wire_grad(const ApplyArgs &a, int64_t b, int f, int D, int e0,
                                          bool v_lane, bool w_lane, float *g) {
  const int64_t p = b / a.chunk, j = b - p * a.chunk;
  const int64_t in_part = a.g_pref[p * a.g_F + f] + j;
  if (in_part >= a.g_cap_rows) return;  // g stays zero (lookup_grad zeroed it)
  const int64_t rec = p * a.g_cap_rows + in_part;
  if (a.g_rec_bf16) {
    const uint16_t *go = static_cast<const uint16_t *>(a.g_rec) + rec * a.g_rec_pitch;
    if (v_lane) {
      const uint32_t *q = reinterpret_cast<const uint32_t *>(go + e0);
#pragma unroll
      for (int i = 0; i < EPL / 2; ++i) {
        const uint32_t x = q[i];
        g[2 * i] = __uint_as_float(x << 16);
        g[2 * i + 1] = __uint_as_float(x & 0xffff0000u);
      }
    } else if (w_lane) {
      g[0] = __uint_as_float(static_cast<uint32_t>(go[D]) << 16);
    }
  } else {
    const float *go = static_cast<const float *>(a.g_rec) + rec * a.g_rec_pitch;
    if (v_lane) {
#pragma unroll
      for (int i = 0; i < EPL; ++i) g[i] = go[e0 + i];
    } else if (w_lane) {
      g[0] = go[D];
    }
  }
}

template <int EPL>
__device__ __forceinline__ void load_f32xN(const float *p, float *v) {
#pragma unroll
  for (int j = 0; j < EPL; j += 4) {
    const float4 x = *reinterpret_cast<const float4 *>(p + j);
    v[j] = x.x;
    v[j + 1] = x.y;
    v[j + 2] = x.z;
    v[j + 3] = x.w;
  }
}

template <int EPL>
__device__ __forceinline__ void load_bf16xN(const uint16_t *p, float *v) {
  if constexpr (EPL == 8) {
    Vec<uint16_t>::to_f32(*reinterpret_cast<const uint4 *>(p), v);
  } else {
    const uint2 r = *reinterpret_cast<const uint2 *>(p);
    v[0] = __uint_as_float(r.x << 16);
    v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16);
    v[3] = __uint_as_float(r.y & 0xffff0000u);
  }
}

// gradient of lookup (b, f) for this lane's EPL elements (w lane: g[0]).  BAG: the
// bag indirection, a template flag instantiated only by the bag entry points, so
// every other kernel compiles exactly as it would without it
template <int EPL, bool BAG = false>
__device__ __forceinline__ void lookup_grad(const ApplyArgs &a, int64_t b, int f, int D, int e0,
                                            bool v_lane, bool w_lane, float *g) {
#pragma unroll
  for (int j = 0; j < EPL; ++j) g[j] = 0.f;
  if (a.g_rec) {
    wire_grad<EPL>(a, b, f, D, e0, v_lane, w_lane, g);
    return;
  }
  if (a.g_occ) {
    const int64_t idx = a.chunk ? (b / a.chunk) * a.chunk_stride + f * a.chunk + b % a.chunk : b;
    const float *go = a.g_occ + idx * a.g_ld;
    if (v_lane)
      load_f32xN<EPL>(go + e0, g);
    else if (w_lane)
      g[0] = go[D];
    return;
  }
  float bs = 0.f;
  if constexpr (BAG) bs = bag_index(a, b, f);  // b becomes the bag (dfm is NULL)
  if (v_lane) {
    // the same arithmetic as mrec_shard_lookup_grad, so sharded and unsharded
    // updates agree
    const int64_t col = static_cast<int64_t>(f) * D + e0;
    if (a.dx) {
      if (a.dx_bf16)
        load_bf16xN<EPL>(static_cast<const uint16_t *>(a.dx) + b * a.dx_ld + col, g);
      else
        load_f32xN<EPL>(static_cast<const float *>(a.dx) + b * a.dx_ld + col, g);
    }
    if (a.dfm) {
      const float c = a.dfm[b];
      float s[EPL], v[EPL];
      load_f32xN<EPL>(a.fm_sum + b * D + e0, s);
      if (a.x0_bf16)
        load_bf16xN<EPL>(static_cast<const uint16_t *>(a.x0) + b * a.x0_ld + col, v);
      else
        load_f32xN<EPL>(static_cast<const float *>(a.x0) + b * a.x0_ld + col, v);
#pragma unroll
      for (int j = 0; j < EPL; ++j) g[j] = fmaf(c, s[j] - v[j], g[j]);
    }
  } else if (w_lane && a.dw) {
    g[0] = a.dw[b];
  }
  if constexpr (BAG) bag_scale_grad<EPL>(bs, v_lane, g);
}

// gradient of lookup (b, f) with the row's current values v (this lane's EPL
// elements, bank dtype widened) for the FM term: the hash-layout apply reads the
// row it updates anyway, so the gathered rows are not re-read from x0
template <int EPL, bool BAG = false>
__device__ __forceinline__ void lookup_grad_v(const ApplyArgs &a, int64_t b, int f, int D, int e0,
                                              bool v_lane, bool w_lane, const float *v, float *g) {
#pragma unroll
  for (int j = 0; j < EPL; ++j) g[j] = 0.f;
  if (a.g_rec) {
    wire_grad<EPL>(a, b, f, D, e0, v_lane, w_lane, g);
    return;
  }
  if (a.g_occ) {
    const int64_t idx = a.chunk ? (b / a.chunk) * a.chunk_stride + f * a.chunk + b % a.chunk : b;
    const float *go = a.g_occ + idx * a.g_ld;
    if (v_lane)
      load_f32xN<EPL>(go + e0, g);
    else if (w_lane)
      g[0] = go[D];
    return;
  }
  float bs = 0.f;
  if constexpr (BAG) bs = bag_index(a, b, f);  // b becomes the bag (dfm is NULL)
  if (v_lane) {
    const int64_t col = static_cast<int64_t>(f) * D + e0;
    if (a.dx) {
      if (a.dx_bf16)
        load_bf16xN<EPL>(static_cast<const uint16_t *>(a.dx) + b * a.dx_ld + col, g);
      else
        load_f32xN<EPL>(static_cast<const float *>(a.dx) + b * a.dx_ld + col, g);
    }
    if (a.dfm) {
      const float c = a.dfm[b];
      float s[EPL];
      load_f32xN<EPL>(a.fm_sum + b * D + e0, s);
#pragma unroll
      for (int j = 0; j < EPL; ++j) g[j] = fmaf(c, s[j] - v[j], g[j]);
    }
  } else if (w_lane && a.dw) {
    g[0] = a.dw[b];
  }
  if constexpr (BAG) bag_scale_grad<EPL>(bs, v_lane, g);
}

template <int EPL, bool BAG = false>
__device__ __forceinline__ void add_lookup_grad_v(const ApplyArgs &a, int64_t b, int f, int D,
                                                  int e0, bool v_lane, bool w_lane, const float *v,
                                                  float *acc) {
  float g[EPL];
  lookup_grad_v<EPL, BAG>(a, b, f, D, e0, v_lane, w_lane, v, g);
#pragma unroll
  for (int j = 0; j < EPL; ++j) acc[j] += g[j];
}

// per-lookup gradient first, then one add into the segment sum
template <int EPL, bool BAG = false>
__device__ __forceinline__ void add_lookup_grad(const ApplyArgs &a, int64_t b, int f, int D,
                                                int e0, bool v_lane, bool w_lane, float *acc) {
  float g[EPL];
  lookup_grad<EPL, BAG>(a, b, f, D, e0, v_lane, w_lane, g);
#pragma unroll
  for (int j = 0; j < EPL; ++j) acc[j] += g[j];
}

// element e0 of global row `grow` (table offset already added): the bank, or the
// dense gradient buffer in DENSE_GRAD mode
// (MODE >= 0: the update mode fixed at compile time, else a.mode)
template <typename T, int MODE = -1>
__device__ __forceinline__ T *row_ptr_g(const BankArgs &bank, const ApplyArgs &a, int64_t grow,
                                        int e0) {
  const int mode = MODE >= 0 ? MODE : a.mode;
  const int64_t off = grow * static_cast<int64_t>(bank.row_stride) + e0;
  return reinterpret_cast<T *>(mode == MREC_BWD_DENSE_GRAD ? static_cast<char *>(a.grad)
                                                            : bank.data) +
         off;
}

template <typename T>
__device__ __forceinline__ T *row_ptr(const BankArgs &bank, const ApplyArgs &a, int f,
                                      int64_t row, int e0) {
  return row_ptr_g<T>(bank, a, bank.row_offset[f] + row, e0);
}

// DENSE_GRAD into a wire record (a.o_rec): the sums the slot row would hold after
// the zeroed buffer's `0 + acc`, rounded to the table dtype as there; the record's
// dwords only (a w lane: its one dword, element D and the zero pad beside it).  An
// entry past its part's cap_rows records is dropped (the unpack flagged it).
template <typename T>
__device__ __forceinline__ void rec_out(const ApplyArgs &a, int64_t grow, int e0, bool v_lane,
                                        const float *acc) {
  constexpr int EPL = Vec<T>::EPL;
  const int64_t fc = static_cast<int64_t>(a.o_F) * a.o_cap;
  const int64_t p = grow / fc, rem = grow - p * fc;
  const int f = static_cast<int>(rem / a.o_cap);
  const int64_t j = rem - static_cast<int64_t>(f) * a.o_cap;
  const int64_t in_part = a.o_pref[p * a.o_F + f] + j;
  if (in_part >= a.o_cap_rows) return;
  uint32_t *dst = a.o_rec + (p * a.o_cap_rows + in_part) * a.o_rec_dw +
                  e0 * static_cast<int>(sizeof(T)) / 4;
  if constexpr (sizeof(T) == 4) {
    if (v_lane) {
#pragma unroll
      for (int k = 0; k < EPL; ++k) dst[k] = __float_as_uint(0.f + acc[k]);
    } else {
      dst[0] = __float_as_uint(0.f + acc[0]);
    }
  } else {
    if (v_lane) {
#pragma unroll
      for (int k = 0; k < EPL / 2; ++k)
        dst[k] = static_cast<uint32_t>(f32_to_bf16_rne(0.f + acc[2 * k])) |
                 (static_cast<uint32_t>(f32_to_bf16_rne(0.f + acc[2 * k + 1])) << 16);
    } else {
      dst[0] = static_cast<uint32_t>(f32_to_bf16_rne(0.f + acc[0]));
    }
  }
}

// new value of this lane's 16 bytes of global row `grow` from its old contents `raw`
template <typename T, int MODE = -1>
__device__ __forceinline__ void apply_row_raw_g(const BankArgs &bank, const ApplyArgs &a,
                                                int64_t grow, int e0, bool v_lane,
                                                const float *acc, const uint4 raw) {
  constexpr int EPL = Vec<T>::EPL;
  if constexpr (MODE == MREC_BWD_DENSE_GRAD) {
    if (a.o_rec) {  // uniform
      rec_out<T>(a, grow, e0, v_lane, acc);
      return;
    }
  }
  const int mode = MODE >= 0 ? MODE : a.mode;
  T *p = row_ptr_g<T, MODE>(bank, a, grow, e0);
  float old[EPL];
  Vec<T>::to_f32(raw, old);
  const int live = v_lane ? EPL : 1;  // w lane: only element D is live
  float nv[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j)
    nv[j] = (mode == MREC_BWD_DENSE_GRAD) ? old[j] + acc[j] : fmaf(-a.lr, acc[j], old[j]);
  uint4 out;
  if constexpr (sizeof(T) == 4) {
    const uint32_t o[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = j < live ? __float_as_uint(nv[j]) : o[j];
    out = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    const uint32_t o[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint16_t h[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int j = 2 * k + q;
        if (j < live) {
          h[q] = (mode == MREC_BWD_SGD_SR)
                     ? f32_to_bf16_sr(nv[j], hash3(a.seed, grow, static_cast<uint32_t>(e0 + j)))
                     : f32_to_bf16_rne(nv[j]);
        } else {
          h[q] = static_cast<uint16_t>(q ? (o[k] >> 16) : (o[k] & 0xffffu));
        }
      }
      w[k] = static_cast<uint32_t>(h[0]) | (static_cast<uint32_t>(h[1]) << 16);
    }
    out = make_uint4(w[0], w[1], w[2], w[3]);
  }
  *reinterpret_cast<uint4 *>(p) = out;
}

template <typename T>
__device__ __forceinline__ void apply_row_raw(const BankArgs &bank, const ApplyArgs &a, int f,
                                              int64_t row, int e0, bool v_lane, const float *acc,
                                              const uint4 raw) {
  apply_row_raw_g<T>(bank, a, bank.row_offset[f] + row, e0, v_lane, acc, raw);
}

template <typename T>
__device__ __forceinline__ void apply_row(const BankArgs &bank, const ApplyArgs &a, int f,
                                          int64_t row, int e0, bool v_lane, const float *acc) {
  const uint4 raw = *reinterpret_cast<const uint4 *>(row_ptr<T>(bank, a, f, row, e0));
  apply_row_raw<T>(bank, a, f, row, e0, v_lane, acc, raw);
}

// Fused-optimizer update of this lane's 16 bytes of global row `grow` with the
// row's summed gradient `acc` (modes ADAGRAD / ROWWISE_ADAGRAD / ADAM).  Called by
// ALL LPR lanes of the row's worker (row-wise Adagrad sums g^2 across them);
// lanes without a live element (`live` false) only take part in that sum.
template <typename T, int LPR>
__device__ __forceinline__ void opt_row_update(const BankArgs &bank, const ApplyArgs &a,
                                               int64_t grow, int e0, bool v_lane, bool w_lane,
                                               bool live, const float *acc, const uint4 raw) {
  constexpr int EPL = Vec<T>::EPL;
  const OptArgs &o = a.opt;
  const int n = v_lane ? EPL : (w_lane ? 1 : 0);
  float g[EPL];
#pragma unroll
  for (int j = 0; j < EPL; ++j) g[j] = acc[j] * o.gscale;
  acc = g;
  float sq = 0.f;
  if (a.mode == MREC_BWD_ROWWISE_ADAGRAD) {
    if (v_lane)
#pragma unroll
      for (int j = 0; j < EPL; ++j) sq = fmaf(acc[j], acc[j], sq);
#pragma unroll
    for (int off = 1; off < LPR; off <<= 1) sq += __shfl_xor(sq, off);
  }
  if (!live) return;
  float p[EPL];
  Vec<T>::to_f32(raw, p);
  if (a.mode == MREC_BWD_ROWWISE_ADAGRAD) {
    float *st = o.s0 + grow * 2 + (v_lane ? 0 : 1);
    const float G = *st + (v_lane ? sq / static_cast<float>(bank.dim) : acc[0] * acc[0]);
    if (e0 == 0 || w_lane) *st = G;
    const float den = sqrtf(G) + o.eps;
#pragma unroll
    for (int j = 0; j < EPL; ++j)
      if (j < n) p[j] = p[j] - a.lr * (acc[j] / den);
  } else if (a.mode == MREC_BWD_ADAGRAD) {
    float *st = o.s0 + grow * o.ld + e0;
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      if (j < n) {
        const float sum = fmaf(acc[j], acc[j], st[j]);
        st[j] = sum;
        p[j] = p[j] - a.lr * (acc[j] / (sqrtf(sum) + o.eps));
      }
    }
  } else {  // MREC_BWD_ADAM
    const int64_t t = *o.d_t;
    const int64_t t0 = o.row_step[grow];
    float *mp = o.s0 + grow * o.ld + e0;
    float *vp = o.s1 + grow * o.ld + e0;
    float m[EPL], v[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      m[j] = j < n ? mp[j] : 0.f;
      v[j] = j < n ? vp[j] : 0.f;
    }
    double b1p = pow(o.beta1, static_cast<double>(t0 + 1));
    double b2p = pow(o.beta2, static_cast<double>(t0 + 1));
    for (int64_t st = t0 + 1; st < t; ++st) {  // the zero-gradient steps this row missed
      const AdamStep sc = adam_scalars(o, a.lr, b1p, b2p);
#pragma unroll
      for (int j = 0; j < EPL; ++j)
        if (j < n) adam_elem(o, sc, a.lr, 0.f, p[j], m[j], v[j]);
      b1p *= o.beta1;
      b2p *= o.beta2;
    }
    const AdamStep sc = adam_scalars(o, a.lr, b1p, b2p);
#pragma unroll
    for (int j = 0; j < EPL; ++j)
      if (j < n) adam_elem(o, sc, a.lr, acc[j], p[j], m[j], v[j]);
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
      if (j < n) {
        mp[j] = m[j];
        vp[j] = v[j];
      }
    }
    if (e0 == 0) o.row_step[grow] = static_cast<int32_t>(t);
  }
  // pack: live elements rounded once (RNE), the rest keep their bits
  T *dst = reinterpret_cast<T *>(bank.data) + grow * static_cast<int64_t>(bank.row_stride) + e0;
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
  uint32_t o4[4];
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o4[j] = j < n ? __float_as_uint(p[j]) : w[j];
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t lo = 2 * k < n ? f32_to_bf16_rne(p[2 * k]) : (w[k] & 0xffffu);
      const uint32_t hi = 2 * k + 1 < n ? f32_to_bf16_rne(p[2 * k + 1]) : (w[k] >> 16);
      o4[k] = lo | (hi << 16);
    }
  }
  *reinterpret_cast<uint4 *>(dst) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
}

// The row update of every apply path: fixed modes by template (MODE >= 0), else
// the runtime mode; all LPR lanes of the worker call it.
template <typename T, int LPR, int MODE>
__device__ __forceinline__ void row_update(const BankArgs &bank, const ApplyArgs &a, int64_t grow,
                                           int e0, bool v_lane, bool w_lane, bool live,
                                           const float *acc, const uint4 raw) {
  if (MODE >= 0 || a.mode <= MREC_BWD_SGD_SR) {
    if (live) apply_row_raw_g<T, MODE>(bank, a, grow, e0, v_lane, acc, raw);
  } else {
    opt_row_update<T, LPR>(bank, a, grow, e0, v_lane, w_lane, live, acc, raw);
  }
}

__device__ __forceinline__ void cswap(int &a, int &b) {
  const int lo = min(a, b), hi = max(a, b);
  a = lo;
  b = hi;
}

// ascending bitonic network on r[0, N) (compile-time indices: stays in VGPRs)
template <int N>
__device__ __forceinline__ void bitonic_sort(int *r) {
#pragma unroll
  for (int k = 2; k <= N; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) {
          if ((i & k) == 0)
            cswap(r[i], r[l]);
          else
            cswap(r[l], r[i]);
        }
      }
}

}  // namespace mrec
