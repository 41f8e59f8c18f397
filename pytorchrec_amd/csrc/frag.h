// The MFMA fragment and operand vocabulary of the fused kernels (gfx950 only).  Not part
// of the ABI.  A kernel file includes this header rather than declaring its own vector
// types, builtin wrappers or runtime-dtype operand helpers; everything device-side is
// __forceinline__, so sharing it costs no instruction.
#pragma once

#include "common.h"

namespace mrec {

// ---------------------------------------------------------------------------
// types: the MFMA operand (bf16 bits as shorts) and accumulator vectors
// ---------------------------------------------------------------------------
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// fragment builders.  One fp32 -> bf16 rounding is RNE (pack_bf16x2, common.h): at most
// 2^-8 relative, half a unit in the last place of bf16's 8-bit significand.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bf16x8 frag_zero8() {
  return __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
}
// eight floats rounded to one fragment
__device__ __forceinline__ bf16x8 frag_pack8(const float *f) {
  return __builtin_bit_cast(bf16x8, make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]),
                                               pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])));
}
// two 16-byte loads of eight consecutive fp32 elements rounded to one fragment
__device__ __forceinline__ bf16x8 frag_from_f32(uint4 a, uint4 b) {
  return __builtin_bit_cast(
      bf16x8, make_uint4(pack_bf16x2(__uint_as_float(a.x), __uint_as_float(a.y)),
                         pack_bf16x2(__uint_as_float(a.z), __uint_as_float(a.w)),
                         pack_bf16x2(__uint_as_float(b.x), __uint_as_float(b.y)),
                         pack_bf16x2(__uint_as_float(b.z), __uint_as_float(b.w))));
}

// ---------------------------------------------------------------------------
// MFMA: D = A B + C, named rows x columns x k
// ---------------------------------------------------------------------------
__device__ __forceinline__ f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_16x16x16(bf16x4 a, bf16x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// ---------------------------------------------------------------------------
// transposing LDS reads (ds_read_b64_tr_b16).  Per 16-lane group a block of 4 rows x 16
// columns of bf16 comes back column-major: lane 4 q + p of the group addresses row q,
// columns 4 p .. + 3, and lane i receives column i of the four rows.  Every lane of the
// wave takes part (callers branch per wave only) and every address must lie in LDS.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bf16x4 lds_tr16_b64(const void *p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4 *)(p));
}
// two blocks, the lane's 8 k values of a k = 32 operand: the one at p, then the one
// `hi_off` elements after it
__device__ __forceinline__ bf16x8 lds_tr16_pair(const uint16_t *p, int hi_off) {
  const bf16x4 lo = lds_tr16_b64(p);
  const bf16x4 hi = lds_tr16_b64(p + hi_off);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// transposing fragment for the k = 16 MFMA: element j is tile[4 (lane >> 4) + j][c0 +
// (lane & 15)]; every address lies inside the tile
__device__ __forceinline__ bf16x4 lds_tr16x4(const uint16_t *tile, int ld, int c0, int lane) {
  const int li = lane & 15;
  return lds_tr16_b64(tile + (4 * (lane >> 4) + (li >> 2)) * ld + c0 + 4 * (li & 3));
}

// ---------------------------------------------------------------------------
// operands whose element type is known at compile time (T: uint16_t for bf16, float)
// ---------------------------------------------------------------------------
// One K-step's fragment from raw 16-byte loads of its 8 elements (one load of a bf16 row,
// two of an fp32 row): s-th fragment of raw[].  Rounding happens here, at use.
template <typename T>
__device__ __forceinline__ bf16x8 frag_from_raw(const uint4 *raw, int s) {
  if constexpr (sizeof(T) == 2)
    return __builtin_bit_cast(bf16x8, raw[s]);
  else
    return frag_from_f32(raw[2 * s], raw[2 * s + 1]);
}
// 8 consecutive elements at p as 16 bytes of bf16, for staging (an fp32 row is rounded here)
template <typename T>
__device__ __forceinline__ uint4 load8_bf16(const char *p) {
  if constexpr (sizeof(T) == 2)
    return *reinterpret_cast<const uint4 *>(p);
  else
    return __builtin_bit_cast(uint4, frag_from_f32(*reinterpret_cast<const uint4 *>(p),
                                                   *reinterpret_cast<const uint4 *>(p + 16)));
}
// element e of a row as the bf16 value the products use
template <typename T>
__device__ __forceinline__ float elem_bf16(const char *row, int e) {
  if constexpr (sizeof(T) == 2)
    return bf16_to_f32(reinterpret_cast<const uint16_t *>(row)[e]);
  else
    return bf16_to_f32(f32_to_bf16_rne(reinterpret_cast<const float *>(row)[e]));
}

// ---------------------------------------------------------------------------
// operands whose element type is a run-time flag: [rows, ld] of bf16 or fp32
// ---------------------------------------------------------------------------
struct MatIn {
  const char *p;
  int64_t ld_bytes;
  int32_t bf16;
};
struct MatOut {
  char *p;
  int64_t ld_bytes;
  int32_t bf16;
};

// elements [col0, col0 + 8) of row `row` as one MFMA fragment (an fp32 row is rounded here)
__device__ __forceinline__ bf16x8 mat_load8(const MatIn &m, int64_t row, int col0) {
  const char *rp = m.p + row * m.ld_bytes;
  if (m.bf16) return __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(rp + 2 * col0));
  return frag_from_f32(*reinterpret_cast<const uint4 *>(rp + 4 * col0),
                       *reinterpret_cast<const uint4 *>(rp + 4 * col0 + 16));
}
// one element as stored (no rounding: bf16 widens exactly)
__device__ __forceinline__ float mat_elem(const MatIn &m, int64_t row, int col) {
  const char *rp = m.p + row * m.ld_bytes;
  if (m.bf16) return bf16_to_f32(reinterpret_cast<const uint16_t *>(rp)[col]);
  return reinterpret_cast<const float *>(rp)[col];
}
// one element as the bf16 value the products use (an fp32 element is rounded first)
__device__ __forceinline__ float mat_elem_bf16(const MatIn &m, int64_t row, int col) {
  const char *rp = m.p + row * m.ld_bytes;
  if (m.bf16) return bf16_to_f32(reinterpret_cast<const uint16_t *>(rp)[col]);
  return bf16_to_f32(f32_to_bf16_rne(reinterpret_cast<const float *>(rp)[col]));
}
__device__ __forceinline__ void mat_store(const MatOut &o, int64_t row, int col, float v) {
  char *rp = o.p + row * o.ld_bytes;
  if (o.bf16)
    reinterpret_cast<uint16_t *>(rp)[col] = f32_to_bf16_rne(v);
  else
    reinterpret_cast<float *>(rp)[col] = v;
}

// ---------------------------------------------------------------------------
// sigmoid(x) and sigmoid'(x) = s (1 - s) from e = exp(-|x|): no overflow, and no
// cancellation in 1 - s
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : e) / (1.f + e);
}
__device__ __forceinline__ float dsigmoid_stable(float x) {
  const float e = expf(-fabsf(x));
  const float d = 1.f + e;
  return e / (d * d);
}

// ---------------------------------------------------------------------------
// host side: the checks and descriptors of a runtime-dtype operand
// ---------------------------------------------------------------------------
inline bool is_float_dtype(mrec_dtype t) { return t == MREC_F32 || t == MREC_BF16; }
inline int64_t elem_bytes(mrec_dtype t) { return t == MREC_F32 ? 4 : 2; }

// a [rows, >= cols] operand or output with 16-byte aligned rows, which the fragment
// loads can take
inline bool rows16_ok(const void *p, int64_t ld, int64_t cols, mrec_dtype t) {
  return p && ld >= cols && (ld * elem_bytes(t)) % 16 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}
inline MatIn mat_in(const void *p, int64_t ld, mrec_dtype t) {
  return MatIn{static_cast<const char *>(p), ld * elem_bytes(t), t == MREC_BF16};
}
inline MatOut mat_out(void *p, int64_t ld, mrec_dtype t) {
  return MatOut{static_cast<char *>(p), ld * elem_bytes(t), t == MREC_BF16};
}

}  // namespace mrec
