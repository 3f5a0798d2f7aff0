// Device and host helpers shared by the fp32 LSTM translation units: lstm_f32.hip (the recurrent
// kernels) and lstmf_grad.hip (the weight / input gradient GEMMs).  Buffer descriptors and their
// loads / stores, the MFMA wrappers, the exact three-term bf16 split of an fp32 value and its
// six-product chain, the LDS typedefs, and the launch helpers both files use.
#pragma once
#include "common.h"
#include "kernels.h"

#include <mutex>
#include <set>

namespace hfrep {

namespace {

typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef int v4i_t __attribute__((ext_vector_type(4)));
constexpr int kOOB = 0x7fff0000;  // voffset past every descriptor's num_records (see lstm2.hip)

__device__ __forceinline__ rsrc_t make_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
__device__ __forceinline__ float ld1(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void st1(float v, rsrc_t r, int voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, voff, soff, 0);
}
__device__ __forceinline__ f32x4 ld4(rsrc_t r, int voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
}
__device__ __forceinline__ f32x4 ld4s(rsrc_t r, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
// one float4 of an X row of XR floats at byte offset voff (+ soff), columns col .. col + 3: one 16-byte
// load when rows are 16-byte aligned; for XR = 35 (the reference's 35 features, staged as a 36-column
// image) four dword loads with the columns >= XR reading zero -- no byte past the row is addressed
template <int XR>
__device__ __forceinline__ f32x4 ldx4(rsrc_t r, int voff, int soff, int col) {
  if constexpr (XR % 4 == 0) {
    return ld4s(r, voff, soff);
  } else {
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      v[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff != kOOB && col + i < XR ? voff + 4 * i : kOOB, soff, 0));
    return v;
  }
}
__device__ __forceinline__ void st4(f32x4 v, rsrc_t r, int voff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_t, v), r, voff, 0, 0);
}
// 16-byte store at byte offset voff + uoff (uoff uniform) with soffset 0.  A buffer store of more
// than 8 bytes whose data VGPRs the next VALU instruction overwrites needs one wait state, and the
// compiler only inserts it when soffset is NOT a register: with the uniform step offset in soffset
// the BPTT's dZ stores wrote the next value for a few 16-byte chunks per 10^5 rows (rows 14 / 15
// of a 32-row block, r02: profiles/archive_scripts/dbg_large_bwd.py, scripts/isa_store_hazard.py)
__device__ __forceinline__ void st16(f32x4 v, rsrc_t r, bool ok, int voff, int uoff) {
  // (unsigned: voff may already be kOOB; the sum stays past every descriptor's size)
  const int off = (int)((unsigned)voff + (unsigned)uoff);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4i_t, v), r, ok ? off : kOOB, 0, 0);
}

// the fp32 LSTM layer: H units, 4H gate columns, 16-column MFMA tiles per wave, units per wave
constexpr int FH = 100, FG = 400, FNT = 7, FUW = 28;
constexpr int DS_KS = 13;  // the 400 gate columns as 13 k-steps of 32 (k = 400..415 zero)

__device__ __forceinline__ f32x4 mma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma32(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) char lds_char;
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t trunc_hi(float a) { return __builtin_bit_cast(uint32_t, a) & 0xffff0000u; }

// three bf16 planes of four fp32 values, packed two per dword (4 VALU per value + 1.5 perms).  Scalar
// on purpose: the pair form (v_pk_add_f32 for the residuals, 4.5 instructions per value) was slower
// beside the MFMAs -- BPTT 7.96 -> 8.34 ms, K = 100 quad weight gradient 14.6 -> 15.4 ms at B = 262 144
// (profiles/r04_ab: gfx950 issues a packed f32 op at more than the cost of two scalar ones).  Plain
// scalars, no ext_vector elements: clang (ROCm 7.2) compiles __builtin_bit_cast(T, vec[i]) / (T, vec.y)
// as a cast of ELEMENT 0 (profiles/r04_ab/README.md; tests/test_isa_hazards.py lints the sources).
__device__ __forceinline__ void split3(const f32x4 v, uint32_t (&p)[3][2]) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    uint32_t hb[2], mb[2], lb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float a = v[2 * e + k];
      const uint32_t u = __builtin_bit_cast(uint32_t, a), h = u & 0xffff0000u;
      const float r1 = a - __builtin_bit_cast(float, h);
      const uint32_t u1 = __builtin_bit_cast(uint32_t, r1), m = u1 & 0xffff0000u;
      const float r2 = r1 - __builtin_bit_cast(float, m);
      hb[k] = h;
      mb[k] = m;
      lb[k] = __builtin_bit_cast(uint32_t, r2);
    }
    // high halves of (x1, x0) -> x0 in the low 16 bits, x1 in the high 16 bits
    p[0][e] = __builtin_amdgcn_perm(hb[1], hb[0], 0x07060302u);
    p[1][e] = __builtin_amdgcn_perm(mb[1], mb[0], 0x07060302u);
    p[2][e] = __builtin_amdgcn_perm(lb[1], lb[0], 0x07060302u);
  }
}
// the three planes of split3 stored as 8-byte slots at base + q * plane (q = h, m, l); split3_store: both
__device__ __forceinline__ void planes_store(const uint32_t (&p)[3][2], lds_char* base, int plane) {
#pragma unroll
  for (int q = 0; q < 3; ++q)
    *reinterpret_cast<__attribute__((address_space(3))) u32x2_t*>(base + q * plane) = u32x2_t{p[q][0], p[q][1]};
}
__device__ __forceinline__ void split3_store(const f32x4 v, lds_char* base, int plane) {
  uint32_t p[3][2];
  split3(v, p);
  planes_store(p, base, plane);
}

// The six products of the three-term split, a = a[0] + a[1] + a[2] (h, m, l planes) times b likewise, in
// the one fixed order lh, hl, mm, mh, hm, hh (smallest terms first) chained onto c; the dropped terms ml,
// lm, ll are <= 2^-24 |a b|.  Every split consumer calls this, so two kernels that feed it the same
// operands and the same c produce the same bits.  The weight gradients pass a ZERO c per tile and chunk
// and add the result to their running sum in VALU fp32 (round to nearest): chaining the products
// straight into the running sum on the matrix pipe drifted (3 M rows: 0.043 vs 0.014 for the exact
// kernel, consistent with a biased rounding of the MFMA's C addition).
__device__ __forceinline__ f32x4 mma_split6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 c) {
  c = mma32(a[2], b[0], c);  // lh
  c = mma32(a[0], b[2], c);  // hl
  c = mma32(a[1], b[1], c);  // mm
  c = mma32(a[1], b[0], c);  // mh
  c = mma32(a[0], b[1], c);  // hm
  return mma32(a[0], b[0], c);  // hh
}

// ---- host side ----
constexpr size_t F_LDS_MAX = 160 * 1024;
// opt a kernel in to the full 160 KiB of dynamic LDS (once per kernel)
inline void allow_lds(const void* k) {
  static std::mutex mu;
  static std::set<const void*> done;
  std::lock_guard<std::mutex> gd(mu);
  if (done.insert(k).second)
    HFREP_CHECK_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F_LDS_MAX));
}
// Precision modes of the fp32 path.  Default: the fp32-accurate kernels -- products of the recurrences
// (K <= 36 forwards, BPTT), both weight gradients and the K = 100 input gradient as the three-term bf16
// split (each fp32 operand = h + m + l by truncation, six of the nine products on the bf16 MFMA with
// fp32 accumulation; error <= 2x the exact kernel's vs fp64, tests/test_kernels_gpu.py).
// HFREP_FP32_EXACT=1: every product on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, an fmaf chain).
inline bool fp32_exact() { return fp32_exact_mode(); }

}  // namespace

}  // namespace hfrep
