// Fused MLP-GAN passes for gfx950: BASELINE configs 3 / 4 (vanilla GAN, GAN/GAN.py:127-204, and the
// MLP WGAN-GP, GAN/WGAN_GP.py:221-288) as one kernel per pass instead of one kernel per layer.
//
// The layer-by-layer engine (models/layers.py) round-tripped every (B*T, 100) activation and adjoint
// through HBM: 607 GB per bf16 WGAN-GP iteration at 2.3 TB/s (profiles/r06_mlp/baseline).  Here a
// wave owns 32 rows and carries them through every layer of the pass in registers:
//
//  * transposed orientation: a layer output is held as Y^T (features x rows) in f32x16 accumulators,
//    32 features per tile, row = lane & 31; register q of lane half h is feature 8(q>>2) + 4h + (q&3).
//    The next layer sums over that feature index, so the accumulator IS its B operand (CDNA4 guide
//    §3 "An accumulator tile as the next MFMA's operand"): bf16 packs registers 8s..8s+7 into the
//    k-step s fragment of v_mfma_f32_32x32x16_bf16, fp32 feeds register r straight into k-step r of the
//    exact v_mfma_f32_32x32x2_f32.  No LDS round trip between layers.
//  * the weights live in LDS as pre-permuted A-fragment images (one ds_read_b128 / b32 per MFMA, lane
//    linear, conflict free), built per workgroup from the fp32 master weights in the prologue: a
//    forward image A[o][k = i] and, where the pass goes backwards, a dgrad image A[i][k = o], both with
//    the k order of the accumulator map above.
//  * LayerNorm, bias, sigmoid / LeakyReLU and the per-row head dot are register epilogues: a row's
//    features sit in one lane's registers plus its lane ^ 32 partner, so every row reduction is 16
//    in-lane adds and one cross-half swap.
//  * only the pass's inputs and outputs touch HBM: noise / windows in, fake windows, the weight-
//    gradient operands (consumed by the streaming wgrad kernels) and per-wave loss partials out.
//
// The WGAN-GP critic of WGAN_GP.py (Dense(100) -> Dense(100) -> Flatten -> Dense(1), all linear) gets a
// specialised step kernel (mlp_wgp_*): for an affine critic the W-terms on real / fake and the
// reverse-over-tangent of the gradient penalty all have adjoints along the same head vector w3_t, so
// their weight-gradient operands are summed per row before they leave the kernel (X2c, X1c, Y3c
// below) and each weight gets ONE streaming wgrad instead of three.
//
// The clipped WGAN of GAN/WGAN.py:147-205 has the generator's Dense -> LReLU -> LN skeleton in its critic
// (linear Dense layers, per-row Dense(1) head, no Flatten), so its two passes compose the same blocks:
// mlp_wgan_critic (one critic update on one batch with its label: wgrad operands u1 / dz2 / dz1, LayerNorm
// and head gradients as per-wave column-sum slabs) and mlp_wgan_critic_dx (the generator step's dfake).
//
// The same critic trained with the gradient penalty (zoo (mlp_ln, wgan_gp)) is not affine, so its penalty is a
// per-row second-order pass: mlp_lngp_norm (g = ds/dx_hat and its squared norm per row) and mlp_lngp_critic
// (tangent forward along v = c_b g, then the reverse over primal and tangent through both LayerNorms).
#pragma once
#include "common.h"
#include "kernels.h"
#include "mfma.h"
#include "mlp.h"

#include <algorithm>
#include <stdexcept>
#include <type_traits>

namespace hfrep {

// fp32 storage with the products on the bf16 matrix pipe: every operand as three exact bf16 planes
// (hi / mid / lo by truncation, 8 mantissa bits each) and 6 of the 9 plane products (the dropped ones
// are < 2^-24 of the product) on v_mfma_f32_32x32x16_bf16 -- the LSTM fp32 kernels' split (lstm_f32.hip
// split3; error within 2x the exact kernel's vs fp64).  Policy tag f32s_t: k-step geometry of bf16.
struct f32s_t {};
struct F3 {
  bf16x8 h, m, l;
};
template <> struct MF<f32s_t> {
  typedef F3 frag;
  // small terms first: the fp32 accumulator rounds them before the large ones arrive
  __device__ __forceinline__ static f32x16 mma(const frag& a, const frag& b, f32x16 c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, c, 0, 0, 0);
  }
};
__device__ __forceinline__ F3 split_f3(const float (&v)[8]) {
  F3 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = v[j];  // (a scalar copy first: tests/test_isa_hazards.py bit_cast lint)
    const uint32_t u = __builtin_bit_cast(uint32_t, a), hb = u & 0xffff0000u;
    const float r1 = a - __builtin_bit_cast(float, hb);
    const uint32_t mb = __builtin_bit_cast(uint32_t, r1) & 0xffff0000u;
    const float r2 = r1 - __builtin_bit_cast(float, mb);
    f.h[j] = (short)(hb >> 16);
    f.m[j] = (short)(mb >> 16);
    f.l[j] = (short)(__builtin_bit_cast(uint32_t, r2) >> 16);
  }
  return f;
}

namespace {

constexpr int MLP_WAVES = 4;  // waves per workgroup (one per SIMD; up to 512 registers per wave)
constexpr int MLP_THREADS = 64 * MLP_WAVES;
constexpr int VEC = 128;      // padded length of every per-feature vector in LDS
constexpr float LN_EPS_F = 1e-3f, LRELU_ALPHA_F = 0.2f, KERAS_EPS_F = 1e-7f;

__device__ __forceinline__ int featq(int q, int h) { return 8 * (q >> 2) + 4 * h + (q & 3); }

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------
// precision policies: k-step structure of the two MFMA forms over the accumulator feature map
// ---------------------------------------------------------------------------------------------------
template <typename T> struct MP;

template <> struct MP<bf16_t> {
  typedef bf16x8 frag;
  static constexpr int steps(int K) { return (K + 15) / 16; }
  // input feature of element e (0..7) of k-step s, lane half h
  __device__ __forceinline__ static int feat(int s, int e, int h) { return 32 * (s >> 1) + featq(8 * (s & 1) + e, h); }
  __device__ __forceinline__ static frag bop(const f32x16* a, int s) {
    const f32x16& t = a[s >> 1];
    const int o = 8 * (s & 1);
    const u32x4_t u = {pk2bf(t[o], t[o + 1]), pk2bf(t[o + 2], t[o + 3]), pk2bf(t[o + 4], t[o + 5]),
                       pk2bf(t[o + 6], t[o + 7])};
    return __builtin_bit_cast(frag, u);
  }
  template <class G> __device__ __forceinline__ static frag make(G get) {
    const u32x4_t u = {pk2bf(get(0), get(1)), pk2bf(get(2), get(3)), pk2bf(get(4), get(5)), pk2bf(get(6), get(7))};
    return __builtin_bit_cast(frag, u);
  }
};

template <> struct MP<float> {
  typedef float frag;
  // k-steps over K features: whole 32-feature tiles take 16, the last partial tile the prefix of
  // registers whose lane-half-0 feature is < K (featq(r, 0) increases with r)
  static constexpr int steps(int K) {
    int n = 16 * (K / 32);
    const int rem = K % 32;
    for (int r = 0; r < 16; ++r)
      if (rem && 8 * (r >> 2) + (r & 3) < rem) ++n;
    return n;
  }
  __device__ __forceinline__ static int feat(int s, int /*e*/, int h) { return 32 * (s >> 4) + featq(s & 15, h); }
  __device__ __forceinline__ static frag bop(const f32x16* a, int s) { return a[s >> 4][s & 15]; }
  template <class G> __device__ __forceinline__ static frag make(G get) { return get(0); }
};

template <> struct MP<f32s_t> {
  typedef F3 frag;
  static constexpr int steps(int K) { return (K + 15) / 16; }
  __device__ __forceinline__ static int feat(int s, int e, int h) { return MP<bf16_t>::feat(s, e, h); }
  __device__ __forceinline__ static frag bop(const f32x16* a, int s) {
    const f32x16& t = a[s >> 1];
    const int o = 8 * (s & 1);
    const float v[8] = {t[o], t[o + 1], t[o + 2], t[o + 3], t[o + 4], t[o + 5], t[o + 6], t[o + 7]};
    return split_f3(v);
  }
  template <class G> __device__ __forceinline__ static frag make(G get) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = get(j);
    return split_f3(v);
  }
};

// ---------------------------------------------------------------------------------------------------
// LDS images (built by the whole workgroup in the prologue)
// ---------------------------------------------------------------------------------------------------
// forward image of W (K x N, row-major fp32): entry (t, s) = A fragment rows o = 32 t .. +31, k-step s
template <typename T, int K, int N>
__device__ void build_fwd(typename MP<T>::frag* img, const float* __restrict__ W) {
  constexpr int S = MP<T>::steps(K), NT = (N + 31) / 32;
  for (int e = threadIdx.x; e < NT * S * 64; e += blockDim.x) {
    const int lane = e & 63, idx = e >> 6, t = idx / S, s = idx - t * S;
    const int o = 32 * t + (lane & 31), h = lane >> 5;
    img[e] = MP<T>::make([&](int j) {
      const int i = MP<T>::feat(s, j, h);
      return (i < K && o < N) ? W[i * N + o] : 0.f;
    });
  }
}
// dgrad image of W (K x N): entry (t, s) = A fragment rows i = 32 t .. +31 (input features), k-step s
// over the N output features
template <typename T, int K, int N>
__device__ void build_dgrad(typename MP<T>::frag* img, const float* __restrict__ W) {
  constexpr int S = MP<T>::steps(N), NT = (K + 31) / 32;
  for (int e = threadIdx.x; e < NT * S * 64; e += blockDim.x) {
    const int lane = e & 63, idx = e >> 6, t = idx / S, s = idx - t * S;
    const int i = 32 * t + (lane & 31), h = lane >> 5;
    img[e] = MP<T>::make([&](int j) {
      const int o = MP<T>::feat(s, j, h);
      return (i < K && o < N) ? W[i * N + o] : 0.f;
    });
  }
}
template <typename T, int K, int N> constexpr int fwd_entries() { return ((N + 31) / 32) * MP<T>::steps(K); }
template <typename T, int K, int N> constexpr int dgrad_entries() { return ((K + 31) / 32) * MP<T>::steps(N); }
template <typename T> constexpr int frag_bytes() { return 64 * (int)sizeof(typename MP<T>::frag); }

__device__ void load_vec(float* dst, const float* __restrict__ src, int n) {
  for (int i = threadIdx.x; i < VEC; i += blockDim.x) dst[i] = (src && i < n) ? src[i] : 0.f;
}

// ---------------------------------------------------------------------------------------------------
// register-level building blocks
// ---------------------------------------------------------------------------------------------------
// out[t] = sum over the KIN input features of img (t, s) x in: one output tile per 32 features of NOUT
// The A fragments of step s + 1 are read while step s's MFMAs issue; the scheduling barrier per step
// keeps hipcc from hoisting the whole image into registers (it did: 208 VGPRs for the fp32 100 x 100
// layer, and spills everywhere).
template <typename T, int KIN, int NOUT>
__device__ __forceinline__ void dense(const f32x16* in, f32x16* out, const typename MP<T>::frag* img, int lane) {
  constexpr int S = MP<T>::steps(KIN), NT = (NOUT + 31) / 32;
  typedef typename MP<T>::frag Fr;
  Fr cur[NT], nxt[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    out[t] = zero16();
    cur[t] = img[(t * S) * 64 + lane];
  }
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s + 1 < S) {
#pragma unroll
      for (int t = 0; t < NT; ++t) nxt[t] = img[(t * S + s + 1) * 64 + lane];
    }
    const Fr b = MP<T>::bop(in, s);
#pragma unroll
    for (int t = 0; t < NT; ++t) out[t] = MF<T>::mma(cur[t], b, out[t]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NT; ++t) cur[t] = nxt[t];
  }
}

// 4 consecutive elements of a row (feature f0 .. f0 + 3), as floats
template <typename T> struct Q4;
template <> struct Q4<bf16_t> {
  __device__ __forceinline__ static float4 ld(const bf16_t* p) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                       __uint_as_float(v.y & 0xffff0000u));
  }
  __device__ __forceinline__ static void st(bf16_t* p, float a, float b, float c, float d) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pk2bf(a, b), pk2bf(c, d));
  }
};
template <> struct Q4<float> {
  __device__ __forceinline__ static float4 ld(const float* p) { return *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ static void st(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
  }
};

// rows (M x K row-major) -> accumulator layout (zeros past M / K)
template <typename T, int K>
__device__ __forceinline__ void load_rows(f32x16* a, const T* __restrict__ x, int64_t row, int64_t M, int h) {
  constexpr int NT = (K + 31) / 32;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < M && f0 < K) v = Q4<T>::ld(x + row * K + f0);
      a[t][4 * g] = v.x; a[t][4 * g + 1] = v.y; a[t][4 * g + 2] = v.z; a[t][4 * g + 3] = v.w;
    }
}
template <typename T, int N>
__device__ __forceinline__ void store_rows(T* __restrict__ y, int64_t row, int64_t M, const f32x16* a, int h) {
  constexpr int NT = (N + 31) / 32;
  if (row >= M) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      if (f0 < N) Q4<T>::st(y + row * N + f0, a[t][4 * g], a[t][4 * g + 1], a[t][4 * g + 2], a[t][4 * g + 3]);
    }
}
// a per-row head vector (w: this row's N weights, fp32) scaled by `sc`, in accumulator layout
template <int N>
__device__ __forceinline__ void head_rows(f32x16* a, const float* __restrict__ w, float sc, bool ok, int h) {
  constexpr int NT = (N + 31) / 32;
  const float* wh = w + 4 * h;  // lane-half base: the per-(t, g) offsets below fold into immediates
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok && f0 < N) v = *reinterpret_cast<const float4*>(wh + 32 * t + 8 * g);
      a[t][4 * g] = sc * v.x; a[t][4 * g + 1] = sc * v.y; a[t][4 * g + 2] = sc * v.z; a[t][4 * g + 3] = sc * v.w;
    }
}
// sum_f a[row, f] * w[f] for this lane's row (both lane halves get the total)
template <int N>
__device__ __forceinline__ float rowdot(const f32x16* a, const float* __restrict__ w, bool ok, int h) {
  constexpr int NT = (N + 31) / 32;
  const float* wh = w + 4 * h;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      if (ok && f0 < N) {
        const float4 v = *reinterpret_cast<const float4*>(wh + 32 * t + 8 * g);
        s = fmaf(a[t][4 * g], v.x, s); s = fmaf(a[t][4 * g + 1], v.y, s);
        s = fmaf(a[t][4 * g + 2], v.z, s); s = fmaf(a[t][4 * g + 3], v.w, s);
      }
    }
  return s + __shfl_xor(s, 32, 64);
}
// a = act(a + b) on features < N, 0 past N (b: LDS vector)
template <int N>
__device__ __forceinline__ void bias_act(f32x16* a, const float* b, int act, int h) {
  constexpr int NT = (N + 31) / 32;
  const float* bh = b + 4 * h;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      const float4 bv = *reinterpret_cast<const float4*>(bh + 32 * t + 8 * g);
      const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = a[t][4 * g + e] + bb[e];
        v = act == ACT_SIGMOID ? sigmoidf_(v) : v;
        a[t][4 * g + e] = f0 + e < N ? v : 0.f;
      }
    }
}
template <int N>
__device__ __forceinline__ void axpy(f32x16* y, float s, const f32x16* x) {
#pragma unroll
  for (int t = 0; t < (N + 31) / 32; ++t) y[t] += s * x[t];
}
__device__ __forceinline__ float lrelu(float v) { return v >= 0.f ? v : LRELU_ALPHA_F * v; }

// LeakyReLU then LayerNorm (eps 1e-3, biased variance) of this lane's row, in place; a holds the
// activation outputs with zeros past N.  Returns the row statistics.
template <int N>
__device__ __forceinline__ void lrelu_ln(f32x16* a, const float* gam, const float* bet, int h, float& mean,
                                         float& rstd) {
  constexpr int NT = (N + 31) / 32;
  const float *gh = gam + 4 * h, *beh = bet + 4 * h;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      a[t][q] = lrelu(a[t][q]);
      s += a[t][q];
    }
  s += __shfl_xor(s, 32, 64);
  mean = s * (1.f / N);
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float d = 32 * t + featq(q, h) < N ? a[t][q] - mean : 0.f;
      v = fmaf(d, d, v);
    }
  v += __shfl_xor(v, 32, 64);
  rstd = 1.f / sqrtf(v * (1.f / N) + LN_EPS_F);
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int f0 = 32 * t + 8 * g + 4 * h;
      const float4 gv = *reinterpret_cast<const float4*>(gh + 32 * t + 8 * g),
                   bv = *reinterpret_cast<const float4*>(beh + 32 * t + 8 * g);
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = (a[t][4 * g + e] - mean) * rstd * gg[e] + bb[e];
        a[t][4 * g + e] = f0 + e < N ? u : 0.f;
      }
    }
}

// Sum over the 32 rows of one lane half of every feature of tile v (transpose-reduce butterfly: 16
// shuffles instead of 80).  Lane l ends with the column sum of register q(l) = 8 b4 + 4 b3 + 2 b2 + b1
// (bk = bit k of l), i.e. feature featq(q(l), h); lanes l and l ^ 1 hold the same value.
// The element reads go through an empty asm: otherwise InstCombine folds select(b, v[8 + i], v[i]) into
// a DYNAMIC extractelement v[b ? 8 + i : i], which the backend lowers as a 16-way v_cmp / v_cndmask
// chain per element (16 live lane masks, spilled to VGPR lanes: 100 VALU per MFMA in mlp_gen_bwd_w).
__device__ __forceinline__ float opaque(float x) {
  asm("" : "+v"(x));
  return x;
}
__device__ __forceinline__ float colsum(const f32x16& v, int lane) {
  float a8[8], a4[4], a2[2];
  bool b = lane & 16;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float lo = opaque(v[i]), hi = opaque(v[8 + i]);
    a8[i] = (b ? hi : lo) + __shfl_xor(b ? lo : hi, 16, 64);
  }
  b = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) a4[i] = (b ? a8[4 + i] : a8[i]) + __shfl_xor(b ? a8[i] : a8[4 + i], 8, 64);
  b = lane & 4;
#pragma unroll
  for (int i = 0; i < 2; ++i) a2[i] = (b ? a4[2 + i] : a4[i]) + __shfl_xor(b ? a4[i] : a4[2 + i], 4, 64);
  b = lane & 2;
  float a1 = (b ? a2[1] : a2[0]) + __shfl_xor(b ? a2[0] : a2[1], 2, 64);
  return a1 + __shfl_xor(a1, 1, 64);
}
__device__ __forceinline__ int colsum_q(int lane) {
  return (((lane >> 4) & 1) << 3) | (((lane >> 3) & 1) << 2) | (((lane >> 2) & 1) << 1) | ((lane >> 1) & 1);
}

// per-wave partial sums -> slab row of this wave
__device__ __forceinline__ void slab_put(float* slab, int L, int k, float v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) slab[((int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6)) * L + k] = v;
}

// Keras binary cross-entropy on a probability p with label y, its p-gradient scaled by inv
// (zero where the [eps, 1 - eps] clip is active): the gan_loss kind-1 contract (ops/reference.py)
__device__ __forceinline__ void bce(float p, float y, float inv, float& lo, float& g) {
  const float o = fminf(fmaxf(p, KERAS_EPS_F), 1.f - KERAS_EPS_F);
  lo = -(y * __logf(o + KERAS_EPS_F) + (1.f - y) * __logf(1.f - o + KERAS_EPS_F));
  const bool inside = p > KERAS_EPS_F && p < 1.f - KERAS_EPS_F;
  g = inside ? -(y / (o + KERAS_EPS_F) - (1.f - y) / (1.f - o + KERAS_EPS_F)) * inv : 0.f;
}

#define MLP_LOOP                                                                                               \
  const int lane = threadIdx.x & 63, h = lane >> 5;                                                            \
  const int64_t ntile = (M + 31) / 32;                                                                         \
  for (int64_t tile = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6); tile < ntile;                      \
       tile += (int64_t)gridDim.x * MLP_WAVES)


// LayerNorm -> LeakyReLU -> sigmoid reverse of one row (the generator's Dense(sigmoid) + LReLU + LN
// blocks): g = dL/du (LN output gradient), y = the sigmoid outputs, (mean, rstd) of lrelu(y); writes
// dL/dz into out (may alias g or y: element-wise after the row sums) and adds the gamma-gradient
// column sums (sum_r g * xhat) into pg.  ACT = ACT_LINEAR: the clip critic's Dense(linear) + LReLU + LN
// blocks (y = the Dense outputs, no sigmoid factor); PG = false: no parameter gradients (pg unused).
template <int N, int ACT = ACT_SIGMOID, bool PG = true>
__device__ __forceinline__ void ln_reverse(const f32x16* g, const f32x16* y, f32x16* out, const float* gam, float mean,
                                           float rstd, int h, int lane, float* pg) {
  constexpr int NT = (N + 31) / 32;
  const float* gh = gam + 4 * h;
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int f0 = 32 * t + 8 * gq + 4 * h;
      const float4 gv = *reinterpret_cast<const float4*>(gh + 32 * t + 8 * gq);
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * gq + e;
        const bool in = f0 + e < N;
        const float xh = in ? (lrelu(y[t][q]) - mean) * rstd : 0.f;
        const float gd = in ? g[t][q] * gg[e] : 0.f;
        m1 += gd;
        m2 = fmaf(gd, xh, m2);
      }
    }
  m1 += __shfl_xor(m1, 32, 64);
  m2 += __shfl_xor(m2, 32, 64);
  m1 *= 1.f / N;
  m2 *= 1.f / N;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x16 px;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int f0 = 32 * t + 8 * gq + 4 * h;
      const float4 gv = *reinterpret_cast<const float4*>(gh + 32 * t + 8 * gq);
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * gq + e;
        const bool in = f0 + e < N;
        const float yv = y[t][q];
        const float xh = in ? (lrelu(yv) - mean) * rstd : 0.f;
        const float dv = in ? g[t][q] : 0.f;
        px[q] = dv * xh;
        float dl = rstd * (dv * gg[e] - m1 - xh * m2);
        dl *= yv >= 0.f ? 1.f : LRELU_ALPHA_F;
        if constexpr (ACT == ACT_SIGMOID) out[t][q] = in ? dl * yv * (1.f - yv) : 0.f;
        else out[t][q] = in ? dl : 0.f;
      }
    }
    if constexpr (PG) pg[t] += colsum(px, lane);
  }
}

// ---------------------------------------------------------------------------------------------------
// LDS plan of one pass: [weight images in the listed order][NV vectors of VEC floats][tail blocks].  The
// kernel takes its pointers and the launcher its dynamic-LDS byte count from the same instantiation, and
// the size and alignment checks run for every plan that is launched.
// ---------------------------------------------------------------------------------------------------
// images of layer L's weight (1: F x H, 2: H x H, 3: H x F): Fwd = build_fwd's, Dgrad = build_dgrad's
template <int L> struct Fwd {};
template <int L> struct Dgrad {};
template <typename P, int F, int H, typename I> struct Img;
template <typename P, int F, int H, int L> struct Img<P, F, H, Fwd<L>> {
  static constexpr int K = L == 1 ? F : H, N = L == 3 ? F : H, layer = L, entries = fwd_entries<P, K, N>();
  __device__ __forceinline__ static int count() { return fwd_entries<P, K, N>(); }
  __device__ __forceinline__ static void build(typename MP<P>::frag* img, const float* W) { build_fwd<P, K, N>(img, W); }
};
template <typename P, int F, int H, int L> struct Img<P, F, H, Dgrad<L>> {
  static constexpr int K = L == 1 ? F : H, N = L == 3 ? F : H, layer = L, entries = dgrad_entries<P, K, N>();
  __device__ __forceinline__ static int count() { return dgrad_entries<P, K, N>(); }
  __device__ __forceinline__ static void build(typename MP<P>::frag* img, const float* W) { build_dgrad<P, K, N>(img, W); }
};
// what follows the vectors: blocks of B bytes each (staging buffers, per-wave accumulators)
template <size_t... B> struct Tail {
  static constexpr size_t bytes = (B + ... + (size_t)0);
  static constexpr bool aligned = ((B % 16 == 0) && ...);
  template <int K> static constexpr size_t off() {
    size_t o = 0;
    int k = 0;
    ((o += k++ < K ? B : 0), ...);
    return o;
  }
};
template <typename P, int F, int H, int NV, typename TAIL, typename... I> struct MlpLds {
  using Fr = typename MP<P>::frag;
  static constexpr int NF = F, NH = H, NVEC = NV;
  template <typename Q> static constexpr size_t img_bytes = (size_t)Img<P, F, H, Q>::entries * frag_bytes<P>();
  static constexpr size_t vec_off = (img_bytes<I> + ... + (size_t)0);
  static constexpr size_t tail_off = vec_off + (size_t)NV * VEC * sizeof(float);
  static constexpr size_t bytes = tail_off + TAIL::bytes;
  static_assert(bytes <= 160 * 1024, "LDS plan exceeds the 160 KB of a workgroup");
  static_assert(vec_off % 16 == 0 && tail_off % 16 == 0 && TAIL::aligned, "16-byte aligned LDS blocks");
  // position of image Q in the plan
  template <typename Q> static constexpr int index() {
    static_assert((std::is_same_v<Q, I> || ...), "image not in this plan");
    int k = 0;
    bool hit = false;
    ((hit = hit || std::is_same_v<Q, I>, k += hit ? 0 : 1), ...);
    return k;
  }
  // The pointers of one workgroup, stepped image by image from the LDS base with the entry counts as calls
  // (not as constants folded into one offset per image): hipcc's code for the row loop depends on when these
  // offsets become constants, and this is the form the kernels were tuned with.
  struct Ptrs {
    Fr* image[sizeof...(I)];
    float* vec;
    template <typename Q> __device__ __forceinline__ const Fr* img() const { return image[index<Q>()]; }
    template <int K> __device__ __forceinline__ unsigned char* tail() const {
      return reinterpret_cast<unsigned char*>(vec + NV * VEC) + TAIL::template off<K>();
    }
  };
  __device__ __forceinline__ static Ptrs ptrs(unsigned char* lds) {
    Ptrs r;
    Fr* p = reinterpret_cast<Fr*>(lds);
    int k = 0;
    ((r.image[k++] = p, p += Img<P, F, H, I>::count() * 64), ...);
    r.vec = reinterpret_cast<float*>(p);
    return r;
  }
  // builds every image from its layer's weight W[layer - 1], in plan order
  __device__ __forceinline__ static Ptrs build(unsigned char* lds, const float* const (&W)[3]) {
    const Ptrs r = ptrs(lds);
    int k = 0;
    (Img<P, F, H, I>::build(r.image[k++], W[Img<P, F, H, I>::layer - 1]), ...);
    return r;
  }
};

// vector slots.  The Dense -> LReLU -> LN stacks (generator, clip critic); slot 6 is the generator's b3 or
// the clip critic's head w3
enum { V_B1, V_G1, V_BE1, V_B2, V_G2, V_BE2, V_B3, V_W3 = V_B3 };
// the affine critic and the GAN discriminator; A_D, A_G: mlp_gan_dx's D = W2 w3 and g = W1 D
enum { A_B1, A_B2, A_W3, A_D, A_G };

// prologues: build the plan's images, load its vectors, barrier
template <class Lds, class W>  // W: MlpGen or MlpClip (the same Dense -> LReLU -> LN parameters up to slot 5)
__device__ __forceinline__ void load_ln_vecs(float* vec, const W& w) {
  constexpr int H = Lds::NH;
  load_vec(vec + V_B1 * VEC, w.b1, H); load_vec(vec + V_G1 * VEC, w.g1, H); load_vec(vec + V_BE1 * VEC, w.be1, H);
  load_vec(vec + V_B2 * VEC, w.b2, H); load_vec(vec + V_G2 * VEC, w.g2, H); load_vec(vec + V_BE2 * VEC, w.be2, H);
}
template <class Lds> __device__ __forceinline__ typename Lds::Ptrs mlp_prologue(unsigned char* lds, const MlpGen& g) {
  const float* const W[3] = {g.W1, g.W2, g.W3};
  const auto p = Lds::build(lds, W);
  load_ln_vecs<Lds>(p.vec, g);
  if constexpr (Lds::NVEC > V_B3) load_vec(p.vec + V_B3 * VEC, g.b3, Lds::NF);
  __syncthreads();
  return p;
}
template <class Lds> __device__ __forceinline__ typename Lds::Ptrs mlp_prologue(unsigned char* lds, const MlpClip& c) {
  const float* const W[3] = {c.W1, c.W2, nullptr};
  const auto p = Lds::build(lds, W);
  load_ln_vecs<Lds>(p.vec, c);
  load_vec(p.vec + V_W3 * VEC, c.w3, Lds::NH);
  __syncthreads();
  return p;
}
template <class Lds> __device__ __forceinline__ typename Lds::Ptrs mlp_prologue(unsigned char* lds, const MlpCritic& c) {
  const float* const W[3] = {c.W1, c.W2, nullptr};
  const auto p = Lds::build(lds, W);
  float* vec = p.vec;
  if constexpr (Lds::NVEC > A_B2) {
    load_vec(vec + A_B1 * VEC, c.b1, Lds::NH);
    load_vec(vec + A_B2 * VEC, c.b2, Lds::NH);
  }
  if constexpr (Lds::NVEC > A_W3) load_vec(vec + A_W3 * VEC, c.w3, Lds::NH);
  __syncthreads();
  return p;
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
template <typename KER>
int mlp_grid(KER kern, size_t lds, int64_t M) {
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), MLP_THREADS, lds) !=
          hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  const int64_t ntile = (M + 31) / 32;
  const int64_t want = (ntile + MLP_WAVES - 1) / MLP_WAVES;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cu_count() * std::min(per_cu, 2)));
}

template <typename KER>
void set_lds(KER kern, size_t lds) {
  if (lds > 64 * 1024)
    HFREP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
}

// Launch of one pass with its plan's LDS.  GRID_TILES: one wave per 32-row tile of n rows, at most two
// workgroups per CU (mlp_grid); GRID_SLAB: exactly mlp_slab_rows(n) / MLP_WAVES workgroups (the passes that
// write a per-wave slab row); GRID_BLOCKS: n workgroups.
enum GridKind { GRID_TILES, GRID_SLAB, GRID_BLOCKS };
template <class Lds, typename KER, typename... A>
void mlp_launch(KER kern, GridKind kind, int64_t n, hipStream_t s, A... args) {
  constexpr size_t lds = Lds::bytes;
  set_lds(kern, lds);
  const int grid = kind == GRID_TILES ? mlp_grid(kern, lds, n) : kind == GRID_SLAB ? mlp_slab_rows(n) / MLP_WAVES : (int)n;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(MLP_THREADS), lds, s, args...);
}

// dispatch over (dtype, F); only the widths of mlp_supported are instantiated (H = 100)
#define MLP_DISPATCH(dt, F, H, ...)                                                          \
  do {                                                                                       \
    if (!mlp_supported(F, H)) throw std::runtime_error("mlp: (F, H) is not instantiated");   \
    if (dt == DT_BF16) {                                                                     \
      using T = bf16_t;                                                                      \
      if (F == 32) { constexpr int FF = 32; __VA_ARGS__ }                                    \
      else { constexpr int FF = 36; __VA_ARGS__ }                                            \
    } else {                                                                                 \
      using T = float;                                                                       \
      if (F == 32) { constexpr int FF = 32; __VA_ARGS__ }                                    \
      else { constexpr int FF = 36; __VA_ARGS__ }                                            \
    }                                                                                        \
  } while (0)

}  // namespace
}  // namespace hfrep
