// Fused MLP-GAN passes for gfx950 (see mlp_dev.h): the LReLU + LayerNorm critic, clipped and under the gradient penalty
#include "mlp_dev.h"

namespace hfrep {

// ===================================================================================================
// clipped WGAN critic (GAN/WGAN.py:147-158): per row Dense(H) -> LReLU -> LN -> Dense(H) -> LReLU -> LN
// -> Dense(1); W loss mean over the M rows of label * s_r (label -1 real, +1 fake; loop :166-205)
// ===================================================================================================
// LDS plans: forward W1 / W2 and dgrad W2 images (+ dgrad W1 for the input gradient) and the seven vectors
// b1 | gamma1 | beta1 | b2 | gamma2 | beta2 | w3; TAIL: the accumulators of mlp_lngp_critic
template <typename T, int F, int H, typename TAIL = Tail<>>
using ClipLds = MlpLds<T, F, H, 7, TAIL, Fwd<1>, Fwd<2>, Dgrad<2>>;
template <typename T, int F, int H> using ClipDxLds = MlpLds<T, F, H, 7, Tail<>, Fwd<1>, Fwd<2>, Dgrad<2>, Dgrad<1>>;

// this lane's row through the critic: x -> u2 (in a), the Dense 2 outputs z2 (in y2), the row statistics
// of both LayerNorms and the score s (without b3).  U1: also store u1 = LN1's output (X operand of gW2).
template <typename T, int F, int H, bool U1>
__device__ __forceinline__ float clip_forward(const f32x16* x, f32x16* a, f32x16* y2,
                                              const typename MP<T>::frag* f1, const typename MP<T>::frag* f2,
                                              const float* vec, T* __restrict__ u1o, int64_t row, int64_t M, int lane,
                                              int h, float& mean1, float& rstd1, float& mean2, float& rstd2) {
  constexpr int NTH = (H + 31) / 32;
  dense<T, F, H>(x, a, f1, lane);
  bias_act<H>(a, vec + V_B1 * VEC, ACT_LINEAR, h);
  lrelu_ln<H>(a, vec + V_G1 * VEC, vec + V_BE1 * VEC, h, mean1, rstd1);
  if constexpr (U1) store_rows<T, H>(u1o, row, M, a, h);
  dense<T, H, H>(a, y2, f2, lane);
  bias_act<H>(y2, vec + V_B2 * VEC, ACT_LINEAR, h);
#pragma unroll
  for (int t = 0; t < NTH; ++t) a[t] = y2[t];
  lrelu_ln<H>(a, vec + V_G2 * VEC, vec + V_BE2 * VEC, h, mean2, rstd2);
  return rowdot<H>(a, vec + V_W3 * VEC, true, h);
}

// One critic update's gradients on one batch x with `label`: ds_r = label / M for every row.  Writes
// the streaming weight-gradient operands u1 (X of gW2), dz2 (dY of gW2), dz1 (dY of gW1; its X is x),
// the per-wave LayerNorm partials (lnslab rows: dgamma1 | dbeta1 | dgamma2 | dbeta2, as mlp_gen_bwd), the
// per-wave head partials (hslab rows: gw3 = sum_r ds_r u2_r (H) | gb3 = sum_r ds_r) and the loss slab
// (column 0: sum_r label * s_r).  Rows past M carry ds = 0: every adjoint of theirs is zero.  y1 is
// recomputed in the reverse (register budget, as mlp_gen_bwd).
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_wgan_critic_kernel(const T* __restrict__ x, MlpClip c, float label,
                                                                      T* __restrict__ u1o, T* __restrict__ dz2o,
                                                                      T* __restrict__ dz1o, float* __restrict__ lnslab,
                                                                      float* __restrict__ hslab,
                                                                      float* __restrict__ slab, int64_t M, float inv) {
  using Lds = ClipLds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>();
  const float* vec = lp.vec;
  const float b3 = c.b3[0];
  const float* gam1 = vec + V_G1 * VEC;
  const float* gam2 = vec + V_G2 * VEC;
  float pg1[NTH], pb1[NTH], pg2[NTH], pb2[NTH], pw3[NTH];  // per-lane column sums (see colsum)
#pragma unroll
  for (int t = 0; t < NTH; ++t) pg1[t] = pb1[t] = pg2[t] = pb2[t] = pw3[t] = 0.f;
  float acc = 0.f, sds = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    const float ds = ok ? label * inv : 0.f;
    f32x16 xr[NTF], a[NTH], y2[NTH], d[NTH];
    float mean1, rstd1, mean2, rstd2;
    // ---- forward (u1 out; z2 and the row statistics kept)
    load_rows<T, F>(xr, x, row, M, h);
    const float sc =
        clip_forward<T, F, H, true>(xr, a, y2, f1, f2, vec, u1o, row, M, lane, h, mean1, rstd1, mean2, rstd2) + b3;
    if (ok && h == 0) {
      acc += label * sc;
      sds += ds;
    }
    // ---- head: gw3 += ds u2; du2 = ds w3 (rank 1)
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      a[t] *= ds;
      pw3[t] += colsum(a[t], lane);
    }
    head_rows<H>(d, vec + V_W3 * VEC, ds, ok, h);
    // ---- LN2 / LReLU reverse -> dz2
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb2[t] += colsum(d[t], lane);
    ln_reverse<H, ACT_LINEAR>(d, y2, d, gam2, mean2, rstd2, h, lane, pg2);
    store_rows<T, H>(dz2o, row, M, d, h);
    // ---- du1 = dz2 W2^T; recompute y1; LN1 / LReLU reverse -> dz1
    dense<T, H, H>(d, y2, d2, lane);  // y2 now holds du1
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb1[t] += colsum(y2[t], lane);
    dense<T, F, H>(xr, a, f1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_LINEAR, h);  // y1
    ln_reverse<H, ACT_LINEAR>(y2, a, a, gam1, mean1, rstd1, h, lane, pg1);
    store_rows<T, H>(dz1o, row, M, a, h);
  }
  // per-wave partials: lanes with bit 0 clear own feature featq(colsum_q(lane), h) of every tile
  const int64_t wv = (int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6);
  float* out = lnslab + wv * 4 * H;
  float* hout = hslab + wv * (H + 1);
  if ((lane & 1) == 0) {
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      const int f = 32 * t + featq(colsum_q(lane), h);
      if (f < H) {
        out[f] = pg1[t];
        out[H + f] = pb1[t];
        out[2 * H + f] = pg2[t];
        out[3 * H + f] = pb2[t];
        hout[f] = pw3[t];
      }
    }
  }
  sds = wave_sum(sds);
  if (lane == 0) hout[H] = sds;
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// This lane's row from x (in xr) down to the input gradient (xr <- ds * d s / d x, ds = the score's adjoint):
// the forward, then the reverse through both LayerNorms without parameter gradients.  Returns the score
// (without b3).  Shared by mlp_wgan_critic_dx and mlp_lngp_norm (plan ClipDxLds).
template <typename T, int F, int H>
__device__ __forceinline__ float clip_dx_row(f32x16* xr, const T* __restrict__ x,
                                             const typename ClipDxLds<T, F, H>::Ptrs& lp, float ds, int64_t row,
                                             int64_t M, bool ok, int lane, int h) {
  constexpr int NTH = (H + 31) / 32;
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>(),
             *d1 = lp.template img<Dgrad<1>>();
  const float* vec = lp.vec;
  f32x16 a[NTH], y2[NTH], d[NTH];
  float mean1, rstd1, mean2, rstd2;
  const float sc = clip_forward<T, F, H, false>(xr, a, y2, f1, f2, vec, static_cast<T*>(nullptr), row, M, lane, h, mean1,
                                                rstd1, mean2, rstd2);
  head_rows<H>(d, vec + V_W3 * VEC, ds, ok, h);  // du2
  ln_reverse<H, ACT_LINEAR, false>(d, y2, d, vec + V_G2 * VEC, mean2, rstd2, h, lane, nullptr);
  dense<T, H, H>(d, y2, d2, lane);  // du1
  load_rows<T, F>(xr, x, row, M, h);  // (reloaded, not held across the reverse: register budget)
  dense<T, F, H>(xr, a, f1, lane);
  bias_act<H>(a, vec + V_B1 * VEC, ACT_LINEAR, h);  // y1
  ln_reverse<H, ACT_LINEAR, false>(y2, a, a, vec + V_G1 * VEC, mean1, rstd1, h, lane, nullptr);
  dense<T, H, F>(a, xr, d1, lane);  // dx
  return sc;
}

// The generator step's dfake through the frozen critic: the same forward, ds_r = -1 / M (loss
// mean(-s)), reverse down to dx = dz1 W1^T.  No parameter gradients.  slab column 0: sum_r -s_r.
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_wgan_critic_dx_kernel(const T* __restrict__ x, MlpClip c,
                                                                         T* __restrict__ dx, float* __restrict__ slab,
                                                                         int64_t M, float inv) {
  constexpr int NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<ClipDxLds<T, F, H>>(lds, c);
  const float b3 = c.b3[0];
  float acc = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    f32x16 xr[NTF];
    load_rows<T, F>(xr, x, row, M, h);
    const float sc = clip_dx_row<T, F, H>(xr, x, lp, -inv, row, M, ok, lane, h) + b3;
    if (ok && h == 0) acc -= sc;
    store_rows<T, F>(dx, row, M, xr, h);
  }
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// ===================================================================================================
// the LReLU + LayerNorm critic under the gradient penalty (model (mlp_ln, wgan_gp)): the W terms are two
// mlp_wgan_critic launches; the penalty adds a first-order pass (mlp_lngp_norm) and the reverse over the
// tangent (mlp_lngp_critic).  Per row, with phi = LReLU, m = phi'(z), xh = (phi(z) - mean) rstd:
//   z1 = x W1 + b1, u1 = gamma1 xh1 + beta1, z2 = u1 W2 + b2, u2 = gamma2 xh2 + beta2, s = u2 . w3 + b3
// ===================================================================================================
// First-order pass: g = ds/dx_hat of every row (mlp_wgan_critic_dx with ds = 1) and its squared norm,
// summed from the fp32 registers before g is rounded to T.  gsq is per row: a sample's T rows may lie in
// different waves and workgroups; mlp_wgp_coef sums them.  xc: a copy of x (the row block in front of g in
// one (2 M, F) buffer, so that [x_hat; g] is one weight-gradient operand; see mlp_lngp_critic).
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_lngp_norm_kernel(const T* __restrict__ x, MlpClip c,
                                                                    T* __restrict__ xc, T* __restrict__ g,
                                                                    float* __restrict__ gsq, int64_t M) {
  constexpr int NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<ClipDxLds<T, F, H>>(lds, c);
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    f32x16 xr[NTF];
    load_rows<T, F>(xr, x, row, M, h);
    store_rows<T, F>(xc, row, M, xr, h);
    clip_dx_row<T, F, H>(xr, x, lp, 1.f, row, M, ok, lane, h);  // g (du2 = w3)
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NTF; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) s = fmaf(xr[t][q], xr[t][q], s);
    s += __shfl_xor(s, 32, 64);
    if (ok && h == 0) gsq[row] = s;
    store_rows<T, F>(g, row, M, xr, h);
  }
}

// An LDS vector re-read at every use: the per-feature vectors never change after the prologue, so without
// this every read of gamma / beta / bias / w3 in the tile loop is recognised as loop invariant and hoisted
// (7 vectors x 64 registers per lane), which spills in the kernel that already holds four H-vectors.
template <typename V>
__device__ __forceinline__ const V* reread(const V* p) {
  int z = 0;
  asm volatile("" : "+v"(z));
  return p + z;
}
// row statistics of LayerNorm(LReLU(z)) without forming its output (z: Dense outputs, zeros past N)
template <int N>
__device__ __forceinline__ void lrelu_stats(const f32x16* z, int h, float& mean, float& rstd) {
  constexpr int NT = (N + 31) / 32;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) s += lrelu(z[t][q]);
  s += __shfl_xor(s, 32, 64);
  mean = s * (1.f / N);
  float v = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float d = 32 * t + featq(q, h) < N ? lrelu(z[t][q]) - mean : 0.f;
      v = fmaf(d, d, v);
    }
  v += __shfl_xor(v, 32, 64);
  rstd = 1.f / sqrtf(v * (1.f / N) + LN_EPS_F);
}

// LReLU + LayerNorm tangent of one row, in place: zd = the Dense tangent z' on entry and
//   u' = gamma rstd (a' - mean(a') - xh mean(xh a')),  a' = m z'
// on exit (the closed form of misc.hip layernorm_tfwd_kernel); z: the Dense outputs, (mean, rstd) of lrelu(z).
template <int N>
__device__ __forceinline__ void ln_tangent(const f32x16* z, f32x16* zd, const float* gam, float mean, float rstd,
                                           int h) {
  constexpr int NT = (N + 31) / 32;
  const float* gh = gam + 4 * h;
  float sa = 0.f, sx = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const bool in = 32 * t + featq(q, h) < N;
      const float zv = z[t][q];
      const float xh = in ? (lrelu(zv) - mean) * rstd : 0.f;
      const float ad = in ? (zv >= 0.f ? 1.f : LRELU_ALPHA_F) * zd[t][q] : 0.f;
      zd[t][q] = ad;
      sa += ad;
      sx = fmaf(xh, ad, sx);
    }
  sa += __shfl_xor(sa, 32, 64);
  sx += __shfl_xor(sx, 32, 64);
  sa *= 1.f / N;
  sx *= 1.f / N;
  const float nmr = -mean * rstd;  // (xh in its fma form below: see ln_treverse_t)
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
        const float xh = fmaf(lrelu(z[t][q]), rstd, nmr);
        const float ad = zd[t][q];
        zd[t][q] = in ? gg[e] * rstd * (ad - sa - xh * sx) : 0.f;
      }
    }
}

// Reverse of that block over primal and tangent (the closed form of misc.hip layernorm_tbwd_kernel, per row
// in registers), in two steps so that only three H-vectors are worked on at a time.  With z the Dense
// outputs, z' the Dense tangent, U / Ud the adjoints of the block's primal / tangent outputs u / u',
// p = gamma Ud, gu = gamma U, a' = m z', q = mean(xh a'), t' = a' - mean(a') - xh q and
// J(w) = rstd (w - mean(w) - xh mean(xh w)) the LayerNorm Jacobian (symmetric):
//   adjoint of a' = J(p)
//   adjoint of a  = J(gu + w) - rstd^2 xh mean(p t'),  w = -rstd (q p + mean(p xh) a')
// (w and the last term: u' depends on the primal through xh and rstd).  LReLU has no second derivative off
// the kink, so both adjoints pass through it as m.  Rows past M carry Ud = U = 0 and z' = 0: all zero.
constexpr int LNGP_ACC = 6;  // column-sum accumulators of mlp_lngp_critic (VEC floats each, per wave)
template <typename T, int F, int H>
using LngpLds = ClipLds<T, F, H, Tail<MLP_WAVES * LNGP_ACC * VEC * sizeof(float)>>;
// acc[feature] += the colsum() value this lane owns (lanes l and l ^ 1 hold the same one: the even lane adds)
__device__ __forceinline__ void col_add(float* acc, int t, float v, int lane, int h) {
  if ((lane & 1) == 0) acc[32 * t + featq(colsum_q(lane), h)] += v;
}
struct LnT {
  float mw, mwx, r2;  // mean(w), mean(w xh), rstd^2 mean(p t')
};
// Tangent step.  In: z, zd = z', Ud.  Out: zd <- the adjoint of z'; pg += column sums of the gamma gradient's
// tangent part Ud rstd t' (= Ud u' / gamma, division free); W3: pw += column sums of u' (the head's gradient,
// layer 2).  FIN (no primal adjoint U, layer 2): z <- the adjoint of z.  Otherwise Ud <- w and the row
// scalars are returned for ln_treverse_p.
template <int N, bool FIN, bool W3>
__device__ __forceinline__ LnT ln_treverse_t(f32x16* z, f32x16* zd, f32x16* Ud, const float* gam, float mean,
                                             float rstd, int h, int lane, float* pg, float* pw) {
  constexpr int NT = (N + 31) / 32;
  const float* gh = gam + 4 * h;
  float sa = 0.f, sq = 0.f, sp = 0.f, spx = 0.f, spa = 0.f;
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
        const float zv = z[t][q];
        const float xh = in ? (lrelu(zv) - mean) * rstd : 0.f;
        const float ad = in ? (zv >= 0.f ? 1.f : LRELU_ALPHA_F) * zd[t][q] : 0.f;
        const float p = in ? gg[e] * Ud[t][q] : 0.f;
        zd[t][q] = ad;
        sa += ad;
        sq = fmaf(xh, ad, sq);
        sp += p;
        spx = fmaf(p, xh, spx);
        spa = fmaf(p, ad, spa);
      }
    }
  sa += __shfl_xor(sa, 32, 64);
  sq += __shfl_xor(sq, 32, 64);
  sp += __shfl_xor(sp, 32, 64);
  spx += __shfl_xor(spx, 32, 64);
  spa += __shfl_xor(spa, 32, 64);
  // The second pass must not reuse the first one's per-element values: xh and p kept in registers are two
  // more live H-vectors, and the kernel spills.  So a' went back into zd above, gamma is read again, and xh
  // is formed as one fma (another expression than the first pass's: not merged with it; 1 ulp apart).
  gh = reread(gh);
  const float nmr = -mean * rstd;
  constexpr float iN = 1.f / N;
  sa *= iN; sq *= iN; sp *= iN; spx *= iN; spa *= iN;
  LnT r;
  r.mw = -rstd * (sq * sp + spx * sa);
  r.mwx = -2.f * rstd * sq * spx;
  r.r2 = rstd * rstd * (spa - sa * sp - sq * spx);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x16 px, ud;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
      const int f0 = 32 * t + 8 * gq + 4 * h;
      const float4 gv = *reinterpret_cast<const float4*>(gh + 32 * t + 8 * gq);
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = 4 * gq + e;
        const bool in = f0 + e < N;
        const float zv = z[t][q];
        const float m = zv >= 0.f ? 1.f : LRELU_ALPHA_F;
        const float xh = in ? fmaf(lrelu(zv), rstd, nmr) : 0.f;
        const float ad = zd[t][q];
        const float udv = in ? Ud[t][q] : 0.f;
        const float p = gg[e] * udv;
        const float tt = in ? rstd * (ad - sa - xh * sq) : 0.f;  // rstd t' = u' / gamma
        const float wv = -rstd * (sq * p + spx * ad);
        px[q] = udv * tt;
        if constexpr (W3) ud[q] = gg[e] * tt;
        zd[t][q] = in ? m * rstd * (p - sp - xh * spx) : 0.f;
        if constexpr (FIN) z[t][q] = in ? m * (rstd * (wv - r.mw - xh * r.mwx) - r.r2 * xh) : 0.f;
        else Ud[t][q] = wv;
      }
    }
    col_add(pg, t, colsum(px, lane), lane, h);
    if constexpr (W3) col_add(pw, t, colsum(ud, lane), lane, h);
  }
  return r;
}
// Primal step.  In: z, U, w (from ln_treverse_t) and its row scalars.  Out: z <- the adjoint of z;
// pg += column sums of the gamma gradient's primal part U xh.
template <int N>
__device__ __forceinline__ void ln_treverse_p(f32x16* z, const f32x16* U, const f32x16* w, const LnT& r,
                                              const float* gam, float mean, float rstd, int h, int lane, float* pg) {
  constexpr int NT = (N + 31) / 32;
  const float* gh = gam + 4 * h;
  float sg = 0.f, sgx = 0.f;
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
        const float xh = in ? (lrelu(z[t][q]) - mean) * rstd : 0.f;
        const float gu = in ? gg[e] * U[t][q] : 0.f;
        sg += gu;
        sgx = fmaf(gu, xh, sgx);
      }
    }
  sg += __shfl_xor(sg, 32, 64);
  sgx += __shfl_xor(sgx, 32, 64);
  gh = reread(gh);  // (as in ln_treverse_t)
  const float nmr = -mean * rstd;
  const float mx = sg * (1.f / N) + r.mw, mxx = sgx * (1.f / N) + r.mwx;
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
        const float zv = z[t][q];
        const float m = zv >= 0.f ? 1.f : LRELU_ALPHA_F;
        const float xh = in ? fmaf(lrelu(zv), rstd, nmr) : 0.f;
        const float uv = in ? U[t][q] : 0.f;
        const float xb = fmaf(gg[e], uv, w[t][q]);
        px[q] = uv * xh;
        z[t][q] = in ? m * (rstd * (xb - mx - xh * mxx) - r.r2 * xh) : 0.f;
      }
    }
    col_add(pg, t, colsum(px, lane), lane, h);
  }
}

// The penalty's parameter gradient: d/dtheta sum_r s'_r, s'_r the tangent of the critic at x_hat_r along
// v_r = c_b g_r (v held fixed; mlp_wgp_coef's c_b carries 2 lambda / B and the norm factor).
//   tangent forward: z1' = v W1, u1' = LN1'(m1 z1'), z2' = u1' W2, u2' = LN2'(m2 z2'), s' = u2' . w3
//   reverse from (adjoint of u2' = w3, adjoint of u2 = 0): ln_treverse_t at LN2, dgrad W2 of both adjoint
//   streams, ln_treverse_t and ln_treverse_p at LN1 (now with a primal adjoint too).  No input gradient.
// Writes the streaming weight-gradient operands (T): u1, u1d = u1' (X of gW2), dz2, dzt2 (dY of gW2),
// dz1, dzt1 (dY of gW1; X = x_hat and g):
//   gW2 = u1^T dz2 + u1d^T dzt2,  gW1 = x_hat^T dz1 + g^T dzt1
// with dzt1 = c_b * (adjoint of z1'), so its X operand is g itself and v never goes to HBM.  The host passes
// each pair as the two row blocks of one (2 M, .) buffer: one streaming product of 2 M rows per weight.  The
// bias gradients gb1 = sum dz1, gb2 = sum dz2 are column sums here (of the primal rows only, in fp32 before
// the operands are rounded), not the products' bias column, which would add the tangent rows.
// lnslab rows (one per wave): dgamma1 | dbeta1 | dgamma2 | gw3 = sum u2' | gb1 | gb2 (dbeta2 = 0: u2 has no
// adjoint; b3 gets nothing).
// Register budget: at most four H-vectors are live (256 of the wave's 512 registers; the VALU reaches only
// the 256 architectural ones), and the element-wise steps work on three.  So z1 and z1' are re-formed from
// x_hat and g for the LN1 reverse (as mlp_wgan_critic recomputes y1), dz2 is read back from the operand just
// stored for its dgrad instead of waiting in registers through LN1's tangent step (same lane, same
// addresses, program order; the bf16 product rounds it to bf16 either way), and the six column-sum
// accumulators live in LDS (6 VEC floats per wave, each feature owned by one lane) instead of 24 registers.
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_lngp_critic_kernel(
    const T* __restrict__ x, const T* __restrict__ g, const float* __restrict__ cvec, MlpClip c, T* __restrict__ u1o,
    T* __restrict__ u1do, T* __restrict__ dz2o, T* __restrict__ dzt2o, T* __restrict__ dz1o, T* __restrict__ dzt1o,
    float* __restrict__ lnslab, int64_t M, int Tn) {
  using Lds = LngpLds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>();
  float* vec = lp.vec;
  const float* gam1 = vec + V_G1 * VEC;
  const float* gam2 = vec + V_G2 * VEC;
  // this wave's column sums dgamma1 | dbeta1 | dgamma2 | gw3 | gb1 | gb2 (see col_add; written and read by
  // this wave only)
  float* accb = reinterpret_cast<float*>(lp.template tail<0>()) + (threadIdx.x >> 6) * LNGP_ACC * VEC;
  for (int i = threadIdx.x & 63; i < LNGP_ACC * VEC; i += 64) accb[i] = 0.f;
  MLP_LOOP {
    float* acc = const_cast<float*>(reread(accb));
    float *pg1 = acc, *pb1 = acc + VEC, *pg2 = acc + 2 * VEC, *pw3 = acc + 3 * VEC;
    float *pz1 = acc + 4 * VEC, *pz2 = acc + 5 * VEC;
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    const float cb = ok ? cvec[row / Tn] : 0.f;
    f32x16 xr[NTF], p0[NTH], p1[NTH], p2[NTH], p3[NTH];
    float mean1, rstd1, mean2, rstd2;
    // ---- layer 1, primal and tangent: p0 = z1, p1 = u1, p2 = z1' -> u1'
    load_rows<T, F>(xr, x, row, M, h);
    dense<T, F, H>(xr, p0, f1, lane);
    bias_act<H>(p0, reread(vec + V_B1 * VEC), ACT_LINEAR, h);
#pragma unroll
    for (int t = 0; t < NTH; ++t) p1[t] = p0[t];
    lrelu_ln<H>(p1, reread(vec + V_G1 * VEC), reread(vec + V_BE1 * VEC), h, mean1, rstd1);
    store_rows<T, H>(u1o, row, M, p1, h);
    load_rows<T, F>(xr, g, row, M, h);
#pragma unroll
    for (int t = 0; t < NTF; ++t) xr[t] *= cb;  // v
    dense<T, F, H>(xr, p2, f1, lane);
    ln_tangent<H>(p0, p2, reread(gam1), mean1, rstd1, h);
    store_rows<T, H>(u1do, row, M, p2, h);
    // ---- layer 2: p0 = z2, p3 = z2'
    dense<T, H, H>(p1, p0, f2, lane);
    bias_act<H>(p0, reread(vec + V_B2 * VEC), ACT_LINEAR, h);
    dense<T, H, H>(p2, p3, f2, lane);
    lrelu_stats<H>(p0, h, mean2, rstd2);
    // ---- LN2 / LReLU reverse over primal and tangent: p0 <- dz2, p3 <- dzt2
    head_rows<H>(p1, reread(vec + V_W3 * VEC), 1.f, ok, h);  // adjoint of u2' = w3 (0 on the rows past M)
    ln_treverse_t<H, true, true>(p0, p3, p1, reread(gam2), mean2, rstd2, h, lane, pg2, pw3);
    store_rows<T, H>(dz2o, row, M, p0, h);
    store_rows<T, H>(dzt2o, row, M, p3, h);
#pragma unroll
    for (int t = 0; t < NTH; ++t) col_add(pz2, t, colsum(p0[t], lane), lane, h);
    // ---- LN1 / LReLU reverse, tangent step first: p2 = adjoint of u1', z1 and z1' again (p1, p3); then
    // p3 <- adjoint of z1', p2 <- w
    dense<T, H, H>(p3, p2, d2, lane);
    load_rows<T, F>(xr, x, row, M, h);
    dense<T, F, H>(xr, p1, f1, lane);
    bias_act<H>(p1, reread(vec + V_B1 * VEC), ACT_LINEAR, h);
    load_rows<T, F>(xr, g, row, M, h);
#pragma unroll
    for (int t = 0; t < NTF; ++t) xr[t] *= cb;
    dense<T, F, H>(xr, p3, f1, lane);
    const LnT lt = ln_treverse_t<H, false, false>(p1, p3, p2, reread(gam1), mean1, rstd1, h, lane, pg1, nullptr);
#pragma unroll
    for (int t = 0; t < NTH; ++t) p3[t] *= cb;
    store_rows<T, H>(dzt1o, row, M, p3, h);
    // ---- primal step: p3 = adjoint of u1 = dz2 W2^T (dz2 back from its operand; the opaque row offset keeps
    // the stored registers from being forwarded to the load, i.e. held); p1 <- dz1
    {
      int zz = 0;
      asm volatile("" : "+v"(zz));
      load_rows<T, H>(p0, dz2o, row + zz, M + zz, h);
    }
    dense<T, H, H>(p0, p3, d2, lane);
#pragma unroll
    for (int t = 0; t < NTH; ++t) col_add(pb1, t, colsum(p3[t], lane), lane, h);
    ln_treverse_p<H>(p1, p3, p2, lt, reread(gam1), mean1, rstd1, h, lane, pg1);
    store_rows<T, H>(dz1o, row, M, p1, h);
#pragma unroll
    for (int t = 0; t < NTH; ++t) col_add(pz1, t, colsum(p1[t], lane), lane, h);
  }
  // per-wave partials: lanes with bit 0 clear own feature featq(colsum_q(lane), h) of every tile
  float* out = lnslab + ((int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6)) * LNGP_ACC * H;
  if ((lane & 1) == 0) {
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      const int f = 32 * t + featq(colsum_q(lane), h);
      if (f < H) {
#pragma unroll
        for (int k = 0; k < LNGP_ACC; ++k) out[k * H + f] = accb[k * VEC + f];
      }
    }
  }
}

// ===================================================================================================
// host launchers (both dtypes; fp32 on the exact products: the split planes of the three 100-wide images
// alone are 196 KB)
// ===================================================================================================
void launch_mlp_wgan_critic(int dt, const void* x, const MlpClip& cr, float label, void* u1, void* dz2, void* dz1,
                            float* lnslab, float* hslab, float* slab, int64_t M, int F, int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<ClipLds<T, FF, 100>>(mlp_wgan_critic_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, label, (T*)u1,
                                    (T*)dz2, (T*)dz1, lnslab, hslab, slab, M, 1.f / (float)M);
  });
}

void launch_mlp_wgan_critic_dx(int dt, const void* x, const MlpClip& cr, void* dx, float* slab, int64_t M, int F,
                               int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<ClipDxLds<T, FF, 100>>(mlp_wgan_critic_dx_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, (T*)dx,
                                      slab, M, 1.f / (float)M);
  });
}

void launch_mlp_lngp_norm(int dt, const void* x, const MlpClip& cr, void* xc, void* g, float* gsq, int64_t M, int F,
                          int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<ClipDxLds<T, FF, 100>>(mlp_lngp_norm_kernel<T, FF, 100>, GRID_TILES, M, s, (const T*)x, cr, (T*)xc, (T*)g,
                                      gsq, M);
  });
}

void launch_mlp_lngp_critic(int dt, const void* x, const void* g, const float* c, const MlpClip& cr, void* u1,
                            void* u1d, void* dz2, void* dzt2, void* dz1, void* dzt1, float* lnslab, float* gg1,
                            float* gbe1, float* gg2, float* gw3, float* gb1, float* gb2, int64_t M, int Tn, int F, int H,
                            hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<LngpLds<T, FF, 100>>(mlp_lngp_critic_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, (const T*)g, c, cr,
                                    (T*)u1, (T*)u1d, (T*)dz2, (T*)dzt2, (T*)dz1, (T*)dzt1, lnslab, M, Tn);
  });
  // fixed-order sums of the per-wave rows [dgamma1 | dbeta1 | dgamma2 | gw3 | gb1 | gb2] into the gradients
  const int P = mlp_slab_rows(M), L = 100;
  launch_mlp_slab_sum_segs(lnslab, P, (int64_t)LNGP_ACC * L, 0, L, 4, gg1, gbe1, gg2, gw3, s);
  launch_mlp_slab_sum_segs(lnslab, P, (int64_t)LNGP_ACC * L, 4 * L, L, 2, gb1, gb2, nullptr, nullptr, s);
}
int mlp_lngp_slab_cols(int H) { return LNGP_ACC * H; }

}  // namespace hfrep
