// Fused MLP-GAN passes for gfx950 (see mlp_dev.h): the affine WGAN-GP critic and the GAN discriminator
#include "mlp_dev.h"

namespace hfrep {

// ===================================================================================================
// WGAN-GP critic (GAN/WGAN_GP.py:238-253): D(x) = sum_t ((x_t W1 + b1) W2 + b2) . w3_t + b3
// ===================================================================================================
// First-order GP pass: g = dD/dx at every row (for an affine critic it does not depend on x:
// dh2 = w3_t, dh1 = W2 dh2, g = W1 dh1) and its squared norm per row.
template <typename T, int F, int H> using WgpNormLds = MlpLds<T, F, H, 0, Tail<>, Dgrad<2>, Dgrad<1>>;
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_wgp_norm_kernel(MlpCritic c, float* __restrict__ gsq, int64_t M,
                                                                   int Tn) {
  using Lds = WgpNormLds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *d2 = lp.template img<Dgrad<2>>(), *d1 = lp.template img<Dgrad<1>>();
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    const int tr = ok ? (int)(row % Tn) : 0;
    f32x16 a[NTH], b[NTH], gg[NTF];
    head_rows<H>(a, c.w3 + (int64_t)tr * H, 1.f, ok, h);
    dense<T, H, H>(a, b, d2, lane);
    dense<T, H, F>(b, gg, d1, lane);
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < NTF; ++t)
#pragma unroll
      for (int q = 0; q < 16; ++q) s = fmaf(gg[t][q], gg[t][q], s);
    s += __shfl_xor(s, 32, 64);
    if (ok && h == 0) gsq[row] = s;
  }
}

// per sample: |g_b| from the T row norms, c_b = -(2 lam / B)(1 - |g_b|) / |g_b| (the gp_coef adjoint,
// ops/reference.py); epart[block] = sum over the block's samples of (1 - |g_b|)^2 (fixed order)
__global__ void __launch_bounds__(256) mlp_wgp_coef_kernel(const float* __restrict__ gsq, int Tn, int64_t B, float lam,
                                                           float* __restrict__ c, float* __restrict__ epart) {
  __shared__ float red[4];
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  float e = 0.f;
  if (b < B) {
    float s = 0.f;
    for (int t = 0; t < Tn; ++t) s += gsq[b * Tn + t];
    const float n = sqrtf(s);
    c[b] = -(2.f * lam / (float)B) * (1.f - n) / fmaxf(n, 1e-30f);
    e = (1.f - n) * (1.f - n);
  }
  e = wave_sum(e);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) epart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One GP critic update's device work per row (b, t):
//   W terms: dL/ds_b = -1/B (real), +1/B (fake)  ->  dh2 = +-w3_t / B, dh1 = +-W2 w3_t / B
//   GP term (reverse over the tangent along v = c_b g): zd1 = v W1, zd2 = zd1 W2; seeds dzd2 = w3_t,
//   dzd1 = W2 w3_t
// Every adjoint of layer 2 is along w3_t and every adjoint of layer 1 along dh1' = W2 w3_t, so each
// weight needs one product with a per-row combined operand:
//   gW2 += X2c^T dY2,  X2c = (h1_fake - h1_real) / B + zd1,  dY2 = w3_t
//   gW1 += X1c^T dY1,  X1c = (x_fake - x_real) / B + v,      dY1 = dh1' = W2 w3_t
//   gw3_t += sum_b Y3c,  Y3c = (h2_fake - h2_real) / B + zd2 = X2c W2   (the b2 terms cancel)
// The bias gradients cancel exactly (-1/B and +1/B per row pair; the tangent has none).  slab: per-wave
// sums of h2 . w3_t over the real and the fake rows (the two W losses).
// the four images of the affine critic and b1 | b2 (mlp_wgp_critic, mlp_wgp_critic_t, mlp_critic_dx)
template <typename T, int F, int H> using Critic4Lds = MlpLds<T, F, H, 2, Tail<>, Fwd<1>, Fwd<2>, Dgrad<2>, Dgrad<1>>;
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_wgp_critic_kernel(
    const T* __restrict__ real, const T* __restrict__ fake, const float* __restrict__ cvec, MlpCritic c,
    T* __restrict__ X2c, T* __restrict__ dY2, T* __restrict__ X1c, T* __restrict__ dY1, T* __restrict__ Y3c,
    float* __restrict__ slab, int64_t M, int Tn, float invB) {
  using Lds = Critic4Lds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>(),
             *d1 = lp.template img<Dgrad<1>>();
  const float* vec = lp.vec;
  float sr = 0.f, sf = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    const int64_t bidx = ok ? row / Tn : 0;
    const float* w3t = c.w3 + (int64_t)(ok ? row - bidx * Tn : 0) * H;
    f32x16 A[NTH], Bv[NTH], X2[NTH], X1[NTF], x[NTF];
    // ---- GP tangent stream
    head_rows<H>(A, w3t, 1.f, ok, h);
    store_rows<T, H>(dY2, row, M, A, h);
    dense<T, H, H>(A, Bv, d2, lane);           // dh1' = W2 w3_t
    store_rows<T, H>(dY1, row, M, Bv, h);
    dense<T, H, F>(Bv, X1, d1, lane);          // g = W1 dh1'
    const float cb = ok ? cvec[bidx] : 0.f;
#pragma unroll
    for (int t = 0; t < NTF; ++t) X1[t] *= cb;  // v
    dense<T, F, H>(X1, X2, f1, lane);          // zd1 = v W1
    // ---- W terms: real (-1/B) then fake (+1/B)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const float sg = pass ? invB : -invB;
      load_rows<T, F>(x, pass ? fake : real, row, M, h);
      axpy<F>(X1, sg, x);
      dense<T, F, H>(x, A, f1, lane);
      bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);      // h1
      axpy<H>(X2, sg, A);
      dense<T, H, H>(A, Bv, f2, lane);
      bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);  // h2
      const float sc = rowdot<H>(Bv, w3t, ok, h);
      if (ok && h == 0) {
        if (pass) sf += sc;
        else sr += sc;
      }
    }
    store_rows<T, F>(X1c, row, M, X1, h);
    store_rows<T, H>(X2c, row, M, X2, h);
    dense<T, H, H>(X2, A, f2, lane);           // Y3c = X2c W2
    store_rows<T, H>(Y3c, row, M, A, h);
  }
  slab_put(slab, 2, 0, sr);
  slab_put(slab, 2, 1, sf);
}

// ---------------------------------------------------------------------------------------------------
// The same critic update with the weight gradients taken in the kernel by per-t column sums (any dtype;
// the fallback where mlp_affine_supported is false).
//
// Rows are walked t-major: wave wid owns t = wid % Tn and takes 32-SAMPLE tiles (rows b T + t,
// b = 32 bt + lane) of that t only.  Every adjoint of such a tile lies along the same vectors (w3_t
// for layer 2, dh1'_t = W2 w3_t for layer 1), so
//   gW2 = sum_t S2[t] (x) w3_t,  gW1 = sum_t S1[t] (x) dh1'_t,  gw3_t = S3[t],
//   S1[t] = sum_b X1c[b, t],  S2[t] = sum_b X2c[b, t],  S3[t] = sum_b Y3c[b, t]
// (X1c, X2c, Y3c the per-row operands of mlp_wgp_critic, computed here in registers as there).  Each
// tile adds its transpose-reduce column sums to ~10 per-lane registers; a wave writes one slab row
// [S1 F | S2 H | S3 H] for its t at the end, and mlp_wgp_tsum_finish reduces the rows of each t in a
// fixed order and forms the outer products.  No per-row operand leaves the kernel.
// ---------------------------------------------------------------------------------------------------
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_wgp_critic_t_kernel(
    const T* __restrict__ real, const T* __restrict__ fake, const float* __restrict__ cvec, MlpCritic c,
    float* __restrict__ tslab, float* __restrict__ slab, int64_t Bn, int Tn, int kper, float invB) {
  using Lds = Critic4Lds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>(),
             *d1 = lp.template img<Dgrad<1>>();
  const float* vec = lp.vec;
  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int wid = blockIdx.x * MLP_WAVES + (threadIdx.x >> 6);
  const int tt = wid % Tn, j = wid / Tn;  // this wave's t and its index among the kper waves of that t
  const float* w3t = c.w3 + (int64_t)tt * H;
  float s1[NTF], s2[NTH], s3[NTH];
#pragma unroll
  for (int i = 0; i < NTF; ++i) s1[i] = 0.f;
#pragma unroll
  for (int i = 0; i < NTH; ++i) s2[i] = s3[i] = 0.f;
  float sr = 0.f, sf = 0.f;
  const int64_t nbt = (Bn + 31) / 32;
  for (int64_t bt = j; j < kper && bt < nbt; bt += kper) {
    const int64_t b = bt * 32 + (lane & 31);
    const bool ok = b < Bn;
    const int64_t row = ok ? b * Tn + tt : 0;
    const int64_t M = ok ? row + 1 : 0;  // load_rows' bound: the lane's own row only
    f32x16 A[NTH], Bv[NTH], X2[NTH], X1[NTF], x[NTF];
    head_rows<H>(A, w3t, 1.f, true, h);
    dense<T, H, H>(A, Bv, d2, lane);            // dh1' = W2 w3_t
    dense<T, H, F>(Bv, X1, d1, lane);           // g = W1 dh1'
    const float cb = ok ? cvec[b] : 0.f;
#pragma unroll
    for (int i = 0; i < NTF; ++i) X1[i] *= cb;  // v
    dense<T, F, H>(X1, X2, f1, lane);           // zd1 = v W1
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const float sg = pass ? invB : -invB;
      load_rows<T, F>(x, pass ? fake : real, row, M, h);
      axpy<F>(X1, sg, x);
      dense<T, F, H>(x, A, f1, lane);
      bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);       // h1
      axpy<H>(X2, sg, A);
      dense<T, H, H>(A, Bv, f2, lane);
      bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);  // h2
      const float sc = rowdot<H>(Bv, w3t, ok, h);
      if (ok && h == 0) {
        if (pass) sf += sc;
        else sr += sc;
      }
    }
    if (!ok) {  // samples past B contribute nothing
#pragma unroll
      for (int i = 0; i < NTH; ++i) X2[i] = zero16();
#pragma unroll
      for (int i = 0; i < NTF; ++i) X1[i] = zero16();
    }
    dense<T, H, H>(X2, A, f2, lane);            // Y3c = X2c W2
#pragma unroll
    for (int i = 0; i < NTF; ++i) s1[i] += colsum(X1[i], lane);
#pragma unroll
    for (int i = 0; i < NTH; ++i) {
      s2[i] += colsum(X2[i], lane);
      s3[i] += colsum(A[i], lane);
    }
  }
  // this wave's per-t partial sums (lanes l, l ^ 1 hold the same column): row wid of tslab
  constexpr int L = F + 2 * H;
  float* out = tslab + (int64_t)wid * L;
  const int fq = featq(colsum_q(lane), h);
  if ((lane & 1) == 0) {
#pragma unroll
    for (int i = 0; i < NTF; ++i)
      if (32 * i + fq < F) out[32 * i + fq] = s1[i];
#pragma unroll
    for (int i = 0; i < NTH; ++i)
      if (32 * i + fq < H) {
        out[F + 32 * i + fq] = s2[i];
        out[F + H + 32 * i + fq] = s3[i];
      }
  }
  slab_put(slab, 2, 0, sr);
  slab_put(slab, 2, 1, sf);
}

// (1) S[t][col] = the fixed-order sum of the kper slab rows of t (rows wid = t + Tn j), and
// D[t][o] = dh1'_t[o] = sum_k W2[o][k] w3_t[k]: tsum = [Tn][L = F + 2 H] then [Tn][H]
__global__ void __launch_bounds__(256) mlp_wgp_tsum_prep_kernel(const float* __restrict__ tslab, MlpCritic c, int F,
                                                                int H, int Tn, int kper, float* __restrict__ tsum) {
  const int L = F + 2 * H;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < Tn * L) {
    const int t = e / L, col = e - t * L;
    float a = 0.f;
    for (int jj = 0; jj < kper; ++jj) a += tslab[(int64_t)(t + Tn * jj) * L + col];
    tsum[e] = a;
  } else if (e < Tn * L + Tn * H) {
    const int q = e - Tn * L, t = q / H, o = q - t * H;
    float d = 0.f;
    for (int k = 0; k < H; ++k) d = fmaf(c.W2[o * H + k], c.w3[t * H + k], d);
    tsum[e] = d;
  }
}
// (2) gW1 += sum_t S1[t] (x) D[t], gW2 += sum_t S2[t] (x) w3_t, gw3_t += S3[t]: one output per thread
__global__ void __launch_bounds__(256) mlp_wgp_tsum_finish_kernel(const float* __restrict__ tsum, MlpCritic c, int F,
                                                                  int H, int Tn, float* __restrict__ gW1,
                                                                  float* __restrict__ gW2, float* __restrict__ gw3) {
  const int L = F + 2 * H;
  const float* D = tsum + Tn * L;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n1 = F * H, n2 = H * H, n3 = Tn * H;
  if (e < n1) {
    const int i = e / H, o = e - i * H;
    float acc = 0.f;
    for (int t = 0; t < Tn; ++t) acc = fmaf(tsum[t * L + i], D[t * H + o], acc);
    gW1[e] += acc;
  } else if (e < n1 + n2) {
    const int q = e - n1, i = q / H, o = q - i * H;
    float acc = 0.f;
    for (int t = 0; t < Tn; ++t) acc = fmaf(tsum[t * L + F + i], c.w3[t * H + o], acc);
    gW2[q] += acc;
  } else if (e < n1 + n2 + n3) {
    const int q = e - n1 - n2, t = q / H, o = q - t * H;
    gw3[q] += tsum[t * L + F + H + o];
  }
}

// ---------------------------------------------------------------------------------------------------
// The affine critic's update from batch sums (mlp_wgp_affine, default; GAN/WGAN_GP.py:238-253, loop
// :255-288).  D(x) = sum_t ((x_t W1 + b1) W2 + b2) . w3_t + b3 is affine in x, so
//   * its input gradient g_t = W1 W2 w3_t is a function of t alone: every sample has the same |g|, the
//     same GP coefficient c = -(2 lam / B)(1 - |g|) / |g| and the same tangent v_t = c g_t;
//   * the per-row operands of mlp_wgp_critic_t enter the gradients only through their sums over the
//     batch, and those are linear in the per-t sums of the inputs (sum_b (x_b W) = (sum_b x_b) W):
//       S1[t] = d_t / B + B v_t,  d_t = sum_b (fake - real)[b, t]
//       S2[t] = S1[t] W1                       (= (d_t W1) / B + B v_t W1: b1 cancels in d)
//       S3[t] = S2[t] W2
//     and the W-loss score sums are sum_t (s_t W1 + B b1) . (W2 w3_t) + B b2 . w3_t.
// So the update reads each input once (mlp_bt_colsum: per-t column sums, HBM-bound) and finishes in
// fp32 in one workgroup; mlp_wgp_tsum_finish forms the T outer products as for mlp_wgp_critic_t.  Same
// gradient and loss pack as the per-row path up to fp32 summation order (and without its bf16 rounding
// of h1 / h2 in the bf16 build).  mode 1 is the generator step's critic input gradient: the per-t
// dfake row -g_t / B (broadcast over the batch by mlp_bcast_rows) and the fake score sum.
// ---------------------------------------------------------------------------------------------------

// part[p][k][col] = sum over rows r = p, p + P, ... < B of y_k[r][col]; y_0 = x0, y_1 = x1 - x0 (the
// difference is formed per row: no cancellation between two large sums).  col < C = T F, 16-byte
// vectors; thread (p, column group) walks its rows with independent loads in flight.
template <typename T>
__global__ void __launch_bounds__(256) mlp_bt_colsum_kernel(const T* __restrict__ x0, const T* __restrict__ x1,
                                                            int64_t B, int C, int P, float* __restrict__ part) {
  constexpr int V = 16 / (int)sizeof(T);
  const int G = C / V;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)G * P) return;
  const int cg = (int)(gid % G), p = (int)(gid / G);
  float a0[V], a1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) a0[j] = a1[j] = 0.f;
  auto unpack = [](const uint4& u, float* f) {
    if constexpr (sizeof(T) == 4) {
      f[0] = __uint_as_float(u.x); f[1] = __uint_as_float(u.y); f[2] = __uint_as_float(u.z); f[3] = __uint_as_float(u.w);
    } else {
      const uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[2 * j] = __uint_as_float(w4[j] << 16);
        f[2 * j + 1] = __uint_as_float(w4[j] & 0xFFFF0000u);
      }
    }
  };
  const int64_t c0 = (int64_t)cg * V;
#pragma unroll 4
  for (int64_t r = p; r < B; r += P) {
    const uint4 u0 = *reinterpret_cast<const uint4*>(x0 + r * C + c0);
    float f0[V];
    unpack(u0, f0);
    if (x1) {
      const uint4 u1 = *reinterpret_cast<const uint4*>(x1 + r * C + c0);
      float f1[V];
      unpack(u1, f1);
#pragma unroll
      for (int j = 0; j < V; ++j) a1[j] += f1[j] - f0[j];
    }
#pragma unroll
    for (int j = 0; j < V; ++j) a0[j] += f0[j];
  }
  const int nk = x1 ? 2 : 1;
  float* o = part + (int64_t)p * nk * C + c0;
#pragma unroll
  for (int j = 0; j < V; j += 4) *reinterpret_cast<f32x4*>(o + j) = f32x4{a0[j], a0[j + 1], a0[j + 2], a0[j + 3]};
  if (x1) {
#pragma unroll
    for (int j = 0; j < V; j += 4)
      *reinterpret_cast<f32x4*>(o + C + j) = f32x4{a1[j], a1[j + 1], a1[j + 2], a1[j + 3]};
  }
}

// One workgroup (1024 threads).  sums: [nk][Tn][F] from mlp_bt_colsum (mode 0: k = 0 real, 1 fake - real;
// mode 1: k = 0 fake).  W1, W2 (row pitch AFP = 101: odd, so the strided reads are bank-conflict free),
// w3 and the per-t tables live in LDS (mlp_affine_lds_bytes; Tn <= mlp_affine_max_t).  D = the (Tn, H)
// table W2 w3_t (also written to the D block of tsum in mode 0).  Mode 0 writes tsum's S1 / S2 / S3 rows,
// slab[0..1] = the real / fake score sums (without b3) and e[0] = B (1 - |g|)^2 (the penalty's sum over
// samples); mode 1 writes gdx = -g / B and slab = {fake score sum, 0}.
constexpr int AFP = 101;
__host__ __device__ constexpr size_t mlp_affine_lds_floats(int F, int H, int Tn) {
  return (size_t)F * AFP + (size_t)H * AFP + (size_t)Tn * (3 * H + F);
}
__global__ void __launch_bounds__(1024) mlp_wgp_affine_kernel(const float* __restrict__ sums, MlpCritic c, int F, int H,
                                                             int Tn, float Bf, float lam, int mode, float* __restrict__ Dg,
                                                             float* __restrict__ tsum, float* __restrict__ slab,
                                                             float* __restrict__ e, float* __restrict__ gdx) {
  extern __shared__ __attribute__((aligned(16))) float als[];
  __shared__ float red[16];
  float* W1 = als;                    // [F][AFP]
  float* W2 = W1 + F * AFP;           // [H][AFP]
  float* w3 = W2 + H * AFP;           // [Tn][H]
  float* D = w3 + Tn * H;             // [Tn][H]
  float* S2 = D + Tn * H;             // [Tn][H]
  float* g = S2 + Tn * H;             // [Tn][F]
  const int tid = threadIdx.x, NT = blockDim.x, L = F + 2 * H;
  for (int q = tid; q < F * H; q += NT) W1[(q / H) * AFP + q % H] = c.W1[q];
  for (int q = tid; q < H * H; q += NT) W2[(q / H) * AFP + q % H] = c.W2[q];
  for (int q = tid; q < Tn * H; q += NT) w3[q] = c.w3[q];
  __syncthreads();
  const float* s0 = sums;           // mode 0: real, mode 1: fake
  const float* sd = sums + Tn * F;  // mode 0: fake - real
  // (A) D[t][o] = sum_k W2[o][k] w3_t[k]
  for (int q = tid; q < Tn * H; q += NT) {
    const int t = q / H, o = q - t * H;
    float d = 0.f;
    for (int k = 0; k < H; ++k) d = fmaf(W2[o * AFP + k], w3[t * H + k], d);
    D[q] = d;
    if (Dg) Dg[q] = d;
  }
  __syncthreads();
  // (B) g[t][i] = sum_o W1[i][o] D[t][o] and |g|^2
  float gs = 0.f;
  for (int q = tid; q < Tn * F; q += NT) {
    const int t = q / F, i = q - t * F;
    float a = 0.f;
    for (int o = 0; o < H; ++o) a = fmaf(W1[i * AFP + o], D[t * H + o], a);
    g[q] = a;
    gs = fmaf(a, a, gs);
    if (mode == 1) gdx[q] = a * (-1.f / Bf);
  }
  const float gsq = block_sum<16>(gs, red);  // (barriers inside: g complete)
  const float n = sqrtf(gsq);
  const float cc = -(2.f * lam / Bf) * (1.f - n) / fmaxf(n, 1e-30f);
  // (C) S1, S2 and the score sums
  float scr = 0.f, scf = 0.f;
  for (int q = tid; q < Tn * H; q += NT) {
    const int t = q / H, o = q - t * H;
    float z = 0.f, dw = 0.f, h0 = 0.f;
    for (int i = 0; i < F; ++i) {
      const float wv = W1[i * AFP + o];
      h0 = fmaf(s0[t * F + i], wv, h0);
      if (mode == 0) {
        z = fmaf(g[t * F + i], wv, z);
        dw = fmaf(sd[t * F + i], wv, dw);
      }
    }
    const float hb = Bf * c.b1[o], tb = Bf * c.b2[o] * w3[q];
    scr += fmaf(h0 + hb, D[q], tb);
    if (mode == 0) {
      const float s2 = dw / Bf + Bf * (cc * z);
      S2[q] = s2;
      tsum[t * L + F + o] = s2;
      scf += fmaf(h0 + dw + hb, D[q], tb);
    }
  }
  if (mode == 0)
    for (int q = tid; q < Tn * F; q += NT) {
      const int t = q / F, i = q - t * F;
      tsum[t * L + i] = sd[q] / Bf + Bf * (cc * g[q]);
    }
  const float sr = block_sum<16>(scr, red);  // (barriers inside: S2 complete)
  const float sf = block_sum<16>(scf, red);
  if (tid == 0) {
    slab[0] = sr;
    slab[1] = mode == 0 ? sf : 0.f;
    if (mode == 0) e[0] = Bf * (1.f - n) * (1.f - n);
  }
  if (mode != 0) return;
  // (D) S3[t][k] = sum_o S2[t][o] W2[o][k]
  for (int q = tid; q < Tn * H; q += NT) {
    const int t = q / H, k = q - t * H;
    float a = 0.f;
    for (int o = 0; o < H; ++o) a = fmaf(S2[t * H + o], W2[o * AFP + k], a);
    tsum[t * L + F + H + k] = a;
  }
}

// out[b][col] = row[col] for every b < B (C = T F columns): thread (p, column group) packs its 16 bytes
// once and stores them to rows p, p + P, ...
template <typename T>
__global__ void __launch_bounds__(256) mlp_bcast_rows_kernel(const float* __restrict__ row, int C, int64_t B, int P,
                                                             T* __restrict__ out) {
  constexpr int V = 16 / (int)sizeof(T);
  const int G = C / V;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)G * P) return;
  const int cg = (int)(gid % G), p = (int)(gid / G), col = cg * V;
  uint4 u;
  if constexpr (sizeof(T) == 4) {
    u = make_uint4(__float_as_uint(row[col]), __float_as_uint(row[col + 1]), __float_as_uint(row[col + 2]),
                   __float_as_uint(row[col + 3]));
  } else {
    u = make_uint4(pk2bf(row[col], row[col + 1]), pk2bf(row[col + 2], row[col + 3]), pk2bf(row[col + 4], row[col + 5]),
                   pk2bf(row[col + 6], row[col + 7]));
  }
#pragma unroll 4
  for (int64_t r = p; r < B; r += P) *reinterpret_cast<uint4*>(out + r * C + col) = u;
}

// ===================================================================================================
// critic input gradient for the generator step (and its loss): the linear WGAN-GP critic (head 0) with
// W(fake, -1) (GAN/WGAN_GP.py:178-189); the GAN discriminator's (head 1) is mlp_gan_dx below
// ===================================================================================================
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_critic_dx_kernel(const T* __restrict__ x, MlpCritic c,
                                                                    T* __restrict__ dx, float* __restrict__ slab,
                                                                    int64_t M, int Tn, float inv) {
  using Lds = Critic4Lds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>(),
             *d1 = lp.template img<Dgrad<1>>();
  const float* vec = lp.vec;
  float acc = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    const float* w3t = c.w3 + (int64_t)(ok ? row % Tn : 0) * H;
    f32x16 A[NTH], Bv[NTH], X[NTF];
    load_rows<T, F>(X, x, row, M, h);
    dense<T, F, H>(X, A, f1, lane);
    bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);
    dense<T, H, H>(A, Bv, f2, lane);
    bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);
    const float sc = rowdot<H>(Bv, w3t, ok, h);
    if (ok && h == 0) acc += sc;
    head_rows<H>(A, w3t, -inv, ok, h);  // dh2: d W(fake, -1) / d s_b = -1 / B
    dense<T, H, H>(A, Bv, d2, lane);  // dh1
    dense<T, H, F>(Bv, X, d1, lane);  // dx
    store_rows<T, F>(dx, row, M, X, h);
  }
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// The generator step's input gradient through the GAN discriminator (head 1), rank-1 form: the hidden
// layers are linear (Dense -> Dense -> Dense(1, sigmoid); _critic_lists checks it), so every row's
// adjoint is dx = dz_row g with ONE vector g = W1 W2 w3 -- computed once per workgroup in the prologue
// instead of two dgrad MFMA passes per row.  No dgrad images: the
// forward images alone leave LDS room for fp32 on the split bf16 products (P = f32s_t).
// forward images and NV vectors: b1 | b2 | w3 (mlp_gan_critic_g), + D | g (mlp_gan_dx)
template <typename P, int F, int H, int NV> using GanFwdLds = MlpLds<P, F, H, NV, Tail<>, Fwd<1>, Fwd<2>>;
template <typename T, int F, int H, typename P = T>
__global__ void __launch_bounds__(MLP_THREADS) mlp_gan_dx_kernel(const T* __restrict__ x, MlpCritic c, float label,
                                                                 T* __restrict__ dx, float* __restrict__ slab, int64_t M,
                                                                 float inv) {
  using Lds = GanFwdLds<P, F, H, 5>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>();
  float* vec = lp.vec;
  for (int o = threadIdx.x; o < VEC; o += blockDim.x) {  // D = W2 w3
    float d = 0.f;
    if (o < H)
      for (int k = 0; k < H; ++k) d = fmaf(c.W2[o * H + k], c.w3[k], d);
    vec[A_D * VEC + o] = d;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < VEC; i += blockDim.x) {  // g = W1 D
    float a = 0.f;
    if (i < F)
      for (int o = 0; o < H; ++o) a = fmaf(c.W1[i * H + o], vec[A_D * VEC + o], a);
    vec[A_G * VEC + i] = a;
  }
  __syncthreads();
  const float b3 = c.b3 ? c.b3[0] : 0.f;
  const float* gh = vec + A_G * VEC + 4 * ((threadIdx.x & 63) >> 5);  // lane-half base (see head_rows)
  float acc = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    f32x16 A[NTH], Bv[NTH], X[NTF];
    load_rows<T, F>(X, x, row, M, h);
    dense<P, F, H>(X, A, f1, lane);
    bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);
    dense<P, H, H>(A, Bv, f2, lane);
    bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);
    const float sc = rowdot<H>(Bv, vec + A_W3 * VEC, ok, h);
    const float p = sigmoidf_(sc + b3);
    float lo, gp;
    bce(p, label, inv, lo, gp);
    if (ok && h == 0) acc += lo;
    const float dz = gp * p * (1.f - p);
#pragma unroll
    for (int t = 0; t < NTF; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 gv = *reinterpret_cast<const float4*>(gh + 32 * t + 8 * g);
        X[t][4 * g] = dz * gv.x; X[t][4 * g + 1] = dz * gv.y; X[t][4 * g + 2] = dz * gv.z; X[t][4 * g + 3] = dz * gv.w;
      }
    store_rows<T, F>(dx, row, M, X, h);
  }
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// ===================================================================================================
// vanilla GAN discriminator update (GAN/GAN.py:187-189): forward, BCE(label) per row, reverse to the
// weight-gradient operands
// ===================================================================================================
template <typename T, int F, int H> using GanCriticLds = MlpLds<T, F, H, 2, Tail<>, Fwd<1>, Fwd<2>, Dgrad<2>>;
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_gan_critic_kernel(const T* __restrict__ x, MlpCritic c, float label,
                                                                     T* __restrict__ h1o, T* __restrict__ dh2o,
                                                                     T* __restrict__ dh1o, T* __restrict__ h2o,
                                                                     T* __restrict__ dz3o, float* __restrict__ slab,
                                                                     int64_t M, float inv) {
  using Lds = GanCriticLds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d2 = lp.template img<Dgrad<2>>();
  const float* vec = lp.vec;
  const float b3 = c.b3 ? c.b3[0] : 0.f;
  float acc = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    f32x16 A[NTH], Bv[NTH], X[NTF];
    load_rows<T, F>(X, x, row, M, h);
    dense<T, F, H>(X, A, f1, lane);
    bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);
    store_rows<T, H>(h1o, row, M, A, h);
    dense<T, H, H>(A, Bv, f2, lane);
    bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);
    store_rows<T, H>(h2o, row, M, Bv, h);
    const float p = sigmoidf_(rowdot<H>(Bv, c.w3, ok, h) + b3);
    float lo, gp;
    bce(p, label, inv, lo, gp);
    const float dz = gp * p * (1.f - p);
    if (ok && h == 0) {
      acc += lo;
      dz3o[row] = Cvt<T>::from_f(dz);
    }
    head_rows<H>(A, c.w3, dz, ok, h);
    store_rows<T, H>(dh2o, row, M, A, h);
    dense<T, H, H>(A, Bv, d2, lane);
    store_rows<T, H>(dh1o, row, M, Bv, h);
  }
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// ---------------------------------------------------------------------------------------------------
// The same discriminator update with its six parameter gradients taken in the kernel.  The hidden
// layers are linear, so every adjoint of a row is that row's scalar dz times a fixed vector:
//   dh2 = dz w3,  dh1 = dz u (u = W2 w3)
// and each weight gradient factorises into a dz-weighted column sum of the layer's own input:
//   gW1 = s1 (x) u,  gW2 = s2 (x) w3,  gw3 = s3,  gb1 = S u,  gb2 = S w3,  gb3 = S
//   s1 = sum_r dz_r x_r,  s2 = sum_r dz_r h1_r,  s3 = sum_r dz_r h2_r,  S = sum_r dz_r.
// Each lane accumulates dz * (x, h1, h2) of its rows in registers over all its tiles (fp32); one
// transpose-reduce butterfly per tile set at the end gives the wave's column sums (slab row of the
// wave: [s1 F | s2 H | s3 H | S]); mlp_gan_grad_finish reduces the slab in a fixed order and forms
// the outer products.  The per-row forward and BCE are the same as mlp_gan_critic's.
// ---------------------------------------------------------------------------------------------------
template <typename T, int F, int H, typename P = T>  // P: product policy (f32s_t: fp32 on split bf16)
__global__ void __launch_bounds__(MLP_THREADS) mlp_gan_critic_g_kernel(const T* __restrict__ x, MlpCritic c, float label,
                                                                       float* __restrict__ gslab,
                                                                       float* __restrict__ slab, int64_t M, float inv) {
  using Lds = GanFwdLds<P, F, H, 3>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, c);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>();
  const float* vec = lp.vec;
  const float b3 = c.b3 ? c.b3[0] : 0.f;
  float acc = 0.f, sdz = 0.f;
  f32x16 ax[NTF], a1[NTH], a2[NTH];
#pragma unroll
  for (int t = 0; t < NTF; ++t) ax[t] = zero16();
#pragma unroll
  for (int t = 0; t < NTH; ++t) a1[t] = a2[t] = zero16();
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    const bool ok = row < M;
    f32x16 A[NTH], Bv[NTH], X[NTF];
    load_rows<T, F>(X, x, row, M, h);
    dense<P, F, H>(X, A, f1, lane);
    bias_act<H>(A, vec + A_B1 * VEC, ACT_LINEAR, h);         // h1
    dense<P, H, H>(A, Bv, f2, lane);
    bias_act<H>(Bv, vec + A_B2 * VEC, ACT_LINEAR, h);  // h2
    const float p = sigmoidf_(rowdot<H>(Bv, vec + A_W3 * VEC, true, h) + b3);
    float lo, gp;
    bce(p, label, inv, lo, gp);
    const float dz = ok ? gp * p * (1.f - p) : 0.f;
    if (ok && h == 0) {
      acc += lo;
      sdz += dz;
    }
#pragma unroll
    for (int t = 0; t < NTF; ++t) ax[t] += dz * X[t];
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      a1[t] += dz * A[t];
      a2[t] += dz * Bv[t];
    }
  }
  constexpr int L = F + 2 * H + 1;
  float* out = gslab + ((int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6)) * L;
  const int fq = featq(colsum_q(lane), h);
#pragma unroll
  for (int t = 0; t < NTF; ++t) {
    const float v = colsum(ax[t], lane);
    if ((lane & 1) == 0 && 32 * t + fq < F) out[32 * t + fq] = v;
  }
#pragma unroll
  for (int t = 0; t < NTH; ++t) {
    const float v1 = colsum(a1[t], lane), v2 = colsum(a2[t], lane);
    if ((lane & 1) == 0 && 32 * t + fq < H) {
      out[F + 32 * t + fq] = v1;
      out[F + H + 32 * t + fq] = v2;
    }
  }
  sdz = wave_sum(sdz);
  if ((threadIdx.x & 63) == 0) out[F + 2 * H] = sdz;
  slab_put(slab, 2, 0, acc);
  slab_put(slab, 2, 1, 0.f);
}

// the six gradients from the reduced sums v = [s1 F | s2 H | s3 H | S] (one workgroup, fp32)
__global__ void __launch_bounds__(256) mlp_gan_grad_finish_kernel(const float* __restrict__ v, MlpCritic c, int F, int H,
                                                                  float* __restrict__ gW1, float* __restrict__ gb1,
                                                                  float* __restrict__ gW2, float* __restrict__ gb2,
                                                                  float* __restrict__ gw3, float* __restrict__ gb3) {
  __shared__ float u[128], w3[128];
  const float* s1 = v;
  const float* s2 = v + F;
  const float* s3 = v + F + H;
  const float S = v[F + 2 * H];
  for (int i = threadIdx.x; i < H; i += blockDim.x) {
    float a = 0.f;
    for (int o = 0; o < H; ++o) a = fmaf(c.W2[i * H + o], c.w3[o], a);  // u = W2 w3
    u[i] = a;
    w3[i] = c.w3[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < F * H; e += blockDim.x) gW1[e] += s1[e / H] * u[e % H];
  for (int e = threadIdx.x; e < H * H; e += blockDim.x) gW2[e] += s2[e / H] * w3[e % H];
  for (int o = threadIdx.x; o < H; o += blockDim.x) {
    gb1[o] += S * u[o];
    gb2[o] += S * w3[o];
    gw3[o] += s3[o];
  }
  if (threadIdx.x == 0) gb3[0] += S;
}

// ===================================================================================================
// host launchers
// ===================================================================================================
void launch_mlp_wgp_norm(int dt, const MlpCritic& c, float* gsq, int64_t M, int Tn, int F, int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H,
               { mlp_launch<WgpNormLds<T, FF, 100>>(mlp_wgp_norm_kernel<T, FF, 100>, GRID_TILES, M, s, c, gsq, M, Tn); });
}

int mlp_wgp_coef_parts(int64_t B) { return (int)((B + 255) / 256); }

void launch_mlp_wgp_coef(const float* gsq, int Tn, int64_t B, float lam, float* c, float* e, hipStream_t s) {
  if (B <= 0) return;
  hipLaunchKernelGGL(mlp_wgp_coef_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, gsq, Tn, B, lam, c, e);
}

void launch_mlp_wgp_critic(int dt, const void* real, const void* fake, const float* c, const MlpCritic& cr,
                           void* X2c, void* dY2, void* X1c, void* dY1, void* Y3c, float* slab, int64_t M, int Tn,
                           int F, int H, hipStream_t s) {
  if (M <= 0) return;
  const float invB = (float)Tn / (float)M;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<Critic4Lds<T, FF, 100>>(mlp_wgp_critic_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)real, (const T*)fake,
                                       c, cr, (T*)X2c, (T*)dY2, (T*)X1c, (T*)dY1, (T*)Y3c, slab, M, Tn, invB);
  });
}

void launch_mlp_critic_dx(int dt, int head, const void* x, const MlpCritic& cr, float label, void* dx, float* slab,
                          int64_t M, int Tn, int F, int H, hipStream_t s) {
  if (M <= 0) return;
  if (head == 0) {  // d/ds_b of the W loss = -1/B (B = M / T samples)
    MLP_DISPATCH(dt, F, H, {
      mlp_launch<Critic4Lds<T, FF, 100>>(mlp_critic_dx_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, (T*)dx, slab,
                                         M, Tn, (float)Tn / (float)M);
    });
    return;
  }
  // head 1: BCE mean over the M rows, rank-1 input gradient; fp32 on the split bf16 products
  MLP_DISPATCH(dt, F, H, {
    if constexpr (std::is_same_v<T, float>) {
      if (!fp32_exact_mode()) {
        mlp_launch<GanFwdLds<f32s_t, FF, 100, 5>>(mlp_gan_dx_kernel<float, FF, 100, f32s_t>, GRID_SLAB, M, s,
                                                  (const float*)x, cr, label, (float*)dx, slab, M, 1.f / (float)M);
        return;
      }
    }
    mlp_launch<GanFwdLds<T, FF, 100, 5>>(mlp_gan_dx_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, label, (T*)dx,
                                         slab, M, 1.f / (float)M);
  });
}

void launch_mlp_gan_critic(int dt, const void* x, const MlpCritic& cr, float label, void* h1, void* dh2, void* dh1,
                           void* h2, void* dz3, float* slab, int64_t M, int F, int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<GanCriticLds<T, FF, 100>>(mlp_gan_critic_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, label,
                                         (T*)h1, (T*)dh2, (T*)dh1, (T*)h2, (T*)dz3, slab, M, 1.f / (float)M);
  });
}

// ---- GAN discriminator update with in-kernel gradients (both dtypes) ----
void launch_mlp_gan_critic_g(int dt, const void* x, const MlpCritic& cr, float label, float* gslab, float* slab,
                             int64_t M, int F, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, 100, {
    if constexpr (std::is_same_v<T, float>) {  // fp32 on the split bf16 products (images: 108 / 117 KB)
      if (!fp32_exact_mode()) {
        mlp_launch<GanFwdLds<f32s_t, FF, 100, 3>>(mlp_gan_critic_g_kernel<float, FF, 100, f32s_t>, GRID_SLAB, M, s,
                                                  (const float*)x, cr, label, gslab, slab, M, 1.f / (float)M);
        return;
      }
    }
    mlp_launch<GanFwdLds<T, FF, 100, 3>>(mlp_gan_critic_g_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)x, cr, label,
                                         gslab, slab, M, 1.f / (float)M);
  });
}

void launch_mlp_gan_grad_finish(const float* v, const MlpCritic& cr, int F, int H, float* gW1, float* gb1, float* gW2,
                                float* gb2, float* gw3, float* gb3, hipStream_t s) {
  hipLaunchKernelGGL(mlp_gan_grad_finish_kernel, dim3(1), dim3(256), 0, s, v, cr, F, H, gW1, gb1, gW2, gb2, gw3, gb3);
}

// ---- GP critic update with per-t column-sum gradients (fp32 / bf16) ----
int mlp_wgpt_waves_per_t(int Tn) { return std::max(1, device_cu_count() * 2 * MLP_WAVES / std::max(1, Tn)); }
int mlp_wgpt_blocks(int Tn) { return (mlp_wgpt_waves_per_t(Tn) * Tn + MLP_WAVES - 1) / MLP_WAVES; }
size_t mlp_wgpt_tsum_floats(int F, int Tn) { return (size_t)Tn * (F + 3 * 100); }

void launch_mlp_wgp_critic_t(int dt, const void* real, const void* fake, const float* c, const MlpCritic& cr,
                             float* tslab, float* tsum, float* slab, int64_t Bn, int Tn, int F, float* gW1, float* gW2,
                             float* gw3, hipStream_t s) {
  if (Bn <= 0) return;
  const int kper = mlp_wgpt_waves_per_t(Tn), P = mlp_wgpt_blocks(Tn);
  const float invB = 1.f / (float)Bn;
  MLP_DISPATCH(dt, F, 100, {
    mlp_launch<Critic4Lds<T, FF, 100>>(mlp_wgp_critic_t_kernel<T, FF, 100>, GRID_BLOCKS, P, s, (const T*)real,
                                       (const T*)fake, c, cr, tslab, slab, Bn, Tn, kper, invB);
  });
  const int H = 100, L = F + 2 * H;
  const int np = Tn * (L + H), nf = F * H + H * H + Tn * H;
  hipLaunchKernelGGL(mlp_wgp_tsum_prep_kernel, dim3((np + 255) / 256), dim3(256), 0, s, tslab, cr, F, H, Tn, kper, tsum);
  hipLaunchKernelGGL(mlp_wgp_tsum_finish_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, tsum, cr, F, H, Tn, gW1, gW2,
                     gw3);
}

// ---- the affine critic's update from batch sums (both dtypes) ----
// the finish kernel keeps W1, W2, w3 and its per-t tables in LDS
static constexpr int kAffineLdsMax = 160 * 1024 - 1024;
bool mlp_affine_supported(int F, int Tn) {
  return mlp_supported(F, 100) && Tn > 0 && (Tn * F) % 8 == 0 &&
         mlp_affine_lds_floats(F, 100, Tn) * sizeof(float) <= (size_t)kAffineLdsMax;
}

// row partitions of mlp_bt_colsum over the C / V column groups: ~1024 threads per CU for bf16, 512 for
// fp32 (measured on config 4: bf16 206 -> 140 us per call at 1024, 2048 no better; fp32 best at 512;
// profiles/r06_affine/colsum_ab)
static int colsum_parts(int dt, int64_t B, int C) {
  const int V = dt == DT_BF16 ? 8 : 4, G = C / V, tpc = dt == DT_BF16 ? 1024 : 512;
  const int64_t want = ((int64_t)device_cu_count() * tpc + G - 1) / G;
  return (int)std::max<int64_t>(1, std::min<int64_t>(B, want));
}
size_t mlp_affine_ws_floats(int dt, int64_t Bn, int Tn, int F) {
  const int H = 100, C = Tn * F;
  // part | sums | tsum (S rows + D) | g   (mode 1 needs less: part | sums | D | g | gdx)
  return (size_t)colsum_parts(dt, Bn, C) * 2 * C + 2 * (size_t)C + (size_t)Tn * (F + 3 * H) + (size_t)Tn * F;
}
// sums[k][col] = sum_b y_k[b][col] (y_0 = x0, y_1 = x1 - x0), fixed order
static void bt_colsum(int dt, const void* x0, const void* x1, int64_t B, int C, float* part, float* sums, hipStream_t s) {
  const int P = colsum_parts(dt, B, C), V = dt == DT_BF16 ? 8 : 4, nk = x1 ? 2 : 1;
  const int grid = (int)(((int64_t)(C / V) * P + 255) / 256);
  if (dt == DT_BF16)
    hipLaunchKernelGGL(mlp_bt_colsum_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)x0, (const bf16_t*)x1, B,
                       C, P, part);
  else
    hipLaunchKernelGGL(mlp_bt_colsum_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)x0, (const float*)x1, B, C,
                       P, part);
  (void)hipMemsetAsync(sums, 0, sizeof(float) * nk * C, s);
  launch_mlp_slab_sum_cols(part, P, (int64_t)nk * C, 0, nk * C, sums, s);
}

void launch_mlp_wgp_affine(int dt, const void* real, const void* fake, const MlpCritic& cr, int64_t Bn, int Tn, int F,
                           float lam, float* ws, float* slab, float* e, float* gW1, float* gW2, float* gw3, hipStream_t s) {
  if (Bn <= 0) return;
  const int H = 100, C = Tn * F, L = F + 2 * H;
  float* part = ws;
  float* sums = part + (size_t)colsum_parts(dt, Bn, C) * 2 * C;
  float* tsum = sums + 2 * C;
  float* g = tsum + (size_t)Tn * (L + H);
  (void)g;
  bt_colsum(dt, real, fake, Bn, C, part, sums, s);
  const size_t lds = mlp_affine_lds_floats(F, H, Tn) * sizeof(float);
  set_lds(mlp_wgp_affine_kernel, lds);
  hipLaunchKernelGGL(mlp_wgp_affine_kernel, dim3(1), dim3(1024), lds, s, sums, cr, F, H, Tn, (float)Bn, lam, 0,
                     tsum + (size_t)Tn * L, tsum, slab, e, (float*)nullptr);
  const int nf = F * H + H * H + Tn * H;
  hipLaunchKernelGGL(mlp_wgp_tsum_finish_kernel, dim3((nf + 255) / 256), dim3(256), 0, s, tsum, cr, F, H, Tn, gW1, gW2,
                     gw3);
}

void launch_mlp_critic_dx_affine(int dt, const void* fake, const MlpCritic& cr, int64_t Bn, int Tn, int F, float* ws,
                                 float* slab, void* dx, hipStream_t s) {
  if (Bn <= 0) return;
  const int H = 100, C = Tn * F;
  float* part = ws;
  float* sums = part + (size_t)colsum_parts(dt, Bn, C) * C;
  float* D = sums + C;
  float* g = D + (size_t)Tn * H;
  float* gdx = g + (size_t)Tn * F;
  (void)D; (void)g;
  bt_colsum(dt, fake, nullptr, Bn, C, part, sums, s);
  const size_t lds = mlp_affine_lds_floats(F, H, Tn) * sizeof(float);
  set_lds(mlp_wgp_affine_kernel, lds);
  hipLaunchKernelGGL(mlp_wgp_affine_kernel, dim3(1), dim3(1024), lds, s, sums, cr, F, H, Tn, (float)Bn, 0.f, 1,
                     (float*)nullptr, (float*)nullptr, slab, (float*)nullptr, gdx);
  const int P = colsum_parts(dt, Bn, C), V = dt == DT_BF16 ? 8 : 4;
  const int grid = (int)(((int64_t)(C / V) * P + 255) / 256);
  if (dt == DT_BF16)
    hipLaunchKernelGGL(mlp_bcast_rows_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, gdx, C, Bn, P, (bf16_t*)dx);
  else
    hipLaunchKernelGGL(mlp_bcast_rows_kernel<float>, dim3(grid), dim3(256), 0, s, gdx, C, Bn, P, (float*)dx);
}

}  // namespace hfrep
