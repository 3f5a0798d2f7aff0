// Fused MLP-GAN passes for gfx950 (see mlp_dev.h): the generator passes, the loss finish and the slab sums
#include "mlp_dev.h"

namespace hfrep {

// ===================================================================================================
// generator forward: noise -> fake (GAN/WGAN_GP.py:221-236 build_generator)
// ===================================================================================================
// P: the product policy (T, or f32s_t for fp32 storage on the split bf16 path)
template <typename P, int F, int H> using GenFwdLds = MlpLds<P, F, H, 7, Tail<>, Fwd<1>, Fwd<2>, Fwd<3>>;
template <typename T, int F, int H, typename P = T>
__global__ void __launch_bounds__(MLP_THREADS) mlp_gen_fwd_kernel(const T* __restrict__ z, MlpGen g,
                                                                  T* __restrict__ out, int64_t M) {
  using Lds = GenFwdLds<P, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, g);
  const auto *i1 = lp.template img<Fwd<1>>(), *i2 = lp.template img<Fwd<2>>(), *i3 = lp.template img<Fwd<3>>();
  const float* vec = lp.vec;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    f32x16 x[NTF], a[NTH], b[NTH];
    float mean, rstd;
    load_rows<T, F>(x, z, row, M, h);
    dense<P, F, H>(x, a, i1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_SIGMOID, h);
    lrelu_ln<H>(a, vec + V_G1 * VEC, vec + V_BE1 * VEC, h, mean, rstd);
    dense<P, H, H>(a, b, i2, lane);
    bias_act<H>(b, vec + V_B2 * VEC, ACT_SIGMOID, h);
    lrelu_ln<H>(b, vec + V_G2 * VEC, vec + V_BE2 * VEC, h, mean, rstd);
    dense<P, H, F>(b, x, i3, lane);
    bias_act<F>(x, vec + V_B3 * VEC, ACT_LINEAR, h);
    store_rows<T, F>(out, row, M, x, h);
  }
}

// ===================================================================================================
// generator reverse pass (GAN/WGAN_GP.py:178-189 / GAN/GAN.py:195-198: the combined model's update)
// from dfake = dL/dG(z): recomputes the forward in registers and writes the weight-gradient operands
// ===================================================================================================
// TAIL: the staging buffers of mlp_gen_bwd_w
template <typename T, int F, int H, typename TAIL = Tail<>>
using GenBwdLds = MlpLds<T, F, H, 6, TAIL, Fwd<1>, Fwd<2>, Dgrad<3>, Dgrad<2>>;
template <typename T, int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_gen_bwd_kernel(const T* __restrict__ z, const T* __restrict__ dfake,
                                                                  MlpGen g, T* __restrict__ dz1o, T* __restrict__ u1o,
                                                                  T* __restrict__ dz2o, T* __restrict__ u2o,
                                                                  float* __restrict__ lnslab, int64_t M) {
  using Lds = GenBwdLds<T, F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, g);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d3 = lp.template img<Dgrad<3>>(),
             *d2 = lp.template img<Dgrad<2>>();
  const float* vec = lp.vec;
  const float* gam1 = vec + V_G1 * VEC;
  const float* gam2 = vec + V_G2 * VEC;
  float pg1[NTH], pb1[NTH], pg2[NTH], pb2[NTH];  // per-lane column sums (see colsum)
#pragma unroll
  for (int t = 0; t < NTH; ++t) pg1[t] = pb1[t] = pg2[t] = pb2[t] = 0.f;
  MLP_LOOP {
    const int64_t row = tile * 32 + (lane & 31);
    f32x16 x[NTF], a[NTH], y2[NTH], d[NTH];
    float mean1, rstd1, mean2, rstd2;
    // ---- forward (u1, u2 out; y2 and the row statistics kept)
    load_rows<T, F>(x, z, row, M, h);
    dense<T, F, H>(x, a, f1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_SIGMOID, h);
    lrelu_ln<H>(a, vec + V_G1 * VEC, vec + V_BE1 * VEC, h, mean1, rstd1);
    store_rows<T, H>(u1o, row, M, a, h);
    dense<T, H, H>(a, y2, f2, lane);
    bias_act<H>(y2, vec + V_B2 * VEC, ACT_SIGMOID, h);
#pragma unroll
    for (int t = 0; t < NTH; ++t) a[t] = y2[t];
    lrelu_ln<H>(a, vec + V_G2 * VEC, vec + V_BE2 * VEC, h, mean2, rstd2);
    store_rows<T, H>(u2o, row, M, a, h);
    // ---- reverse: du2 = dfake W3^T, LN2 / LReLU / sigmoid reverse -> dz2
    load_rows<T, F>(x, dfake, row, M, h);
    dense<T, F, H>(x, d, d3, lane);
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb2[t] += colsum(d[t], lane);
    ln_reverse<H>(d, y2, d, gam2, mean2, rstd2, h, lane, pg2);
    store_rows<T, H>(dz2o, row, M, d, h);
    // ---- du1 = dz2 W2^T; recompute y1; LN1 / LReLU / sigmoid reverse -> dz1
    dense<T, H, H>(d, y2, d2, lane);  // y2 now holds du1
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb1[t] += colsum(y2[t], lane);
    load_rows<T, F>(x, z, row, M, h);
    dense<T, F, H>(x, a, f1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_SIGMOID, h);  // y1
    ln_reverse<H>(y2, a, a, gam1, mean1, rstd1, h, lane, pg1);
    store_rows<T, H>(dz1o, row, M, a, h);
  }
  // per-wave LN partials: lanes with bit 0 clear own feature featq(colsum_q(lane), h) of every tile
  float* out = lnslab + ((int64_t)blockIdx.x * MLP_WAVES + (threadIdx.x >> 6)) * 4 * H;
  if ((lane & 1) == 0) {
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      const int f = 32 * t + featq(colsum_q(lane), h);
      if (f < H) {
        out[f] = pg1[t];
        out[H + f] = pb1[t];
        out[2 * H + f] = pg2[t];
        out[3 * H + f] = pb2[t];
      }
    }
  }
}

// Transposed staging of mlp_gen_bwd_w: 32 rows per wave, feature-major [f][row] bf16 with pitch WQ.  The 8-row
// runs the MFMA fragments need are contiguous, so every operand is one 16-byte read; WQ = 136 bf16 makes those
// reads conflict-free (272 B row stride = 68 dwords: 16 lanes hit 16 distinct 4-bank groups).
constexpr int WQ = 136;  // pitch (bf16) of a transposed staging row: 128 rows + 8

__device__ __forceinline__ float dpp_xor1(float v) {
  // quad_perm [1, 0, 3, 2]: the value of lane ^ 1
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, true));
}
// this lane's row rr (block-local, 0..127) of accumulator tiles a -> img[f][rr] for f < N.  The
// (even, odd) row pair of a feature is one dword: both lanes of the pair write it (same address, same
// value; the odd lane's halves are rotated into place by one v_alignbit), so there is no per-store
// exec mask.  Feature validity is compile-time except the last tile's features fb .. fb + 3 < N <=
// fb + 7, which only lane half 0 holds (one masked group).
template <int N>
__device__ __forceinline__ void stage_t(unsigned short* img, const f32x16* a, int rr, int h) {
  constexpr int NT = (N + 31) / 32, REM = N - 32 * (NT - 1);
  unsigned short* base = img + (rr & ~1) + 4 * h * WQ;
  const uint32_t rot = (rr & 1) * 16;
  uint32_t part[4];
  int pf[4], np = 0;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int fb = 8 * (q >> 2) + (q & 3);  // feature (in the tile) of this register in lane half 0
      if (t == NT - 1 && fb >= REM) continue;
      const float v = a[t][q];
      const float p = dpp_xor1(v);
      const uint32_t w0 = pk2bf(v, p);
      const uint32_t w = __builtin_amdgcn_alignbit(w0, w0, rot);
      if (t < NT - 1 || fb + 4 < REM) {
        *reinterpret_cast<uint32_t*>(base + (32 * t + fb) * WQ) = w;
      } else {
        pf[np & 3] = fb;  // at most 4 such features (REM - 4 .. REM - 1)
        part[np++ & 3] = w;
      }
    }
  if (np && h == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < np) *reinterpret_cast<uint32_t*>(base + (32 * (NT - 1) + pf[q]) * WQ) = part[q];
  }
}

// ---------------------------------------------------------------------------------------------------
// The generator reverse with its six parameter gradients (W1, b1, W2, b2, W3, b3) accumulated in the
// kernel (bf16), 4 waves walk 128-row block tiles together, stage the
// X / dY operands of each weight transposed in LDS and run the block's rows as the k dimension of
// gW = X^T dY on v_mfma_f32_32x32x16_bf16.  The bias gradients come out of the same MFMAs: every X
// image has a row of ones after its last feature (written once), so C row K of gW is sum_r dY[r].
// Four staging buffers, reused as the chain produces operands (two barriers per weight):
//   A: u1 -> dz1     B: u2 -> dz2     C: dfake     D: noise
//   gW3 (+ gb3): X = u2 (B), dY = dfake (C); wave w owns input tile w, every output tile
//   gW2 (+ gb2): X = u1 (A), dY = dz2 (B);   wave w owns output tile w
//   gW1 (+ gb1): X = noise (D), dY = dz1 (A); wave w owns output tile w
// LayerNorm parameter gradients stay the per-wave colsum partials of mlp_gen_bwd (lnslab).
// ---------------------------------------------------------------------------------------------------
// the four staging buffers A, B, C, D behind the plan of mlp_gen_bwd (A, B, D with their ones row)
template <int F, int H>
using GbwLds = GenBwdLds<bf16_t, F, H,
                         Tail<(size_t)(H + 1) * WQ * 2, (size_t)(H + 1) * WQ * 2, (size_t)F * WQ * 2, (size_t)(F + 1) * WQ * 2>>;

// rows past M stage zeros
template <int N>
__device__ __forceinline__ void stage_t_ok(unsigned short* img, f32x16* a, int rr, int h, bool ok) {
  if (!ok) {
#pragma unroll
    for (int t = 0; t < (N + 31) / 32; ++t) a[t] = zero16();
  }
  stage_t<N>(img, a, rr, h);
}
// gW[tile] += X^T dY over the block's 128 rows: A = rows of the X image (clamped to row KX: the ones
// row or a discarded one), B = row `col` of the dY image
template <int NI>
__device__ __forceinline__ void wgrad_block(f32x16* acc, const unsigned short* X, int i0, int KX,
                                            const unsigned short* Y, int col, int cl, int h) {
#pragma unroll 2
  for (int ks = 0; ks < 8; ++ks) {
    const int r0 = 16 * ks + 8 * h;
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(Y + col * WQ + r0);
#pragma unroll
    for (int it = 0; it < NI; ++it) {
      const int i = min(i0 + 32 * it + cl, KX);
      acc[it] = MF<bf16_t>::mma(*reinterpret_cast<const bf16x8*>(X + i * WQ + r0), b, acc[it]);
    }
  }
}

// acc[ot] += X^T dY for ONE input row i of X and NO output tiles (B = rows 32 ot + lane of the dY
// image, clamped to KY - 1)
template <int NO>
__device__ __forceinline__ void wgrad_block_out(f32x16* acc, const unsigned short* X, int i, const unsigned short* Y,
                                                int KY, int cl, int h) {
#pragma unroll 2
  for (int ks = 0; ks < 8; ++ks) {
    const int r0 = 16 * ks + 8 * h;
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(X + i * WQ + r0);
#pragma unroll
    for (int ot = 0; ot < NO; ++ot) {
      const int o = min(32 * ot + cl, KY - 1);
      acc[ot] = MF<bf16_t>::mma(a, *reinterpret_cast<const bf16x8*>(Y + o * WQ + r0), acc[ot]);
    }
  }
}

template <int F, int H>
__global__ void __launch_bounds__(MLP_THREADS) mlp_gen_bwd_w_kernel(const bf16_t* __restrict__ z,
                                                                    const bf16_t* __restrict__ dfake, MlpGen g,
                                                                    float* __restrict__ gslab,
                                                                    float* __restrict__ lnslab, int64_t M) {
  using T = bf16_t;
  using Lds = GbwLds<F, H>;
  constexpr int NTH = (H + 31) / 32, NTF = (F + 31) / 32, NX1 = (F + 1 + 31) / 32;
  static_assert((H + 1 + 31) / 32 == NTH, "the ones row of the H-wide images fits the last input tile");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const auto lp = mlp_prologue<Lds>(lds, g);
  const auto *f1 = lp.template img<Fwd<1>>(), *f2 = lp.template img<Fwd<2>>(), *d3 = lp.template img<Dgrad<3>>(),
             *d2 = lp.template img<Dgrad<2>>();
  const float* vec = lp.vec;
  unsigned short* bA = reinterpret_cast<unsigned short*>(lp.template tail<0>());
  unsigned short* bB = reinterpret_cast<unsigned short*>(lp.template tail<1>());
  unsigned short* bC = reinterpret_cast<unsigned short*>(lp.template tail<2>());
  unsigned short* bD = reinterpret_cast<unsigned short*>(lp.template tail<3>());
  // the ones rows (bf16 1.0), written once; their first readers run behind the barriers S0 and S1 of the first tile
  for (int r = threadIdx.x; r < 128; r += blockDim.x) {
    bA[H * WQ + r] = 0x3F80;
    bB[H * WQ + r] = 0x3F80;
    bD[F * WQ + r] = 0x3F80;
  }
  const int lane = threadIdx.x & 63, h = lane >> 5, w = threadIdx.x >> 6, cl = lane & 31;
  const int rr = 32 * w + cl;
  const float* gam1 = vec + V_G1 * VEC;
  const float* gam2 = vec + V_G2 * VEC;
  float pg1[NTH], pb1[NTH], pg2[NTH], pb2[NTH];
#pragma unroll
  for (int t = 0; t < NTH; ++t) pg1[t] = pb1[t] = pg2[t] = pb2[t] = 0.f;
  f32x16 gW3[NTF], gW2[NTH], gW1[NX1];
#pragma unroll
  for (int i = 0; i < NTF; ++i) gW3[i] = zero16();
#pragma unroll
  for (int i = 0; i < NTH; ++i) gW2[i] = zero16();
#pragma unroll
  for (int i = 0; i < NX1; ++i) gW1[i] = zero16();
  const int64_t nbt = (M + 127) / 128;
  for (int64_t bt = blockIdx.x; bt < nbt; bt += gridDim.x) {
    const int64_t row = bt * 128 + rr;
    const bool ok = row < M;
    f32x16 x[NTF], a[NTH], y2[NTH], d[NTH];
    float mean1, rstd1, mean2, rstd2;
    __syncthreads();  // S0: the previous block tile's gW1 reads (A, D) are done
    load_rows<T, F>(x, z, row, M, h);
    stage_t_ok<F>(bD, x, rr, h, ok);
    dense<T, F, H>(x, a, f1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_SIGMOID, h);
    lrelu_ln<H>(a, vec + V_G1 * VEC, vec + V_BE1 * VEC, h, mean1, rstd1);  // u1
    dense<T, H, H>(a, y2, f2, lane);
    stage_t_ok<H>(bA, a, rr, h, ok);
    bias_act<H>(y2, vec + V_B2 * VEC, ACT_SIGMOID, h);
#pragma unroll
    for (int t = 0; t < NTH; ++t) a[t] = y2[t];
    lrelu_ln<H>(a, vec + V_G2 * VEC, vec + V_BE2 * VEC, h, mean2, rstd2);  // u2
    stage_t_ok<H>(bB, a, rr, h, ok);
    load_rows<T, F>(x, dfake, row, M, h);  // zeros past M
    stage_t<F>(bC, x, rr, h);
    dense<T, F, H>(x, d, d3, lane);        // du2 = dfake W3^T
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb2[t] += colsum(d[t], lane);
    ln_reverse<H>(d, y2, d, gam2, mean2, rstd2, h, lane, pg2);  // dz2 (y2 dead from here)
    __syncthreads();  // S1: u1, u2, dfake, noise staged
    __builtin_amdgcn_sched_barrier(0);
    wgrad_block_out<NTF>(gW3, bB, min(32 * w + cl, H), bC, F, cl, h);  // gW3[i in tile w][o = 32 ot + cl]
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // S2: the gW3 reads of B are done
    stage_t_ok<H>(bB, d, rr, h, ok);
    dense<T, H, H>(d, y2, d2, lane);  // y2 now holds du1
    __syncthreads();  // S2b: dz2 staged
    __builtin_amdgcn_sched_barrier(0);
    wgrad_block<NTH>(gW2, bA, 0, H, bB, min(32 * w + cl, H - 1), cl, h);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < NTH; ++t) pb1[t] += colsum(y2[t], lane);
    load_rows<T, F>(x, z, row, M, h);
    dense<T, F, H>(x, a, f1, lane);
    bias_act<H>(a, vec + V_B1 * VEC, ACT_SIGMOID, h);  // y1
    ln_reverse<H>(y2, a, a, gam1, mean1, rstd1, h, lane, pg1);  // dz1
    __syncthreads();  // S3: the gW2 reads of A are done
    stage_t_ok<H>(bA, a, rr, h, ok);
    __syncthreads();  // S3b: dz1 staged
    __builtin_amdgcn_sched_barrier(0);
    wgrad_block<NX1>(gW1, bD, 0, F, bA, min(32 * w + cl, H - 1), cl, h);
    __builtin_amdgcn_sched_barrier(0);
  }
  // partial gradients of this workgroup: [W1 F x H][b1 H][W2 H x H][b2 H][W3 H x F][b3 F]
  constexpr int oB1 = F * H, oW2 = oB1 + H, oB2 = oW2 + H * H, oW3 = oB2 + H, oB3 = oW3 + H * F, L = oB3 + F;
  float* gs = gslab + (int64_t)blockIdx.x * L;
  {
    const int o = 32 * w + cl;  // gW2 / gW1 output column
    if (o < H) {
#pragma unroll
      for (int it = 0; it < NTH; ++it)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = 32 * it + featq(q, h);
          if (i < H) gs[oW2 + i * H + o] = gW2[it][q];
          else if (i == H) gs[oB2 + o] = gW2[it][q];
        }
#pragma unroll
      for (int it = 0; it < NX1; ++it)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = 32 * it + featq(q, h);
          if (i < F) gs[i * H + o] = gW1[it][q];
          else if (i == F) gs[oB1 + o] = gW1[it][q];
        }
    }
#pragma unroll
    for (int ot = 0; ot < NTF; ++ot) {
      const int o3 = 32 * ot + cl;
      if (o3 < F) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = 32 * w + featq(q, h);
          if (i < H) gs[oW3 + i * F + o3] = gW3[ot][q];
          else if (i == H) gs[oB3 + o3] = gW3[ot][q];
        }
      }
    }
  }
  float* out = lnslab + ((int64_t)blockIdx.x * MLP_WAVES + w) * 4 * H;
  if ((lane & 1) == 0) {
#pragma unroll
    for (int t = 0; t < NTH; ++t) {
      const int f = 32 * t + featq(colsum_q(lane), h);
      if (f < H) {
        out[f] = pg1[t];
        out[H + f] = pb1[t];
        out[2 * H + f] = pg2[t];
        out[3 * H + f] = pb2[t];
      }
    }
  }
}

// ===================================================================================================
// fixed-order reductions
// ===================================================================================================
__global__ void __launch_bounds__(256) mlp_finish_kernel(const float* __restrict__ slab, int P,
                                                         const float* __restrict__ e, int64_t ne, int mode, float invB,
                                                         const float* __restrict__ b3p, float lam,
                                                         float* __restrict__ out) {
  __shared__ float red[3][4];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < P; i += 256) {
    s0 += slab[2 * i];
    s1 += slab[2 * i + 1];
  }
  for (int64_t i = threadIdx.x; i < ne; i += 256) s2 += e[i];
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = s0;
    red[1][w] = s1;
    red[2][w] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float b3 = b3p ? b3p[0] : 0.f;
    const float a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const float b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const float c = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    if (mode == 0) {
      const float wr = -(a * invB + b3), wf = b * invB + b3, pen = c * invB;
      out[0] = wr + wf + lam * pen;
      out[1] = wr;
      out[2] = wf;
      out[3] = pen;
    } else if (mode == 1) {  // generator W loss on the fake rows: W(fake, -1) = -mean s
      out[0] = -(a * invB + b3);
      out[1] = out[2] = out[3] = 0.f;
    } else {  // BCE: the slab holds the per-row losses; invB = 1 / rows gives their mean
      out[0] = a * invB;
      out[1] = out[2] = out[3] = 0.f;
    }
  }
}

// out[k][j] += sum_p slab[p][k L + j] for the nseg segments: 64 elements per workgroup, the 16 waves
// split the P rows (4 partial sums each so loads overlap), combined in a fixed order (deterministic)
// (slab rows have `stride` floats; the summed columns start at col0)
__global__ void __launch_bounds__(1024) mlp_slab_sum_kernel(const float* __restrict__ slab, int P, int64_t stride,
                                                            int col0, int L, int nseg, float* __restrict__ o0,
                                                            float* __restrict__ o1, float* __restrict__ o2,
                                                            float* __restrict__ o3) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane, n = nseg * L;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n) {
    const float* col = slab + col0 + i;
    int p = wv;
    for (; p + 48 < P; p += 64) {
      s0 += col[(int64_t)p * stride];
      s1 += col[(int64_t)(p + 16) * stride];
      s2 += col[(int64_t)(p + 32) * stride];
      s3 += col[(int64_t)(p + 48) * stride];
    }
    for (; p < P; p += 16) s0 += col[(int64_t)p * stride];
  }
  part[wv][lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (wv == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += part[w][lane];
    const int k = i / L, j = i - k * L;
    float* o = k == 0 ? o0 : k == 1 ? o1 : k == 2 ? o2 : o3;
    if (o) o[j] += t;
  }
}

// ===================================================================================================
// host launchers
// ===================================================================================================
bool mlp_supported(int F, int H) { return H == 100 && (F == 32 || F == 36); }

int mlp_slab_rows(int64_t M) {
  const int64_t ntile = (M + 31) / 32;
  const int64_t want = (ntile + MLP_WAVES - 1) / MLP_WAVES;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)device_cu_count() * 2)) * MLP_WAVES;
}

void launch_mlp_gen_fwd(int dt, const void* noise, const MlpGen& g, void* out, int64_t M, int F, int H,
                        hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    // fp32 at F = 32: the split bf16 products (the three weight planes fit LDS: 136 KB; F = 36 needs 166)
    if constexpr (std::is_same_v<T, float> && FF == 32) {
      if (!fp32_exact_mode()) {
        mlp_launch<GenFwdLds<f32s_t, 32, 100>>(mlp_gen_fwd_kernel<float, 32, 100, f32s_t>, GRID_TILES, M, s,
                                               (const float*)noise, g, (float*)out, M);
        return;
      }
    }
    mlp_launch<GenFwdLds<T, FF, 100>>(mlp_gen_fwd_kernel<T, FF, 100>, GRID_TILES, M, s, (const T*)noise, g, (T*)out, M);
  });
}

void launch_mlp_gen_bwd(int dt, const void* noise, const void* dfake, const MlpGen& g, void* dz1, void* u1,
                        void* dz2, void* u2, float* lnslab, int64_t M, int F, int H, hipStream_t s) {
  if (M <= 0) return;
  MLP_DISPATCH(dt, F, H, {
    mlp_launch<GenBwdLds<T, FF, 100>>(mlp_gen_bwd_kernel<T, FF, 100>, GRID_SLAB, M, s, (const T*)noise, (const T*)dfake,
                                      g, (T*)dz1, (T*)u1, (T*)dz2, (T*)u2, lnslab, M);
  });
}

// ---- generator reverse with in-kernel parameter gradients (bf16) ----
int mlp_gbw_blocks(int64_t M) {
  const int64_t nbt = (M + 127) / 128;
  return (int)std::max<int64_t>(1, std::min<int64_t>(nbt, (int64_t)device_cu_count()));
}

void launch_mlp_gen_bwd_w(const void* noise, const void* dfake, const MlpGen& g, float* gslab, float* lnslab, int64_t M,
                          int F, hipStream_t s) {
  if (M <= 0) return;
  const bf16_t *z = (const bf16_t*)noise, *df = (const bf16_t*)dfake;
  const int P = mlp_gbw_blocks(M);
  if (F == 32) mlp_launch<GbwLds<32, 100>>(mlp_gen_bwd_w_kernel<32, 100>, GRID_BLOCKS, P, s, z, df, g, gslab, lnslab, M);
  else if (F == 36) mlp_launch<GbwLds<36, 100>>(mlp_gen_bwd_w_kernel<36, 100>, GRID_BLOCKS, P, s, z, df, g, gslab, lnslab, M);
  else throw std::runtime_error("mlp_gen_bwd_w: F in {32, 36}");
}

void launch_mlp_finish(const float* slab, int P, const float* e, int64_t n_e, int mode, float invB, const float* b3,
                       float lam, float* out, hipStream_t s) {
  hipLaunchKernelGGL(mlp_finish_kernel, dim3(1), dim3(256), 0, s, slab, P, e, n_e, mode, invB, b3, lam, out);
}

void launch_mlp_slab_sum_segs(const float* slab, int P, int64_t stride, int col0, int L, int nseg, float* o0, float* o1,
                              float* o2, float* o3, hipStream_t s) {
  hipLaunchKernelGGL(mlp_slab_sum_kernel, dim3((nseg * L + 63) / 64), dim3(1024), 0, s, slab, P, stride, col0, L, nseg,
                     o0, o1, o2, o3);
}
void launch_mlp_slab_sum(const float* slab, int P, int L, float* out, hipStream_t s) {
  launch_mlp_slab_sum_segs(slab, P, L, 0, L, 1, out, nullptr, nullptr, nullptr, s);
}
void launch_mlp_slab_sum4(const float* slab, int P, int L, float* o0, float* o1, float* o2, float* o3, hipStream_t s) {
  launch_mlp_slab_sum_segs(slab, P, (int64_t)4 * L, 0, L, 4, o0, o1, o2, o3, s);
}
void launch_mlp_slab_sum_cols(const float* slab, int P, int64_t stride, int col0, int L, float* out, hipStream_t s) {
  launch_mlp_slab_sum_segs(slab, P, stride, col0, L, 1, out, nullptr, nullptr, nullptr, s);
}

}  // namespace hfrep
