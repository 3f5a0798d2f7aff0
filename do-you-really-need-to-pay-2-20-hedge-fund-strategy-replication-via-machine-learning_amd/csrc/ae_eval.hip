// Factor-autoencoder evaluation on the device (gfx950): the in-sample and out-of-sample reconstruction
// metrics (R^2, RMSE) of every autoencoder of a study in one launch chain, with the reference's
// every-window OOS procedure (Autoencoder_encapsulate.py:115-131: a MinMaxScaler refit on every
// expanding window x_test[:i]) and no scaled copy of the data anywhere.
//
// ae_window_table: per (window, column) the refit scaler (scale_, min_: bitwise data/scaler.py) and
//   ss_tot of the scaled window; a panel's table is shared by every autoencoder evaluated on it.
// ae_recon_metrics<BF>: one wave per (autoencoder, window).  Lanes stride the window's rows; a row is
//   scaled in fp64 (the host's `transform`), rounded to the compute dtype (the host's upload), run
//   through lrelu(lrelu(xs We) Wd) with dense_lrelu<BF>'s arithmetic (ae.hip: fp32 fmaf over the input
//   index ascending, rounding at the pre-activation and at the LeakyReLU output), and its residual
//   against the UNROUNDED fp64 xs is squared into per-lane, per-column fp64 sums.  The wave reduces
//   them by a fixed butterfly: a window's result depends on nothing but its own rows and weights (no
//   atomics, no dependence on the grid, on other windows or on other jobs).
//
// Registers: ae_recon_metrics needs 254 VGPRs, no scratch, two waves per SIMD.  That rests on two pieces of
// compiler steering in the kernel (the scaler row read through volatile LDS pointers, and an empty asm that
// makes the residual reload its panel row); after a toolchain change check the kernel's line of
// -Rpass-analysis=kernel-resource-usage again (profiles/ae_metrics_device/kernel_resource_usage.txt).
//
// Brute force over rows is the design: windows sharing a scaler could share predictions, but every
// window standing alone keeps the kernel simple and its results independent of the window list.
#include "ae_dev.h"
#include "common.h"
#include "kernels.h"

// the fp64 expressions below are numpy's, operation by operation (a multiply, then an add): the build's
// -ffp-contract=fast must not fuse them.  (The fp32 forward calls fmaf explicitly.)
#pragma clang fp contract(off)

namespace hfrep {

namespace {

// fixed-order wave reductions of one double per lane: every lane gets the result
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ void __launch_bounds__(kWave)
ae_window_table_kernel(const double* __restrict__ X, const int* __restrict__ ends, double* __restrict__ scale,
                       double* __restrict__ mn, double* __restrict__ sstot, int A, int n, int W, bool refit) {
  // one wave per (window, column), the longest windows first (`ends` ascends)
  const int w = W - 1 - (int)(blockIdx.x / A), c = blockIdx.x % A, lane = threadIdx.x;
  const int i = min(max(ends[w], 0), n);
  const double* __restrict__ x = X + (size_t)c * n;
  double sc = 1.0, m0 = 0.0;
  if (refit && i > 0) {
    double lo = x[0], hi = x[0];
    for (int r = lane; r < i; r += kWave) {
      lo = fmin(lo, x[r]);
      hi = fmax(hi, x[r]);
    }
    lo = wave_min_d(lo);
    hi = wave_max_d(hi);
    double rng = hi - lo;
    if (rng == 0.0) rng = 1.0;
    sc = 1.0 / rng;
    m0 = 0.0 - lo * sc;
  }
  // two-pass ss_tot of the scaled column: lane partials over rows ascending, then the butterfly
  double s = 0.0;
  for (int r = lane; r < i; r += kWave) s += x[r] * sc + m0;
  const double mean = wave_sum_d(s) / (double)max(i, 1);
  double q = 0.0;
  for (int r = lane; r < i; r += kWave) {
    const double d = (x[r] * sc + m0) - mean;
    q += d * d;
  }
  q = wave_sum_d(q);
  if (lane == 0) {
    const size_t o = (size_t)w * A + c;
    scale[o] = sc;
    mn[o] = m0;
    sstot[o] = q;
  }
}

template <bool BF>
__global__ void __launch_bounds__(kWave)
ae_recon_metrics_kernel(const AeEvalJob* __restrict__ jobs, int njobs, const int* __restrict__ work, int A) {
  const int ji = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
  if (ji < 0 || ji >= njobs) return;
  const AeEvalJob& J = jobs[ji];
  if (w < 0 || w >= J.W) return;
  const int n = J.n, k = J.k, lane = threadIdx.x;
  const int i = min(max(J.ends[w], 0), n);
  const double* __restrict__ X = J.X;
  // weights as the forward reads them: encoder transposed (unit j's A inputs contiguous), decoder as
  // stored (unit j's A outputs contiguous), rows padded with zeros to 32 so that the loops below run
  // in 4-wide steps (a zero weight times the zero input of a padding column adds +0: exact)
  __shared__ __attribute__((aligned(16))) float weT[AE_MAXK * AE_MAXA], wd[AE_MAXK * AE_MAXA];
  // the window's scaler row: read through volatile pointers, as LDS broadcasts where they are used (hoisted
  // out of the row loop the 64 doubles would cost 128 VGPRs and the second wave per SIMD)
  __shared__ double sc_[AE_MAXA], mn_[AE_MAXA], st[AE_MAXA];
  volatile double* sc = sc_;
  volatile double* mn = mn_;
  for (int e = lane; e < k * AE_MAXA; e += kWave) {
    const int j = e / AE_MAXA, a = e % AE_MAXA;
    weT[e] = a < A ? rnd<BF>(J.We[a * k + j]) : 0.f;
    wd[e] = a < A ? rnd<BF>(J.Wd[j * A + a]) : 0.f;
  }
  if (lane < AE_MAXA) {
    const bool in = lane < A;
    sc[lane] = in ? J.scale[(size_t)w * A + lane] : 0.0;
    mn[lane] = in ? J.mn[(size_t)w * A + lane] : 0.0;
    st[lane] = in ? J.sstot[(size_t)w * A + lane] : 0.0;
  }
  __syncthreads();
  double acc[AE_MAXA];
#pragma unroll
  for (int c = 0; c < AE_MAXA; ++c) acc[c] = 0.0;
  for (int r = lane; r < i; r += kWave) {
    float x[AE_MAXA], y[AE_MAXA];
#pragma unroll
    for (int c = 0; c < AE_MAXA; ++c) {
      double xs = 0.0;
      if (c < A) xs = X[(size_t)c * n + r] * sc[c] + mn[c];
      x[c] = rnd<BF>((float)xs);
      y[c] = 0.f;
    }
    for (int j = 0; j < k; ++j) {
      float s = 0.f;
#pragma unroll
      for (int a = 0; a < AE_MAXA; a += 4) {
        if (a < A) {
          const float4 wv = *reinterpret_cast<const float4*>(&weT[j * AE_MAXA + a]);
          s = fmaf(x[a], wv.x, s);
          s = fmaf(x[a + 1], wv.y, s);
          s = fmaf(x[a + 2], wv.z, s);
          s = fmaf(x[a + 3], wv.w, s);
        }
      }
      const float h = rnd<BF>(lrelu(rnd<BF>(s)));
      // the decoder's sums grow by one hidden unit at a time: input index ascending, as dense_lrelu
#pragma unroll
      for (int c = 0; c < AE_MAXA; c += 4) {
        if (c < A) {
          const float4 wv = *reinterpret_cast<const float4*>(&wd[j * AE_MAXA + c]);
          y[c] = fmaf(h, wv.x, y[c]);
          y[c + 1] = fmaf(h, wv.y, y[c + 1]);
          y[c + 2] = fmaf(h, wv.z, y[c + 2]);
          y[c + 3] = fmaf(h, wv.w, y[c + 3]);
        }
      }
    }
    // the residual's unrounded fp64 xs is computed again (the same three operations on the same operands,
    // a cache hit) instead of being held across the forward: 64 VGPRs less.  The empty asm keeps the
    // compiler from reusing the first load.
    asm volatile("" ::: "memory");
#pragma unroll
    for (int c = 0; c < AE_MAXA; ++c) {
      if (c < A) {
        const double xs = X[(size_t)c * n + r] * sc[c] + mn[c];
        const double d = xs - (double)rnd<BF>(lrelu(rnd<BF>(y[c])));
        acc[c] += d * d;
      }
    }
  }
  // per column: ss_res over the wave, then r2_score's and rmse's column values; their means in
  // ascending column order (every lane computes them, lane 0 stores)
  double r2 = 0.0, rm = 0.0;
#pragma unroll
  for (int c = 0; c < AE_MAXA; ++c) {
    if (c < A) {
      const double ssr = wave_sum_d(acc[c]), sst = st[c];
      r2 += sst != 0.0 ? 1.0 - ssr / sst : (ssr == 0.0 ? 1.0 : 0.0);
      rm += sqrt(ssr / (double)max(i, 1));
    }
  }
  if (lane == 0) {
    J.r2[w] = r2 / (double)A;
    J.rmse[w] = rm / (double)A;
  }
}

}  // namespace

void launch_ae_window_table(const double* X, const int* ends, double* scale, double* mn, double* sstot, int A, int n,
                            int W, bool refit, hipStream_t s) {
  if (W <= 0 || A <= 0) return;
  hipLaunchKernelGGL(ae_window_table_kernel, dim3((unsigned)W * (unsigned)A), dim3(kWave), 0, s, X, ends, scale, mn, sstot,
                     A, n, W, refit);
}

void launch_ae_recon_metrics(bool bf16, const AeEvalJob* jobs, int njobs, const int* work, int nwork, int A,
                             hipStream_t s) {
  if (njobs <= 0 || nwork <= 0) return;
  if (bf16)
    hipLaunchKernelGGL(ae_recon_metrics_kernel<true>, dim3(nwork), dim3(kWave), 0, s, jobs, njobs, work, A);
  else
    hipLaunchKernelGGL(ae_recon_metrics_kernel<false>, dim3(nwork), dim3(kWave), 0, s, jobs, njobs, work, A);
}

}  // namespace hfrep
