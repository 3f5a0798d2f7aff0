// GAN_eval's marginal-shape, temporal and classifier metrics on the device (GAN/GAN_eval.py: ks_test,
// ACF, lp_dist, kl_div / js_div / Inception_score).  fp32 inputs, float64 sums (and float64 arithmetic
// where the formula needs it), partials per workgroup or per wave reduced in one fixed order: no
// atomics, so every result is a pure function of the inputs, bit for bit (the contract of wdist.hip).
//
//   ks_stat         two-sample Kolmogorov-Smirnov statistic per column against a pre-sorted sample
//   acf_mean        sample-averaged autocorrelation of every feature of (N, T, F) windows
//   nb_divergences  KL / JS sums of paired Gaussian-naive-Bayes posteriors of real and fake series
//   lp_cols         column-wise sum |d|, sum d^2, max |d| of a difference
#include "chunk_sort.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>

namespace hfrep {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// ======================================================================================== KS
// The chunk-sorted keys of a column are merged into one ascending column (ks_merge_pass: runs of L
// keys into runs of 2 L, ping-pong between two workspaces), then
// D_f = max_v |c_x(v) - c_r(v)| / n over every v of x[:, f] and of ref_sorted[f], with the right-
// continuous counts c_x(v) = upper_bound(sorted x[:, f], v) and c_r(v) = upper_bound(ref_sorted[f], v).
// Integer maximum, one division: exact whatever the reduction order.
// The counts compare total-order keys; the QUERY key of -0 is that of +0 (the two compare equal as
// floats, but have adjacent keys), so zeros of either sign on either side count as one value.  A NaN
// in x[:, f] or ref_sorted[f] makes D_f NaN (every element of both is visited as a query).
constexpr int kKsElems = 2048;  // query points per workgroup (8 per thread)
constexpr int kMergeTile = 4096;  // merged keys per workgroup; divides kChunk, so a tile lies in one pair of runs

// grid (ceil(n / kMergeTile), F).  Column f of src is sorted in runs of L keys (the last run may be
// shorter); run pair p = (A, B) merges into dst[p 2L ..), A first among equal keys.  The workgroup
// owns merged positions [d0, d1) of its pair: the merge-path split of a diagonal d is the a in
// [max(0, d - lenB), min(d, lenA)] with A[a - 1] <= B[d - a] and B[d - a - 1] < A[a], found by binary
// search; the keys A[a0 .. a1) and B[b0 .. b1) go to LDS and every key's place is its own index plus its
// rank in the other part (lower_bound for a key of A, upper_bound for a key of B: a permutation).
__global__ void __launch_bounds__(kThreads) ks_merge_pass(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                          int n, int L) {
  __shared__ uint32_t s[kMergeTile];
  __shared__ int split[2];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int o0 = blockIdx.x * kMergeTile, o1 = min(n, o0 + kMergeTile);  // o0 < n: the grid has ceil(n / tile) tiles
  const int base = (int)((int64_t)o0 / (2 * (int64_t)L) * (2 * (int64_t)L));
  const int lenA = min(L, n - base), lenB = min(L, n - base - lenA);  // lenA >= 1, lenB >= 0
  const uint32_t* A = src + (size_t)f * n + base;
  const uint32_t* B = A + lenA;  // never read when lenB == 0
  if (tid < 2) {
    const int d = (tid == 0 ? o0 : o1) - base;  // 0 <= d <= lenA + lenB
    int lo = max(0, d - lenB), hi = min(d, lenA);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;  // lo <= mid < hi: 0 <= mid < lenA and 0 <= d - 1 - mid < lenB
      if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
      else hi = mid;
    }
    split[tid] = lo;
  }
  __syncthreads();
  const int a0 = split[0], a1 = split[1], b0 = o0 - base - a0, b1 = o1 - base - a1;
  const int na = a1 - a0, nb = b1 - b0;  // na + nb = o1 - o0 <= kMergeTile
  for (int i = tid; i < na; i += kThreads) s[i] = A[a0 + i];
  for (int j = tid; j < nb; j += kThreads) s[na + j] = B[b0 + j];
  __syncthreads();
  uint32_t* out = dst + (size_t)f * n + o0;
  for (int i = tid; i < na; i += kThreads) out[i + bound<false>(s + na, nb, s[i])] = s[i];
  for (int j = tid; j < nb; j += kThreads) out[j + bound<true>(s, na, s[na + j])] = s[na + j];
}

__device__ __forceinline__ uint32_t ks_query_key(uint32_t bits) {
  return key_of(bits == 0x80000000u ? 0u : bits);
}

// number of elements of the ascending floats a[0 .. len) whose key is <= key
__device__ __forceinline__ int ks_upper_f32(const float* __restrict__ a, int len, uint32_t key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key_of(__float_as_uint(a[mid])) <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// grid (nblk, F, 2): z = 0 queries the elements of x (ws: its columns as ascending keys), z = 1 those of
// the reference
__global__ void __launch_bounds__(kThreads) ks_eval(const uint32_t* __restrict__ ws, const float* __restrict__ ref,
                                                    double* __restrict__ slab, int n, int F, int nblk) {
  __shared__ double part[kWaves];
  const int f = blockIdx.y, side = blockIdx.z, tid = threadIdx.x;
  const uint32_t* col = ws + (size_t)f * n;
  const float* rcol = ref + (size_t)f * n;
  double best = 0.0;  // max |c_x - c_r| so far (an integer), or NaN
  const int g0 = blockIdx.x * kKsElems;
  for (int e = 0; e < kKsElems / kThreads; ++e) {
    const int g = g0 + e * kThreads + tid;
    if (g < n) {
      const float v = side == 0 ? value_of(col[g]) : rcol[g];
      if (v != v) {
        best = __longlong_as_double(0x7FF8000000000000ll);
      } else {
        const uint32_t key = ks_query_key(__float_as_uint(v));
        const int cx = bound<true>(col, n, key), cr = ks_upper_f32(rcol, n, key);
        const double d = (double)abs(cx - cr);
        if (d > best) best = d;  // false once best is NaN: the NaN stays
      }
    }
  }
  // NaN-keeping maximum: within the wave, then the waves in order
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(best, off, 64);
    if (o > best || o != o) best = o;
  }
  if ((tid & 63) == 0) part[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    double t = part[0];
    for (int w = 1; w < kWaves; ++w)
      if (part[w] > t || part[w] != part[w]) t = part[w];
    slab[((size_t)f * 2 + side) * nblk + blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(kThreads) ks_finish(const double* __restrict__ slab, double* __restrict__ out, int n,
                                                      int F, int nblk) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const double* p = slab + (size_t)f * 2 * nblk;
  double t = 0.0;
  for (int b = 0; b < 2 * nblk; ++b)
    if (p[b] > t || p[b] != p[b]) t = p[b];
  out[f] = t / (double)n;
}

// ======================================================================================== ACF
// One workgroup per window at a time: the T x F tile is loaded coalesced into LDS, thread f forms the
// mean and the lag-0 sum of feature f over T in float64, then item i = k F + f (lag k of feature f)
// belongs to thread i % kThreads, which adds sum_t (x_t - m)(x_{t+k} - m) / lag0 to its float64
// accumulator in LDS.  The workgroup walks windows b, b + nblk, ...; its accumulators are one slab row.
// k >= T is NaN and a constant series is 0 / 0 = NaN, as in numpy.
// dynamic LDS: float tile[T F]; double mean[F], den[F], acc[items]
__global__ void __launch_bounds__(kThreads) acf_accum(const float* __restrict__ x, double* __restrict__ slab, int N,
                                                      int T, int F, int L) {
  extern __shared__ double acf_lds[];
  const int items = L * F, tid = threadIdx.x;
  double* mean = acf_lds;
  double* den = mean + F;
  double* acc = den + F;
  float* tile = reinterpret_cast<float*>(acc + items);
  for (int i = tid; i < items; i += kThreads) acc[i] = 0.0;
  const int TF = T * F;
  for (int w = blockIdx.x; w < N; w += gridDim.x) {
    const float* src = x + (size_t)w * TF;
    __syncthreads();  // the previous window's readers are done with the tile
    for (int i = tid; i < TF; i += kThreads) tile[i] = src[i];
    __syncthreads();
    for (int f = tid; f < F; f += kThreads) {
      double s = 0.0;
      for (int t = 0; t < T; ++t) s += (double)tile[t * F + f];
      const double m = s / (double)T;
      double q = 0.0;
      for (int t = 0; t < T; ++t) {
        const double d = (double)tile[t * F + f] - m;
        q += d * d;
      }
      mean[f] = m;
      den[f] = q;
    }
    __syncthreads();
    for (int i = tid; i < items; i += kThreads) {
      const int k = i / F, f = i - k * F;
      double r = __longlong_as_double(0x7FF8000000000000ll);
      if (k < T) {
        const double m = mean[f];
        double s = 0.0;
        for (int t = 0; t + k < T; ++t) s += ((double)tile[t * F + f] - m) * ((double)tile[(t + k) * F + f] - m);
        r = s / den[f];
      }
      acc[i] += r;
    }
  }
  double* row = slab + (size_t)blockIdx.x * items;
  for (int i = tid; i < items; i += kThreads) row[i] = acc[i];
}

// out[f (L) + k] = (sum over the slab rows, in order, of item k F + f) / N
__global__ void __launch_bounds__(kThreads) acf_finish(const double* __restrict__ slab, double* __restrict__ out, int N,
                                                       int F, int L, int nblk) {
  const int items = L * F, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= items) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += slab[(size_t)b * items + i];
  const int k = i / F, f = i - k * F;
  out[f * L + k] = t / (double)N;
}

// ======================================================================================== NB
// Series r = (n, f) is x[n, :, f].  Lane c of a wave holds class c: jll_c = log_prior_c
// - 1/2 sum_t log(2 pi var_ct) - 1/2 sum_t (x_t - theta_ct)^2 / var_ct, the posteriors are
// exp(jll - logsumexp(jll)) with a wave-level maximum and sum, and the class sums of the rel_entr
// terms are wave-level sums (butterfly: a fixed order, every lane holds the total).  All float64.
// A workgroup stages one real and one fake window in LDS and its waves take the series f = wave,
// wave + 4, ...; every wave keeps its four running sums and writes one slab row.
// TAB_LDS: theta and var are staged in LDS as (T, C) tables (conflict-free across the lanes); else
// each lane walks its own rows of the (C, T) tables in global memory (L1 / L2 resident).
// dynamic LDS: [double th[T C], va[T C]] float real[T F], fake[T F]
__device__ __forceinline__ double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// scipy.special.rel_entr: x log(x / y) for x, y > 0; 0 for x == 0, y >= 0; +inf otherwise
__device__ __forceinline__ double rel_entr(double x, double y) {
  if (x != x || y != y) return x + y;
  if (x > 0.0 && y > 0.0) return x * log(x / y);
  if (x == 0.0 && y >= 0.0) return 0.0;
  return __longlong_as_double(0x7FF0000000000000ll);
}

template <bool TAB_LDS>
__global__ void __launch_bounds__(kThreads) nb_accum(const float* __restrict__ real, const float* __restrict__ fake,
                                                     const double* __restrict__ theta, const double* __restrict__ var,
                                                     const double* __restrict__ log_prior, double* __restrict__ slab,
                                                     int N, int T, int F) {
  extern __shared__ double nb_lds[];
  const int C = F, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int TF = T * F;
  double* th = nb_lds;
  double* va = th + (TAB_LDS ? TF : 0);
  float* tr = reinterpret_cast<float*>(va + (TAB_LDS ? TF : 0));
  float* tf = tr + TF;
  if (TAB_LDS) {
    for (int i = tid; i < TF; i += kThreads) {
      const int c = i / T, t = i - c * T;
      th[t * C + c] = theta[i];
      va[t * C + c] = var[i];
    }
    __syncthreads();
  }
  const bool on = lane < C;
  const int c = on ? lane : 0;
  const double* thc = TAB_LDS ? th + c : theta + (size_t)c * T;
  const double* vac = TAB_LDS ? va + c : var + (size_t)c * T;
  const int ts = TAB_LDS ? C : 1;  // table stride between time steps
  double base = 0.0;               // log_prior_c - 1/2 sum_t log(2 pi var_ct)
  {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += log(2.0 * 3.14159265358979323846 * vac[t * ts]);
    base = log_prior[c] - 0.5 * s;
  }
  const double ninf = __longlong_as_double(0xFFF0000000000000ll);
  double a_kl = 0.0, a_skl = 0.0, a_js = 0.0, a_sjs = 0.0;
  for (int w = blockIdx.x; w < N; w += gridDim.x) {
    __syncthreads();  // the previous window's readers are done with the tiles
    const float* sr = real + (size_t)w * TF;
    const float* sf = fake + (size_t)w * TF;
    for (int i = tid; i < TF; i += kThreads) {
      tr[i] = sr[i];
      tf[i] = sf[i];
    }
    __syncthreads();
    for (int f = wave; f < F; f += kWaves) {
      double qr = 0.0, qf = 0.0;
      for (int t = 0; t < T; ++t) {
        const double m = thc[t * ts], v = vac[t * ts];
        const double dr = (double)tr[t * F + f] - m, df = (double)tf[t * F + f] - m;
        qr += dr * dr / v;
        qf += df * df / v;
      }
      const double jr = on ? base - 0.5 * qr : ninf, jf = on ? base - 0.5 * qf : ninf;
      const double mr = wave_max(jr), mf = wave_max(jf);
      const double er = on ? exp(jr - mr) : 0.0, ef = on ? exp(jf - mf) : 0.0;
      const double lr = log(wave_sum(er)) + mr, lf = log(wave_sum(ef)) + mf;
      const double pr = exp(jr - lr), pf = exp(jf - lf);
      const double mid = 0.5 * (pf + pr);
      const double kl = wave_sum(on ? rel_entr(pf, pr) : 0.0);
      const double js = 0.5 * wave_sum(on ? rel_entr(pf, mid) : 0.0) + 0.5 * wave_sum(on ? rel_entr(pr, mid) : 0.0);
      a_kl += kl;
      a_skl += sqrt(kl);
      a_js += js;
      a_sjs += sqrt(js);
    }
  }
  if (lane == 0) {
    double* row = slab + ((size_t)blockIdx.x * kWaves + wave) * 4;
    row[0] = a_kl;
    row[1] = a_skl;
    row[2] = a_js;
    row[3] = a_sjs;
  }
}

__global__ void __launch_bounds__(64) nb_finish(const double* __restrict__ slab, double* __restrict__ out, int rows) {
  const int j = threadIdx.x;
  if (j >= 4) return;
  double t = 0.0;
  for (int r = 0; r < rows; ++r) t += slab[(size_t)r * 4 + j];
  out[j] = t;
}

// ======================================================================================== Lp
// grid (nblk, column tiles of CW = min(F, 256)): thread tid holds column tid % CW of the rows
// tid / CW, tid / CW + R, ... (R = 256 / CW) of its workgroup's row range, so a wave reads consecutive
// addresses; the R partials of a column are combined in row-offset order, one slab entry per
// workgroup, and lp_finish combines the workgroups in order.  d = double(a) - double(b).
__global__ void __launch_bounds__(kThreads) lp_accum(const float* __restrict__ a, const float* __restrict__ b,
                                                     double* __restrict__ slab, int n, int F, int CW, int rows_per) {
  __shared__ double part[3][kThreads];
  const int tid = threadIdx.x, R = kThreads / CW;
  const int cl = tid % CW, ro = tid / CW, col = blockIdx.y * CW + cl;
  const int r0 = blockIdx.x * rows_per, r1 = min(n, r0 + rows_per);
  double s1 = 0.0, s2 = 0.0, mx = 0.0;
  if (ro < R && col < F) {
    for (int r = r0 + ro; r < r1; r += R) {
      const size_t at = (size_t)r * F + col;
      const double d = fabs((double)a[at] - (double)b[at]);
      s1 += d;
      s2 += d * d;
      if (d > mx || d != d) mx = d;  // a NaN stays
    }
  }
  part[0][tid] = s1;
  part[1][tid] = s2;
  part[2][tid] = mx;
  __syncthreads();
  if (tid < CW && col < F) {
    for (int q = 1; q < R; ++q) {
      s1 += part[0][q * CW + cl];
      s2 += part[1][q * CW + cl];
      const double o = part[2][q * CW + cl];
      if (o > mx || o != o) mx = o;
    }
    double* row = slab + (size_t)blockIdx.x * 3 * F;
    row[col] = s1;
    row[F + col] = s2;
    row[2 * F + col] = mx;
  }
}

__global__ void __launch_bounds__(kThreads) lp_finish(const double* __restrict__ slab, double* __restrict__ out, int F,
                                                      int nblk) {
  const int i = blockIdx.x * kThreads + threadIdx.x;  // (kind, column)
  if (i >= 3 * F) return;
  double t = 0.0;
  if (i < 2 * F) {
    for (int b = 0; b < nblk; ++b) t += slab[(size_t)b * 3 * F + i];
  } else {
    for (int b = 0; b < nblk; ++b) {
      const double o = slab[(size_t)b * 3 * F + i];
      if (o > t || o != o) t = o;
    }
  }
  out[i] = t;
}

constexpr size_t kLdsMax = 160 * 1024;

template <typename KER>
void allow_lds(KER kern, size_t lds) {
  if (lds > 64 * 1024)
    HFREP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kLdsMax));
}

}  // namespace

// ---- KS ----
int ks_blocks(int n) { return (n + kKsElems - 1) / kKsElems; }

void launch_ks_stat(const float* x, const float* ref_sorted, uint32_t* ws, uint32_t* ws2, double* slab, double* out,
                    int n, int F, hipStream_t s) {
  const int chunks = (n + kChunk - 1) / kChunk, nblk = ks_blocks(n);
  hipLaunchKernelGGL(wdist_chunk_sort<false>, dim3(chunks, F), dim3(kSortThreads), 0, s, x, ws, n, F);
  for (int64_t L = kChunk; L < n; L *= 2) {  // ws2 is touched only when n > kChunk
    hipLaunchKernelGGL(ks_merge_pass, dim3((n + kMergeTile - 1) / kMergeTile, F), dim3(kThreads), 0, s, ws, ws2, n,
                       (int)L);
    std::swap(ws, ws2);
  }
  hipLaunchKernelGGL(ks_eval, dim3(nblk, F, 2), dim3(kThreads), 0, s, ws, ref_sorted, slab, n, F, nblk);
  hipLaunchKernelGGL(ks_finish, dim3((F + kThreads - 1) / kThreads), dim3(kThreads), 0, s, slab, out, n, F, nblk);
}

// ---- ACF ----
size_t acf_lds_bytes(int T, int F, int L) { return (size_t)(2 * F + L * F) * 8 + (size_t)T * F * 4; }
bool acf_supported(int T, int F, int nlags) { return nlags >= 0 && acf_lds_bytes(T, F, nlags + 1) <= kLdsMax; }
int acf_blocks(int N) { return std::min(N, 1024); }

void launch_acf_mean(const float* x, double* slab, double* out, int N, int T, int F, int nlags, hipStream_t s) {
  const int L = nlags + 1, nblk = acf_blocks(N), items = L * F;
  const size_t lds = acf_lds_bytes(T, F, L);
  allow_lds(acf_accum, lds);
  hipLaunchKernelGGL(acf_accum, dim3(nblk), dim3(kThreads), lds, s, x, slab, N, T, F, L);
  hipLaunchKernelGGL(acf_finish, dim3((items + kThreads - 1) / kThreads), dim3(kThreads), 0, s, slab, out, N, F, L, nblk);
}

// ---- NB ----
bool nb_supported(int T, int F) { return T >= 1 && F >= 1 && F <= 64 && T <= 168; }
int nb_blocks(int N) { return std::min(N, 1024); }
int nb_slab_rows(int N) { return nb_blocks(N) * kWaves; }

void launch_nb_divergences(const float* real, const float* fake, const double* theta, const double* var,
                           const double* log_prior, double* slab, double* out, int N, int T, int F, hipStream_t s) {
  const int nblk = nb_blocks(N);
  const size_t tiles = (size_t)T * F * 8, tabs = (size_t)T * F * 16;
  if (tiles + tabs <= kLdsMax) {
    allow_lds(nb_accum<true>, tiles + tabs);
    hipLaunchKernelGGL(nb_accum<true>, dim3(nblk), dim3(kThreads), tiles + tabs, s, real, fake, theta, var, log_prior,
                       slab, N, T, F);
  } else {
    allow_lds(nb_accum<false>, tiles);
    hipLaunchKernelGGL(nb_accum<false>, dim3(nblk), dim3(kThreads), tiles, s, real, fake, theta, var, log_prior, slab,
                       N, T, F);
  }
  hipLaunchKernelGGL(nb_finish, dim3(1), dim3(64), 0, s, slab, out, nblk * kWaves);
}

// ---- Lp ----
int lp_blocks(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 1024); }

void launch_lp_cols(const float* a, const float* b, double* slab, double* out, int64_t n, int F, hipStream_t s) {
  const int nblk = lp_blocks(n), CW = std::min(F, kThreads);
  const int rows_per = (int)((n + nblk - 1) / nblk);
  hipLaunchKernelGGL(lp_accum, dim3(nblk, (F + CW - 1) / CW), dim3(kThreads), 0, s, a, b, slab, (int)n, F, CW, rows_per);
  hipLaunchKernelGGL(lp_finish, dim3((3 * F + kThreads - 1) / kThreads), dim3(kThreads), 0, s, slab, out, F, nblk);
}

}  // namespace hfrep
