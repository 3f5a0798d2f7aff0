// Per-feature 1-D Wasserstein distance of a sample against a pre-sorted reference sample of the
// same size (the W-dist parity metric, GAN/GAN_eval.py:309-326, computed on the device).
//
// For equal sample sizes W1 of two empirical distributions is the mean absolute difference of
// their order statistics: W1_f = (1/n) sum_i |xs_f[i] - ref_f[i]|.  The reference sample is fixed
// and arrives sorted; the generated sample x (n, F) is sorted here, without ever materialising the
// merged column:
//
//   (a) wdist_chunk_sort: grid (chunks, F); a workgroup gathers up to kChunk values of column f,
//       maps them to order-preserving 32-bit keys, bitonic-sorts them in LDS and writes the sorted
//       keys of its chunk (valid length only) to the workspace;
//   (b) wdist_rank_pair: the element at local index j of chunk c has the global rank
//         j + sum_{c' < c} upper_bound(chunk c', key) + sum_{c' > c} lower_bound(chunk c', key)
//       (the asymmetry makes the ranks a permutation when equal keys sit in different chunks); its
//       term |double(v) - double(ref_f[rank])| is summed in float64, one partial per workgroup;
//   (c) wdist_finish: one workgroup sums the partials in a fixed order and writes the F per-feature
//       distances and their mean.
//
// No atomics: the result is a pure function of the inputs, bit for bit.
//
// Keys: the IEEE bit pattern with the sign bit flipped (positive) or all bits flipped (negative) is
// a TOTAL order over every bit pattern: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  A float
// comparison would not be one (NaN), and a sorting network fed a non-order may move the +inf pads
// of a short chunk in front of real values.  With the total order the pads (key 0xFFFFFFFF, itself
// the key of a NaN) stay behind every other key, every binary search runs over a chunk's VALID
// length, and the rank is < n by construction for any input: j < len_c and each count <= len_c'.
// A NaN or an infinity in column f pairs with a finite reference value and makes W1_f (and the mean)
// non-finite; the other columns do not see it.
#include "common.h"
#include "kernels.h"

namespace hfrep {

namespace {

constexpr int kChunk = 16384;       // keys per sorted chunk: 64 KB of LDS, two workgroups per CU
constexpr int kSortThreads = 1024;
constexpr int kPairThreads = 256;
constexpr int kPairElems = 2048;    // elements per rank-and-pair workgroup (8 per thread)

__device__ __forceinline__ uint32_t key_of(uint32_t bits) {
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  const uint32_t bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  return __uint_as_float(bits);
}

template <bool BF16>
__global__ void __launch_bounds__(kSortThreads) wdist_chunk_sort(const void* __restrict__ x, uint32_t* __restrict__ ws,
                                                                 int n, int F) {
  __shared__ uint32_t s[kChunk];
  const int c = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int base = c * kChunk;
  const int len = min(kChunk, n - base);  // >= 1: the grid has ceil(n / kChunk) chunks
  int P = 1;                              // the sorting network's size: the next power of two >= len
  while (P < len) P <<= 1;
  for (int i = tid; i < P; i += kSortThreads) {
    uint32_t k = 0xFFFFFFFFu;  // pad: not below any key
    if (i < len) {
      const size_t at = (size_t)(base + i) * F + f;
      const uint32_t bits = BF16 ? ((uint32_t) reinterpret_cast<const uint16_t*>(x)[at] << 16)
                                 : reinterpret_cast<const uint32_t*>(x)[at];
      k = key_of(bits);
    }
    s[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kSortThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // t with a zero inserted at bit log2(j)
        const int hi = lo | j;
        const uint32_t a = s[lo], b = s[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) {
          s[lo] = b;
          s[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  uint32_t* dst = ws + (size_t)f * n + base;
  for (int i = tid; i < len; i += kSortThreads) dst[i] = s[i];
}

// number of keys <= key (UPPER) or < key in the sorted a[0 .. len)
template <bool UPPER>
__device__ __forceinline__ int bound(const uint32_t* __restrict__ a, int len, uint32_t key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint32_t v = a[mid];
    if (UPPER ? (v <= key) : (v < key)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(kPairThreads) wdist_rank_pair(const uint32_t* __restrict__ ws,
                                                                const float* __restrict__ ref, double* __restrict__ slab,
                                                                int n, int F, int nblk) {
  __shared__ double part[kPairThreads / 64];
  const int f = blockIdx.y, tid = threadIdx.x;
  const uint32_t* col = ws + (size_t)f * n;
  const float* rcol = ref + (size_t)f * n;
  const int chunks = (n + kChunk - 1) / kChunk;
  double acc = 0.0;
  const int g0 = blockIdx.x * kPairElems;
  for (int e = 0; e < kPairElems / kPairThreads; ++e) {
    const int g = g0 + e * kPairThreads + tid;
    if (g < n) {
      const uint32_t key = col[g];
      const int c = g / kChunk;
      int rank = g - c * kChunk;  // < len_c
      for (int o = 0; o < chunks; ++o) {
        if (o == c) continue;
        const int len = min(kChunk, n - o * kChunk);
        rank += o < c ? bound<true>(col + (size_t)o * kChunk, len, key) : bound<false>(col + (size_t)o * kChunk, len, key);
      }
      acc += fabs((double)value_of(key) - (double)rcol[rank]);
    }
  }
  // fixed-order tree within the wave, then the waves in order
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = part[0];
    for (int w = 1; w < kPairThreads / 64; ++w) t += part[w];
    slab[(size_t)f * nblk + blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(256) wdist_finish(const double* __restrict__ slab, double* __restrict__ out, int n,
                                                    int F, int nblk) {
  __shared__ double w1[1024];  // F <= 1024
  for (int f = threadIdx.x; f < F; f += 256) {
    const double* p = slab + (size_t)f * nblk;
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += p[b];
    t /= (double)n;
    w1[f] = t;
    out[f] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int f = 0; f < F; ++f) t += w1[f];
    out[F] = t / (double)F;
  }
}

}  // namespace

int wdist_blocks(int n) { return (n + kPairElems - 1) / kPairElems; }

void launch_wdist_sorted(int dt, const void* x, const float* ref_sorted, uint32_t* ws, double* slab, double* out, int n,
                         int F, hipStream_t s) {
  const int chunks = (n + kChunk - 1) / kChunk, nblk = wdist_blocks(n);
  if (dt == DT_BF16)
    hipLaunchKernelGGL(wdist_chunk_sort<true>, dim3(chunks, F), dim3(kSortThreads), 0, s, x, ws, n, F);
  else
    hipLaunchKernelGGL(wdist_chunk_sort<false>, dim3(chunks, F), dim3(kSortThreads), 0, s, x, ws, n, F);
  hipLaunchKernelGGL(wdist_rank_pair, dim3(nblk, F), dim3(kPairThreads), 0, s, ws, ref_sorted, slab, n, F, nblk);
  hipLaunchKernelGGL(wdist_finish, dim3(1), dim3(256), 0, s, slab, out, n, F, nblk);
}

}  // namespace hfrep
