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
// Keys, the chunk sort and the binary searches: chunk_sort.h (a total order over every bit pattern, so the
// pads of a short chunk stay behind every other key and the rank is < n by construction for any input:
// j < len_c and each count <= len_c').
// A NaN or an infinity in column f pairs with a finite reference value and makes W1_f (and the mean)
// non-finite; the other columns do not see it.
#include "chunk_sort.h"
#include "common.h"
#include "kernels.h"

namespace hfrep {

namespace {

constexpr int kPairThreads = 256;
constexpr int kPairElems = 2048;    // elements per rank-and-pair workgroup (8 per thread)

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
