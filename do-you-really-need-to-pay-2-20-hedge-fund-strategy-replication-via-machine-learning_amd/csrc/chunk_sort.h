// Total-order keys, the in-LDS chunk sort and the binary searches over sorted chunks: shared by the
// W-dist kernels (wdist.hip) and the two-sample KS statistic (evalm.hip).
//
// Keys: the IEEE bit pattern with the sign bit flipped (positive) or all bits flipped (negative) is
// a TOTAL order over every bit pattern: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  A float
// comparison would not be one (NaN), and a sorting network fed a non-order may move the +inf pads
// of a short chunk in front of real values.  With the total order the pads (key 0xFFFFFFFF, itself
// the key of a NaN) stay behind every other key and every binary search runs over a chunk's VALID
// length.
#pragma once
#include "common.h"

namespace hfrep {

namespace {

constexpr int kChunk = 16384;       // keys per sorted chunk: 64 KB of LDS, two workgroups per CU
constexpr int kSortThreads = 1024;

__device__ __forceinline__ uint32_t key_of(uint32_t bits) {
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t key) {
  const uint32_t bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  return __uint_as_float(bits);
}

// grid (chunks, F): the workgroup gathers up to kChunk values of column f of x (n, F), maps them to
// keys, bitonic-sorts them in LDS and writes the sorted keys of its chunk (valid length only) to
// ws (F, n)
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

}  // namespace

}  // namespace hfrep
