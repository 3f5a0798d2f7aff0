// Device helpers shared by the factor-autoencoder kernels (ae.hip: the fit; ae_eval.hip: the IS / OOS
// reconstruction metrics): the size limits and the two rounding points of a Dense + LeakyReLU layer.
#pragma once

#include "common.h"

namespace hfrep {

constexpr int AE_MAXA = 32, AE_MAXK = 32;

// the value as the activation dtype stores it (bf16 round-to-nearest-even in BF mode)
template <bool BF>
__device__ __forceinline__ float rnd(float v) {
  if constexpr (BF) return bf2f(f2bf(v));
  else return v;
}
__device__ __forceinline__ float lrelu(float x) { return x >= 0.f ? x : 0.2f * x; }

}  // namespace hfrep
