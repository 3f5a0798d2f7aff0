// Debug poison allocator shared by the op binding files (bindings.cpp, bindings_mlp.cpp).
//
// Debug poison mode (HFREP_POISON=1 or set_debug_poison(True)): every op output / workspace is
// allocated filled with NaN instead of uninitialised, so an element a kernel fails to write shows
// up as a non-finite loss or gradient (tests/test_gpu_runtime.py).  Off by default (it costs a
// fill per output).  Tapes are exempt: their padded unit lanes are unwritten by design and never
// read.
#pragma once
#include <ATen/ATen.h>

#include <atomic>
#include <cmath>

namespace hfrep {

// the one flag of the library (defined in bindings.cpp; initialised from HFREP_POISON)
std::atomic<bool>& poison_flag();

inline at::Tensor out_empty(at::IntArrayRef sizes, const at::TensorOptions& o) {
  return poison_flag().load(std::memory_order_relaxed) ? at::full(sizes, NAN, o) : at::empty(sizes, o);
}
inline at::Tensor out_empty_like(const at::Tensor& t) {
  return poison_flag().load(std::memory_order_relaxed) ? at::full_like(t, NAN) : at::empty_like(t);
}

}  // namespace hfrep
