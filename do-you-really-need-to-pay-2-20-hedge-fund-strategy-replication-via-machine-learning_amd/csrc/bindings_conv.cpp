// torch op registrations of the direct causal conv1d kernels (csrc/conv1d.hip), a fragment of the hfrep
// library (bindings.cpp holds the rest).  Same conventions: host-side validation, outputs and workspaces
// through the caching allocator (out_empty: covered by the debug poison mode), launches on the tensor's
// current HIP stream (graph-capturable), CUDA dispatch key only.
//
// Activations are contiguous (B, T, C) tensors of one dtype (fp32 or bf16); W is the fp32 master kernel
// (k, C_in, C_out).  A shape conv1d_supported declines is an error here: the Python layer
// (ops/functional.py) asks first and keeps such shapes on the im2col route.
#include <torch/extension.h>
#include <torch/library.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include "kernels.h"
#include "poison.h"

#include <algorithm>
#include <cstdint>

namespace {

using at::Tensor;
using c10::optional;
using hfrep::out_empty;

inline hipStream_t cur_stream(const Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}
#define GUARD(t) c10::hip::HIPGuardMasqueradingAsCUDA _guard((t).device())

inline int act_dt(const Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 3, "conv1d ops: ", what, " must be a contiguous (B, T, C) GPU tensor");
  // (the kernels stage rows with vector loads of four elements, 16 bytes in fp32: with C % 4 == 0 every
  // row is as aligned as the base)
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "conv1d ops: ", what, " must be 16-byte aligned");
  if (t.scalar_type() == at::kBFloat16) return hfrep::DT_BF16;
  TORCH_CHECK(t.scalar_type() == at::kFloat, "conv1d ops: float32 or bfloat16 activations");
  return hfrep::DT_F32;
}
inline void check_w(const Tensor& W, const Tensor& like, const char* what) {
  TORCH_CHECK(W.is_cuda() && W.device() == like.device() && W.scalar_type() == at::kFloat && W.is_contiguous() && W.dim() == 3,
              "conv1d ops: ", what, " must be a contiguous fp32 (k, C_in, C_out) tensor on the activations' device");
}
inline void check_b(const optional<Tensor>& b, int64_t Cout, const Tensor& like, const char* what) {
  if (!b.has_value()) return;
  TORCH_CHECK(b->is_cuda() && b->device() == like.device() && b->scalar_type() == at::kFloat && b->is_contiguous() &&
                  b->numel() == Cout,
              "conv1d ops: ", what, " must be a contiguous fp32 (C_out) tensor on the activations' device");
}
inline int dt_code(at::ScalarType st) {
  TORCH_CHECK(st == at::kFloat || st == at::kBFloat16, "conv1d ops: float32 or bfloat16");
  return st == at::kBFloat16 ? hfrep::DT_BF16 : hfrep::DT_F32;
}

bool conv1d_supported_op(int64_t Cin, int64_t Cout, int64_t k, int64_t dil, at::ScalarType dtype) {
  if (dtype != at::kFloat && dtype != at::kBFloat16) return false;
  if (Cin < 1 || Cin > 4096 || Cout < 1 || Cout > 4096 || k < 1 || k > 4096 || dil < 1) return false;
  return hfrep::conv1d_supported(dt_code(dtype), (int)Cin, (int)Cout, (int)k, (int)std::min<int64_t>(dil, INT32_MAX));
}

// y[b,t,o] = act(bias[o] + sum_j sum_i x[b, t - s_j, i] W[j,i,o]),  s_j = (k - 1 - j) dil
Tensor conv1d_causal_fwd(Tensor x, Tensor W, optional<Tensor> bias, int64_t dil, int64_t act) {
  const int dt = act_dt(x, "x");
  check_w(W, x, "W");
  const int64_t B = x.size(0), Tn = x.size(1), Cin = x.size(2), k = W.size(0), Cout = W.size(2);
  TORCH_CHECK(W.size(1) == Cin, "conv1d_causal_fwd: W (k, C_in, C_out) against x (B, T, C_in)");
  check_b(bias, Cout, x, "bias");
  TORCH_CHECK(conv1d_supported_op(Cin, Cout, k, dil, x.scalar_type()), "conv1d_causal_fwd: shape not supported (conv1d_supported)");
  GUARD(x);
  Tensor y = out_empty({B, Tn, Cout}, x.options());
  const int d = (int)std::min<int64_t>(dil, INT32_MAX);
  TORCH_CHECK(hfrep::launch_conv1d_fwd(dt, x.data_ptr(), W.data_ptr<float>(), bias.has_value() ? bias->data_ptr<float>() : nullptr,
                                       y.data_ptr(), (int)B, (int)Tn, (int)Cin, (int)Cout, (int)k, d, (int)act, cur_stream(x)),
              "conv1d_causal_fwd: no kernel for this shape");
  return y;
}

// dx[b,t,i] = sum_j sum_o dz[b, t + s_j, o] W[j,i,o]
Tensor conv1d_causal_dgrad(Tensor dz, Tensor W, int64_t dil) {
  const int dt = act_dt(dz, "dz");
  check_w(W, dz, "W");
  const int64_t B = dz.size(0), Tn = dz.size(1), Cout = dz.size(2), k = W.size(0), Cin = W.size(1);
  TORCH_CHECK(W.size(2) == Cout, "conv1d_causal_dgrad: W (k, C_in, C_out) against dz (B, T, C_out)");
  TORCH_CHECK(conv1d_supported_op(Cin, Cout, k, dil, dz.scalar_type()), "conv1d_causal_dgrad: shape not supported (conv1d_supported)");
  GUARD(dz);
  Tensor dx = out_empty({B, Tn, Cin}, dz.options());
  const int d = (int)std::min<int64_t>(dil, INT32_MAX);
  TORCH_CHECK(hfrep::launch_conv1d_dgrad(dt, dz.data_ptr(), W.data_ptr<float>(), dx.data_ptr(), (int)B, (int)Tn, (int)Cin,
                                         (int)Cout, (int)k, d, cur_stream(dz)),
              "conv1d_causal_dgrad: no kernel for this shape");
  return dx;
}

// gW[j,i,o] += sum_b sum_{t >= s_j} x[b, t - s_j, i] dz[b,t,o];  gb[o] += sum_{b,t} dz[b,t,o]
void conv1d_causal_wgrad_(Tensor x, Tensor dz, Tensor gW, optional<Tensor> gb, int64_t dil) {
  const int dt = act_dt(x, "x");
  TORCH_CHECK(act_dt(dz, "dz") == dt, "conv1d_causal_wgrad_: x and dz must have one dtype");
  check_w(gW, x, "gW");
  const int64_t B = x.size(0), Tn = x.size(1), Cin = x.size(2), Cout = dz.size(2), k = gW.size(0);
  TORCH_CHECK(dz.size(0) == B && dz.size(1) == Tn && dz.device() == x.device(), "conv1d_causal_wgrad_: x (B, T, C_in) against dz (B, T, C_out)");
  TORCH_CHECK(gW.size(1) == Cin && gW.size(2) == Cout, "conv1d_causal_wgrad_: gW (k, C_in, C_out)");
  check_b(gb, Cout, x, "gb");
  TORCH_CHECK(conv1d_supported_op(Cin, Cout, k, dil, x.scalar_type()), "conv1d_causal_wgrad_: shape not supported (conv1d_supported)");
  GUARD(x);
  Tensor ws = out_empty({(int64_t)hfrep::conv1d_wgrad_workspace_floats((int)B, (int)Tn, (int)Cin, (int)Cout, (int)k, gb.has_value())},
                        x.options().dtype(at::kFloat));
  const int d = (int)std::min<int64_t>(dil, INT32_MAX);
  TORCH_CHECK(hfrep::launch_conv1d_wgrad(dt, x.data_ptr(), dz.data_ptr(), gW.data_ptr<float>(),
                                         gb.has_value() ? gb->data_ptr<float>() : nullptr, (int)B, (int)Tn, (int)Cin, (int)Cout,
                                         (int)k, d, ws.data_ptr<float>(), cur_stream(x)),
              "conv1d_causal_wgrad_: no kernel for this shape");
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(hfrep, m) {
  m.def("conv1d_supported(int C_in, int C_out, int k, int dil, ScalarType dtype) -> bool", &conv1d_supported_op);  // no tensor inputs: catch-all kernel
  m.def("conv1d_causal_fwd(Tensor x, Tensor W, Tensor? bias, int dil, int act) -> Tensor");
  m.def("conv1d_causal_dgrad(Tensor dz, Tensor W, int dil) -> Tensor");
  m.def("conv1d_causal_wgrad_(Tensor x, Tensor dz, Tensor(a!) gW, Tensor(b!)? gb, int dil) -> ()");
}

TORCH_LIBRARY_IMPL(hfrep, CUDA, m) {
  m.impl("conv1d_causal_fwd", &conv1d_causal_fwd);
  m.impl("conv1d_causal_dgrad", &conv1d_causal_dgrad);
  m.impl("conv1d_causal_wgrad_", &conv1d_causal_wgrad_);
}
