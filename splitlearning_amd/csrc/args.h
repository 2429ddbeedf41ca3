// The host-argument vocabulary of the bindings and the native executors: the current stream, the
// error check, optional tensors, the tensor checks (each takes the operand's name), dict entries
// and the optimizer hyper-parameters of a config dict.  Host-only; everything is inline and
// allocation-free, so a helper may be called inside a step loop.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <array>
#include <vector>

#include "host.h"

namespace sl {
namespace args {

using OptT = c10::optional<at::Tensor>;

inline void ck(hipError_t e, const char* what) { TORCH_CHECK(e == hipSuccess, what, ": ", hipGetErrorString(e)); }
inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// the device's wall-clock rate (s_memrealtime ticks per ms); 100 MHz where the runtime has none
inline int clock_khz(int dev) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) khz = 100000;
  return khz;
}

inline bool has(const OptT& t) { return t.has_value() && t->defined(); }
inline float* opt_ptr(const OptT& t) { return has(t) ? t->data_ptr<float>() : nullptr; }

inline void need_cuda(const at::Tensor& t, const char* name) { TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor"); }
inline void need_f32(const at::Tensor& t, const char* name) {
  need_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
}
// 2-D with unit column stride (scalar access only)
inline void need_2d(const at::Tensor& t, const char* name) {
  need_f32(t, name);
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1, name, " must be 2-D with unit column stride");
}
// row-major 2-D with unit column stride and 16-byte aligned rows (float4 loads)
inline void need_rows(const at::Tensor& t, const char* name) {
  need_2d(t, name);
  TORCH_CHECK(t.stride(0) % 4 == 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) % 16) == 0, name,
              " rows must be 16-byte aligned");
}
// a contiguous GPU tensor of dtype `ty` on the current device; under_2gb: for kernels that index
// it with 32-bit byte offsets
inline void need_dense(const at::Tensor& t, at::ScalarType ty, const char* name, bool under_2gb = false) {
  need_cuda(t, name);
  TORCH_CHECK(t.scalar_type() == ty, name, " must be ",
              ty == at::kFloat ? "float32" : ty == at::kByte ? "uint8" : ty == at::kInt ? "int32" : "int8");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.get_device() == c10::hip::current_device(), name, " must be on the current device");
  if (under_2gb) TORCH_CHECK(t.numel() * (int64_t)t.element_size() < (int64_t(1) << 31), name, " must be under 2 GB");
}

// an optional contiguous fp32 workspace: {null, 0} when absent
struct Ws {
  float* p = nullptr;
  int64_t n = 0;
};
inline Ws opt_ws(const OptT& ws, const char* name = "ws") {
  if (!has(ws)) return {};
  need_f32(*ws, name);
  TORCH_CHECK(ws->is_contiguous(), name, " contiguous");
  return {ws->data_ptr<float>(), ws->numel()};
}

// d[key] as a tensor (absent or None: missing); `who` prefixes the message
inline at::Tensor dict_tensor(const pybind11::dict& d, const char* key, const char* who) {
  TORCH_CHECK(d.contains(key) && !d[key].is_none(), who, ": missing '", key, "'");
  return d[key].cast<at::Tensor>();
}
// a contiguous fp32 GPU tensor, as the executors hold their parameters and state
inline bool dense_f32(const at::Tensor& t) { return t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous(); }

// kind / lr / beta1 / beta2 / eps / wd / momentum of a config dict; at(t): the descriptor of
// optimizer step t (Adam's bias corrections folded in, host.h)
struct OptCfg {
  int kind = 1;
  double lr = 0, beta1 = 0, beta2 = 0, eps = 0, wd = 0, mom = 0;
  SlOpt at(int64_t t) const { return make_opt_raw(kind, lr, beta1, beta2, eps, wd, mom, t, nullptr); }
};
inline OptCfg read_opt(const pybind11::dict& d) {
  OptCfg o;
  o.kind = d["kind"].cast<int>();
  TORCH_CHECK(o.kind == 1 || o.kind == 2, "SGD-momentum or Adam");
  o.lr = d["lr"].cast<double>();
  o.beta1 = d["beta1"].cast<double>();
  o.beta2 = d["beta2"].cast<double>();
  o.eps = d["eps"].cast<double>();
  o.wd = d["wd"].cast<double>();
  o.mom = d["momentum"].cast<double>();
  return o;
}

// The three {W, b, s0, s1, sb0, sb1} records of a server tail, cfg["layers"], with the checks every
// executor makes: three dicts; W / b / s0 / sb0 present, s1 / sb1 (Adam's v) read where given;
// each a contiguous fp32 GPU tensor; W [N, K] with s0 of its shape and one bias per row; the
// widths chained fc1 -> fc2 -> fc3.  Which of s1 / sb1 must be there, and any rule on N or K,
// stays with the executor.
struct TailLayer {
  at::Tensor W, b, s0, s1, sb0, sb1;   // s1 / sb1 undefined where absent
  int N = 0, K = 0;
  float* v() const { return s1.defined() ? s1.data_ptr<float>() : nullptr; }
  float* vb() const { return sb1.defined() ? sb1.data_ptr<float>() : nullptr; }
};
inline std::array<TailLayer, 3> read_tail_layers(const pybind11::dict& cfg, const char* who) {
  const auto layers = cfg["layers"].cast<std::vector<pybind11::dict>>();
  TORCH_CHECK(layers.size() == 3, who, " drives the 3-layer server tail");
  std::array<TailLayer, 3> Ls;
  for (int i = 0; i < 3; ++i) {
    const pybind11::dict& d = layers[i];
    TailLayer& L = Ls[i];
    L.W = dict_tensor(d, "W", who);
    L.b = dict_tensor(d, "b", who);
    L.s0 = dict_tensor(d, "s0", who);
    L.sb0 = dict_tensor(d, "sb0", who);
    if (d.contains("s1") && !d["s1"].is_none()) L.s1 = dict_tensor(d, "s1", who);
    if (d.contains("sb1") && !d["sb1"].is_none()) L.sb1 = dict_tensor(d, "sb1", who);
    for (const at::Tensor* t : {&L.W, &L.b, &L.s0, &L.sb0}) TORCH_CHECK(dense_f32(*t), who, ": layer tensors: f32 GPU");
    TORCH_CHECK(L.W.dim() == 2 && L.s0.sizes() == L.W.sizes() && L.b.numel() == L.W.size(0), who, ": layer shapes");
    L.N = (int)L.W.size(0);
    L.K = (int)L.W.size(1);
  }
  TORCH_CHECK(Ls[1].K == Ls[0].N && Ls[2].K == Ls[1].N, who, ": layer chain shapes");
  return Ls;
}

}  // namespace args
}  // namespace sl
