// pybind11 bindings of the second extension module, splitlearning_amd._C2: kernel families added
// after _C's surface was pinned (tests/data/native_surface.json).  It links the torch libraries
// and amdhip64 only, and its sources include only headers whose contents are inline (common.h,
// args.h, host.h), so _C and _C2 load into one process without sharing a non-inline symbol.
#include "args.h"
#include "cuttopk.h"

namespace {

using namespace sl::args;

// a contiguous 2-D GPU tensor of dtype `ty` on the current device
void topk_need(const at::Tensor& t, at::ScalarType ty, const char* name) {
  need_dense(t, ty, name);
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
}

// dense [R, K] fp32 against values [R, k] fp32 (where given) and indices [R, k] int32
sl::TopkShape topk_shape(const at::Tensor& dense, const char* dname, const at::Tensor* values, const at::Tensor& indices) {
  topk_need(dense, at::kFloat, dname);
  if (values) topk_need(*values, at::kFloat, "values");
  topk_need(indices, at::kInt, "indices");
  const int64_t R = dense.size(0), K = dense.size(1), k = indices.size(1);
  TORCH_CHECK(K < (int64_t(1) << 31) && R < (int64_t(1) << 31), "cut top-k: R and K must be under 2^31");
  TORCH_CHECK(k >= 1 && k <= K, "cut top-k: need 1 <= k <= K, got k = ", k, ", K = ", K);
  TORCH_CHECK(indices.size(0) == R, "indices must be [R, k]");
  if (values) TORCH_CHECK(values->size(0) == R && values->size(1) == k, "values must be [R, k]");
  return sl::TopkShape{(int)R, (int)K, (int)k};
}

void same_shape(const at::Tensor& a, const at::Tensor& b, const char* what) {
  topk_need(a, at::kFloat, what);
  TORCH_CHECK(a.sizes() == b.sizes(), what, " must have the dense tensor's shape");
}

void cut_topk(const at::Tensor& x, at::Tensor& values, at::Tensor& indices) {
  const sl::TopkShape s = topk_shape(x, "x", &values, indices);
  ck(sl::cut_topk(x.data_ptr<float>(), values.data_ptr<float>(), indices.data_ptr<int32_t>(), nullptr, s, cur_stream()),
     "cut_topk");
}

void cut_topk_dense(const at::Tensor& x, at::Tensor& y, at::Tensor& values, at::Tensor& indices) {
  const sl::TopkShape s = topk_shape(x, "x", &values, indices);
  same_shape(y, x, "y");
  ck(sl::cut_topk(x.data_ptr<float>(), values.data_ptr<float>(), indices.data_ptr<int32_t>(), y.data_ptr<float>(), s,
                  cur_stream()),
     "cut_topk_dense");
}

void cut_scatter(const at::Tensor& values, const at::Tensor& indices, at::Tensor& y) {
  const sl::TopkShape s = topk_shape(y, "y", &values, indices);
  ck(sl::cut_scatter(values.data_ptr<float>(), indices.data_ptr<int32_t>(), y.data_ptr<float>(), s, cur_stream()),
     "cut_scatter");
}

void cut_mask(const at::Tensor& d, const at::Tensor& indices, at::Tensor& dx) {
  const sl::TopkShape s = topk_shape(d, "d", nullptr, indices);
  same_shape(dx, d, "dx");
  ck(sl::cut_mask(d.data_ptr<float>(), indices.data_ptr<int32_t>(), dx.data_ptr<float>(), s, cur_stream()), "cut_mask");
}

void cut_gather(const at::Tensor& d, const at::Tensor& indices, at::Tensor& values) {
  const sl::TopkShape s = topk_shape(d, "d", &values, indices);
  ck(sl::cut_gather(d.data_ptr<float>(), indices.data_ptr<int32_t>(), values.data_ptr<float>(), s, cur_stream()),
     "cut_gather");
}

}  // namespace

PYBIND11_MODULE(_C2, m) {
  m.doc() = "splitlearning_amd gfx950 (MI355X) HIP kernels, second module";
  m.def("cut_topk", &cut_topk);
  m.def("cut_topk_dense", &cut_topk_dense);
  m.def("cut_scatter", &cut_scatter);
  m.def("cut_mask", &cut_mask);
  m.def("cut_gather", &cut_gather);
  m.attr("cut_topk_lds_floats") = (int64_t)sl::kCutTopkLdsFloats;
  m.attr("arch") = "gfx950";
}
