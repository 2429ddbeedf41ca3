// Python bindings for the gfx950 kernels (pybind11 module `splitlearning_amd._C`).
//
// Each binding validates its operands on the host (a kernel must never see an operand its
// grid does not assume) with the shared checks of args.h, fetches the current HIP stream from
// the PyTorch-ROCm stream registry and calls the launcher (kernels.h and the per-family
// headers).  All buffers are caller-allocated so the same calls can be captured into a HIP
// graph.  The executors and the hand-off stress entry register themselves (sl_register_*).
//
// Optimizer hyper-parameters travel as (kind, lr, beta1, beta2, eps, wd, momentum, t, dyn):
// kind 0 = write the gradient into s0, 1 = SGD(momentum), 2 = Adam (L2 weight decay);
// `dyn` != 0 is the device address of {step_size, inv_bc2_sqrt} used instead of t
// (graph replay).  Dropout seeds likewise: (seed, dseed) with dseed = device address
// of {seed_lo, seed_hi} or 0.
#include <torch/extension.h>

#include "args.h"
#include "common.h"
#include "conv2d.h"
#include "cutcodec.h"
#include "fused.h"
#include "groupnorm.h"
#include "kernels.h"
#include "optim.h"

namespace {

using namespace sl::args;   // OptT, cur_stream, has, opt_ptr, opt_ws, the need_* checks

SlOpt make_opt(int64_t kind, double lr, double beta1, double beta2, double eps, double wd, double momentum,
               int64_t t, int64_t dyn) {
  if (kind == 2 && !dyn) TORCH_CHECK(t >= 1, "Adam step count must be >= 1");
  return sl::make_opt_raw((int)kind, lr, beta1, beta2, eps, wd, momentum, t, reinterpret_cast<const float*>(dyn));
}

Epi make_epi(const OptT& bias, bool relu, double drop_p, uint64_t seed, int64_t col_off, int64_t dseed) {
  return sl::make_epi_raw(opt_ptr(bias), relu, drop_p, seed, (int)col_off, reinterpret_cast<const uint32_t*>(dseed));
}

#define OPT_ARGS int64_t kind, double lr, double beta1, double beta2, double eps, double wd, double momentum, \
                 int64_t t, int64_t dyn
#define OPT_PASS make_opt(kind, lr, beta1, beta2, eps, wd, momentum, t, dyn)

// ---------------------------------------------------------------- conv
void check_x(const at::Tensor& x) {
  need_cuda(x, "x");
  TORCH_CHECK(x.is_contiguous() && x.numel() % 784 == 0, "x must be contiguous [N,784]");
  TORCH_CHECK(x.scalar_type() == at::kByte || x.scalar_type() == at::kFloat, "x must be uint8 or float32");
}
void check_params(const at::Tensor& w, const at::Tensor& b) {
  need_f32(w, "w");
  need_f32(b, "b");
  TORCH_CHECK(w.numel() == 288 && b.numel() == 32 && w.is_contiguous() && b.is_contiguous(), "conv params 32x1x3x3");
}
void check_idx(const at::Tensor& idx, int64_t B) {
  need_cuda(idx, "idx");
  TORCH_CHECK(idx.scalar_type() == at::kLong && idx.is_contiguous() && idx.numel() >= B, "idx int64 [B]");
}
void check_slab(const at::Tensor& slab, int64_t B) {
  need_f32(slab, "slab");
  TORCH_CHECK(slab.is_contiguous() && slab.numel() >= B * 320, "slab workspace [B,320]");
}

// The operands of the front-conv bindings, checked, as the launchers take them.  A binding
// names the tensors it has (Has); the others stay null in the result.
struct FrontState {   // the optimizer state of w and b: first moments / momentum, Adam's second or None
  const at::Tensor& s0w;
  const OptT& s1w;
  const at::Tensor& s0b;
  const OptT& s1b;
};
struct FrontHas {
  const at::Tensor *idx = nullptr, *y = nullptr, *am = nullptr, *labels = nullptr, *slab = nullptr;
  const FrontState* state = nullptr;
  const char* labels_name = "labels";
};
struct Front {
  const void* x = nullptr;
  bool u8 = false;
  float *w = nullptr, *b = nullptr, *y = nullptr, *slab = nullptr;
  float *s0w = nullptr, *s1w = nullptr, *s0b = nullptr, *s1b = nullptr;
  uint8_t* am = nullptr;
  const int64_t *idx = nullptr, *labels = nullptr;
};
Front front_args(const at::Tensor& x, const at::Tensor& w, const at::Tensor& b, int64_t B, const FrontHas& h) {
  Front f;
  check_x(x);
  check_params(w, b);
  f.x = x.data_ptr();
  f.u8 = x.scalar_type() == at::kByte;
  f.w = w.data_ptr<float>();
  f.b = b.data_ptr<float>();
  if (h.idx) {
    check_idx(*h.idx, B);
    f.idx = h.idx->data_ptr<int64_t>();
  }
  if (h.slab) {
    check_slab(*h.slab, B);
    f.slab = h.slab->data_ptr<float>();
  }
  if (h.y) {
    need_f32(*h.y, "y");
    TORCH_CHECK(h.y->is_contiguous() && h.y->numel() >= B * 5408, "y too small");
    f.y = h.y->data_ptr<float>();
  }
  if (h.am) {
    TORCH_CHECK(h.am->scalar_type() == at::kByte && h.am->is_contiguous() && h.am->numel() >= B * 5408,
                "am too small");
    f.am = h.am->data_ptr<uint8_t>();
  }
  if (h.labels) {
    need_cuda(*h.labels, h.labels_name);
    TORCH_CHECK(h.labels->scalar_type() == at::kLong && h.labels->is_contiguous() &&
                    h.labels->numel() == x.numel() / 784,
                h.labels_name, " int64 [N]");
    f.labels = h.labels->data_ptr<int64_t>();
  }
  if (h.state) {
    const FrontState& st = *h.state;
    TORCH_CHECK(st.s0w.numel() == 288 && st.s0b.numel() == 32, "optimizer state");
    f.s0w = st.s0w.data_ptr<float>();
    f.s0b = st.s0b.data_ptr<float>();
    f.s1w = opt_ptr(st.s1w);
    f.s1b = opt_ptr(st.s1b);
  }
  return f;
}

void check_lab_out(const at::Tensor& lab_out, int64_t B) {
  need_cuda(lab_out, "lab_out");
  TORCH_CHECK(lab_out.scalar_type() == at::kLong && lab_out.is_contiguous() && lab_out.numel() >= B,
              "lab_out int64 [B]");
}

// lab_in / lab_out (optional, together): the shard's labels [N] and the batch's gathered
// labels [B], written by the forward kernel (no separate index launch).
void conv_fwd(const at::Tensor& x, const at::Tensor& idx, int64_t B, const at::Tensor& w, const at::Tensor& b,
              at::Tensor& y, at::Tensor& am, const OptT& lab_in, const OptT& lab_out) {
  FrontHas h;
  h.idx = &idx, h.y = &y, h.am = &am;
  TORCH_CHECK(lab_in.has_value() == lab_out.has_value(), "lab_in and lab_out go together");
  if (lab_in.has_value()) h.labels = &*lab_in, h.labels_name = "lab_in";
  const Front f = front_args(x, w, b, B, h);
  int64_t* lo = nullptr;
  if (lab_in.has_value()) {
    check_lab_out(*lab_out, B);
    lo = lab_out->data_ptr<int64_t>();
  }
  ck(sl::conv_fwd(f.x, f.u8, f.idx, 0, (int)B, f.w, f.b, f.y, f.am, cur_stream(), f.labels, lo, nullptr),
        "conv_fwd");
}

ConvPending make_pending(const at::Tensor& slab, int64_t pB, at::Tensor& s0w, const OptT& s1w, at::Tensor& s0b,
                         const OptT& s1b, SlOpt o) {
  check_slab(slab, pB);
  TORCH_CHECK(pB >= 1, "pending batch");
  TORCH_CHECK(s0w.numel() == 288 && s0b.numel() == 32, "optimizer state");
  return ConvPending{slab.data_ptr<float>(), (int)pB, s0w.data_ptr<float>(), opt_ptr(s1w), s0b.data_ptr<float>(),
                     opt_ptr(s1b), o};
}

// Forward with a deferred optimizer step applied in-kernel (FrontEngine, split modes):
// (pslab, pB, states, opt of that step) is the last backward's update, not yet stored.
void conv_fwd_pending(const at::Tensor& x, const at::Tensor& idx, int64_t B, const at::Tensor& w, const at::Tensor& b,
                      at::Tensor& y, at::Tensor& am, const at::Tensor& lab_in, at::Tensor& lab_out,
                      const at::Tensor& pslab, int64_t pB, at::Tensor& s0w, const OptT& s1w, at::Tensor& s0b,
                      const OptT& s1b, OPT_ARGS) {
  FrontHas h;
  h.idx = &idx, h.y = &y, h.am = &am, h.labels = &lab_in, h.labels_name = "lab_in";
  const Front f = front_args(x, w, b, B, h);
  check_lab_out(lab_out, B);
  const ConvPending p = make_pending(pslab, pB, s0w, s1w, s0b, s1b, OPT_PASS);
  ck(sl::conv_fwd(f.x, f.u8, f.idx, 0, (int)B, f.w, f.b, f.y, f.am, cur_stream(), f.labels,
                     lab_out.data_ptr<int64_t>(), &p),
        "conv_fwd_pending");
}

// SISA local step: fused gather+conv+pool+softmax-CE(5408)+dW partials, then reduce+optimizer.
void conv_local_step(const at::Tensor& x, const at::Tensor& idx, const at::Tensor& labels, int64_t B, at::Tensor& w,
                     at::Tensor& b, at::Tensor& slab, at::Tensor& loss_rows, at::Tensor& s0w, const OptT& s1w,
                     at::Tensor& s0b, const OptT& s1b, OPT_ARGS) {
  const FrontState state{s0w, s1w, s0b, s1b};
  FrontHas h;
  h.idx = &idx, h.slab = &slab, h.labels = &labels, h.state = &state;
  const Front f = front_args(x, w, b, B, h);
  need_f32(loss_rows, "loss_rows");
  TORCH_CHECK(loss_rows.numel() >= B, "loss_rows");
  ck(sl::conv_local_step(f.x, f.u8, f.idx, f.labels, (int)B, f.w, f.b, f.slab, loss_rows.data_ptr<float>(), f.s0w,
                            f.s1w, f.s0b, f.s1b, OPT_PASS, cur_stream()),
        "conv_local_step");
}

// the optimizer of a whole epoch: OptCfg::at(t) behind the launchers' callback
SlOpt epoch_opt(void* ctx, int64_t t) {
  const OptCfg& e = *static_cast<const OptCfg*>(ctx);
  if (e.kind == 2) TORCH_CHECK(t >= 1, "Adam step count must be >= 1");
  return e.at(t);
}

void check_order(const at::Tensor& order) {
  need_cuda(order, "order");
  TORCH_CHECK(order.scalar_type() == at::kLong && order.is_contiguous() && order.dim() == 1, "order int64 [n]");
}

// A whole SISA local epoch: ceil(n/B) client steps over `order` (the last one partial, like
// DataLoader(drop_last=False)), optimizer steps t0, t0+1, ...  One launch per step: each
// step's kernel applies the previous step's optimizer update in its prologue
// (conv.hip: conv_local_epoch).
void conv_local_epoch(const at::Tensor& x, const at::Tensor& order, const at::Tensor& labels, int64_t B,
                      at::Tensor& w, at::Tensor& b, at::Tensor& slab, at::Tensor& loss_rows, at::Tensor& s0w,
                      const OptT& s1w, at::Tensor& s0b, const OptT& s1b, int64_t kind, double lr, double beta1,
                      double beta2, double eps, double wd, double momentum, int64_t t0, at::Tensor& ws) {
  check_order(order);
  const int64_t n = order.numel();
  TORCH_CHECK(B >= 1 && B <= 4096, "batch size");
  const FrontState state{s0w, s1w, s0b, s1b};
  FrontHas h;
  h.slab = &slab, h.labels = &labels, h.state = &state;
  const Front f = front_args(x, w, b, B, h);
  need_f32(loss_rows, "loss_rows");
  TORCH_CHECK(loss_rows.is_contiguous() && loss_rows.numel() >= n, "loss_rows [n]");
  need_f32(ws, "ws");
  TORCH_CHECK(ws.is_contiguous(), "ws contiguous");
  TORCH_CHECK(kind == 1 || kind == 2, "local epoch: SGD-momentum or Adam");
  const hipStream_t st = cur_stream();
  OptCfg ctx{(int)kind, lr, beta1, beta2, eps, wd, momentum};
  ck(sl::conv_local_epoch(f.x, f.u8, order.data_ptr<int64_t>(), n, (int)B, f.labels, f.w, f.b, f.s0w, f.s1w, f.s0b,
                             f.s1b, ws.data_ptr<float>(), ws.numel(), loss_rows.data_ptr<float>(), &epoch_opt, &ctx,
                             t0, st),
        "conv_local_epoch");
}

// Local epochs of k co-located Alices stepped together, one launch per step for all of
// them (conv.hip: conv_local_epoch_multi).  alices: [(x, order, labels, w, b, s0w, s1w, s0b,
// s1b, ws, loss_rows, t0)]; every Alice shares the optimizer hyper-parameters.  `table`:
// uint8 GPU workspace >= table_bytes(k, max steps).
void conv_local_epoch_multi(py::list alices, int64_t B, int64_t kind, double lr, double beta1, double beta2, double eps,
                            double wd, double momentum, at::Tensor& table) {
  const int k = (int)alices.size();
  TORCH_CHECK(k >= 1 && k <= 64, "1..64 co-located Alices");
  TORCH_CHECK(B >= 1 && B <= 1024, "batch size");
  TORCH_CHECK(kind == 1 || kind == 2, "local epoch: SGD-momentum or Adam");
  need_cuda(table, "table");
  TORCH_CHECK(table.scalar_type() == at::kByte && table.is_contiguous(), "table uint8 workspace");
  std::vector<MultiAlice> al(k);
  for (int a = 0; a < k; ++a) {
    auto t = alices[a].cast<py::tuple>();
    TORCH_CHECK(t.size() == 12, "alice tuple (x, order, labels, w, b, s0w, s1w, s0b, s1b, ws, loss_rows, t0)");
    auto x = t[0].cast<at::Tensor>();
    auto order = t[1].cast<at::Tensor>();
    auto labels = t[2].cast<at::Tensor>();
    auto w = t[3].cast<at::Tensor>();
    auto b = t[4].cast<at::Tensor>();
    auto s0w = t[5].cast<at::Tensor>();
    auto s1w = t[6].cast<OptT>();
    auto s0b = t[7].cast<at::Tensor>();
    auto s1b = t[8].cast<OptT>();
    auto ws = t[9].cast<at::Tensor>();
    auto loss = t[10].cast<at::Tensor>();
    check_order(order);
    const FrontState state{s0w, s1w, s0b, s1b};
    FrontHas h;
    h.labels = &labels, h.state = &state;
    const Front f = front_args(x, w, b, B, h);
    TORCH_CHECK(f.u8, "co-located epochs read uint8 shards");
    need_f32(ws, "ws");
    TORCH_CHECK(ws.is_contiguous() && ws.numel() >= 2 * B * 320 + 2 * 960, "ws");
    need_f32(loss, "loss_rows");
    TORCH_CHECK(loss.is_contiguous() && loss.numel() >= order.numel(), "loss_rows [n]");
    al[a] = MultiAlice{x.data_ptr<uint8_t>(), order.data_ptr<int64_t>(), order.numel(), f.labels, f.w, f.b, f.s0w,
                       f.s1w, f.s0b, f.s1b, ws.data_ptr<float>(), ws.numel(), loss.data_ptr<float>(),
                       t[11].cast<int64_t>()};
    if (kind == 2) TORCH_CHECK(al[a].s1w && al[a].s1b, "Adam second moments");
  }
  OptCfg ctx{(int)kind, lr, beta1, beta2, eps, wd, momentum};
  ck(sl::conv_local_epoch_multi(al.data(), k, (int)B, &epoch_opt, &ctx, table.data_ptr(), table.numel(),
                                   cur_stream()),
        "conv_local_epoch_multi");
}

// Frozen-front forwards of up to 16 co-located Alices, one launch per `chunk` rows for all of
// them (conv.hip: conv_fwd_multi).  alices: [(x uint8 [N, 784], idx int64 [n] or None (rows
// 0 .. n), n, w, b, y [n, 5408])].
void conv_fwd_multi(py::list alices, int64_t chunk) {
  const int k = (int)alices.size();
  TORCH_CHECK(k >= 1 && k <= kFrontFwdMax, "1..16 Alices per launch");
  TORCH_CHECK(chunk >= 1 && chunk <= 65535, "chunk rows");
  FrontFwdSet set{};
  set.k = k;
  for (int a = 0; a < k; ++a) {
    auto t = alices[a].cast<py::tuple>();
    TORCH_CHECK(t.size() == 6, "alice tuple (x, idx, n, w, b, y)");
    auto x = t[0].cast<at::Tensor>();
    auto idx = t[1].cast<OptT>();
    const int64_t n = t[2].cast<int64_t>();
    auto w = t[3].cast<at::Tensor>();
    auto b = t[4].cast<at::Tensor>();
    auto y = t[5].cast<at::Tensor>();
    check_x(x);
    TORCH_CHECK(x.scalar_type() == at::kByte, "uint8 shards");
    check_params(w, b);
    TORCH_CHECK(n >= 0, "n");
    if (idx.has_value()) {
      check_idx(*idx, n);
    } else {
      TORCH_CHECK(n <= x.numel() / 784, "rows beyond the shard");
    }
    need_f32(y, "y");
    TORCH_CHECK(y.is_contiguous() && y.numel() >= n * 5408, "y [n, 5408]");
    set.d[a] = FrontFwdDesc{x.data_ptr<uint8_t>(), idx.has_value() ? idx->data_ptr<int64_t>() : nullptr, n,
                            w.data_ptr<float>(), b.data_ptr<float>(), y.data_ptr<float>()};
  }
  ck(sl::conv_fwd_multi(set, chunk, cur_stream()), "conv_fwd_multi");
}

// Split-mode client backward: dW partials from the cut gradient, then reduce+optimizer
// (conv_bwd_step), or deferred (conv_bwd_defer): this step's dW/db partials into `slab` (no update
// launch); workgroup 0 stores the pending update of the previous step (pslab / pB / its opt), if any.
Front bwd_args(const at::Tensor& dy, const at::Tensor& y, const at::Tensor& am, const at::Tensor& x,
               const at::Tensor& idx, int64_t B, at::Tensor& w, at::Tensor& b, at::Tensor& slab, at::Tensor& s0w,
               const OptT& s1w, at::Tensor& s0b, const OptT& s1b) {
  need_f32(dy, "dy");
  need_f32(y, "y");
  TORCH_CHECK(dy.is_contiguous() && y.is_contiguous() && dy.numel() >= B * 5408 && y.numel() >= B * 5408, "dy/y");
  const FrontState state{s0w, s1w, s0b, s1b};
  FrontHas h;
  h.idx = &idx, h.slab = &slab, h.am = &am, h.state = &state;
  return front_args(x, w, b, B, h);
}

void conv_bwd_step(const at::Tensor& dy, const at::Tensor& y, const at::Tensor& am, const at::Tensor& x,
                   const at::Tensor& idx, int64_t B, at::Tensor& w, at::Tensor& b, at::Tensor& slab, at::Tensor& s0w,
                   const OptT& s1w, at::Tensor& s0b, const OptT& s1b, OPT_ARGS) {
  const Front f = bwd_args(dy, y, am, x, idx, B, w, b, slab, s0w, s1w, s0b, s1b);
  ck(sl::conv_bwd_step(dy.data_ptr<float>(), y.data_ptr<float>(), f.am, f.x, f.u8, f.idx, (int)B, f.w, f.b, f.slab,
                       f.s0w, f.s1w, f.s0b, f.s1b, OPT_PASS, cur_stream(), false, nullptr),
     "conv_bwd_step");
}

void conv_bwd_defer(const at::Tensor& dy, const at::Tensor& y, const at::Tensor& am, const at::Tensor& x,
                    const at::Tensor& idx, int64_t B, at::Tensor& w, at::Tensor& b, at::Tensor& slab, const OptT& pslab,
                    int64_t pB, at::Tensor& s0w, const OptT& s1w, at::Tensor& s0b, const OptT& s1b, OPT_ARGS) {
  const Front f = bwd_args(dy, y, am, x, idx, B, w, b, slab, s0w, s1w, s0b, s1b);
  ConvPending p{};
  if (has(pslab)) {
    TORCH_CHECK(pslab->data_ptr<float>() != slab.data_ptr<float>(), "pending and new slabs must differ");
    p = make_pending(*pslab, pB, s0w, s1w, s0b, s1b, OPT_PASS);
  }
  ck(sl::conv_bwd_step(dy.data_ptr<float>(), y.data_ptr<float>(), f.am, f.x, f.u8, f.idx, (int)B, f.w, f.b, f.slab,
                       f.s0w, f.s1w, f.s0b, f.s1b, SlOpt{}, cur_stream(), true, has(pslab) ? &p : nullptr),
     "conv_bwd_defer");
}

// U-shape head (Linear + CE) forward, data gradient and optimizer step in one launch.
void head_step(const at::Tensor& X, at::Tensor& W, const OptT& b, const at::Tensor& y, int64_t ignore, double scale,
               bool mask_dx, at::Tensor& loss_rows, at::Tensor& dX, at::Tensor& s0w, const OptT& s1w, const OptT& s0b,
               const OptT& s1b, OPT_ARGS) {
  need_rows(X, "X");
  need_rows(W, "W");
  const int64_t M = X.size(0), K = X.size(1), C = W.size(0);
  TORCH_CHECK(X.is_contiguous() && W.is_contiguous() && W.size(1) == K, "X [M,K], W [C,K] contiguous");
  TORCH_CHECK(M * K <= 4096 && C * K <= 4096 && M * C <= 1024, "head_step: layer too large for one workgroup");
  need_cuda(y, "y");
  TORCH_CHECK(y.scalar_type() == at::kLong && y.numel() == M, "labels int64 [M]");
  need_f32(loss_rows, "loss_rows");
  need_f32(dX, "dX");
  TORCH_CHECK(loss_rows.numel() >= M && dX.is_contiguous() && dX.numel() == M * K, "outputs");
  TORCH_CHECK(s0w.numel() == C * K && s0w.is_contiguous(), "state");
  if (has(b)) TORCH_CHECK(b->numel() == C && s0b.has_value(), "bias state");
  ck(sl::head_step(X.data_ptr<float>(), W.data_ptr<float>(), opt_ptr(b), y.data_ptr<int64_t>(), ignore, (float)scale,
                      loss_rows.data_ptr<float>(), dX.data_ptr<float>(), s0w.data_ptr<float>(), opt_ptr(s1w), opt_ptr(s0b),
                      opt_ptr(s1b), (int)M, (int)K, (int)C, OPT_PASS, mask_dx, cur_stream()),
        "head_step");
}

// Store a deferred update (FrontEngine.flush).
void conv_apply(const at::Tensor& pslab, int64_t pB, at::Tensor& w, at::Tensor& b, at::Tensor& s0w, const OptT& s1w,
                at::Tensor& s0b, const OptT& s1b, OPT_ARGS) {
  check_params(w, b);
  const ConvPending p = make_pending(pslab, pB, s0w, s1w, s0b, s1b, OPT_PASS);
  ck(sl::conv_apply(p, w.data_ptr<float>(), b.data_ptr<float>(), cur_stream()), "conv_apply");
}

// ---------------------------------------------------------------- linear
void linear_fwd(const at::Tensor& X, const at::Tensor& W, const OptT& bias, at::Tensor& Y, bool relu, double drop_p,
                uint64_t seed, int64_t col_off, int64_t dseed, const OptT& ws) {
  need_rows(X, "X");
  need_rows(W, "W");
  need_2d(Y, "Y");
  const int64_t M = X.size(0), K = X.size(1), N = W.size(0);
  TORCH_CHECK(W.size(1) == K && K % 4 == 0, "W must be [N,K] with K % 4 == 0");
  TORCH_CHECK(Y.size(0) == M && Y.size(1) == N, "Y must be [M,N]");
  if (has(bias)) TORCH_CHECK(bias->numel() == N && bias->is_contiguous(), "bias [N]");
  const Ws w = opt_ws(ws);
  ck(sl::linear_fwd(X.data_ptr<float>(), (int)X.stride(0), W.data_ptr<float>(), (int)W.stride(0),
                       Y.data_ptr<float>(), (int)Y.stride(0), (int)M, (int)N, (int)K,
                       make_epi(bias, relu, drop_p, seed, col_off, dseed), w.p, w.n, cur_stream()),
        "linear_fwd");
}

// P: [M, N] pre-activations, or [S, M, N] contiguous split-K partial slabs (summed here).
void linear_epilogue(const at::Tensor& P, const OptT& bias, at::Tensor& Y, bool relu, double drop_p, uint64_t seed,
                     int64_t col_off, int64_t dseed) {
  need_2d(Y, "Y");
  int S = 1;
  int64_t slab = 0;
  if (P.dim() == 3) {
    need_f32(P, "P");
    TORCH_CHECK(P.is_contiguous() && P.size(1) == Y.size(0) && P.size(2) == Y.size(1), "P [S,M,N]");
    S = (int)P.size(0);
    slab = P.size(1) * P.size(2);
  } else {
    need_2d(P, "P");
    TORCH_CHECK(P.sizes() == Y.sizes(), "P/Y shape");
  }
  const int64_t M = Y.size(0), N = Y.size(1);
  if (has(bias)) TORCH_CHECK(bias->numel() == N, "bias [N]");
  ck(sl::linear_epilogue(P.data_ptr<float>(), (int)P.stride(P.dim() - 2), Y.data_ptr<float>(), (int)Y.stride(0),
                            (int)M, (int)N, make_epi(bias, relu, drop_p, seed, col_off, dseed), S, slab, cur_stream()),
        "linear_epilogue");
}

// dX = mask(dZ . W): the skinny kernels (linear.hip), or (nn: many rows) the in-tree NN-layout MFMA
// GEMM (gemm.hip), which also needs N % 4 == 0 and 16-byte aligned rows of dZ
void dgrad(bool nn, const at::Tensor& dZ, const at::Tensor& W, const OptT& hprev, double scale, at::Tensor& dX,
           const OptT& ws) {
  need_2d(dZ, "dZ");
  need_rows(W, "W");
  need_2d(dX, "dX");
  const int64_t M = dZ.size(0), N = dZ.size(1), K = W.size(1);
  TORCH_CHECK(W.size(0) == N && K % 4 == 0 && (!nn || N % 4 == 0),
              nn ? "W must be [N,K], N and K % 4 == 0" : "W must be [N,K] with K % 4 == 0");
  TORCH_CHECK(dX.size(0) == M && dX.size(1) == K, "dX must be [M,K]");
  if (nn) TORCH_CHECK(dZ.stride(0) % 4 == 0 && W.stride(0) % 4 == 0, "rows 16-B aligned");
  const float* hp = nullptr;
  int ldh = 0;
  if (has(hprev)) {
    need_2d(*hprev, "hprev");
    TORCH_CHECK(hprev->size(0) == M && hprev->size(1) == K, "hprev shape");
    hp = hprev->data_ptr<float>();
    ldh = (int)hprev->stride(0);
  }
  const Ws w = opt_ws(ws);
  const float *dz = dZ.data_ptr<float>(), *wt = W.data_ptr<float>();
  float* dx = dX.data_ptr<float>();
  const int ldz = (int)dZ.stride(0), ldw = (int)W.stride(0), ldx = (int)dX.stride(0);
  if (nn)
    ck(sl::gemm_nn_dgrad(dz, ldz, wt, ldw, hp, ldh, (float)scale, dx, ldx, (int)M, (int)N, (int)K, w.p, w.n,
                            cur_stream()),
          "gemm_nn_dgrad");
  else
    ck(sl::linear_dgrad(dz, ldz, wt, ldw, hp, ldh, (float)scale, dx, ldx, w.p, w.n, (int)M, (int)N, (int)K,
                           cur_stream()),
          "linear_dgrad");
}
void linear_dgrad(const at::Tensor& dZ, const at::Tensor& W, const OptT& hprev, double scale, at::Tensor& dX,
                  const OptT& ws) {
  dgrad(false, dZ, W, hprev, scale, dX, ws);
}
void gemm_nn_dgrad(const at::Tensor& dZ, const at::Tensor& W, const OptT& hprev, double scale, at::Tensor& dX,
                   const OptT& ws) {
  dgrad(true, dZ, W, hprev, scale, dX, ws);
}

void linear_wgrad_opt(const at::Tensor& dZ, const at::Tensor& A, at::Tensor& W, at::Tensor& s0, const OptT& s1,
                      const OptT& bias, const OptT& sb0, const OptT& sb1, OPT_ARGS) {
  need_2d(dZ, "dZ");
  need_rows(A, "A");
  need_rows(W, "W");
  need_rows(s0, "s0");
  const int64_t M = dZ.size(0), N = dZ.size(1), K = A.size(1);
  TORCH_CHECK(A.size(0) == M && W.size(0) == N && W.size(1) == K && K % 4 == 0, "shapes");
  TORCH_CHECK(s0.sizes() == W.sizes() && s0.stride(0) == W.stride(0), "s0 like W");
  if (has(s1)) TORCH_CHECK(s1->sizes() == W.sizes() && s1->stride(0) == W.stride(0), "s1");
  if (kind == 2) TORCH_CHECK(has(s1), "Adam needs s1");
  if (has(bias))
    TORCH_CHECK(bias->numel() == N && sb0.has_value() && sb0->numel() == N, "bias state");
  ck(sl::linear_wgrad_opt(dZ.data_ptr<float>(), (int)dZ.stride(0), A.data_ptr<float>(), (int)A.stride(0),
                             W.data_ptr<float>(), (int)W.stride(0), s0.data_ptr<float>(), opt_ptr(s1), opt_ptr(bias),
                             opt_ptr(sb0), opt_ptr(sb1), (int)M, (int)N, (int)K, OPT_PASS, cur_stream()),
        "linear_wgrad_opt");
}

void opt_flat(at::Tensor& p, const at::Tensor& g, at::Tensor& s0, const OptT& s1, OPT_ARGS) {
  need_f32(p, "p");
  need_f32(g, "g");
  need_f32(s0, "s0");
  TORCH_CHECK(p.is_contiguous() && g.is_contiguous() && s0.is_contiguous(), "contiguous");
  TORCH_CHECK(g.numel() == p.numel() && s0.numel() == p.numel(), "sizes");
  ck(sl::opt_flat(p.data_ptr<float>(), g.data_ptr<float>(), s0.data_ptr<float>(), opt_ptr(s1), p.numel(), OPT_PASS,
                     cur_stream()),
        "opt_flat");
}

// ---------------------------------------------------------------- multi-tensor optimizer
// optim.hip: lists of flat fp32 tensors, cut into launches of at most kMultiOptMax entries.
void need_flat(const at::Tensor& t, const at::Tensor& like, const char* name) {
  need_f32(t, name);
  TORCH_CHECK(t.device() == like.device(), name, " must be on the parameters' device");
  TORCH_CHECK(t.is_contiguous() && t.numel() == like.numel(), name, " must be contiguous with the parameter's numel");
}

// Appends `e` (n > 0 elements) to the table, launching the table first when it is full.
template <class Launch>
void table_add(sl::MultiOptTable& tab, sl::MultiOptTensor e, Launch&& launch) {
  const int64_t nc = (e.n + sl::kMultiOptChunk - 1) / sl::kMultiOptChunk;
  TORCH_CHECK(nc <= INT32_MAX, "tensor too large for one launch");
  if (tab.k == sl::kMultiOptMax || (int64_t)tab.chunks + nc > INT32_MAX) {
    launch(tab);
    tab.k = tab.chunks = 0;
  }
  e.chunk0 = tab.chunks;
  tab.t[tab.k++] = e;
  tab.chunks += (int)nc;
}

// One optimizer step over params[i] with grads[i] and state s0s[i] (, s1s[i] for Adam); s0s
// may be empty for SGD without momentum.  gscale: a device float every gradient is multiplied
// by first (clipping), or None.  Zero-element tensors are skipped.
void multi_opt(const std::vector<at::Tensor>& ps, const std::vector<at::Tensor>& gs,
               const std::vector<at::Tensor>& s0s, const std::vector<at::Tensor>& s1s, OPT_ARGS, const OptT& gscale) {
  TORCH_CHECK(kind == 1 || kind == 2, "multi_opt: kind 1 (SGD) or 2 (Adam)");
  const size_t k = ps.size();
  const bool has_s0 = !s0s.empty();
  TORCH_CHECK(gs.size() == k, "multi_opt: one gradient per parameter");
  TORCH_CHECK(s0s.size() == k || (!has_s0 && kind == 1 && momentum == 0.0), "multi_opt: one s0 per parameter");
  TORCH_CHECK(kind != 2 || s1s.size() == k, "multi_opt: Adam needs one s1 per parameter");
  if (k == 0) return;
  const float* gsc = nullptr;
  if (has(gscale)) {
    need_f32(*gscale, "gscale");
    TORCH_CHECK(gscale->numel() >= 1 && gscale->device() == ps[0].device(), "gscale: a float on the parameters' device");
    gsc = gscale->data_ptr<float>();
  }
  const SlOpt o = OPT_PASS;
  const hipStream_t st = cur_stream();
  auto launch = [&](const sl::MultiOptTable& tab) { ck(sl::multi_opt(tab, o, gsc, st), "multi_opt"); };
  sl::MultiOptTable tab{};
  for (size_t i = 0; i < k; ++i) {
    need_f32(ps[i], "param");
    TORCH_CHECK(ps[i].is_contiguous() && ps[i].device() == ps[0].device(), "params: contiguous, on one device");
    need_flat(gs[i], ps[i], "grad");
    if (has_s0) need_flat(s0s[i], ps[i], "s0");
    if (kind == 2) need_flat(s1s[i], ps[i], "s1");
    if (ps[i].numel() == 0) continue;
    table_add(tab, sl::MultiOptTensor{ps[i].data_ptr<float>(), gs[i].data_ptr<float>(),
                                      has_s0 ? s0s[i].data_ptr<float>() : nullptr,
                                      kind == 2 ? s1s[i].data_ptr<float>() : nullptr, ps[i].numel(), 0},
              launch);
  }
  if (tab.k) launch(tab);
}

// Global L2 norm of `gs`: out3 = {sum of squares, norm, min(1, max_norm / (norm + 1e-6))},
// through one partial sum per chunk in `ws`.  Deterministic (no atomics, fixed orders).
void grad_norm(const std::vector<at::Tensor>& gs, double max_norm, at::Tensor& out3, at::Tensor& ws) {
  need_f32(out3, "out3");
  need_f32(ws, "workspace");
  TORCH_CHECK(out3.is_contiguous() && out3.numel() >= 3 && ws.is_contiguous(), "out3 [3], contiguous workspace");
  TORCH_CHECK(ws.device() == out3.device(), "workspace on out3's device");
  int64_t total = 0;
  for (const auto& g : gs) {
    need_f32(g, "grad");
    TORCH_CHECK(g.is_contiguous() && g.device() == out3.device(), "grads: contiguous, on out3's device");
    total += (g.numel() + sl::kMultiOptChunk - 1) / sl::kMultiOptChunk;
  }
  TORCH_CHECK(ws.numel() >= total, "grad_norm workspace: one float per chunk");
  const hipStream_t st = cur_stream();
  float* slots = ws.data_ptr<float>();
  auto launch = [&](const sl::MultiOptTable& tab) {
    ck(sl::grad_sumsq(tab, slots, st), "grad_sumsq");
    slots += tab.chunks;
  };
  sl::MultiOptTable tab{};
  for (const auto& g : gs) {
    if (g.numel() == 0) continue;
    table_add(tab, sl::MultiOptTensor{nullptr, g.data_ptr<float>(), nullptr, nullptr, g.numel(), 0}, launch);
  }
  if (tab.k) launch(tab);
  ck(sl::grad_norm_finish(ws.data_ptr<float>(), total, (float)max_norm, out3.data_ptr<float>(), st), "grad_norm_finish");
}

// ---------------------------------------------------------------- general 3x3 conv (conv2d.hip)
// x [B, Cin, H, W], w [Cout, Cin, 3, 3], y / dy / am [B, Cout, Hy, Wy]: contiguous, fp32 (am
// uint8), on the current device, each under 2 GB (the kernels index with 32-bit byte offsets).
void conv_need(const at::Tensor& t, const char* name, bool u8 = false) {
  need_dense(t, u8 ? at::kByte : at::kFloat, name, true);
}

sl::Conv2dShape conv_shape(at::IntArrayRef x, at::IntArrayRef w, int64_t pad, bool relu, int64_t pool) {
  TORCH_CHECK(x.size() == 4 && w.size() == 4, "conv3x3: x [B, Cin, H, W], w [Cout, Cin, 3, 3]");
  TORCH_CHECK(w[1] == x[1] && w[2] == 3 && w[3] == 3, "conv3x3: w must be [Cout, Cin, 3, 3]");
  TORCH_CHECK(pad == 0 || pad == 1, "conv3x3: padding 0 or 1");
  TORCH_CHECK(pool == 0 || pool == 2, "conv3x3: pool 0 (none) or 2");
  TORCH_CHECK(x[0] >= 1 && x[1] >= 1 && w[0] >= 1 && x[2] >= 3 && x[3] >= 3, "conv3x3: empty or too small input");
  sl::Conv2dShape s;
  s.B = (int)x[0], s.Cin = (int)x[1], s.H = (int)x[2], s.W = (int)x[3], s.Cout = (int)w[0];
  s.pad = (int)pad, s.relu = relu, s.pool = pool == 2;
  s.Ho = s.H + 2 * s.pad - 2, s.Wo = s.W + 2 * s.pad - 2;
  s.Hy = s.pool ? s.Ho / 2 : s.Ho, s.Wy = s.pool ? s.Wo / 2 : s.Wo;
  TORCH_CHECK(s.Hy >= 1 && s.Wy >= 1, "conv3x3: the pooled conv output must be at least 2x2");
  // the un-stored conv output is indexed with 32-bit integers too
  TORCH_CHECK((int64_t)s.B * s.Cout * s.Ho * s.Wo < (int64_t(1) << 29), "conv3x3: conv output too large");
  return s;
}

void conv_check_y(const at::Tensor& t, const sl::Conv2dShape& s, const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.size(0) == s.B && t.size(1) == s.Cout && t.size(2) == s.Hy && t.size(3) == s.Wy, name,
              " must be [B, Cout, Hy, Wy]");
}

void conv3x3_fwd(const at::Tensor& x, const at::Tensor& w, const OptT& bias, at::Tensor& y, const OptT& am,
                 int64_t pad, bool relu, int64_t pool) {
  const sl::Conv2dShape s = conv_shape(x.sizes(), w.sizes(), pad, relu, pool);
  conv_need(x, "x");
  conv_need(w, "w");
  conv_need(y, "y");
  conv_check_y(y, s, "y");
  const bool has_b = has(bias);
  if (has_b) {
    conv_need(*bias, "bias");
    TORCH_CHECK(bias->numel() == s.Cout, "bias [Cout]");
  }
  TORCH_CHECK(has(am) == (bool)s.pool, "am goes with pooling");
  if (s.pool) {
    conv_need(*am, "am", true);
    conv_check_y(*am, s, "am");
  }
  ck(sl::conv3x3_fwd(x.data_ptr<float>(), w.data_ptr<float>(), has_b ? bias->data_ptr<float>() : nullptr,
                        y.data_ptr<float>(), s.pool ? am->data_ptr<uint8_t>() : nullptr, s, cur_stream()),
        "conv3x3_fwd");
}

// dy, y (, am) of the forward -> the operands of both backward kernels
const uint8_t* conv_check_bwd(const at::Tensor& dy, const at::Tensor& y, const OptT& am,
                              const sl::Conv2dShape& s) {
  conv_need(dy, "dy");
  conv_need(y, "y");
  conv_check_y(dy, s, "dy");
  conv_check_y(y, s, "y");
  TORCH_CHECK(has(am) == (bool)s.pool, "am goes with pooling");
  if (!s.pool) return nullptr;
  conv_need(*am, "am", true);
  conv_check_y(*am, s, "am");
  return am->data_ptr<uint8_t>();
}

void conv3x3_dgrad(const at::Tensor& dy, const at::Tensor& y, const OptT& am, const at::Tensor& w, at::Tensor& dx,
                   int64_t pad, bool relu, int64_t pool) {
  const sl::Conv2dShape s = conv_shape(dx.sizes(), w.sizes(), pad, relu, pool);
  conv_need(w, "w");
  conv_need(dx, "dx");
  const uint8_t* a = conv_check_bwd(dy, y, am, s);
  ck(sl::conv3x3_dgrad(dy.data_ptr<float>(), y.data_ptr<float>(), a, w.data_ptr<float>(), dx.data_ptr<float>(), s,
                          cur_stream()),
        "conv3x3_dgrad");
}

int64_t conv3x3_wgrad_ws(std::vector<int64_t> x_shape, std::vector<int64_t> w_shape, int64_t pad, int64_t pool) {
  const sl::Conv2dShape s = conv_shape(x_shape, w_shape, pad, false, pool);
  return (int64_t)sl::conv3x3_wgrad_slabs(s) * s.Cout * (s.Cin * 9 + 1);
}

void conv3x3_wgrad(const at::Tensor& dy, const at::Tensor& y, const OptT& am, const at::Tensor& x, at::Tensor& ws,
                   at::Tensor& dw, const OptT& db, int64_t pad, bool relu, int64_t pool) {
  const sl::Conv2dShape s = conv_shape(x.sizes(), dw.sizes(), pad, relu, pool);
  conv_need(x, "x");
  conv_need(dw, "dw");
  conv_need(ws, "workspace");
  TORCH_CHECK(ws.numel() >= (int64_t)sl::conv3x3_wgrad_slabs(s) * s.Cout * (s.Cin * 9 + 1), "conv3x3_wgrad workspace");
  const bool has_b = has(db);
  if (has_b) {
    conv_need(*db, "db");
    TORCH_CHECK(db->numel() == s.Cout, "db [Cout]");
  }
  const uint8_t* a = conv_check_bwd(dy, y, am, s);
  ck(sl::conv3x3_wgrad(dy.data_ptr<float>(), y.data_ptr<float>(), a, x.data_ptr<float>(), ws.data_ptr<float>(),
                          dw.data_ptr<float>(), has_b ? db->data_ptr<float>() : nullptr, s, cur_stream()),
        "conv3x3_wgrad");
}

// ---------------------------------------------------------------- GroupNorm (groupnorm.hip)
// x / dx [B, C, *], y / dy / am [B, C, *] or [B, C, H / 2, W / 2] with pooling, mean / rstd [B, G],
// w / b / dw / db [C] (all four absent without the affine): contiguous, fp32 (am uint8), on the
// current device, each under 2 GB.
sl::GroupNormShape gn_shape(at::IntArrayRef x, int64_t groups, double eps, bool relu, int64_t pool) {
  TORCH_CHECK(x.size() >= 2, "group_norm: x [B, C, *]");
  TORCH_CHECK(pool == 0 || pool == 2, "group_norm: pool 0 (none) or 2");
  TORCH_CHECK(groups >= 1 && x[1] >= 1 && x[1] % groups == 0, "group_norm: C must be a multiple of the groups");
  int64_t L = 1;
  for (size_t i = 2; i < x.size(); ++i) L *= x[i];
  TORCH_CHECK(x[0] >= 1 && L >= 1, "group_norm: empty input");
  TORCH_CHECK(x[0] * x[1] * L < (int64_t(1) << 29), "group_norm: input too large");
  sl::GroupNormShape s{};
  s.B = (int)x[0], s.C = (int)x[1], s.G = (int)groups, s.L = (int)L;
  s.relu = relu, s.pool = pool == 2, s.eps = (float)eps;
  if (s.pool) {
    TORCH_CHECK(x.size() == 4 && x[2] >= 2 && x[3] >= 2, "group_norm: pooling needs [B, C, H, W] with H, W >= 2");
    s.H = (int)x[2], s.W = (int)x[3], s.Hy = s.H / 2, s.Wy = s.W / 2;
  }
  return s;
}

void gn_check_y(const at::Tensor& t, const at::Tensor& x, const sl::GroupNormShape& s, const char* name, bool u8) {
  conv_need(t, name, u8);
  if (s.pool) {
    TORCH_CHECK(t.dim() == 4 && t.size(0) == s.B && t.size(1) == s.C && t.size(2) == s.Hy && t.size(3) == s.Wy, name,
                " must be [B, C, H / 2, W / 2]");
  } else {
    TORCH_CHECK(t.sizes() == x.sizes(), name, " must have x's shape");
  }
}

void gn_check_vec(const at::Tensor& t, int64_t numel, const char* name) {
  conv_need(t, name);
  TORCH_CHECK(t.numel() == numel, name, " has the wrong number of elements");
}

// the affine's two vectors: both or neither
bool gn_affine(const OptT& w, const OptT& b, int C, const char* wn, const char* bn) {
  const bool has_w = has(w), has_b = has(b);
  TORCH_CHECK(has_w == has_b, "group_norm: ", wn, " and ", bn, " go together");
  if (has_w) {
    gn_check_vec(*w, C, wn);
    gn_check_vec(*b, C, bn);
  }
  return has_w;
}

const uint8_t* gn_check_am(const OptT& am, const at::Tensor& x, const sl::GroupNormShape& s) {
  TORCH_CHECK(has(am) == (bool)s.pool, "am goes with pooling");
  if (!s.pool) return nullptr;
  gn_check_y(*am, x, s, "am", true);
  return am->data_ptr<uint8_t>();
}

void group_norm_fwd(const at::Tensor& x, const OptT& w, const OptT& b, at::Tensor& y, at::Tensor& mean,
                    at::Tensor& rstd, const OptT& am, int64_t groups, double eps, bool relu, int64_t pool) {
  const sl::GroupNormShape s = gn_shape(x.sizes(), groups, eps, relu, pool);
  conv_need(x, "x");
  gn_check_y(y, x, s, "y", false);
  gn_check_vec(mean, (int64_t)s.B * s.G, "mean");
  gn_check_vec(rstd, (int64_t)s.B * s.G, "rstd");
  const bool affine = gn_affine(w, b, s.C, "weight", "bias");
  const uint8_t* a = gn_check_am(am, x, s);
  ck(sl::group_norm_fwd(x.data_ptr<float>(), affine ? w->data_ptr<float>() : nullptr,
                           affine ? b->data_ptr<float>() : nullptr, y.data_ptr<float>(), mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), const_cast<uint8_t*>(a), s, cur_stream()),
        "group_norm_fwd");
}

void group_norm_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& mean, const at::Tensor& rstd,
                    const OptT& w, const OptT& b, const OptT& am, const OptT& dx, const OptT& ws, const OptT& dw,
                    const OptT& db, int64_t groups, bool relu, int64_t pool) {
  const sl::GroupNormShape s = gn_shape(x.sizes(), groups, 0.0, relu, pool);
  conv_need(x, "x");
  gn_check_y(dy, x, s, "dy", false);
  gn_check_vec(mean, (int64_t)s.B * s.G, "mean");
  gn_check_vec(rstd, (int64_t)s.B * s.G, "rstd");
  const bool affine = gn_affine(w, b, s.C, "weight", "bias");
  TORCH_CHECK(gn_affine(dw, db, s.C, "dweight", "dbias") == affine, "group_norm: dweight / dbias go with the affine");
  const bool has_ws = has(ws);
  TORCH_CHECK(has_ws == affine, "group_norm: the workspace goes with the affine");
  if (affine) {
    conv_need(*ws, "workspace");
    TORCH_CHECK(ws->numel() >= (int64_t)s.B * s.C * 2, "group_norm workspace: [B, C, 2]");
  }
  const bool need_dx = has(dx);
  if (need_dx) {
    conv_need(*dx, "dx");
    TORCH_CHECK(dx->sizes() == x.sizes(), "dx must have x's shape");
  }
  const uint8_t* a = gn_check_am(am, x, s);
  ck(sl::group_norm_bwd(dy.data_ptr<float>(), x.data_ptr<float>(), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                           affine ? w->data_ptr<float>() : nullptr, affine ? b->data_ptr<float>() : nullptr, a,
                           need_dx ? dx->data_ptr<float>() : nullptr, affine ? ws->data_ptr<float>() : nullptr,
                           affine ? dw->data_ptr<float>() : nullptr, affine ? db->data_ptr<float>() : nullptr, s,
                           cur_stream()),
        "group_norm_bwd");
}

// ---------------------------------------------------------------- cut codec (cutcodec.hip)
// x / y [R, K] fp32, payload int8 [R, K] (8 bits) or uint8 [R, ceil(K / 2)] (4 bits), scales fp32
// [R, ceil(K / group)]: contiguous, on the current device.  R, K < 2^31; the kernels index in 64 bits.
void cut_need(const at::Tensor& t, at::ScalarType ty, const char* name) {
  need_dense(t, ty, name);
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
}

sl::CutShape cut_shape(int64_t R, int64_t K, int64_t bits, int64_t group, uint64_t seed, bool stochastic) {
  TORCH_CHECK(bits == 8 || bits == 4, "cut codec: bits must be 8 or 4");
  TORCH_CHECK(group == 16 || group == 32 || group == 64 || group == 128 || group == 256,
              "cut codec: group must be 16, 32, 64, 128 or 256");
  TORCH_CHECK(R >= 1 && K >= 1, "cut codec: empty input");
  TORCH_CHECK(R < (int64_t(1) << 31) && K < (int64_t(1) << 31), "cut codec: R and K must be below 2^31");
  sl::CutShape s{};
  s.R = (int)R, s.K = (int)K, s.group = (int)group, s.ng = (int)((K + group - 1) / group), s.bits = (int)bits;
  s.stochastic = stochastic, s.seed_lo = (uint32_t)seed, s.seed_hi = (uint32_t)(seed >> 32);
  return s;
}

void cut_check_wire(const at::Tensor& payload, const at::Tensor& scales, const sl::CutShape& s) {
  if (s.bits == 8) cut_need(payload, at::kChar, "payload");
  else cut_need(payload, at::kByte, "payload");
  cut_need(scales, at::kFloat, "scales");
  const int64_t kb = s.bits == 8 ? s.K : ((int64_t)s.K + 1) / 2;
  TORCH_CHECK(payload.size(0) == s.R && payload.size(1) == kb, "payload must be [R, K] (8 bits) or [R, ceil(K / 2)] (4 bits)");
  TORCH_CHECK(scales.size(0) == s.R && scales.size(1) == s.ng, "scales must be [R, ceil(K / group)]");
}

void cut_pack(const at::Tensor& x, at::Tensor& payload, at::Tensor& scales, int64_t bits, int64_t group, uint64_t seed,
              bool stochastic) {
  cut_need(x, at::kFloat, "x");
  const sl::CutShape s = cut_shape(x.size(0), x.size(1), bits, group, seed, stochastic);
  cut_check_wire(payload, scales, s);
  TORCH_CHECK(payload.device() == x.device() && scales.device() == x.device(), "cut_pack: tensors on different devices");
  ck(sl::cut_pack(x.data_ptr<float>(), payload.data_ptr(), scales.data_ptr<float>(), s, cur_stream()), "cut_pack");
}

void cut_unpack(const at::Tensor& payload, const at::Tensor& scales, at::Tensor& y, int64_t bits, int64_t group) {
  cut_need(y, at::kFloat, "y");
  const sl::CutShape s = cut_shape(y.size(0), y.size(1), bits, group, 0, false);
  cut_check_wire(payload, scales, s);
  TORCH_CHECK(payload.device() == y.device() && scales.device() == y.device(), "cut_unpack: tensors on different devices");
  ck(sl::cut_unpack(payload.data_ptr(), scales.data_ptr<float>(), y.data_ptr<float>(), s, cur_stream()), "cut_unpack");
}

void cut_roundtrip(const at::Tensor& x, at::Tensor& y, int64_t bits, int64_t group, uint64_t seed, bool stochastic) {
  cut_need(x, at::kFloat, "x");
  cut_need(y, at::kFloat, "y");
  TORCH_CHECK(y.sizes() == x.sizes() && y.device() == x.device(), "cut_roundtrip: y must have x's shape and device");
  const sl::CutShape s = cut_shape(x.size(0), x.size(1), bits, group, seed, stochastic);
  ck(sl::cut_roundtrip(x.data_ptr<float>(), y.data_ptr<float>(), s, cur_stream()), "cut_roundtrip");
}

// ---------------------------------------------------------------- loss / metrics
void softmax_ce(const at::Tensor& x, const at::Tensor& y, int64_t ignore, double scale, at::Tensor& loss_rows,
                const OptT& d) {
  need_2d(x, "logits");
  const int64_t M = x.size(0), C = x.size(1);
  need_cuda(y, "labels");
  TORCH_CHECK(y.scalar_type() == at::kLong && y.numel() == M && y.is_contiguous(), "labels int64 [M]");
  need_f32(loss_rows, "loss_rows");
  TORCH_CHECK(loss_rows.numel() >= M, "loss_rows");
  float* dp = nullptr;
  int ldd = 0;
  if (has(d)) {
    need_2d(*d, "dlogits");
    TORCH_CHECK(d->size(0) == M && d->size(1) == C, "dlogits shape");
    dp = d->data_ptr<float>();
    ldd = (int)d->stride(0);
  }
  ck(sl::softmax_ce(x.data_ptr<float>(), (int)x.stride(0), y.data_ptr<int64_t>(), ignore, (float)scale,
                       loss_rows.data_ptr<float>(), dp, ldd, (int)M, (int)C, cur_stream()),
        "softmax_ce");
}

void relu_mask(const at::Tensor& d, const at::Tensor& h, double scale, at::Tensor& out) {
  need_f32(d, "d");
  need_f32(h, "h");
  need_f32(out, "out");
  TORCH_CHECK(d.is_contiguous() && h.is_contiguous() && out.is_contiguous() && d.numel() == h.numel() &&
                  out.numel() == d.numel(),
              "relu_mask: contiguous tensors of one size");
  ck(sl::relu_mask(d.data_ptr<float>(), h.data_ptr<float>(), (float)scale, out.data_ptr<float>(), d.numel(),
                      cur_stream()),
        "relu_mask");
}

void eval_counters(const at::Tensor& x, const at::Tensor& y, int64_t omit, at::Tensor& counters) {
  need_2d(x, "logits");
  TORCH_CHECK(y.scalar_type() == at::kLong && y.numel() == x.size(0) && y.is_contiguous(), "labels");
  TORCH_CHECK(counters.scalar_type() == at::kLong && counters.numel() >= 6 && counters.is_contiguous(), "counters");
  need_cuda(counters, "counters");
  ck(sl::eval_counters(x.data_ptr<float>(), (int)x.stride(0), y.data_ptr<int64_t>(), omit,
                          reinterpret_cast<unsigned long long*>(counters.data_ptr<int64_t>()), (int)x.size(0),
                          (int)x.size(1), cur_stream()),
        "eval_counters");
}

// Partial products into a workspace; return the number of slabs S (result = ws[:S*M*cols]).
int64_t linear_fwd_partial(const at::Tensor& X, const at::Tensor& W, at::Tensor& ws, int64_t max_split) {
  need_rows(X, "X");
  need_rows(W, "W");
  need_f32(ws, "ws");
  TORCH_CHECK(ws.is_contiguous(), "ws contiguous");
  const int64_t M = X.size(0), K = X.size(1), N = W.size(0);
  TORCH_CHECK(W.size(1) == K && K % 4 == 0, "W must be [N,K] with K % 4 == 0");
  int S = 1;
  ck(sl::linear_fwd_partial(X.data_ptr<float>(), (int)X.stride(0), W.data_ptr<float>(), (int)W.stride(0), (int)M,
                               (int)N, (int)K, ws.data_ptr<float>(), ws.numel(), (int)max_split, &S, cur_stream()),
        "linear_fwd_partial");
  return S;
}

// ---------------------------------------------------------------- fused server step
// P2: fc2 partial sums, [S2, M, N2] split-K slabs or a reduced [M, N2] tensor.
void server_head3(const at::Tensor& P2, const OptT& b2, bool relu2, double drop2, uint64_t seed2, int64_t dseed2,
                  const at::Tensor& W3, const OptT& b3, const at::Tensor& y, int64_t ignore, double scale,
                  at::Tensor& h2, at::Tensor& dlog, at::Tensor& dz2, at::Tensor& loss_rows, at::Tensor& ws, int64_t G,
                  const OptT& gscale) {
  need_f32(P2, "P2");
  TORCH_CHECK(P2.is_contiguous() && (P2.dim() == 2 || P2.dim() == 3), "P2 [S,M,N2] or [M,N2] contiguous");
  const int64_t S2 = P2.dim() == 3 ? P2.size(0) : 1;
  const int64_t M = P2.size(P2.dim() - 2), N2 = P2.size(P2.dim() - 1);
  need_rows(W3, "W3");
  const int64_t C = W3.size(0);
  TORCH_CHECK(W3.size(1) == N2 && N2 % 4 == 0 && W3.stride(0) % 4 == 0 && C <= 4096, "W3 [C, N2], N2 % 4 == 0");
  need_f32(ws, "ws");
  TORCH_CHECK(ws.is_contiguous() && ws.numel() >= (int64_t)sl::head3_slices((int)N2) * M * C, "head workspace");
  need_cuda(y, "labels");
  TORCH_CHECK(G >= 1 && C % G == 0, "C % groups");
  TORCH_CHECK(y.scalar_type() == at::kLong && y.numel() == M * G && y.is_contiguous(), "labels int64 [M, groups]");
  if (has(gscale)) {
    need_f32(*gscale, "gscale");
    TORCH_CHECK(gscale->is_contiguous() && gscale->numel() == M * G, "gscale [M, groups]");
  }
  for (auto* t : {&h2, &dz2}) {
    need_f32(*t, "h2/dz2");
    TORCH_CHECK(t->is_contiguous() && t->size(0) == M && t->size(1) == N2, "h2/dz2 [M,N2]");
  }
  need_f32(dlog, "dlog");
  TORCH_CHECK(dlog.is_contiguous() && dlog.size(0) == M && dlog.size(1) == C, "dlog [M,C]");
  need_f32(loss_rows, "loss_rows");
  TORCH_CHECK(loss_rows.numel() >= M * G, "loss_rows [M, groups]");
  ck(sl::server_head3(P2.data_ptr<float>(), (int)S2, M * N2, make_epi(b2, relu2, drop2, seed2, 0, dseed2),
                         W3.data_ptr<float>(), (int)W3.stride(0), opt_ptr(b3), y.data_ptr<int64_t>(), ignore,
                         (float)scale, h2.data_ptr<float>(), dlog.data_ptr<float>(), dz2.data_ptr<float>(),
                         loss_rows.data_ptr<float>(), ws.data_ptr<float>(), ws.numel(), (int)M, (int)N2, (int)C,
                         cur_stream(), nullptr, (int)G, opt_ptr(gscale)),
        "server_head3");
}

// layers: up to 3 tuples (dz, A, W, s0, s1, bias, sb0, sb1).
// xn / pn (optional): next batch [mn, K0] -> its split-K partial pre-activations of layer 0
// with the updated weights, pn = [ceil(K0/256), mn, N0].
void wgrad_group(const std::vector<py::tuple>& layers, int64_t M, const OptT& xn, const OptT& pn, OPT_ARGS) {
  TORCH_CHECK(!layers.empty() && layers.size() <= 3, "1..3 layers");
  sl::WgGroup g{};
  g.n = (int)layers.size();
  for (size_t i = 0; i < layers.size(); ++i) {
    const py::tuple& L = layers[i];
    TORCH_CHECK(L.size() == 8, "layer tuple (dz, A, W, s0, s1, bias, sb0, sb1)");
    auto opt = [&](int j) -> OptT { return L[j].is_none() ? OptT() : OptT(L[j].cast<at::Tensor>()); };
    const at::Tensor dz = L[0].cast<at::Tensor>();
    const at::Tensor A = L[1].cast<at::Tensor>();
    at::Tensor W = L[2].cast<at::Tensor>();
    at::Tensor s0 = L[3].cast<at::Tensor>();
    need_rows(A, "A");
    need_rows(W, "W");
    need_rows(s0, "s0");
    const int64_t N = W.size(0), K = W.size(1);
    TORCH_CHECK(A.size(0) == M && A.size(1) == K && K % 4 == 0, "A [M,K]");
    TORCH_CHECK(s0.sizes() == W.sizes() && s0.stride(0) == W.stride(0), "s0 like W");
    OptT s1 = opt(4), bias = opt(5), sb0 = opt(6), sb1 = opt(7);
    if (kind == 2) TORCH_CHECK(s1.has_value() && s1->sizes() == W.sizes() && s1->stride(0) == W.stride(0), "s1");
    if (bias.has_value()) TORCH_CHECK(bias->numel() == N && sb0.has_value() && sb0->numel() == N, "bias state");
    sl::WgDesc& d = g.d[i];
    need_2d(dz, "dz");
    TORCH_CHECK(dz.size(0) == M && dz.size(1) == N, "dz [M,N]");
    d.dz = dz.data_ptr<float>();
    d.ldz = (int)dz.stride(0);
    d.A = A.data_ptr<float>();
    d.lda = (int)A.stride(0);
    d.W = W.data_ptr<float>();
    d.ldw = (int)W.stride(0);
    d.s0 = s0.data_ptr<float>();
    d.s1 = opt_ptr(s1);
    d.bias = opt_ptr(bias);
    d.sb0 = opt_ptr(sb0);
    d.sb1 = opt_ptr(sb1);
    d.N = (int)N;
    d.K = (int)K;
  }
  if (has(xn)) {
    TORCH_CHECK(has(pn), "pn needed with xn");
    need_rows(*xn, "xn");
    need_f32(*pn, "pn");
    const int64_t K0 = g.d[0].K, N0 = g.d[0].N, mn = xn->size(0);
    TORCH_CHECK(xn->size(1) == K0 && mn >= 1 && mn <= 64, "xn [mn<=64, K0]");
    TORCH_CHECK(pn->is_contiguous() && pn->numel() >= (K0 + 255) / 256 * mn * N0, "pn [K0/256, mn, N0]");
    g.xn = xn->data_ptr<float>();
    g.ldxn = (int)xn->stride(0);
    g.mn = (int)mn;
    g.pn = pn->data_ptr<float>();
  }
  ck(sl::wgrad_group(g, (int)M, OPT_PASS, cur_stream()), "wgrad_group");
}

}  // namespace

void sl_register_comm(pybind11::module& m);
void sl_register_engine(pybind11::module& m);
void sl_register_split(pybind11::module& m);
void sl_register_resident(pybind11::module& m);
void sl_register_hybrid(pybind11::module& m);
void sl_register_vanilla(pybind11::module& m);
void sl_register_ushape(pybind11::module& m);
void sl_register_handoff(pybind11::module& m);

PYBIND11_MODULE(_C, m) {
  m.doc() = "splitlearning_amd gfx950 (MI355X) HIP kernels";
  sl_register_comm(m);
  sl_register_engine(m);
  sl_register_split(m);
  sl_register_resident(m);
  sl_register_hybrid(m);
  sl_register_vanilla(m);
  sl_register_ushape(m);
  sl_register_handoff(m);
  m.def("conv_fwd", &conv_fwd);
  m.def("conv_local_step", &conv_local_step);
  m.def("conv_bwd_step", &conv_bwd_step);
  m.def("conv_bwd_defer", &conv_bwd_defer);
  m.def("conv_fwd_pending", &conv_fwd_pending);
  m.def("conv_apply", &conv_apply);
  m.def("head_step", &head_step);
  m.def("conv_local_epoch", &conv_local_epoch);
  m.def("conv_local_epoch_multi", &conv_local_epoch_multi);
  m.def("conv_fwd_multi", &conv_fwd_multi);
  m.def("alice_step_desc_bytes", []() { return (int64_t)sl::alice_step_desc_bytes(); });
  m.def("linear_fwd", &linear_fwd);
  m.def("linear_epilogue", &linear_epilogue);
  m.def("linear_dgrad", &linear_dgrad);
  m.def("gemm_nn_dgrad", &gemm_nn_dgrad);
  m.def("linear_wgrad_opt", &linear_wgrad_opt);
  m.def("opt_flat", &opt_flat);
  m.def("multi_opt", &multi_opt);
  m.def("grad_norm", &grad_norm);
  m.def("conv3x3_fwd", &conv3x3_fwd);
  m.def("conv3x3_dgrad", &conv3x3_dgrad);
  m.def("conv3x3_wgrad", &conv3x3_wgrad);
  m.def("conv3x3_wgrad_ws", &conv3x3_wgrad_ws);
  m.def("group_norm_fwd", &group_norm_fwd);
  m.def("group_norm_bwd", &group_norm_bwd);
  m.def("cut_pack", &cut_pack);
  m.def("cut_unpack", &cut_unpack);
  m.def("cut_roundtrip", &cut_roundtrip);
  m.attr("multi_opt_chunk") = (int64_t)sl::kMultiOptChunk;
  m.attr("multi_opt_max") = (int64_t)sl::kMultiOptMax;
  m.def("softmax_ce", &softmax_ce);
  m.def("eval_counters", &eval_counters);
  m.def("relu_mask", &relu_mask);
  m.def("server_head3", &server_head3);
  m.def("head3_slices", [](int64_t n2) { return (int64_t)sl::head3_slices((int)n2); });
  m.def("linear_fwd_partial", &linear_fwd_partial);
  m.def("wgrad_group", &wgrad_group);
  // Kernel-variant slots for A/B runs of work in progress (0 = the default everywhere).  A
  // slot lives only while its alternative is being measured; the losers are removed with the
  // numbers kept in docs/PERF.md.  In use:
  //   11 fp32 products of M > 128 rows: 1 = the in-tree tiled GEMM instead of hipBLASLt
  m.def("set_variant", [](int64_t slot, int64_t v) {
    TORCH_CHECK(slot >= 0 && slot < 24, "variant slot");
    sl::g_variant[slot] = (int)v;
  });
  m.def("get_variant", [](int64_t slot) {
    TORCH_CHECK(slot >= 0 && slot < 24, "variant slot");
    return (int64_t)sl::g_variant[slot];
  });
  // compute dtype of the GEMM-shaped kernels (forward / data-gradient products): fp32 (exact
  // v_mfma_f32_*_f32) or bf16 (operands rounded to bf16, bf16 MFMA, fp32 accumulation);
  // parameters, optimizer state and the fused optimizer update stay fp32 either way
  m.def("set_compute_dtype", [](const std::string& d) {
    TORCH_CHECK(d == "fp32" || d == "bf16", "compute dtype fp32 | bf16");
    sl::g_bf16 = d == "bf16" ? 1 : 0;
  });
  m.def("get_compute_dtype", []() { return std::string(sl::g_bf16 ? "bf16" : "fp32"); });
  // gemm_nn_dgrad's split over the reduction: 0 = its own choice (default), else forced (sweeps)
  m.def("set_gemm_nn_splits", [](int s) { sl::g_nn_splits = s < 0 ? 0 : s; });
  m.def("set_gemm_nn_form", [](int wm) { sl::g_nn_wm = (wm == 2 || wm == 4) ? wm : 0; });
  m.def("set_gemm_nt_splits", [](int s) { sl::g_nt_splits = s < 0 ? 0 : s; });
  m.attr("arch") = "gfx950";
}
