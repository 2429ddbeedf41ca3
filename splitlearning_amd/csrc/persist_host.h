// Host scaffold shared by the executors of the persistent one-launch epochs (resident_exec.cpp,
// hybrid_exec.cpp, vanilla_exec.cpp, ushape_exec.cpp): the per-step tables handed to the kernels
// (dropout seed words, Adam scalars, row counts) and the chunked launch loop with its error-word
// and fault-injection rules.  The table layouts belong to the kernels (resident.h / hybrid.h
// adam[S][4], vanilla.h adam[S][4], ushape.h tabf[S][8]); only the loops that fill them are here.
#pragma once
#include <torch/extension.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "args.h"
#include "host.h"
#include "resident.h"

namespace sl {
namespace host {

// a tail layer's parameters and optimizer state as the kernels take them (v / vb null without Adam)
inline ResLayer res_layer(const args::TailLayer& L) {
  return ResLayer{L.W.data_ptr<float>(), L.s0.data_ptr<float>(), L.v(),
                  L.b.data_ptr<float>(), L.sb0.data_ptr<float>(), L.vb()};
}

inline at::Tensor upload(const std::vector<float>& v, const at::Device& dev) {
  return at::from_blob(const_cast<float*>(v.data()), {(int64_t)v.size()}, at::TensorOptions().dtype(at::kFloat)).to(dev);
}

// [S][4] seed words {fc1 lo, hi, fc2 lo, hi} of the forward counts fwd_count + 1 .. fwd_count + S
// (host.h step_seed of layers 0 and 1), int32 on dev
inline at::Tensor step_seeds(int64_t S, int64_t seed_base, int64_t fwd_count, const at::Device& dev) {
  std::vector<int32_t> seeds(4 * S);
  for (int64_t i = 0; i < S; ++i)
    for (int l = 0; l < 2; ++l) {
      const uint64_t s = step_seed((uint64_t)seed_base, (uint64_t)l, (uint64_t)(fwd_count + 1 + i));
      seeds[4 * i + 2 * l] = (int32_t)(uint32_t)(s & 0xffffffffull);
      seeds[4 * i + 2 * l + 1] = (int32_t)(uint32_t)(s >> 32);
    }
  return at::from_blob(seeds.data(), {4 * S}, at::TensorOptions().dtype(at::kInt)).to(dev);
}

// Adam's {step_size, 1 / sqrt(bc2)} of optimizer steps t + 1 .. into tab[stride * i + off],
// [.. + 1]; opt_at(step) is the executor's make_opt_raw of that step
template <typename OptAt>
inline void fill_adam(std::vector<float>& tab, int stride, int off, int64_t t, OptAt opt_at) {
  const int64_t S = (int64_t)tab.size() / stride;
  for (int64_t i = 0; i < S; ++i) {
    const SlOpt o = opt_at(t + 1 + i);
    tab[stride * i + off] = o.step_size;
    tab[stride * i + off + 1] = o.inv_bc2_sqrt;
  }
}

// The CE scale 1 / rows_at(i) into tab[stride * i + off_inv] and, for off_rows >= 0, the row
// count itself into tab[stride * i + off_rows]
template <typename RowsAt>
inline void fill_rows(std::vector<float>& tab, int stride, int off_inv, int off_rows, RowsAt rows_at) {
  const int64_t S = (int64_t)tab.size() / stride;
  for (int64_t i = 0; i < S; ++i) {
    const int64_t rows = rows_at(i);
    tab[stride * i + off_inv] = (float)(1.0 / (double)rows);
    if (off_rows >= 0) tab[stride * i + off_rows] = (float)rows;
  }
}

// One epoch of S steps as launches of at most max_steps steps.  The error word (device address
// err_word, err its one-int tensor) is cleared once, on the stream: a wait that gave up in an
// earlier run, whose exception the caller handled, must not make this one give up.  A chunk whose
// wait gave up leaves the word set, and the host reads it before issuing the next chunk (one sync
// per chunk of thousands of steps), so no later chunk runs on half-updated state: the kernels
// read the word only inside a wait that is not already met and cannot be relied on to stop by
// themselves.  chunk(s0, ns, fault) issues steps [s0, s0 + ns); fault is the tests' injected
// fault_step mapped into the chunk (-1: none), disarmed after the epoch (one fault per arming).
// Returns the error word after the last chunk (one sync per epoch); `what` names the executor in
// the one message raised here.
template <typename F>
inline int run_chunks(const char* what, int* err_word, const at::Tensor& err, hipStream_t st, int64_t S,
                      int64_t max_steps, int64_t& fault_step, F chunk) {
  TORCH_CHECK(hipMemsetAsync(err_word, 0, sizeof(int), st) == hipSuccess, what, " error word");
  const int64_t cs = std::max<int64_t>(1, std::min(S, max_steps));
  for (int64_t s0 = 0; s0 < S; s0 += cs) {
    if (s0 > 0 && err.item<int>() != 0) break;
    const int64_t ns = std::min(cs, S - s0);
    chunk(s0, ns, fault_step >= s0 && fault_step < s0 + ns ? (int)(fault_step - s0) : -1);
  }
  fault_step = -1;
  return err.item<int>();
}

}  // namespace host
}  // namespace sl
