// Multi-tensor optimizer step and global gradient norm (optim.hip): one launch walks a list
// of fp32 tensors cut into fixed-size chunks of elements, one workgroup per chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace sl {

// Elements per chunk: 256 threads x 2 f32x4 per array, so an Adam workgroup has 8 16-byte
// loads per thread in flight and stays at 8 waves per SIMD.  Chunks start at multiples of
// kMultiOptChunk elements inside a tensor, so a 16-byte aligned tensor has aligned chunks.
constexpr int kMultiOptChunk = 2048;
// Tensors per launch: the table travels by value in the kernel arguments (64 x 48 B + 8 B,
// with SlOpt and gscale 3.1 KB of the 4 KB a launch may carry).
constexpr int kMultiOptMax = 64;

struct MultiOptTensor {
  float* p;
  const float* g;
  float* s0;   // Adam m / SGD momentum buffer (null: SGD without momentum)
  float* s1;   // Adam v
  int64_t n;
  int chunk0;  // index of this tensor's first chunk within the launch
};
struct MultiOptTable {
  MultiOptTensor t[kMultiOptMax];
  int k;       // tensors in use
  int chunks;  // chunks of all tensors = workgroups of the launch
};

// One optimizer step (o.kind 1 = SGD, 2 = Adam) over every tensor of `tab`; `gscale`, when
// set, points at a device float every gradient element is multiplied by first.
hipError_t multi_opt(const MultiOptTable& tab, SlOpt o, const float* gscale, hipStream_t st);
// Sum of squares of every chunk of the table's gradients -> slots[0 .. tab.chunks).
hipError_t grad_sumsq(const MultiOptTable& tab, float* slots, hipStream_t st);
// out3 = {sum of slots, its square root, min(1, max_norm / (norm + 1e-6))}
hipError_t grad_norm_finish(const float* slots, int64_t nslots, float max_norm, float* out3, hipStream_t st);

}  // namespace sl
