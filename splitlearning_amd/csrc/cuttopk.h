// Cut sparsifier (cuttopk.hip): per-row magnitude top-k of the tensor that crosses the cut, for
// splitlearning_amd.nn.CutTopK / cut_sparsify / cut_densify / cut_sparse_grad.  Built into the
// second extension module, _C2 (bindings2.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sl {

// A row of up to this many floats is copied to LDS by the first selection pass and read from
// there by the later ones; a longer row is re-read from global memory.  With the histogram and
// the alignment slack that is 65104 bytes of LDS, under the 64 KB a launch gets without opting in.
constexpr int kCutTopkLdsFloats = 16000;

// x, y, d, dx fp32 [R, K]; values fp32 [R, k]; indices int32 [R, k], ascending in a row.
// 1 <= k <= K < 2^31.
struct TopkShape {
  int R, K, k;
};

// The k largest |x| of each row (ties at the threshold: lowest columns) as values + indices;
// y, when given, also receives the dense row (x on the support, +0.0 elsewhere) in the same pass.
hipError_t cut_topk(const float* x, float* values, int32_t* indices, float* y, TopkShape s, hipStream_t st);
// y = 0 everywhere but y[r, indices[r, j]] = values[r, j]; an index outside [0, K) is skipped
hipError_t cut_scatter(const float* values, const int32_t* indices, float* y, TopkShape s, hipStream_t st);
// dx = d on the support, 0 elsewhere (cut_scatter of cut_gather, one launch)
hipError_t cut_mask(const float* d, const int32_t* indices, float* dx, TopkShape s, hipStream_t st);
// values[r, j] = d[r, indices[r, j]] (0 for an index outside [0, K))
hipError_t cut_gather(const float* d, const int32_t* indices, float* values, TopkShape s, hipStream_t st);

}  // namespace sl
