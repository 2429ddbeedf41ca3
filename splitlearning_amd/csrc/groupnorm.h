// GroupNorm + optional ReLU + optional 2x2 max-pool (groupnorm.hip): forward, backward and the
// parameter-gradient sum of splitlearning_amd.nn.FusedGroupNorm.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sl {

// x [B, C, L] (L = the product of the trailing dimensions, H * W with pooling) -> y [B, C, Ly]:
// Ly = L without pooling and floor(H / 2) * floor(W / 2) with it.  A (sample, group) pair is one
// contiguous span of n = (C / G) * L floats of x.
struct GroupNormShape {
  int B, C, G, L, H, W, Hy, Wy, relu, pool;
  float eps;
};

// Floats of a span the kernels keep in LDS between their passes; a longer span is re-read
// (groupnorm.hip says why the switch-over lies here).
constexpr int kGroupNormLdsFloats = 16000;

// y, mean / rstd [B, G] (and am, the 2-bit window position of the maximum, with pooling).
// w and b are both null without the affine.
hipError_t group_norm_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd,
                          uint8_t* am, GroupNormShape s, hipStream_t st);
// dx [B, C, L] (null: no input gradient) and, with the affine, dw / db [C] through the
// [B, C, 2] workspace ws of per-sample channel sums {sum dz, sum dz * xh}.
hipError_t group_norm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                          const float* b, const uint8_t* am, float* dx, float* ws, float* dw, float* db,
                          GroupNormShape s, hipStream_t st);

}  // namespace sl
