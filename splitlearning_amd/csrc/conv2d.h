// General 3x3 convolution (stride 1, padding 0 or 1) + optional ReLU + optional 2x2 max-pool
// as implicit GEMMs (conv2d.hip): forward, data gradient and weight gradient of
// splitlearning_amd.nn.FusedConv2d.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sl {

// x [B, Cin, H, W] -> conv output [B, Cout, Ho, Wo] (never stored) -> y [B, Cout, Hy, Wy]:
// Hy x Wy is Ho x Wo without pooling and floor(Ho / 2) x floor(Wo / 2) with it.
struct Conv2dShape {
  int B, Cin, Cout, H, W, Ho, Wo, Hy, Wy, pad, relu, pool;
};

// Pixels of the reduction one workgroup of the weight gradient covers at the least; the number
// of slabs follows from the shape alone, so two runs sum in the same order.
constexpr int kConvWgradMinSlab = 256;
constexpr int kConvWgradMaxSlabs = 256;

// y (and am, the 2-bit window position of the maximum, with pooling); bias may be null.
hipError_t conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* am, Conv2dShape s,
                       hipStream_t st);
// dx [B, Cin, H, W] from the gradient of y; am is null without pooling.
hipError_t conv3x3_dgrad(const float* dy, const float* y, const uint8_t* am, const float* w, float* dx,
                         Conv2dShape s, hipStream_t st);
// Slabs the weight gradient splits its reduction into; ws holds slabs * Cout * (Cin * 9 + 1) floats.
int conv3x3_wgrad_slabs(const Conv2dShape& s);
// dw [Cout, Cin, 3, 3] and db [Cout] (db may be null).
hipError_t conv3x3_wgrad(const float* dy, const float* y, const uint8_t* am, const float* x, float* ws, float* dw,
                         float* db, Conv2dShape s, hipStream_t st);

}  // namespace sl
