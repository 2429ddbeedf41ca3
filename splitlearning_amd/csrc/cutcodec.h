// Cut-layer codec (cutcodec.hip): int8 / int4 block quantisation of the tensor that crosses the
// cut, for splitlearning_amd.nn.CutCodec / cut_pack / cut_unpack.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sl {

// x [R, K] fp32, cut into ng = ceil(K / group) groups per row (the last may be short; a group
// never spans rows).  bits 8: payload int8 [R, K].  bits 4: payload uint8 [R, ceil(K / 2)], column
// 2j in the low nibble of byte j.  scales fp32 [R, ng].  group is one of 16, 32, 64, 128, 256.
struct CutShape {
  int R, K, group, ng, bits;
  int stochastic;              // 0: round to nearest even, 1: floor(x * inv + u(seed, row, column))
  uint32_t seed_lo, seed_hi;
};

hipError_t cut_pack(const float* x, void* payload, float* scales, CutShape s, hipStream_t st);
hipError_t cut_unpack(const void* payload, const float* scales, float* y, CutShape s, hipStream_t st);
// unpack(pack(x)) in one pass: x is read once and y written once, nothing else touches memory
hipError_t cut_roundtrip(const float* x, float* y, CutShape s, hipStream_t st);

}  // namespace sl
