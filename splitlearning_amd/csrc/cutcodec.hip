// Cut-layer codec for user models (splitlearning_amd.nn.CutCodec, cut_pack, cut_unpack): the
// activation that crosses the cut, and its gradient, as int8 or int4 with one fp32 scale per group
// of 16 .. 256 consecutive elements of a row.
//
// Reference ops: ops/torch_ops.py cut_pack / cut_unpack / cut_roundtrip are the definition, and the
// kernels match them bit for bit.  Per group, in fp32:
//
//   absmax = max |x|, scale = absmax / qmax, inv = absmax > 0 ? qmax / absmax : 0   (IEEE divisions)
//   nearest     q = clamp(rint(x * inv), -qmax, qmax)
//   stochastic  q = clamp(floor((x * inv) + u), -qmax, qmax), u = (hash32(seed, row, column) >> 8) * 2^-24,
//               the product and the sum rounded separately (no FMA)
//   dequantise  x^ = float(q) * scale
//
// All three kernels stream: every input byte is read once and every output byte written once, there
// is no LDS, no atomic and no workspace, and the only cross-lane traffic is the group maximum.
//
// Lane mapping.  A lane owns EPL consecutive columns of one group: 4 at 8 bits and 8 at 4 bits, so
// that its payload is one dword either way.  A group is group / EPL consecutive lanes (2 .. 64, a
// power of two) and a wave holds 64 * EPL / group whole groups; the group maximum is a DPP
// reduction over those lanes (sl_group_max), with ds_bpermute swaps only past a 16-lane row.  The
// groups of the whole tensor are numbered row by row, and a wave takes consecutive numbers, so its
// lanes are all at work at group = 16 and at group = 256, and with K < group as well (a wave then
// spans several rows); only the lanes past the end of a row's short last group idle.  The grid is a
// grid-stride loop over those wave-sized pieces, sized from the shape alone.
//
// Alignment.  A lane's columns start at a multiple of EPL, so its fp32 address is 16-byte aligned
// exactly when base + row * K is: the test is per lane, rows of an odd K take every phase, and a
// lane whose address is aligned and whose columns are all inside the row moves float4s; any other
// lane (a misaligned row, the partial lane at the end of a row) moves single floats, which the
// neighbouring lanes still coalesce.  The payload dword is stored whole under the same test on its
// own address, and byte by byte otherwise.  Every access is guarded by the row's length.
#include "cutcodec.h"

#include "common.h"

namespace sl {

namespace {

constexpr int kCutThreads = 256;
// 8 workgroups of 4 waves per CU on 256 CUs: every wave slot of the device once
constexpr int kCutMaxBlocks = 2048;

template <int BITS>
struct CutFmt {
  static constexpr int EPL = BITS == 8 ? 4 : 8;     // columns per lane = one payload dword
  static constexpr float QMAX = BITS == 8 ? 127.f : 7.f;
};

// What a lane owns in one step of the loop: n columns (0 when it idles) starting at `col` of group g
// of `row`.  first = the (row, group) number of the wave's lane 0.
struct CutLane {
  int64_t row;
  uint32_t g, col;
  int n;
  bool lead;      // the group's first lane (stores the scale)
};

template <int EPL>
__device__ __forceinline__ CutLane cut_lane(const CutShape& s, int64_t first, int lane) {
  const int lpg = s.group / EPL;                   // a power of two
  const int64_t row0 = first / s.ng;
  const uint32_t off = (uint32_t)(first - row0 * s.ng) + (uint32_t)(lane >> __builtin_ctz(lpg));   // < ng + 64
  CutLane l;
  l.row = row0 + off / (uint32_t)s.ng;
  l.g = off % (uint32_t)s.ng;
  const int sub = lane & (lpg - 1);
  l.col = l.g * (uint32_t)s.group + (uint32_t)(sub * EPL);      // < K + 256 < 2^32
  l.lead = sub == 0;
  l.n = 0;
  if (l.row < s.R && l.col < (uint32_t)s.K) l.n = (int)min((uint32_t)EPL, (uint32_t)s.K - l.col);
  return l;
}

__device__ __forceinline__ float cut_group_max(float m, int lpg) {
  switch (lpg) {
    case 2: return sl_group_max<2>(m);
    case 4: return sl_group_max<4>(m);
    case 8: return sl_group_max<8>(m);
    case 16: return sl_group_max<16>(m);
    case 32: return sl_group_max<32>(m);
    default: return sl_group_max<64>(m);
  }
}

// n <= EPL floats at p; the rest of v is 0
template <int EPL>
__device__ __forceinline__ void cut_ld(const float* p, int n, float (&v)[EPL]) {
  if (n == EPL && ((uintptr_t)p & 15) == 0) {
#pragma unroll
    for (int j = 0; j < EPL / 4; ++j) {
      const float4 t = reinterpret_cast<const float4*>(p)[j];
      v[4 * j] = t.x, v[4 * j + 1] = t.y, v[4 * j + 2] = t.z, v[4 * j + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = i < n ? p[i] : 0.f;
  }
}

template <int EPL>
__device__ __forceinline__ void cut_st(float* p, int n, const float (&v)[EPL]) {
  if (n == EPL && ((uintptr_t)p & 15) == 0) {
#pragma unroll
    for (int j = 0; j < EPL / 4; ++j)
      reinterpret_cast<float4*>(p)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < EPL; ++i)
      if (i < n) p[i] = v[i];
  }
}

// The group's scale from the lane's columns, and their integers q (0 past n).
template <int BITS, bool STOCH>
__device__ __forceinline__ float cut_quantise(const CutShape& s, const CutLane& l, const float (&v)[CutFmt<BITS>::EPL],
                                              int (&q)[CutFmt<BITS>::EPL]) {
  constexpr int EPL = CutFmt<BITS>::EPL;
  constexpr float Q = CutFmt<BITS>::QMAX;
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) m = fmaxf(m, fabsf(v[i]));
  m = cut_group_max(m, s.group / EPL);
  const float scale = m / Q;
  const float inv = m > 0.f ? Q / m : 0.f;
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    float t = __fmul_rn(v[i], inv);
    if (STOCH) {
      const uint32_t h = sl_hash32(s.seed_lo, s.seed_hi, (uint32_t)l.row, l.col + i);
      t = floorf(__fadd_rn(t, (float)(h >> 8) * 0x1p-24f));
    } else {
      t = rintf(t);
    }
    q[i] = i < l.n ? (int)fminf(fmaxf(t, -Q), Q) : 0;
  }
  return scale;
}

// the lane's payload dword: 4 bytes or 8 nibbles, two's complement, first column lowest
template <int BITS>
__device__ __forceinline__ uint32_t cut_word(const int (&q)[CutFmt<BITS>::EPL]) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < CutFmt<BITS>::EPL; ++i) w |= ((uint32_t)q[i] & (BITS == 8 ? 0xFFu : 0xFu)) << (BITS * i);
  return w;
}

template <int BITS>
__device__ __forceinline__ int cut_field(uint32_t w, int i) {
  return (int)(w << (32 - BITS * (i + 1))) >> (32 - BITS);      // sign-extending shift
}

// bytes of a row's payload and of a lane's n columns
template <int BITS>
__device__ __forceinline__ int64_t cut_row_bytes(int K) {
  return BITS == 8 ? (int64_t)K : ((int64_t)K + 1) / 2;
}
template <int BITS>
__device__ __forceinline__ int cut_lane_bytes(int n) {
  return BITS == 8 ? n : (n + 1) / 2;
}

template <int BITS>
__device__ __forceinline__ uint8_t* cut_payload_at(const void* payload, const CutShape& s, const CutLane& l) {
  return (uint8_t*)payload + l.row * cut_row_bytes<BITS>(s.K) + (BITS == 8 ? l.col : l.col / 2);
}

#define CUT_LOOP(EPL_)                                                                             \
  const int lane = threadIdx.x & 63;                                                               \
  const int gpw = 64 * (EPL_) / s.group;                                                           \
  const int64_t total = (int64_t)s.R * s.ng;                                                       \
  const int64_t step = (int64_t)gridDim.x * (kCutThreads / 64) * gpw;                              \
  for (int64_t first = ((int64_t)blockIdx.x * (kCutThreads / 64) + (threadIdx.x >> 6)) * gpw; first < total; first += step)

template <int BITS, bool STOCH>
__global__ void __launch_bounds__(kCutThreads)
cut_pack_kernel(const float* __restrict__ x, void* __restrict__ payload, float* __restrict__ scales, CutShape s) {
  constexpr int EPL = CutFmt<BITS>::EPL;
  CUT_LOOP(EPL) {
    const CutLane l = cut_lane<EPL>(s, first, lane);
    float v[EPL];
    int q[EPL];
    cut_ld<EPL>(x + l.row * s.K + l.col, l.n, v);
    const float scale = cut_quantise<BITS, STOCH>(s, l, v, q);      // every lane takes part in the maximum
    if (!l.n) continue;
    if (l.lead) scales[l.row * s.ng + l.g] = scale;
    const uint32_t w = cut_word<BITS>(q);
    uint8_t* p = cut_payload_at<BITS>(payload, s, l);
    if (l.n == EPL && ((uintptr_t)p & 3) == 0) {
      *reinterpret_cast<uint32_t*>(p) = w;
    } else {
      const int nb = cut_lane_bytes<BITS>(l.n);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nb) p[i] = (uint8_t)(w >> (8 * i));
    }
  }
}

template <int BITS>
__global__ void __launch_bounds__(kCutThreads)
cut_unpack_kernel(const void* __restrict__ payload, const float* __restrict__ scales, float* __restrict__ y,
                  CutShape s) {
  constexpr int EPL = CutFmt<BITS>::EPL;
  CUT_LOOP(EPL) {
    const CutLane l = cut_lane<EPL>(s, first, lane);
    if (!l.n) continue;
    const float scale = scales[l.row * s.ng + l.g];
    const uint8_t* p = cut_payload_at<BITS>(payload, s, l);
    uint32_t w = 0;
    if (l.n == EPL && ((uintptr_t)p & 3) == 0) {
      w = *reinterpret_cast<const uint32_t*>(p);
    } else {
      const int nb = cut_lane_bytes<BITS>(l.n);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nb) w |= (uint32_t)p[i] << (8 * i);
    }
    float v[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = (float)cut_field<BITS>(w, i) * scale;
    cut_st<EPL>(y + l.row * s.K + l.col, l.n, v);
  }
}

template <int BITS, bool STOCH>
__global__ void __launch_bounds__(kCutThreads)
cut_roundtrip_kernel(const float* __restrict__ x, float* __restrict__ y, CutShape s) {
  constexpr int EPL = CutFmt<BITS>::EPL;
  CUT_LOOP(EPL) {
    const CutLane l = cut_lane<EPL>(s, first, lane);
    float v[EPL];
    int q[EPL];
    cut_ld<EPL>(x + l.row * s.K + l.col, l.n, v);
    const float scale = cut_quantise<BITS, STOCH>(s, l, v, q);
    if (!l.n) continue;
#pragma unroll
    for (int i = 0; i < EPL; ++i) v[i] = (float)q[i] * scale;
    cut_st<EPL>(y + l.row * s.K + l.col, l.n, v);
  }
}

#undef CUT_LOOP

dim3 cut_grid(const CutShape& s) {
  const int gpw = 64 * (s.bits == 8 ? 4 : 8) / s.group;
  const int64_t waves = ((int64_t)s.R * s.ng + gpw - 1) / gpw;
  const int64_t blocks = (waves + kCutThreads / 64 - 1) / (kCutThreads / 64);
  return dim3((unsigned)(blocks < kCutMaxBlocks ? blocks : kCutMaxBlocks));
}

}  // namespace

hipError_t cut_pack(const float* x, void* payload, float* scales, CutShape s, hipStream_t st) {
  const dim3 grid = cut_grid(s), block(kCutThreads);
  if (s.bits == 8) {
    if (s.stochastic) hipLaunchKernelGGL((cut_pack_kernel<8, true>), grid, block, 0, st, x, payload, scales, s);
    else hipLaunchKernelGGL((cut_pack_kernel<8, false>), grid, block, 0, st, x, payload, scales, s);
  } else {
    if (s.stochastic) hipLaunchKernelGGL((cut_pack_kernel<4, true>), grid, block, 0, st, x, payload, scales, s);
    else hipLaunchKernelGGL((cut_pack_kernel<4, false>), grid, block, 0, st, x, payload, scales, s);
  }
  return hipGetLastError();
}

hipError_t cut_unpack(const void* payload, const float* scales, float* y, CutShape s, hipStream_t st) {
  const dim3 grid = cut_grid(s), block(kCutThreads);
  if (s.bits == 8) hipLaunchKernelGGL(cut_unpack_kernel<8>, grid, block, 0, st, payload, scales, y, s);
  else hipLaunchKernelGGL(cut_unpack_kernel<4>, grid, block, 0, st, payload, scales, y, s);
  return hipGetLastError();
}

hipError_t cut_roundtrip(const float* x, float* y, CutShape s, hipStream_t st) {
  const dim3 grid = cut_grid(s), block(kCutThreads);
  if (s.bits == 8) {
    if (s.stochastic) hipLaunchKernelGGL((cut_roundtrip_kernel<8, true>), grid, block, 0, st, x, y, s);
    else hipLaunchKernelGGL((cut_roundtrip_kernel<8, false>), grid, block, 0, st, x, y, s);
  } else {
    if (s.stochastic) hipLaunchKernelGGL((cut_roundtrip_kernel<4, true>), grid, block, 0, st, x, y, s);
    else hipLaunchKernelGGL((cut_roundtrip_kernel<4, false>), grid, block, 0, st, x, y, s);
  }
  return hipGetLastError();
}

}  // namespace sl
