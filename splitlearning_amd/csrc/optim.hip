// Multi-tensor optimizer step and deterministic global gradient norm for user-written
// models (splitlearning_amd/optim.py: FusedSGD / FusedAdam).
//
// The engines fuse the optimizer into the weight-gradient stream; an autograd user has the
// gradients materialised, so what is left to fuse is the launch count: one pass over
// (parameter, gradient, state) of the whole model in one launch.  The tensor list is cut
// into chunks of kMultiOptChunk elements, one workgroup per chunk; the workgroup finds its
// (tensor, offset) in a chunk-prefix table that travels by value in the kernel arguments
// (gradient pointers change with every zero_grad(set_to_none=True), so there is nothing to
// copy to the device and nothing that can go stale).  Pure streaming: 16-byte loads and
// stores, no LDS in the step kernel, 8 loads per thread in flight for Adam.
#include "optim.h"

namespace sl {
namespace {

constexpr int kThreads = 256;
constexpr int kVecs = kMultiOptChunk / (4 * kThreads);  // f32x4 per thread and array
static_assert(kVecs * 4 * kThreads == kMultiOptChunk, "chunk = whole f32x4 rounds of the workgroup");
static_assert(sizeof(MultiOptTable) + sizeof(SlOpt) + sizeof(void*) <= 3584, "kernel arguments stay well under 4 KB");

// The tensor holding chunk c: the last entry whose first chunk is <= c.  c is the workgroup
// index, so the search is uniform and runs on scalar loads of the kernel arguments.
__device__ __forceinline__ int find_tensor(const MultiOptTable& tab, int c) {
  int lo = 0, hi = tab.k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.t[mid].chunk0 <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// The step touches every byte once, so its 16-byte accesses carry the non-temporal hint:
// measured against plain accesses it is 7 % faster for Adam at model2_sisa's 32 M parameters
// and 12 - 14 % with clipping on (presumably the gradients the norm pass just read stay
// cached), and within the spread at the U-shape model2's 5.5 M (docs/PERF.md, "Fused
// optimizers").
__device__ __forceinline__ f32x4 ld4(const float* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
}
__device__ __forceinline__ void st4(float* p, f32x4 v) {
  __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
}

template <bool ADAM>
__global__ __launch_bounds__(kThreads) void multi_opt_kernel(const MultiOptTable tab, const SlOpt o,
                                                             const float* __restrict__ gscale) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const MultiOptTensor T = tab.t[find_tensor(tab, c)];
  const int64_t base = (int64_t)(c - T.chunk0) * kMultiOptChunk;
  const int64_t left = T.n - base;
  const int n = left < kMultiOptChunk ? (int)left : kMultiOptChunk;
  float* __restrict__ p = T.p + base;
  const float* __restrict__ g = T.g + base;
  float* __restrict__ s0 = T.s0 ? T.s0 + base : nullptr;
  float* __restrict__ s1 = ADAM ? T.s1 + base : nullptr;
  // clipping: a separately rounded multiply, so the step equals one on a pre-scaled gradient
  const bool scaled = gscale != nullptr;
  const float gs = scaled ? *gscale : 1.f;

  // f32x4 body; the whole tensor goes the scalar way when one of its pointers is not
  // 16-byte aligned (chunk offsets are multiples of 16 bytes)
  const int nvec = aligned16(T.p, T.g, T.s0, ADAM ? T.s1 : nullptr) ? n >> 2 : 0;
  f32x4 pv[kVecs], gv[kVecs], av[kVecs], bv[kVecs];
#pragma unroll
  for (int u = 0; u < kVecs; ++u) {
    const int i = tid + u * kThreads;
    if (i < nvec) {
      pv[u] = ld4(p + 4 * i);
      gv[u] = ld4(g + 4 * i);
      av[u] = s0 ? ld4(s0 + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
      if (ADAM) bv[u] = ld4(s1 + 4 * i);
    }
  }
#pragma unroll
  for (int u = 0; u < kVecs; ++u) {
    const int i = tid + u * kThreads;
    if (i < nvec) {
      if (scaled) {
#pragma unroll
        for (int j = 0; j < 4; ++j) gv[u][j] = __fmul_rn(gv[u][j], gs);
      }
      sl_opt_update4<ADAM>(o, pv[u], gv[u], av[u], bv[u]);
      st4(p + 4 * i, pv[u]);
      if (s0) st4(s0 + 4 * i, av[u]);
      if (ADAM) st4(s1 + 4 * i, bv[u]);
    }
  }
  // the last n % 4 elements of a tensor, or all of an unaligned one
  for (int i = nvec * 4 + tid; i < n; i += kThreads) {
    float pp = p[i], gg = g[i], a0 = s0 ? s0[i] : 0.f, a1 = ADAM ? s1[i] : 0.f;
    if (scaled) gg = __fmul_rn(gg, gs);
    sl_opt_update(o, pp, gg, a0, a1);
    p[i] = pp;
    if (s0) s0[i] = a0;
    if (ADAM) s1[i] = a1;
  }
}

// Workgroup total of `acc`, to thread 0: DPP wave sums, then the waves in wave order.
__device__ __forceinline__ float block_sum_fixed(float acc) {
  __shared__ float wsum[kThreads / SL_WAVE];
  acc = sl_wave_sum(acc);
  if ((threadIdx.x & (SL_WAVE - 1)) == 0) wsum[threadIdx.x / SL_WAVE] = acc;
  __syncthreads();
  float s = wsum[0];
#pragma unroll
  for (int w = 1; w < kThreads / SL_WAVE; ++w) s += wsum[w];
  return s;
}

// Stage 1 of the gradient norm: chunk c's sum of squares -> slots[c].  Every step has a fixed
// order (per-lane accumulators, DPP wave sum, waves in order) and there are no atomics, so
// the same gradients give the same bits.
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(const MultiOptTable tab, float* __restrict__ slots) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const MultiOptTensor T = tab.t[find_tensor(tab, c)];
  const int64_t base = (int64_t)(c - T.chunk0) * kMultiOptChunk;
  const int64_t left = T.n - base;
  const int n = left < kMultiOptChunk ? (int)left : kMultiOptChunk;
  const float* __restrict__ g = T.g + base;
  const int nvec = aligned16(T.g, nullptr, nullptr, nullptr) ? n >> 2 : 0;
  f32x4 gv[kVecs];
#pragma unroll
  for (int u = 0; u < kVecs; ++u) {
    const int i = tid + u * kThreads;
    gv[u] = i < nvec ? *reinterpret_cast<const f32x4*>(g + 4 * i) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < kVecs; ++u)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(gv[u][j], gv[u][j], acc);
  for (int i = nvec * 4 + tid; i < n; i += kThreads) acc = fmaf(g[i], g[i], acc);
  const float s = block_sum_fixed(acc);
  if (tid == 0) slots[c] = s;
}

// Stage 2, one workgroup: thread i adds slots i, i + 256, ... in slot order, then the same
// fixed-order workgroup sum; {sumsq, norm, coef} with torch.nn.utils.clip_grad_norm_'s rule.
__global__ __launch_bounds__(kThreads) void grad_norm_finish_kernel(const float* __restrict__ slots, int64_t nslots,
                                                                    float max_norm, float* __restrict__ out3) {
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < nslots; i += kThreads) acc += slots[i];
  const float sumsq = block_sum_fixed(acc);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(sumsq);
    const float coef = max_norm / (norm + 1e-6f);
    out3[0] = sumsq;
    out3[1] = norm;
    out3[2] = coef > 1.f ? 1.f : coef;  // a NaN norm stays NaN, as torch's clamp(max=1) keeps it
  }
}

}  // namespace

hipError_t multi_opt(const MultiOptTable& tab, SlOpt o, const float* gscale, hipStream_t st) {
  if (tab.chunks <= 0) return hipSuccess;
  if (o.kind != 1 && o.kind != 2) return hipErrorInvalidValue;
  if (o.kind == 2) multi_opt_kernel<true><<<tab.chunks, kThreads, 0, st>>>(tab, o, gscale);
  else multi_opt_kernel<false><<<tab.chunks, kThreads, 0, st>>>(tab, o, gscale);
  return hipGetLastError();
}

hipError_t grad_sumsq(const MultiOptTable& tab, float* slots, hipStream_t st) {
  if (tab.chunks <= 0) return hipSuccess;
  grad_sumsq_kernel<<<tab.chunks, kThreads, 0, st>>>(tab, slots);
  return hipGetLastError();
}

hipError_t grad_norm_finish(const float* slots, int64_t nslots, float max_norm, float* out3, hipStream_t st) {
  grad_norm_finish_kernel<<<1, kThreads, 0, st>>>(slots, nslots, max_norm, out3);
  return hipGetLastError();
}

}  // namespace sl
