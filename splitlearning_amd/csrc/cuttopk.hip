// Cut sparsifier for user models (splitlearning_amd.nn.CutTopK, cut_sparsify, cut_densify,
// cut_sparse_grad): of each sample's activation only the k entries of largest magnitude cross the
// cut, as values + column indices, and the gradient comes back on the same support.
//
// Reference ops: ops/torch_ops.py cut_topk / cut_scatter / cut_gather are the definition, and the
// kernels match them bit for bit.  x [R, K] fp32; the key of an element is the bit pattern of |x|
// (so -0.0 and 0.0 are equal, and keys order as magnitudes do); a row's support is the k columns
// with the largest keys, the lowest columns winning among equal keys at the threshold; indices
// come out ascending.
//
// One 256-thread workgroup owns a row (grid = R, a row is never split, row offsets are 64-bit).
//
// Selection is a radix select on the key, most significant byte first.  Each of the four passes
// counts, in a 256-bin LDS histogram (integer LDS atomics: the counts do not depend on the order
// of arrival), the byte of every key that matches the prefix found so far; wave 0 then walks the
// bins from the top to the one that holds the k-th largest key and keeps how many are still wanted
// inside it.  After pass four the threshold key T and need = k - #{key > T} are known.  A last pass
// in column order selects key > T, and key == T while fewer than `need` equal keys lie in lower
// columns.  The output slot of a selected element is the number of selected elements in lower
// columns: #{key > T before} + min(#{key == T before}, need), an ordered workgroup-wide prefix of
// the two counters (lane scan, wave totals through LDS, a running base from chunk to chunk).  So
// indices are ascending with no sort, and with DENSE the dense row is written in the same pass.
//
// Where the row lives.  A row of up to kCutTopkLdsFloats floats is copied to LDS by the first pass
// and the other four read it there; a longer row is re-read from global memory (L2).
//
// Alignment.  A row is walked in quads that start at 16-byte boundaries of its own address: with
// phase = floats of the row's start past such a boundary, quad q holds columns 4 q - phase ..
// 4 q - phase + 3.  A quad that lies inside the row is therefore one aligned float4 load whatever
// K and the base pointer are; the first and last quads of a row may be partial and move single
// floats.  Stores to y test their own address, since y need not share x's phase.
//
// All stores are plain vector stores; there is no floating-point atomic and no workspace.
#include "cuttopk.h"

#include "common.h"

namespace sl {

namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / SL_WAVE;
// quads a thread loads before it works on the first: a workgroup is 4 waves on its CU, and with one
// float4 per lane in flight a long row is bound by the latency of its loads
constexpr int kTopkUnroll = 4;
// dynamic LDS, in dwords: hist[256], ctl[16], then the row (none for a row that stays in global
// memory).  ctl[0] = the pass's threshold byte, ctl[1] = keys still wanted inside it,
// ctl[8 + 4 * parity + wave] = a wave's packed totals in the ordered pass.
constexpr int kTopkHist = 256;
constexpr int kTopkCtl = 16;

__device__ __forceinline__ uint32_t topk_key(float v) { return __builtin_bit_cast(uint32_t, v) & 0x7FFFFFFFu; }

// Quad at column c0 (= 4 q - phase as uint32, wrapping below 0 for the first quad of a shifted
// row): one float4 when it lies inside the row, else guarded floats; 0 outside the row.
__device__ __forceinline__ void topk_ld(const float* __restrict__ xr, uint32_t c0, uint32_t K, float (&v)[4]) {
  if (c0 < K && K - c0 >= 4u) {
    const float4 t = *reinterpret_cast<const float4*>(xr + c0);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t c = c0 + e;
      v[e] = c < K ? xr[c] : 0.f;
    }
  }
}

// Quad q of the row from global memory or from its LDS copy; 0 past the row's last quad.
__device__ __forceinline__ void topk_fetch(const float* __restrict__ xr, const float* row, uint32_t q, uint32_t nq,
                                           uint32_t c0, uint32_t K, bool from_global, float (&v)[4]) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (q >= nq) return;
  if (from_global) {
    topk_ld(xr, c0, K, v);
  } else {
    const float4 t = reinterpret_cast<const float4*>(row)[q];
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
}

__device__ __forceinline__ void topk_st(float* __restrict__ yr, uint32_t c0, uint32_t K, const float (&v)[4]) {
  if (c0 < K && K - c0 >= 4u && ((uintptr_t)(yr + c0) & 15) == 0) {
    *reinterpret_cast<float4*>(yr + c0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t c = c0 + e;
      if (c < K) yr[c] = v[e];
    }
  }
}

// ++hist[bin] for every active lane.  Keys of one row share their leading bytes far more often
// than not, and 64 LDS atomics on one address serialise: the two most common bins of the wave are
// added once each by a leader lane, the rest lane by lane.  Call with the whole wave.
__device__ __forceinline__ void topk_count(uint32_t* hist, uint32_t bin, bool active, int lane) {
  uint64_t todo = __ballot(active);
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (todo == 0) return;
    const int lead = __ffsll((unsigned long long)todo) - 1;
    const uint32_t lb = (uint32_t)__builtin_amdgcn_readlane((int)bin, lead);
    const uint64_t same = __ballot(active && bin == lb);
    if (lane == lead) atomicAdd(&hist[lb], (uint32_t)__popcll((unsigned long long)same));
    active = active && bin != lb;
    todo &= ~same;
  }
  if (active) atomicAdd(&hist[bin], 1u);
}

// inclusive sum over the lanes 0 .. lane of the wave
__device__ __forceinline__ uint32_t topk_wave_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < SL_WAVE; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, SL_WAVE);
    if (lane >= d) v += t;
  }
  return v;
}

template <bool DENSE>
__global__ void __launch_bounds__(kTopkThreads)
cut_topk_kernel(const float* __restrict__ x, float* __restrict__ values, int32_t* __restrict__ indices,
                float* __restrict__ y, TopkShape s, int in_lds) {
  extern __shared__ __attribute__((aligned(16))) uint32_t topk_smem[];
  uint32_t* hist = topk_smem;
  uint32_t* ctl = topk_smem + kTopkHist;
  float* row = reinterpret_cast<float*>(topk_smem + kTopkHist + kTopkCtl);      // 16-byte aligned

  const int tid = threadIdx.x, lane = tid & (SL_WAVE - 1), wave = tid / SL_WAVE;
  const int64_t r = blockIdx.x;
  const float* xr = x + r * s.K;
  const uint32_t K = (uint32_t)s.K;
  const uint32_t phase = (uint32_t)((uintptr_t)xr >> 2) & 3u;
  const uint32_t nq = (K + phase + 3u) >> 2;

  hist[tid] = 0;
  __syncthreads();

  // ---- four counting passes: prefix = the bytes of T found so far, rem = keys wanted under it
  uint32_t prefix = 0, rem = (uint32_t)s.k;
  for (int p = 0; p < 4; ++p) {
    const int shift = 24 - 8 * p;
    const uint32_t himask = ~(0xFFFFFFFFu >> (8 * p));      // the bytes above this pass's
    for (uint32_t q0 = 0; q0 < nq; q0 += kTopkThreads * kTopkUnroll) {
      float v[kTopkUnroll][4];
#pragma unroll
      for (int u = 0; u < kTopkUnroll; ++u) {       // every load of the step before the first count
        const uint32_t q = q0 + u * kTopkThreads + tid;
        topk_fetch(xr, row, q, nq, 4u * q - phase, K, p == 0 || !in_lds, v[u]);
        if (p == 0 && in_lds && q < nq)
          reinterpret_cast<float4*>(row)[q] = make_float4(v[u][0], v[u][1], v[u][2], v[u][3]);
      }
#pragma unroll
      for (int u = 0; u < kTopkUnroll; ++u) {
        const uint32_t c0 = 4u * (q0 + u * kTopkThreads + tid) - phase;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t key = topk_key(v[u][e]);
          topk_count(hist, (key >> shift) & 255u, c0 + e < K && (key & himask) == prefix, lane);
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns bins 255 - 4 l .. 252 - 4 l, so lanes ascend as bins descend
      const int b0 = 255 - 4 * lane;
      uint32_t h[4], c = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = hist[b0 - j];
        hist[b0 - j] = 0;
        c += h[j];
      }
      const uint32_t incl = topk_wave_scan(c, lane);
      uint32_t above = incl - c;
      if (above < rem && rem <= incl) {       // exactly one lane: at least rem keys match the prefix
        int byte = b0 - 3;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!found) {
            if (rem <= above + h[j]) byte = b0 - j, found = true;
            else above += h[j];
          }
        }
        ctl[0] = (uint32_t)byte;
        ctl[1] = rem - above;
      }
    }
    __syncthreads();
    prefix |= ctl[0] << shift;
    rem = ctl[1];
  }

  // ---- the ordered pass
  const uint32_t T = prefix, need = rem, k = (uint32_t)s.k;
  float* vr = values + r * s.k;
  int32_t* ir = indices + r * s.k;
  float* yr = DENSE ? y + r * s.K : nullptr;
  uint32_t base_g = 0, base_e = 0;
  static_assert(kTopkUnroll % 2 == 0, "the wave totals alternate between two sets, chunk by chunk");
  for (uint32_t q0 = 0; q0 < nq; q0 += kTopkThreads * kTopkUnroll) {
    float vs[kTopkUnroll][4];
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {
      const uint32_t q = q0 + u * kTopkThreads + tid;
      topk_fetch(xr, row, q, nq, 4u * q - phase, K, !in_lds, vs[u]);
    }
#pragma unroll
    for (int u = 0; u < kTopkUnroll; ++u) {           // chunk by chunk, in column order
      if (q0 + u * kTopkThreads >= nq) break;         // the same for the whole workgroup
      const uint32_t q = q0 + u * kTopkThreads + tid, c0 = 4u * q - phase;
      const float (&v)[4] = vs[u];
      const int par = u & 1;
      bool isg[4], ise[4];
      uint32_t mine = 0;                        // #{key > T} << 16 | #{key == T}: at most 1024 each per chunk
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t key = topk_key(v[e]);
        const bool ok = c0 + e < K;
        isg[e] = ok && key > T;
        ise[e] = ok && key == T;
        mine += ((uint32_t)isg[e] << 16) + (uint32_t)ise[e];
      }
      const uint32_t incl = topk_wave_scan(mine, lane);
      uint32_t* tot = ctl + 8 + kTopkWaves * par;       // two sets: one barrier per chunk is enough
      if (lane == SL_WAVE - 1) tot[wave] = incl;
      __syncthreads();
      uint32_t before = incl - mine, all = 0;
#pragma unroll
      for (int w = 0; w < kTopkWaves; ++w) {
        const uint32_t t = tot[w];
        all += t;
        if (w < wave) before += t;
      }
      uint32_t g = base_g + (before >> 16), eq = base_e + (before & 0xFFFFu);
      base_g += all >> 16;
      base_e += all & 0xFFFFu;
      float out[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool sel = isg[e] || (ise[e] && eq < need);
        if (sel) {
          const uint32_t slot = g + min(eq, need);
          if (slot < k) {
            vr[slot] = v[e];
            ir[slot] = (int32_t)(c0 + e);
          }
        }
        g += isg[e];
        eq += ise[e];
        out[e] = sel ? v[e] : 0.f;
      }
      if (DENSE && q < nq) topk_st(yr, c0, K, out);
    }
  }
}

// y row = 0, then y[indices[j]] = values[j] (or d[indices[j]] with GATHER); the fill and the
// scatter of a row belong to this workgroup and the barrier orders them.
template <bool GATHER>
__global__ void __launch_bounds__(kTopkThreads)
cut_scatter_kernel(const float* __restrict__ src, const int32_t* __restrict__ indices, float* __restrict__ y,
                   TopkShape s) {
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  float* yr = y + r * s.K;
  const uint32_t K = (uint32_t)s.K;
  const uint32_t phase = (uint32_t)((uintptr_t)yr >> 2) & 3u;
  const uint32_t nq = (K + phase + 3u) >> 2;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t q = tid; q < nq; q += kTopkThreads) topk_st(yr, 4u * q - phase, K, zero);
  __threadfence_block();
  __syncthreads();
  const int32_t* ir = indices + r * s.k;
  const float* sr = GATHER ? src + r * s.K : src + r * s.k;
  for (uint32_t j = tid; j < (uint32_t)s.k; j += kTopkThreads) {
    const uint32_t c = (uint32_t)ir[j];
    if (c < K) yr[c] = GATHER ? sr[c] : sr[j];      // an index outside the row is never stored through
  }
}

__global__ void __launch_bounds__(kTopkThreads)
cut_gather_kernel(const float* __restrict__ d, const int32_t* __restrict__ indices, float* __restrict__ values,
                  TopkShape s) {
  const int64_t r = blockIdx.x;
  const float* dr = d + r * s.K;
  const int32_t* ir = indices + r * s.k;
  float* vr = values + r * s.k;
  for (uint32_t j = threadIdx.x; j < (uint32_t)s.k; j += kTopkThreads) {
    const uint32_t c = (uint32_t)ir[j];
    vr[j] = c < (uint32_t)s.K ? dr[c] : 0.f;
  }
}

}  // namespace

hipError_t cut_topk(const float* x, float* values, int32_t* indices, float* y, TopkShape s, hipStream_t st) {
  if (s.R == 0) return hipSuccess;
  const int in_lds = s.K <= kCutTopkLdsFloats;
  // the row's quads: up to 3 floats of phase in front and 3 of padding behind
  const size_t lds = sizeof(uint32_t) * (kTopkHist + kTopkCtl) + (in_lds ? sizeof(float) * 4 * ((s.K + 6) / 4) : 0);
  const dim3 grid((unsigned)s.R), block(kTopkThreads);
  if (y) hipLaunchKernelGGL(cut_topk_kernel<true>, grid, block, lds, st, x, values, indices, y, s, in_lds);
  else hipLaunchKernelGGL(cut_topk_kernel<false>, grid, block, lds, st, x, values, indices, y, s, in_lds);
  return hipGetLastError();
}

hipError_t cut_scatter(const float* values, const int32_t* indices, float* y, TopkShape s, hipStream_t st) {
  if (s.R == 0) return hipSuccess;
  hipLaunchKernelGGL(cut_scatter_kernel<false>, dim3((unsigned)s.R), dim3(kTopkThreads), 0, st, values, indices, y, s);
  return hipGetLastError();
}

hipError_t cut_mask(const float* d, const int32_t* indices, float* dx, TopkShape s, hipStream_t st) {
  if (s.R == 0) return hipSuccess;
  hipLaunchKernelGGL(cut_scatter_kernel<true>, dim3((unsigned)s.R), dim3(kTopkThreads), 0, st, d, indices, dx, s);
  return hipGetLastError();
}

hipError_t cut_gather(const float* d, const int32_t* indices, float* values, TopkShape s, hipStream_t st) {
  if (s.R == 0) return hipSuccess;
  hipLaunchKernelGGL(cut_gather_kernel, dim3((unsigned)s.R), dim3(kTopkThreads), 0, st, d, indices, values, s);
  return hipGetLastError();
}

}  // namespace sl
