// GroupNorm [+ ReLU] [+ MaxPool2d(2, 2)] for user models (splitlearning_amd.nn.FusedGroupNorm).
//
// Reference ops: nn.GroupNorm(G, C, eps, affine), F.relu, F.max_pool2d(2, 2) and their autograd
// (ops/torch_ops.py group_norm_fwd / group_norm_bwd are the ground truth).
//
// A (sample, group) pair is one contiguous span of n = (C / G) * L floats of the NCHW input, and
// one 256-thread workgroup owns it in the forward and in the backward.  All three kernels are
// memory-bound: the aim is one HBM read of every input and one write of every output.
//
//   forward   sum -> mean, sum of squared deviations from that mean -> rstd (two passes in fp32,
//             never E[x^2] - mean^2), then z = (x - mean) * rstd * w[c] + b[c], ReLU, and with
//             pooling the maximum of each 2x2 window and its 2-bit position (2 * dy + dx, the
//             first in row-major order on a tie: the meaning of conv2d.hip's am).  Only y, mean,
//             rstd and am are stored.  The row / column torch's floor rule leaves out of every
//             window is in the statistics and produces no output.
//   backward  dz = dy routed back through the pool and the ReLU; the ReLU decision is recomputed
//             from x, mean, rstd, w, b through gn_pre, the function the forward calls, so it is
//             bitwise the forward's.  Pass A: one wave per channel of the group forms sum dz and
//             sum dz * xh (xh = (x - mean) * rstd), stores the pair to the [B, C, 2] workspace
//             when there is an affine, and adds it, weighted, to its partial of the two group
//             means.  Pass B: dx = rstd * (w dz - mean(w dz) - xh mean(w dz xh)), skipped when no
//             input gradient is wanted.
//   param     dw[c], db[c] = the workspace summed over b in index order.
//
// No atomics: every sum has a fixed order (lane tree, waves 0..3, samples 0..B-1), so two runs
// agree bitwise.
//
// Where the span lives between the passes.  The statistics need the whole span before the first
// output can be formed, so the span is read, reduced, and used again.  A span of up to
// kGroupNormLdsFloats (16000 floats, 62.5 KB) is copied to LDS by the first pass and every later
// pass reads LDS: x comes from HBM once.  The bound is the 64 KB of LDS a launch may ask for
// without opting in to more; at that size two workgroups still share a CU's 160 KB, and the
// workgroup asks only for its own span, so the small spans of typical layers (2704 floats at
// model1_sisa's conv output with 8 groups) leave room for 8 workgroups per CU.  Registers are
// not used for this: 256 threads x the 512-register budget of __launch_bounds__(256) would hold
// more, but only through a fully unrolled, span-length-specialised loop.  A longer span is
// re-read from global memory; its 2nd and 3rd reads hit the 4 MB L2 of the XCD for spans below
// that size (the 512 KB span of one 32-channel 64 x 64 group does).
//
// Loads are 16 bytes wide wherever an address is 16-byte aligned: a span is swept as a scalar
// head up to the first aligned address, float4s, and a scalar tail (n = 50 starts every second
// group 8 bytes off).  The LDS image is shifted by the same phase, so its float4 accesses are
// aligned where the global ones are.
#include "groupnorm.h"

#include "common.h"

namespace sl {

namespace {

constexpr int kGnThreads = 256;

// The pre-activation.  The backward recomputes the forward's value with this same function.
__device__ __forceinline__ float gn_pre(float x, float mean, float rstd, float w, float b) {
  return fmaf((x - mean) * rstd, w, b);
}

// Elements 0 .. n - 1 behind p, strided over nt workers: f1(i) for the scalar head and tail,
// f4(i) where p + i is 16-byte aligned and i + 3 < n.
template <class F1, class F4>
__device__ __forceinline__ void gn_sweep(const void* p, int n, int t, int nt, F1 f1, F4 f4) {
  const int mis = (int)(((uintptr_t)p >> 2) & 3);
  const int head = min(n, (4 - mis) & 3);
  const int nv = (n - head) >> 2;
  for (int i = t; i < head; i += nt) f1(i);
#pragma unroll 4
  for (int k = t; k < nv; k += nt) f4(head + 4 * k);
  for (int i = head + 4 * nv + t; i < n; i += nt) f1(i);
}

// four floats at p: one 16-byte load when p is aligned
__device__ __forceinline__ float4 gn_ld4(const float* p) {
  if (((uintptr_t)p & 15) == 0) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void gn_st4(float* p, float4 v) {
  if (((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<float4*>(p) = v;
  } else {
    p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
  }
}

// Sum over the workgroup in a fixed order, returned to every thread.  One red[4] per call site.
__device__ __forceinline__ float gn_block_sum(float v, float* red) {
  v = sl_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Copy the span to LDS (same 16-byte phase as the global span) and return the sum.
template <bool LDS>
__device__ __forceinline__ float gn_stage(const float* xs, float* sp, int n) {
  float sum = 0.f;
  gn_sweep(
      xs, n, threadIdx.x, kGnThreads,
      [&](int i) {
        const float v = xs[i];
        if (LDS) sp[i] = v;
        sum += v;
      },
      [&](int i) {
        const float4 v = *reinterpret_cast<const float4*>(xs + i);
        if (LDS) *reinterpret_cast<float4*>(sp + i) = v;
        sum += (v.x + v.y) + (v.z + v.w);
      });
  return sum;
}

// ------------------------------------------------------------------ forward
template <bool LDS>
__global__ void __launch_bounds__(kGnThreads)
group_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                      float* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                      uint8_t* __restrict__ am, GroupNormShape s) {
  extern __shared__ __attribute__((aligned(16))) float gn_lds[];
  __shared__ float red[2][4];
  const int tid = threadIdx.x;
  const int sg = blockIdx.x, g = sg % s.G;
  const int cpg = s.C / s.G, n = cpg * s.L, c0 = g * cpg;
  const float* xs = x + (int64_t)sg * n;
  float* sp = gn_lds + (((uintptr_t)xs >> 2) & 3);     // sp[i] = xs[i], at most n + 3 floats of LDS
  const float* src = LDS ? sp : xs;

  const float mean = gn_block_sum(gn_stage<LDS>(xs, sp, n), red[0]) / (float)n;   // its barrier publishes sp
  float ssd = 0.f;
  gn_sweep(
      xs, n, tid, kGnThreads,
      [&](int i) {
        const float d = src[i] - mean;
        ssd += d * d;
      },
      [&](int i) {
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
        ssd += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      });
  const float rstd = 1.f / sqrtf(gn_block_sum(ssd, red[1]) / (float)n + s.eps);
  if (tid == 0) {
    mean_out[sg] = mean;
    rstd_out[sg] = rstd;
  }

  auto act = [&](float v, int c) {
    const float z = gn_pre(v, mean, rstd, w ? w[c0 + c] : 1.f, b ? b[c0 + c] : 0.f);
    return s.relu ? fmaxf(z, 0.f) : z;
  };
  if (!s.pool) {
    float* ys = y + (int64_t)sg * n;
    gn_sweep(
        ys, n, tid, kGnThreads, [&](int i) { ys[i] = act(src[i], i / s.L); },
        [&](int i) {
          const float4 v = gn_ld4(src + i);
          const float in[4] = {v.x, v.y, v.z, v.w};
          float out[4];
          int c = i / s.L, r = i - c * s.L;
#pragma unroll
          for (int e = 0; e < 4; ++e, ++r) {
            while (r >= s.L) r -= s.L, ++c;
            out[e] = act(in[e], c);
          }
          *reinterpret_cast<float4*>(ys + i) = make_float4(out[0], out[1], out[2], out[3]);
        });
    return;
  }
  // one 2x2 window per thread and step: the four values, their maximum and its position stay in
  // registers
  const int Ly = s.Hy * s.Wy, ny = cpg * Ly;
  float* ys = y + (int64_t)sg * ny;
  uint8_t* as = am + (int64_t)sg * ny;
  for (int t = tid; t < ny; t += kGnThreads) {
    const int c = t / Ly, rem = t - c * Ly, ph = rem / s.Wy, pw = rem - ph * s.Wy;
    const float* p = src + c * s.L + 2 * ph * s.W + 2 * pw;
    const float v[4] = {act(p[0], c), act(p[1], c), act(p[s.W], c), act(p[s.W + 1], c)};
    float best = v[0];
    int at = 0;
#pragma unroll
    for (int r = 1; r < 4; ++r)
      if (v[r] > best) {                  // strict: a tie stays at the lowest position
        best = v[r];
        at = r;
      }
    ys[t] = best;
    as[t] = (uint8_t)at;
  }
}

// ------------------------------------------------------------------ backward
template <bool LDS>
__global__ void __launch_bounds__(kGnThreads)
group_norm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                      const float* __restrict__ rstd, const float* __restrict__ w, const float* __restrict__ b,
                      const uint8_t* __restrict__ am, float* __restrict__ dx, float* __restrict__ ws,
                      GroupNormShape s) {
  extern __shared__ __attribute__((aligned(16))) float gn_lds[];
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int sg = blockIdx.x, g = sg % s.G, bb = sg / s.G;
  const int cpg = s.C / s.G, n = cpg * s.L, c0 = g * cpg;
  const int Ly = s.pool ? s.Hy * s.Wy : s.L;
  const float* xs = x + (int64_t)sg * n;
  float* sp = gn_lds + (((uintptr_t)xs >> 2) & 3);
  const float* src = LDS ? sp : xs;
  const float* dys = dy + (int64_t)sg * cpg * Ly;
  const uint8_t* ams = s.pool ? am + (int64_t)sg * cpg * Ly : nullptr;
  const float mu = mean[sg], rs = rstd[sg];
  if (LDS) {
    gn_stage<true>(xs, sp, n);
    __syncthreads();
  }

  // pass A: wave wv owns channels wv, wv + 4, ... of the group
  float a1 = 0.f, a2 = 0.f;
  for (int j = wv; j < cpg; j += 4) {
    const float wc = w ? w[c0 + j] : 1.f, bc = b ? b[c0 + j] : 0.f;
    const float* xr = src + j * s.L;
    const float* dr = dys + j * Ly;
    float s1 = 0.f, s2 = 0.f;
    auto add = [&](float gv, float xv) {
      if (s.relu && !(gn_pre(xv, mu, rs, wc, bc) > 0.f)) gv = 0.f;
      s1 += gv;
      s2 += gv * ((xv - mu) * rs);
    };
    if (s.pool) {
      // only a window's maximum has a gradient
      for (int t = lane; t < Ly; t += 64) {
        const int ph = t / s.Wy, pw = t - ph * s.Wy, a = ams[j * Ly + t] & 3;
        add(dr[t], xr[(2 * ph + (a >> 1)) * s.W + 2 * pw + (a & 1)]);
      }
    } else {
      gn_sweep(
          dr, s.L, lane, 64, [&](int i) { add(dr[i], xr[i]); },
          [&](int i) {
            const float4 gv = *reinterpret_cast<const float4*>(dr + i), xv = gn_ld4(xr + i);
            add(gv.x, xv.x), add(gv.y, xv.y), add(gv.z, xv.z), add(gv.w, xv.w);
          });
    }
    s1 = sl_wave_sum(s1);
    s2 = sl_wave_sum(s2);
    if (ws && lane == 0) {
      float* o = ws + ((int64_t)bb * s.C + c0 + j) * 2;
      o[0] = s1, o[1] = s2;
    }
    a1 += wc * s1;
    a2 += wc * s2;
  }
  if (lane == 0) red[0][wv] = a1, red[1][wv] = a2;
  __syncthreads();
  if (!dx) return;
  const float m1 = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)n;
  const float m2 = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)n;

  // pass B: every element of the span, the pixels the pool dropped included (their dz is 0).
  // (c, h, q) = channel, row, column; without pooling a channel is one row of L columns.
  const int Wr = s.pool ? s.W : s.L;
  float* dxs = dx + (int64_t)sg * n;
  auto one = [&](float xv, float gv, int c, int h, int q) {
    const float wc = w ? w[c0 + c] : 1.f, bc = b ? b[c0 + c] : 0.f;
    if (s.pool) {
      gv = 0.f;
      if (h < 2 * s.Hy && q < 2 * s.Wy) {
        const int o = c * Ly + (h >> 1) * s.Wy + (q >> 1);
        if ((ams[o] & 3) == 2 * (h & 1) + (q & 1)) gv = dys[o];
      }
    }
    if (s.relu && !(gn_pre(xv, mu, rs, wc, bc) > 0.f)) gv = 0.f;
    return rs * (wc * gv - m1 - ((xv - mu) * rs) * m2);
  };
  gn_sweep(
      dxs, n, tid, kGnThreads,
      [&](int i) {
        const int c = i / s.L, r = i - c * s.L, h = r / Wr;
        dxs[i] = one(src[i], s.pool ? 0.f : dys[i], c, h, r - h * Wr);
      },
      [&](int i) {
        const float4 xv = gn_ld4(src + i);
        const float4 gv = s.pool ? make_float4(0.f, 0.f, 0.f, 0.f) : gn_ld4(dys + i);
        const float xin[4] = {xv.x, xv.y, xv.z, xv.w}, gin[4] = {gv.x, gv.y, gv.z, gv.w};
        float out[4];
        int c = i / s.L, r = i - c * s.L, h = r / Wr, q = r - h * Wr;
#pragma unroll
        for (int e = 0; e < 4; ++e, ++q, ++r) {
          while (r >= s.L) r -= s.L, ++c, h = 0, q = 0;
          if (q >= Wr) q = 0, ++h;
          out[e] = one(xin[e], gin[e], c, h, q);
        }
        *reinterpret_cast<float4*>(dxs + i) = make_float4(out[0], out[1], out[2], out[3]);
      });
}

// dw[c] / db[c] = the per-sample channel sums added in sample order
__global__ void __launch_bounds__(kGnThreads)
group_norm_param_kernel(const float* __restrict__ ws, int B, int C, float* __restrict__ dw, float* __restrict__ db) {
  const int c = blockIdx.x * kGnThreads + threadIdx.x;
  if (c >= C) return;
  db[c] = sum_slabs(ws + 2 * c, B, 2 * (int64_t)C);
  dw[c] = sum_slabs(ws + 2 * c + 1, B, 2 * (int64_t)C);
}

// LDS bytes of a workgroup's span image, 0 = the span is re-read from global memory
size_t gn_lds_bytes(const GroupNormShape& s) {
  const int64_t n = (int64_t)(s.C / s.G) * s.L;
  return n + 3 <= kGroupNormLdsFloats ? (size_t)((n + 3) * 4 + 15) / 16 * 16 : 0;
}

}  // namespace

hipError_t group_norm_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd,
                          uint8_t* am, GroupNormShape s, hipStream_t st) {
  const size_t lds = gn_lds_bytes(s);
  const dim3 grid(s.B * s.G), block(kGnThreads);
  if (lds) hipLaunchKernelGGL(group_norm_fwd_kernel<true>, grid, block, lds, st, x, w, b, y, mean, rstd, am, s);
  else hipLaunchKernelGGL(group_norm_fwd_kernel<false>, grid, block, 0, st, x, w, b, y, mean, rstd, am, s);
  return hipGetLastError();
}

hipError_t group_norm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* w,
                          const float* b, const uint8_t* am, float* dx, float* ws, float* dw, float* db,
                          GroupNormShape s, hipStream_t st) {
  const size_t lds = gn_lds_bytes(s);
  const dim3 grid(s.B * s.G), block(kGnThreads);
  if (lds) hipLaunchKernelGGL(group_norm_bwd_kernel<true>, grid, block, lds, st, dy, x, mean, rstd, w, b, am, dx, ws, s);
  else hipLaunchKernelGGL(group_norm_bwd_kernel<false>, grid, block, 0, st, dy, x, mean, rstd, w, b, am, dx, ws, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !ws) return e;
  hipLaunchKernelGGL(group_norm_param_kernel, dim3((s.C + kGnThreads - 1) / kGnThreads), block, 0, st, ws, s.B, s.C,
                     dw, db);
  return hipGetLastError();
}

}  // namespace sl
