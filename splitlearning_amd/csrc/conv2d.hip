// General 3x3 convolution (stride 1, padding 0 | 1) [+ ReLU] [+ MaxPool2d(2, 2)] for user
// models (splitlearning_amd.nn.FusedConv2d): three implicit GEMMs on the exact-fp32
// v_mfma_f32_16x16x4_f32, the instruction gemm.hip uses.
//
// Reference ops: nn.Conv2d(Cin, Cout, 3, padding=p), F.relu, F.max_pool2d(2, 2) and their
// autograd (ops/torch_ops.py conv3x3_fwd / conv3x3_dgrad / conv3x3_wgrad are the ground truth).
//
//   forward   M = conv output pixels, N = Cout,        K = Cin * 9   (k = ci * 9 + kh * 3 + kw)
//   dgrad     M = input pixels,       N = Cin,         K = Cout * 9  (k = co * 9 + kh * 3 + kw)
//   wgrad     M = Cout,               N = Cin * 9 + 1, K = conv output pixels
//
// No patch matrix exists in memory: every operand element is gathered (and, for the backward
// kernels, turned from dy into the conv-resolution gradient dz) as it is staged into LDS.
// Padding and every M / N / K tail are zero-filled by buffer loads whose offset is sent out of
// range (gemm.hip's gemm_ld).
//
// With pooling the pixel index is window-ordered: m = 4 * window + position, window = (b, ph,
// pw), position = 2 * dy + dx.  The 16x16x4 accumulator gives lane l rows 4 * (l / 16) + r of
// column l % 16, so the four registers of one lane are the four conv outputs of one pooling
// window of one channel: bias, ReLU, max and argmax are register-local and only the pooled
// value and its 2-bit position are stored.  The row / column torch's floor rule leaves out of
// every window is never computed in the forward and contributes dz = 0 in the backward.
//
// One 256-thread workgroup computes a 64 x 64 tile (2 x 2 waves of 32 x 32, each 2 x 2 MFMA
// blocks), K staged 16 at a time through double-buffered LDS: the next stage's gathers are
// issued before this stage's MFMAs and written to the other buffer after them.
//
// The weight gradient splits its reduction over gridDim.z slabs of pixels; every slab stores
// its raw 64 x 64 partial tile and conv_wgrad_sum_kernel adds the slabs in index order (the
// project's sum_slabs pattern: no floating-point atomics, two runs agree bitwise).  db is the
// extra column N = Cin * 9 of the pixel operand, all ones.
#include "conv2d.h"

#include "common.h"

#include <algorithm>

namespace sl {

namespace {

constexpr int kBM = 64, kBN = 64, kBK = 16, kLD = kBK + 4;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}
// element `elem` of a float buffer, 0 when !in (the offset is past every operand: < 2 GB each)
__device__ __forceinline__ float conv_ld(__amdgpu_buffer_rsrc_t rs, bool in, int elem) {
  const int off = in ? elem * 4 : 0x7ffffff0;
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, 0));
}
__device__ __forceinline__ int conv_ld_u8(__amdgpu_buffer_rsrc_t rs, bool in, int elem) {
  const int off = in ? elem : 0x7ffffff0;
  return (int)__builtin_amdgcn_raw_buffer_load_b8(rs, off, 0, 0);
}

// A conv-output pixel of the GEMM's pixel index m: natural (b, oh, ow) order without pooling,
// 4 * window + position with it.  yo = offset of its y element inside a [Hy, Wy] plane.
struct ConvPix {
  int b, oh, ow, yo, pos;
};
__device__ __forceinline__ ConvPix conv_pix(const Conv2dShape& s, int m) {
  ConvPix p;
  const int hw = s.Hy * s.Wy;
  const int wi = s.pool ? m >> 2 : m;
  p.pos = m & 3;
  p.b = wi / hw;
  p.yo = wi - p.b * hw;
  const int yh = p.yo / s.Wy, yw = p.yo - yh * s.Wy;
  p.oh = s.pool ? 2 * yh + (p.pos >> 1) : yh;
  p.ow = s.pool ? 2 * yw + (p.pos & 1) : yw;
  return p;
}

// dz at one conv-output pixel from the gradient of y: dy where the pixel is its window's
// maximum (pos == am) and the ReLU is active (y > 0), else 0.  idx = the y element.
struct ConvDz {
  __amdgpu_buffer_rsrc_t dy, y, am;
  int relu, pool;
};
__device__ __forceinline__ float conv_dz(const ConvDz& d, bool in, int idx, int pos) {
  float g = conv_ld(d.dy, in, idx);
  if (d.relu) g = conv_ld(d.y, in, idx) > 0.f ? g : 0.f;
  if (d.pool) g = conv_ld_u8(d.am, in, idx) == pos ? g : 0.f;
  return g;
}

// One 16-wide K stage of a wave's 32 x 32 tile.  A lane reads one float4 of its A row and of
// its B row and feeds component c to sub-step c (lane group lq covers k = 4 lq + c).
__device__ __forceinline__ void conv_mma(const float (*As)[kLD], const float (*Bs)[kLD], f32x4 (&acc)[2][2], int wm,
                                         int wn, int li, int lq) {
  f32x4 a[2], b[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    a[i] = *reinterpret_cast<const f32x4*>(&As[wm + 16 * i + li][4 * lq]);
    b[i] = *reinterpret_cast<const f32x4*>(&Bs[wn + 16 * i + li][4 * lq]);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][c], b[j][c], acc[i][j], 0, 0, 0);
}

// The staged main loop shared by the three kernels: gload(k0) gathers a thread's 4 + 4
// elements of the stage at k0 into registers, sstore(buf) writes them to LDS buffer buf.
template <class GLoad, class SStore>
__device__ __forceinline__ void conv_mainloop(float (*As)[kBM][kLD], float (*Bs)[kBN][kLD], f32x4 (&acc)[2][2],
                                              int kb, int nk, GLoad gload, SStore sstore) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, li = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  gload(kb);
  sstore(0);
  __syncthreads();
  for (int s = 0; s < nk; ++s) {
    const int buf = s & 1;
    // unconditional (the last stage reloads its own block, unused), as in gemm.hip
    gload(kb + (s + 1 < nk ? s + 1 : s) * kBK);
    __builtin_amdgcn_sched_barrier(0);
    conv_mma(As[buf], Bs[buf], acc, wm, wn, li, lq);
    __builtin_amdgcn_sched_barrier(0);
    sstore(buf ^ 1);   // its last readers finished before the previous barrier
    __syncthreads();
  }
}

// ------------------------------------------------------------------ forward
__global__ void __launch_bounds__(256)
conv3x3_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                   float* __restrict__ y, uint8_t* __restrict__ am, Conv2dShape s, int M) {
  __shared__ __attribute__((aligned(16))) float As[2][kBM][kLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][kBN][kLD];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int K = s.Cin * 9, HW = s.H * s.W;
  const __amdgpu_buffer_rsrc_t rx = conv_rsrc(x, (int64_t)s.B * s.Cin * HW * 4);
  const __amdgpu_buffer_rsrc_t rw = conv_rsrc(w, (int64_t)s.Cout * K * 4);
  // A: this thread stages row arow (one output pixel), k = k0 + 4 akq + j
  const int arow = tid & 63, akq = tid >> 6;
  const bool aok = m0 + arow < M;
  const ConvPix p = conv_pix(s, m0 + arow);
  const int ih0 = p.oh - s.pad, iw0 = p.ow - s.pad;
  const int xbase = p.b * s.Cin * HW + ih0 * s.W + iw0;
  // B: row brow (one output channel), k = k0 + 4 bkq + j
  const int brow = tid >> 2, bkq = tid & 3;
  const bool bok = n0 + brow < s.Cout;
  const int wbase = (n0 + brow) * K;
  float ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 4 * akq + j, ci = k / 9, r = k - 9 * ci, kh = r / 3, kw = r - 3 * kh;
      const bool in = aok && k < K && (unsigned)(ih0 + kh) < (unsigned)s.H && (unsigned)(iw0 + kw) < (unsigned)s.W;
      ra[j] = conv_ld(rx, in, xbase + ci * HW + kh * s.W + kw);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 4 * bkq + j;
      rb[j] = conv_ld(rw, bok && k < K, wbase + k);
    }
  };
  auto sstore = [&](int buf) {
    *reinterpret_cast<float4*>(&As[buf][arow][4 * akq]) = make_float4(ra[0], ra[1], ra[2], ra[3]);
    *reinterpret_cast<float4*>(&Bs[buf][brow][4 * bkq]) = make_float4(rb[0], rb[1], rb[2], rb[3]);
  };
  f32x4 acc[2][2];
  conv_mainloop(As, Bs, acc, 0, (K + kBK - 1) / kBK, gload, sstore);

  // epilogue: lane (li, lq) of block (i, j) holds pixels mb .. mb + 3 of channel n
  const int lane = tid & 63, wv = tid >> 6;
  const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, li = lane & 15, lq = lane >> 4;
  const int hw = s.Hy * s.Wy;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + li;
    if (n >= s.Cout) continue;
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int mb = m0 + wm + 16 * i + 4 * lq;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[i][j][r] + bv;
        if (s.relu) v[r] = fmaxf(v[r], 0.f);
      }
      if (s.pool) {
        if (mb >= M) continue;            // M is a multiple of 4: a window is whole or absent
        const int wi = mb >> 2, b = wi / hw, yo = wi - b * hw;
        float best = v[0];
        int at = 0;
#pragma unroll
        for (int r = 1; r < 4; ++r)
          if (v[r] > best) {              // strict: a tie stays at the lowest position
            best = v[r];
            at = r;
          }
        const int o = (b * s.Cout + n) * hw + yo;
        y[o] = best;
        am[o] = (uint8_t)at;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = mb + r;
          if (m >= M) continue;
          const int b = m / hw, yo = m - b * hw;
          y[(b * s.Cout + n) * hw + yo] = v[r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ data gradient
// dx[b, ci, h, w] = sum over (co, kh, kw) of dz[b, co, h + pad - kh, w + pad - kw] w[co, ci, kh, kw]
__global__ void __launch_bounds__(256)
conv3x3_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const uint8_t* __restrict__ am,
                     const float* __restrict__ w, float* __restrict__ dx, Conv2dShape s, int M) {
  __shared__ __attribute__((aligned(16))) float As[2][kBM][kLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][kBN][kLD];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int K = s.Cout * 9, HW = s.H * s.W, hw = s.Hy * s.Wy;
  const int64_t ny = (int64_t)s.B * s.Cout * hw;
  const ConvDz dz{conv_rsrc(dy, ny * 4), conv_rsrc(y, ny * 4), conv_rsrc(am, am ? ny : 0), s.relu, s.pool};
  const __amdgpu_buffer_rsrc_t rw = conv_rsrc(w, (int64_t)s.Cout * s.Cin * 9 * 4);
  // A: row arow = one input pixel (b, h, w)
  const int arow = tid & 63, akq = tid >> 6;
  const bool aok = m0 + arow < M;
  const int ab = (m0 + arow) / HW, arem = (m0 + arow) - ab * HW, ah = arem / s.W, aw = arem - ah * s.W;
  // B: row brow = one input channel
  const int brow = tid >> 2, bkq = tid & 3;
  const bool bok = n0 + brow < s.Cin;
  float ra[4], rb[4];
  auto gload = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 4 * akq + j, co = k / 9, r = k - 9 * co, kh = r / 3, kw = r - 3 * kh;
      const int oh = ah + s.pad - kh, ow = aw + s.pad - kw;
      const int yh = s.pool ? oh >> 1 : oh, yw = s.pool ? ow >> 1 : ow;
      // oh, ow >= 0 and inside the pooled (or whole) conv output; the floor rule's left-out
      // row / column has yh == Hy or yw == Wy and reads as 0
      const bool in = aok && k < K && oh >= 0 && ow >= 0 && yh < s.Hy && yw < s.Wy;
      ra[j] = conv_dz(dz, in, ((ab * s.Cout + co) * s.Hy + yh) * s.Wy + yw, 2 * (oh & 1) + (ow & 1));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + 4 * bkq + j, co = k / 9, r = k - 9 * co;
      rb[j] = conv_ld(rw, bok && k < K, (co * s.Cin + n0 + brow) * 9 + r);
    }
  };
  auto sstore = [&](int buf) {
    *reinterpret_cast<float4*>(&As[buf][arow][4 * akq]) = make_float4(ra[0], ra[1], ra[2], ra[3]);
    *reinterpret_cast<float4*>(&Bs[buf][brow][4 * bkq]) = make_float4(rb[0], rb[1], rb[2], rb[3]);
  };
  f32x4 acc[2][2];
  conv_mainloop(As, Bs, acc, 0, (K + kBK - 1) / kBK, gload, sstore);

  const int lane = tid & 63, wv = tid >> 6;
  const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, li = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + li;
    if (n >= s.Cin) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * lq + r;
        if (m >= M) continue;
        const int b = m / HW, rem = m - b * HW;
        dx[(b * s.Cin + n) * HW + rem] = acc[i][j][r];
      }
  }
}

// ------------------------------------------------------------------ weight gradient
// P[z][co][n] = sum over the pixels of slab z of dz[pixel, co] * (n < Cin 9 ? x patch : 1)
__global__ void __launch_bounds__(256)
conv3x3_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const uint8_t* __restrict__ am,
                     const float* __restrict__ x, float* __restrict__ P, Conv2dShape s, int R, int kc) {
  __shared__ __attribute__((aligned(16))) float As[2][kBM][kLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][kBN][kLD];
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int C9 = s.Cin * 9, N1 = C9 + 1, HW = s.H * s.W, hw = s.Hy * s.Wy;
  const int64_t ny = (int64_t)s.B * s.Cout * hw;
  const ConvDz dz{conv_rsrc(dy, ny * 4), conv_rsrc(y, ny * 4), conv_rsrc(am, am ? ny : 0), s.relu, s.pool};
  const __amdgpu_buffer_rsrc_t rx = conv_rsrc(x, (int64_t)s.B * s.Cin * HW * 4);
  const int kb = (int)blockIdx.z * kc, ke = min(R, kb + kc);
  // this thread stages pixel k0 + kl of rows rg + 16 j of both operands
  const int kl = tid & 15, rg = tid >> 4;
  int boff[4], bkh[4], bkw[4];     // B row n -> (ci, kh, kw): the same for every stage
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + rg + 16 * j, ci = n / 9, r = n - 9 * ci;
    bkh[j] = r / 3 - s.pad;
    bkw[j] = r - 3 * (r / 3) - s.pad;
    boff[j] = ci * HW;
  }
  float ra[4], rb[4];
  auto gload = [&](int k0) {
    const int kk = k0 + kl;
    const bool ok = kk < ke;
    const ConvPix p = conv_pix(s, kk);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = m0 + rg + 16 * j;
      ra[j] = conv_dz(dz, ok && co < s.Cout, (p.b * s.Cout + co) * hw + p.yo, p.pos);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + rg + 16 * j, ih = p.oh + bkh[j], iw = p.ow + bkw[j];
      const bool in = ok && n < C9 && (unsigned)ih < (unsigned)s.H && (unsigned)iw < (unsigned)s.W;
      const float v = conv_ld(rx, in, p.b * s.Cin * HW + boff[j] + ih * s.W + iw);
      rb[j] = (n == C9 && ok) ? 1.f : v;     // the bias column
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      As[buf][rg + 16 * j][kl] = ra[j];
      Bs[buf][rg + 16 * j][kl] = rb[j];
    }
  };
  f32x4 acc[2][2];
  conv_mainloop(As, Bs, acc, kb, (ke - kb + kBK - 1) / kBK, gload, sstore);

  const int lane = tid & 63, wv = tid >> 6;
  const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32, li = lane & 15, lq = lane >> 4;
  float* Pz = P + (int64_t)blockIdx.z * s.Cout * N1;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn + 16 * j + li;
    if (n >= N1) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * lq + r;
        if (m < s.Cout) Pz[(int64_t)m * N1 + n] = acc[i][j][r];
      }
  }
}

// dw / db = the slabs of P added in index order
__global__ void __launch_bounds__(256)
conv_wgrad_sum_kernel(const float* __restrict__ P, int S, int Cout, int C9, float* __restrict__ dw,
                      float* __restrict__ db) {
  const int N1 = C9 + 1, total = Cout * N1;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float a = 0.f;
  for (int z = 0; z < S; ++z) a += P[(int64_t)z * total + i];
  const int co = i / N1, n = i - co * N1;
  if (n < C9) dw[co * C9 + n] = a;
  else if (db) db[co] = a;
}

// pixels of the implicit GEMMs' conv-output index (window-ordered with pooling)
int conv_pixels(const Conv2dShape& s) { return s.B * s.Hy * s.Wy * (s.pool ? 4 : 1); }

struct WgradSplit {
  int S, kc;
};
WgradSplit wgrad_split(const Conv2dShape& s) {
  const int R = conv_pixels(s);
  const int tiles = ((s.Cout + kBM - 1) / kBM) * ((s.Cin * 9 + 1 + kBN - 1) / kBN);
  int S = std::min(std::max(1, 512 / tiles), (R + kConvWgradMinSlab - 1) / kConvWgradMinSlab);
  S = std::max(1, std::min(S, kConvWgradMaxSlabs));
  const int kc = ((R + S - 1) / S + kBK - 1) / kBK * kBK;
  return {(R + kc - 1) / kc, kc};
}

}  // namespace

hipError_t conv3x3_fwd(const float* x, const float* w, const float* bias, float* y, uint8_t* am, Conv2dShape s,
                       hipStream_t st) {
  const int M = conv_pixels(s);
  if (M == 0) return hipSuccess;
  const dim3 grid((M + kBM - 1) / kBM, (s.Cout + kBN - 1) / kBN);
  hipLaunchKernelGGL(conv3x3_fwd_kernel, grid, dim3(256), 0, st, x, w, bias, y, am, s, M);
  return hipGetLastError();
}

hipError_t conv3x3_dgrad(const float* dy, const float* y, const uint8_t* am, const float* w, float* dx,
                         Conv2dShape s, hipStream_t st) {
  const int M = s.B * s.H * s.W;
  if (M == 0) return hipSuccess;
  const dim3 grid((M + kBM - 1) / kBM, (s.Cin + kBN - 1) / kBN);
  hipLaunchKernelGGL(conv3x3_dgrad_kernel, grid, dim3(256), 0, st, dy, y, am, w, dx, s, M);
  return hipGetLastError();
}

int conv3x3_wgrad_slabs(const Conv2dShape& s) { return wgrad_split(s).S; }

hipError_t conv3x3_wgrad(const float* dy, const float* y, const uint8_t* am, const float* x, float* ws, float* dw,
                         float* db, Conv2dShape s, hipStream_t st) {
  const int R = conv_pixels(s), C9 = s.Cin * 9;
  const WgradSplit sp = wgrad_split(s);
  const dim3 grid((s.Cout + kBM - 1) / kBM, (C9 + 1 + kBN - 1) / kBN, sp.S);
  hipLaunchKernelGGL(conv3x3_wgrad_kernel, grid, dim3(256), 0, st, dy, y, am, x, ws, s, R, sp.kc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int total = s.Cout * (C9 + 1);
  hipLaunchKernelGGL(conv_wgrad_sum_kernel, dim3((total + 255) / 256), dim3(256), 0, st, ws, sp.S, s.Cout, C9, dw, db);
  return hipGetLastError();
}

}  // namespace sl
