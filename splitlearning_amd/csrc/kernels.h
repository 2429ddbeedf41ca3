// Host entry points of conv.hip, linear.hip, loss.hip and gemm.hip, declared once.  Every caller
// (the bindings, the executors, and the kernel files that call across each other) includes this
// header, and so does each defining file: a drifted signature is a compile error.  The newer
// kernel families keep their own headers (fused.h, optim.h, conv2d.h, groupnorm.h, cutcodec.h,
// handoff.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace sl {

// ---------------------------------------------------------------- conv.hip (the 1 -> 32 front)
hipError_t conv_fwd(const void* x, bool x_u8, const int64_t* idx, int64_t row0, int B, const float* w,
                    const float* b, float* y, uint8_t* am, hipStream_t st, const int64_t* lab_in,
                    int64_t* lab_out, const ConvPending* pend);
hipError_t conv_fwd_multi(const FrontFwdSet& set, int64_t chunk, hipStream_t st);
hipError_t conv_local_step(const void* x, bool x_u8, const int64_t* idx, const int64_t* labels, int B, float* w,
                           float* b, float* slab, float* loss_rows, float* s0w, float* s1w, float* s0b, float* s1b,
                           SlOpt o, hipStream_t st);
hipError_t conv_local_epoch(const void* x, bool x_u8, const int64_t* order, int64_t n, int B, const int64_t* labels,
                            float* w, float* b, float* s0w, float* s1w, float* s0b, float* s1b, float* ws,
                            int64_t ws_elems, float* loss_rows, SlOpt (*opt)(void*, int64_t), void* optctx,
                            int64_t t0, hipStream_t st);
hipError_t conv_local_epoch_multi(const MultiAlice* al, int k, int B, SlOpt (*opt)(void*, int64_t), void* optctx,
                                  void* table, int64_t table_bytes, hipStream_t st);
size_t alice_step_desc_bytes();
hipError_t conv_bwd_step(const float* dy, const float* y, const uint8_t* am, const void* x, bool x_u8,
                         const int64_t* idx, int B, float* w, float* b, float* slab, float* s0w, float* s1w,
                         float* s0b, float* s1b, SlOpt o, hipStream_t st, bool defer, const ConvPending* pend);
hipError_t conv_apply(const ConvPending& p, float* w, float* b, hipStream_t st);

// ---------------------------------------------------------------- linear.hip
hipError_t linear_fwd(const float* X, int ldx, const float* W, int ldw, float* Y, int ldy, int M, int N, int K,
                      Epi e, float* ws, int64_t ws_elems, hipStream_t st);
hipError_t linear_fwd_partial(const float* X, int ldx, const float* W, int ldw, int M, int N, int K, float* ws,
                              int64_t ws_elems, int max_split, int* S_out, hipStream_t st);
hipError_t linear_epilogue(const float* P, int ldp, float* Y, int ldy, int M, int N, Epi e, int S, int64_t slab,
                           hipStream_t st);
hipError_t linear_dgrad(const float* dZ, int ldz, const float* W, int ldw, const float* hprev, int ldh,
                        float scale, float* dX, int ldx, float* ws, int64_t ws_elems, int M, int N, int K,
                        hipStream_t st);
hipError_t dgrad_reduce(const float* P, int S, int64_t slab, const float* hprev, int ldh, float scale, float* out,
                        int ldo, int M, int K, hipStream_t st);
hipError_t linear_wgrad_opt(const float* dZ, int ldz, const float* A, int lda, float* W, int ldw, float* s0,
                            float* s1, float* bias, float* sb0, float* sb1, int M, int N, int K, SlOpt o,
                            hipStream_t st);
hipError_t opt_flat(float* p, const float* g, float* s0, float* s1, int64_t n, SlOpt o, hipStream_t st);

// ---------------------------------------------------------------- gemm.hip
hipError_t gemm_nt(const float* X, int ldx, const float* W, int ldw, float* Y, int ldy, int M, int N, int K, Epi e,
                   bool bf16, float* ws, int64_t ws_elems, hipStream_t st);
hipError_t gemm_nn_dgrad(const float* dZ, int ldz, const float* W, int ldw, const float* hprev, int ldh, float scale,
                         float* dX, int ldx, int M, int R, int K, float* ws, int64_t ws_elems, hipStream_t st);

// ---------------------------------------------------------------- loss.hip
hipError_t relu_mask(const float* d, const float* h, float scale, float* out, int64_t n, hipStream_t st);
hipError_t softmax_ce(const float* x, int ldx, const int64_t* y, int64_t ignore, float scale, float* loss_rows,
                      float* d, int ldd, int M, int C, hipStream_t st);
hipError_t eval_counters(const float* x, int ldx, const int64_t* y, int64_t omit, unsigned long long* counters,
                         int M, int C, hipStream_t st);
hipError_t head_step(const float* X, float* W, float* b, const int64_t* y, int64_t ignore, float scale,
                     float* loss_rows, float* dX, float* s0w, float* s1w, float* s0b, float* s1b, int M, int K, int C,
                     SlOpt o, bool mask_dx, hipStream_t st);

}  // namespace sl
