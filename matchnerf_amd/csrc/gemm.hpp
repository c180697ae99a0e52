// The strided MFMA GEMM of the training path and the Linear-layer wrappers built on it (gemm.hip; used by decoder_backward.hip and
// encoder_backward.hip).
#pragma once
#include "common.hpp"

// C[I,J] (+)= sum_k A(i,k) B(k,j) (+ bias[j]);  mode 0: C = ..   1: C += ..   2: atomicAdd (split-K)
// math 0: exact f32, 1: split-bf16 (six products), 2: split-fp16 with row gains (three products); 1 and 2 for I, J >= 128
void gemm_with(hipStream_t st, const float* a, long long sa_i, long long sa_k, const float* b, long long sb_k, long long sb_j, float* c,
               long long sc_i, const float* bias, int I, int J, int K, int mode, int math_b6);
// the same with the process's math (MNERF_GEMM_MATH, read once)
void gemm(hipStream_t st, const float* a, long long sa_i, long long sa_k, const float* b, long long sb_k, long long sb_j, float* c,
          long long sc_i, const float* bias, int I, int J, int K, int mode);
// Y[N,M] = X[N,K] W[M,K]^T + bias          (torch Linear; ldx / ldw / ldy = row strides)
void linear_fwd(hipStream_t st, const float* x, long long ldx, const float* w, long long ldw, const float* bias, float* y, long long ldy,
                int N, int M, int K, bool add = false);
// dX[N,K] (+)= dY[N,M] W[M,K]
void linear_bwd_data(hipStream_t st, const float* dy, long long lddy, const float* w, long long ldw, float* dx, long long lddx, int N,
                     int M, int K, bool add);
// dW[M,K] += dY[N,M]^T X[N,K]
void linear_bwd_weight(hipStream_t st, const float* dy, long long lddy, const float* x, long long ldx, float* dw, long long lddw, int N,
                       int M, int K);
// out[j] += sum_n x[n, j]   (bias gradients, LayerNorm gain / shift gradients)
void colsum(hipStream_t st, const float* x, long long ldx, int N, int M, float* out);
