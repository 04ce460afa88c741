// The GemmParams of one dense problem C[M][N] = A[M][K] W^T + bias on a weight matrix W [N][K]
// (K contiguous): what every engine's linear helper starts from.
#pragma once
#include "gemm.h"

namespace zasr {

// A / C are typed by the GEMM that runs the problem (f32, or bf16 for gemm_bf16's a_bf16 / c_bf16)
inline GemmParams dense_gemm_params(const float* W, const float* bias, int N, int K, const void* A,
                                    int lda, int M, void* C, int ldc) {
  GemmParams p{};
  p.A = reinterpret_cast<const float*>(A);
  p.lda = lda;
  p.B = W;
  p.sbk = 1;
  p.sbn = K;
  p.C = reinterpret_cast<float*>(C);
  p.ldc = ldc;
  p.bias = bias;
  p.M = p.max_M = M;
  p.N = N;
  p.K = K;
  return p;
}

}  // namespace zasr
