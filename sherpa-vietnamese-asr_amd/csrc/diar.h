// Speaker-diarization clustering on the device: the spectral embedding of Senko's
// SpectralCluster (core/speaker_diarization_senko_campp_optimized.py:183-233) up to the k
// smallest eigenpairs of its Laplacian.  DESIGN.md 4f has the algorithm.
//
//   similarity  Xn = X / (|X|_2 + 1e-10) row-wise, M = Xn Xn^T, float32 throughout (:183-189)
//   prune       per row the N - n_elems largest entries survive, the rest become 0 (:201-207).
//               Entries equal to the threshold value are kept from the lowest column index up;
//               the reference's argsort leaves the order of ties undefined.
//   symmetrise  M <- 0.5 (M + M^T) in place, diagonal <- 0, deg[i] = sum_j |M_ij| in float64
//               (:209-215).  L = diag(deg) - M is never stored.
//   eigs        Chebyshev-filtered subspace iteration on a 32-column float64 block.
//
// No floating-point atomics: every sum has a fixed order, results are bit-identical from run to
// run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "device_mem.h"

namespace zasr {

constexpr int kDiarMinN = 2, kDiarMaxN = 8192, kDiarMaxD = 512;
constexpr int kDiarB = 32;        // block width: every block buffer is [N][32] float64, columns
                                  // past min(32, N) are zero
constexpr int kDiarMaxK = 16;     // eigenpairs asked for at most
constexpr int kDiarChebDegree = 24;
constexpr int kDiarMaxPasses = 200;
constexpr int kDiarRowsPerBlock = 32;      // rows of L one workgroup of the FMA product makes
constexpr int kDiarRowsPerBlockMfma = 64;  // and of the float64-MFMA product
constexpr int kDiarMaxSplit = 16;      // column ranges a row tile is split over at most
constexpr int kDiarGramRows = 256;     // rows one workgroup of gram_partial sums

// ---- kernels (diar_kernels.hip) ----
// Xn[i] = X[i] / (|X[i]| + 1e-10), rows of D floats (ldn >= D, the padding columns are zeroed)
void launch_diar_normalise(const float* X, int N, int D, float* Xn, int ldn, hipStream_t st);
// M = Xn Xn^T for a D the MFMA GEMM does not take
void launch_diar_similarity_plain(const float* Xn, int N, int D, int ldn, float* M, hipStream_t st);
// zero all but the `keep` largest entries of every row (keep in [1, N])
void launch_diar_prune(float* M, int N, int keep, hipStream_t st);
void launch_diar_symmetrise(float* M, int N, hipStream_t st);
void launch_diar_degree(const float* M, int N, double* deg, hipStream_t st);
// out = alpha ((L V1) - c V1) - beta V0 with L = diag(deg) - M; V0 may be null when beta == 0.
// `partial` holds split * N * 32 doubles when split > 1.
void launch_diar_lap_block(const float* M, const double* deg, int N, const double* V1,
                           const double* V0, double* out, double alpha, double c, double beta,
                           int split, double* partial, hipStream_t st);
int diar_lap_split(int N);
bool diar_lap_mfma();  // the float64-MFMA form of the product is selected
// G[32][32] = A^T B, row tiles summed in tile order; partial holds cdiv(N, 256) * 1024 doubles
void launch_diar_gram(const double* A, const double* B, int N, double* partial, double* G,
                      hipStream_t st);
// out = A RA (+ B RB when B is not null); RA / RB are [32][32] row-major on the device
void launch_diar_block_mul(const double* A, const double* RA, const double* B, const double* RB,
                           int N, double* out, hipStream_t st);

class DiarEngine {
 public:
  explicit DiarEngine(int device);
  void similarity(const float* d_X, int N, int D, float* d_M, hipStream_t st);
  void prune(float* d_M, int N, double pval, int min_pnum, double* d_deg, hipStream_t st);
  // lambdas [k], vecs [N][k] on the host; returns the outer passes
  int eigs(const float* d_M, const double* d_deg, int N, int k, double* lambdas, double* vecs,
           hipStream_t st);
  int spectral_embed(const float* X, bool x_on_device, int N, int D, double pval, int min_pnum,
                     int k, double* lambdas, double* vecs, hipStream_t st);
  long last_applications = 0;  // block Laplacian products of the last eigs
  std::mutex mu;

 private:
  int device_ = 0;
  Workspace ws_;
};

// the symmetric eigenproblem of the b x b Rayleigh-Ritz and Gram matrices: cyclic Jacobi, A
// [n][n] row-major in, eigenvalues ascending in w, eigenvectors in the columns of Q [n][n]
void jacobi_eigh(std::vector<double>& A, int n, std::vector<double>& w, std::vector<double>& Q);
// n_elems of p_pruning (:202-204), as Python computes it
int diar_prune_count(int N, double pval, int min_pnum);

}  // namespace zasr
