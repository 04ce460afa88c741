// Kernels of the diarization clustering (diar.h): cosine similarity, the per-row prune, the
// in-place symmetrise, degrees, and the float64 block products of the eigen-solver.  Every sum
// has a fixed order (no floating-point atomics; the prune's histogram counts are integers).
#include "common.h"
#include "diar.h"

namespace zasr {

namespace {

constexpr int kT = 256;  // threads per workgroup of every kernel here

// ---- similarity ----
// one wave per row: the squared norm in float64 (fixed butterfly order), the division in float32
__global__ __launch_bounds__(kT) void diar_normalise_kernel(const float* __restrict__ X, int N,
                                                            int D, float* __restrict__ Xn,
                                                            int ldn) {
  const int row = blockIdx.x * (kT / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const float* x = X + (long)row * D;
  double ss = 0.0;
  for (int k = lane; k < D; k += kWave) ss += (double)x[k] * (double)x[k];
  ss = wave_sum_d(ss);
  const float den = (float)sqrt(ss) + 1e-10f;
  float* o = Xn + (long)row * ldn;
  for (int k = lane; k < ldn; k += kWave) o[k] = k < D ? x[k] / den : 0.f;
}

// M[i][j] = sum_k Xn[i][k] Xn[j][k], 16 x 16 outputs per workgroup (any D)
__global__ __launch_bounds__(kT) void diar_similarity_plain_kernel(const float* __restrict__ Xn,
                                                                   int N, int D, int ldn,
                                                                   float* __restrict__ M) {
  __shared__ float As[16][17], Bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  float acc = 0.f;
  for (int k0 = 0; k0 < D; k0 += 16) {
    const int k = k0 + tx;
    As[ty][tx] = (i0 + ty < N && k < D) ? Xn[(long)(i0 + ty) * ldn + k] : 0.f;
    Bs[ty][tx] = (j0 + ty < N && k < D) ? Xn[(long)(j0 + ty) * ldn + k] : 0.f;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) acc = fmaf(As[ty][kk], Bs[tx][kk], acc);
    __syncthreads();
  }
  if (i0 + ty < N && j0 + tx < N) M[(long)(i0 + ty) * N + j0 + tx] = acc;
}

// ---- prune ----
// order-preserving key of a float: a larger value has a larger key
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per row, the row in LDS.  An 8-bit radix select from the top digit down finds
// the key of the keep-th largest entry and how many entries equal to it survive; those are
// taken from the lowest column index up (a scan over per-thread contiguous column ranges).
__global__ __launch_bounds__(kT) void diar_prune_kernel(float* __restrict__ M, int N, int keep) {
  extern __shared__ float row[];  // [N]
  __shared__ unsigned hist[256];
  __shared__ int scan[kT];
  __shared__ unsigned s_digit, s_remaining;
  const int tid = threadIdx.x;
  float* g = M + (long)blockIdx.x * N;
  for (int j = tid; j < N; j += kT) row[j] = g[j];
  if (tid == 0) s_remaining = (unsigned)keep;
  unsigned prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (int j = tid; j < N; j += kT) {
      const unsigned key = order_key(row[j]);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned rem = s_remaining;
      int d = 255;
      while (d > 0 && hist[d] < rem) {
        rem -= hist[d];
        --d;
      }
      s_digit = (unsigned)d;
      s_remaining = rem;
    }
    __syncthreads();
    prefix |= s_digit << shift;
    mask |= 255u << shift;
  }
  const unsigned thr = prefix;
  const int ties_kept = (int)s_remaining;
  const int seg = (N + kT - 1) / kT;
  const int jb = min(N, tid * seg), je = min(N, jb + seg);
  int cnt = 0;
  for (int j = jb; j < je; ++j) cnt += order_key(row[j]) == thr;
  scan[tid] = cnt;
  __syncthreads();
  for (int o = 1; o < kT; o <<= 1) {  // inclusive scan
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int rank = scan[tid] - cnt;  // ties in lower columns
  for (int j = jb; j < je; ++j) {
    const unsigned key = order_key(row[j]);
    if (key < thr) {
      row[j] = 0.f;
    } else if (key == thr) {
      if (rank >= ties_kept) row[j] = 0.f;
      ++rank;
    }
  }
  __syncthreads();
  for (int j = tid; j < N; j += kT) g[j] = row[j];
}

// ---- symmetrise ----
// Tile pair (bi, bj), bi <= bj: both 32 x 32 tiles through LDS, each written once.
__global__ __launch_bounds__(kT) void diar_symmetrise_kernel(float* __restrict__ M, int N) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  __shared__ float A[32][33], B[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, j = bj * 32 + tx;
    A[r][tx] = (i < N && j < N) ? M[(long)i * N + j] : 0.f;
    const int i2 = bj * 32 + r, j2 = bi * 32 + tx;
    B[r][tx] = (i2 < N && j2 < N) ? M[(long)i2 * N + j2] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, j = bj * 32 + tx;
    if (i < N && j < N) M[(long)i * N + j] = i == j ? 0.f : 0.5f * (A[r][tx] + B[tx][r]);
    if (bi != bj) {
      const int i2 = bj * 32 + r, j2 = bi * 32 + tx;
      if (i2 < N && j2 < N) M[(long)i2 * N + j2] = 0.5f * (B[r][tx] + A[tx][r]);
    }
  }
}

// deg[i] = sum_j |M[i][j]|: per-thread strided sums, then a fixed tree
__global__ __launch_bounds__(kT) void diar_degree_kernel(const float* __restrict__ M, int N,
                                                         double* __restrict__ deg) {
  __shared__ double s[kT];
  const float* g = M + (long)blockIdx.x * N;
  double a = 0.0;
  for (int j = threadIdx.x; j < N; j += kT) a += (double)fabsf(g[j]);
  s[threadIdx.x] = a;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) deg[blockIdx.x] = s[0];
}

// ---- the block Laplacian product ----
__device__ __forceinline__ double lap_epilogue(double mv, double degi, double v1, const double* V0,
                                               long at, double alpha, double c, double beta) {
  const double lv = degi * v1 - mv;
  double o = alpha * (lv - c * v1);
  if (beta != 0.0) o -= beta * V0[at];
  return o;
}

// A workgroup makes rows [32 bx, +32) x 32 columns of M V1 over the columns [by chunk, +chunk)
// of M: 64-column slabs of M (float32, transposed into LDS) against the matching 64 rows of V1
// (float64), every thread a 2 x 2 patch, the next slab's global loads in flight under the
// FMAs.  M is read once per application.  DIRECT (one column range): the Chebyshev update in
// the epilogue; otherwise the sums go to partial[by] and diar_lap_reduce_kernel adds the ranges
// in order and applies it.
template <bool DIRECT>
__global__ __launch_bounds__(kT) void diar_lap_kernel(const float* __restrict__ M,
                                                      const double* __restrict__ deg, int N,
                                                      const double* __restrict__ V1,
                                                      const double* __restrict__ V0,
                                                      double* __restrict__ out, double alpha,
                                                      double c, double beta, int chunk,
                                                      double* __restrict__ partial) {
  constexpr int TR = kDiarRowsPerBlock, JT = 64, LDM = TR + 2;
  __shared__ __align__(16) float Ms[JT * LDM];
  __shared__ __align__(16) double Vs[JT * kDiarB];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * TR;
  const int j_begin = blockIdx.y * chunk, j_end = min(N, j_begin + chunk);
  const int cp = tid & 15, rp = tid >> 4;
  const int lcol = tid & 63, lrow = tid >> 6;
  float mreg[8];
  double vreg[8];
  auto gload = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = r0 + lrow + 4 * q, j = j0 + lcol;
      mreg[q] = (i < N && j < j_end) ? M[(long)i * N + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + kT * q, j = j0 + (e >> 5);
      vreg[q] = j < j_end ? V1[(long)j * kDiarB + (e & 31)] : 0.0;
    }
  };
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  if (j_begin < j_end) gload(j_begin);
  for (int j0 = j_begin; j0 < j_end; j0 += JT) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) Ms[lcol * LDM + lrow + 4 * q] = mreg[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) Vs[tid + kT * q] = vreg[q];
    __syncthreads();
    if (j0 + JT < j_end) gload(j0 + JT);
#pragma unroll 8
    for (int jj = 0; jj < JT; ++jj) {
      const float2 m = *reinterpret_cast<const float2*>(&Ms[jj * LDM + 2 * rp]);
      const double2 v = *reinterpret_cast<const double2*>(&Vs[jj * kDiarB + 2 * cp]);
      acc[0][0] = fma((double)m.x, v.x, acc[0][0]);
      acc[0][1] = fma((double)m.x, v.y, acc[0][1]);
      acc[1][0] = fma((double)m.y, v.x, acc[1][0]);
      acc[1][1] = fma((double)m.y, v.y, acc[1][1]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int i = r0 + 2 * rp + a;
    if (i >= N) continue;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const long at = (long)i * kDiarB + 2 * cp + b;
      if constexpr (DIRECT)
        out[at] = lap_epilogue(acc[a][b], deg[i], V1[at], V0, at, alpha, c, beta);
      else
        partial[(long)blockIdx.y * N * kDiarB + at] = acc[a][b];
    }
  }
}

// The same product on the float64 MFMA (v_mfma_f64_16x16x4_f64): a workgroup of four waves
// makes 64 rows, each wave 16 rows x 32 columns as two 16 x 16 tiles.  Per step of 4 columns of
// M a lane supplies M[row lane & 15][column lane >> 4] (float32 widened) as A and
// V1[row lane >> 4][column lane & 15] of each tile as B.  C/D of this instruction: column
// lane & 15, row (lane >> 4) + 4 reg -- not the f32 forms' map.
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <bool DIRECT>
__global__ __launch_bounds__(kT) void diar_lap_mfma_kernel(const float* __restrict__ M,
                                                           const double* __restrict__ deg, int N,
                                                           const double* __restrict__ V1,
                                                           const double* __restrict__ V0,
                                                           double* __restrict__ out, double alpha,
                                                           double c, double beta, int chunk,
                                                           double* __restrict__ partial) {
  constexpr int TR = kDiarRowsPerBlockMfma, JT = 64, LDM = JT + 4;
  __shared__ __align__(16) float Ms[TR * LDM];
  __shared__ __align__(16) double Vs[JT * kDiarB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * TR;
  const int j_begin = blockIdx.y * chunk, j_end = min(N, j_begin + chunk);
  const int lcol = tid & 63, lrow = tid >> 6;
  float mreg[16];
  double vreg[8];
  auto gload = [&](int j0) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = r0 + lrow + 4 * q, j = j0 + lcol;
      mreg[q] = (i < N && j < j_end) ? M[(long)i * N + j] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + kT * q, j = j0 + (e >> 5);
      vreg[q] = j < j_end ? V1[(long)j * kDiarB + (e & 31)] : 0.0;
    }
  };
  f64x4 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[t][r] = 0.0;
  if (j_begin < j_end) gload(j_begin);
  const int arow = wave * 16 + (lane & 15), kq = lane >> 4;
  for (int j0 = j_begin; j0 < j_end; j0 += JT) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16; ++q) Ms[(lrow + 4 * q) * LDM + lcol] = mreg[q];
#pragma unroll
    for (int q = 0; q < 8; ++q) Vs[tid + kT * q] = vreg[q];
    __syncthreads();
    if (j0 + JT < j_end) gload(j0 + JT);
#pragma unroll 4
    for (int jj = 0; jj < JT; jj += 4) {
      const double a = (double)Ms[arow * LDM + jj + kq];
      const double b0 = Vs[(jj + kq) * kDiarB + (lane & 15)];
      const double b1 = Vs[(jj + kq) * kDiarB + 16 + (lane & 15)];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc[1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = r0 + wave * 16 + kq + 4 * r;
    if (i >= N) continue;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const long at = (long)i * kDiarB + 16 * t + (lane & 15);
      if constexpr (DIRECT)
        out[at] = lap_epilogue(acc[t][r], deg[i], V1[at], V0, at, alpha, c, beta);
      else
        partial[(long)blockIdx.y * N * kDiarB + at] = acc[t][r];
    }
  }
}

__global__ __launch_bounds__(kT) void diar_lap_reduce_kernel(const double* __restrict__ partial,
                                                             int split,
                                                             const double* __restrict__ deg, int N,
                                                             const double* __restrict__ V1,
                                                             const double* __restrict__ V0,
                                                             double* __restrict__ out, double alpha,
                                                             double c, double beta) {
  const long at = (long)blockIdx.x * kT + threadIdx.x;
  if (at >= (long)N * kDiarB) return;
  double mv = 0.0;
  for (int s = 0; s < split; ++s) mv += partial[(long)s * N * kDiarB + at];
  out[at] = lap_epilogue(mv, deg[at / kDiarB], V1[at], V0, at, alpha, c, beta);
}

// ---- small reductions ----
// partial[blk][a][b] = sum over the workgroup's 256 rows of A[i][a] B[i][b], rows in order
__global__ __launch_bounds__(kT) void diar_gram_partial_kernel(const double* __restrict__ A,
                                                               const double* __restrict__ B, int N,
                                                               double* __restrict__ partial) {
  __shared__ double As[64 * kDiarB], Bs[64 * kDiarB];
  const int tid = threadIdx.x;
  const int a = tid >> 3, b0 = (tid & 7) * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int row0 = blockIdx.x * kDiarGramRows;
  for (int sub = 0; sub < kDiarGramRows; sub += 64) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = tid + kT * q, i = row0 + sub + (e >> 5);
      As[e] = i < N ? A[(long)i * kDiarB + (e & 31)] : 0.0;
      Bs[e] = i < N ? B[(long)i * kDiarB + (e & 31)] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < 64; ++r) {
      const double av = As[r * kDiarB + a];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = fma(av, Bs[r * kDiarB + b0 + q], acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) partial[(long)blockIdx.x * 1024 + a * kDiarB + b0 + q] = acc[q];
}

__global__ __launch_bounds__(kT) void diar_gram_reduce_kernel(const double* __restrict__ partial,
                                                              int nblk, double* __restrict__ G) {
  const int e = blockIdx.x * kT + threadIdx.x;  // < 1024
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(long)b * 1024 + e];
  G[e] = s;
}

// out[i][c] = sum_k A[i][k] RA[k][c] (+ sum_k B[i][k] RB[k][c]), 8 rows per workgroup
__global__ __launch_bounds__(kT) void diar_block_mul_kernel(const double* __restrict__ A,
                                                            const double* __restrict__ RA,
                                                            const double* __restrict__ B,
                                                            const double* __restrict__ RB, int N,
                                                            double* __restrict__ out) {
  __shared__ double Rs[2][kDiarB * kDiarB];
  __shared__ double Xs[2][8 * kDiarB];
  const int tid = threadIdx.x;
  const int r = tid >> 5, c = tid & 31;
  const int i = blockIdx.x * 8 + r;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    Rs[0][tid + kT * q] = RA[tid + kT * q];
    Rs[1][tid + kT * q] = B ? RB[tid + kT * q] : 0.0;
  }
  Xs[0][tid] = i < N ? A[(long)i * kDiarB + c] : 0.0;
  Xs[1][tid] = (B && i < N) ? B[(long)i * kDiarB + c] : 0.0;
  __syncthreads();
  double acc = 0.0;
#pragma unroll 8
  for (int k = 0; k < kDiarB; ++k) acc = fma(Xs[0][r * kDiarB + k], Rs[0][k * kDiarB + c], acc);
  if (B) {
#pragma unroll 8
    for (int k = 0; k < kDiarB; ++k) acc = fma(Xs[1][r * kDiarB + k], Rs[1][k * kDiarB + c], acc);
  }
  if (i < N) out[(long)i * kDiarB + c] = acc;
}

}  // namespace

void launch_diar_normalise(const float* X, int N, int D, float* Xn, int ldn, hipStream_t st) {
  ZASR_LAUNCH(diar_normalise_kernel, dim3(cdiv(N, kT / kWave)), dim3(kT), 0, st, X, N, D, Xn, ldn);
}

void launch_diar_similarity_plain(const float* Xn, int N, int D, int ldn, float* M,
                                  hipStream_t st) {
  ZASR_LAUNCH(diar_similarity_plain_kernel, dim3(cdiv(N, 16), cdiv(N, 16)), dim3(kT), 0, st, Xn, N,
              D, ldn, M);
}

void launch_diar_prune(float* M, int N, int keep, hipStream_t st) {
  ZASR_REQUIRE(keep >= 1 && keep <= N && N <= kDiarMaxN, "diar prune: keep outside [1, N]");
  if (keep == N) return;
  ZASR_LAUNCH(diar_prune_kernel, dim3(N), dim3(kT), (size_t)N * sizeof(float), st, M, N, keep);
}

void launch_diar_symmetrise(float* M, int N, hipStream_t st) {
  const int t = cdiv(N, 32);
  ZASR_LAUNCH(diar_symmetrise_kernel, dim3(t, t), dim3(kT), 0, st, M, N);
}

void launch_diar_degree(const float* M, int N, double* deg, hipStream_t st) {
  ZASR_LAUNCH(diar_degree_kernel, dim3(N), dim3(kT), 0, st, M, N, deg);
}

// ZASR_DIAR_LAP=fma | mfma picks the product kernel (development A/B; DESIGN.md 4f has both
// times); the default is the faster one
bool diar_lap_mfma() {
  static const bool on = [] {
    const char* e = getenv("ZASR_DIAR_LAP");
    return e == nullptr || std::string(e) != "fma";
  }();
  return on;
}

// column ranges per row tile: enough workgroups to fill the device twice over at small N
int diar_lap_split(int N) {
  const int tiles = cdiv(N, diar_lap_mfma() ? kDiarRowsPerBlockMfma : kDiarRowsPerBlock);
  int split = std::min(kDiarMaxSplit, std::max(1, cdiv(512, tiles)));
  split = std::min(split, cdiv(N, 64));
  const int chunk = cdiv(cdiv(N, split), 64) * 64;
  return cdiv(N, chunk);
}

void launch_diar_lap_block(const float* M, const double* deg, int N, const double* V1,
                           const double* V0, double* out, double alpha, double c, double beta,
                           int split, double* partial, hipStream_t st) {
  ZASR_REQUIRE(beta == 0.0 || V0 != nullptr, "diar lap: beta needs V0");
  const bool mfma = diar_lap_mfma();
  const int tiles = cdiv(N, mfma ? kDiarRowsPerBlockMfma : kDiarRowsPerBlock);
  if (split <= 1) {
    const int chunk = cdiv(N, 64) * 64;
    if (mfma)
      ZASR_LAUNCH((diar_lap_mfma_kernel<true>), dim3(tiles, 1), dim3(kT), 0, st, M, deg, N, V1, V0,
                  out, alpha, c, beta, chunk, partial);
    else
      ZASR_LAUNCH((diar_lap_kernel<true>), dim3(tiles, 1), dim3(kT), 0, st, M, deg, N, V1, V0, out,
                  alpha, c, beta, chunk, partial);
    return;
  }
  const int chunk = cdiv(cdiv(N, split), 64) * 64;
  ZASR_REQUIRE((long)chunk * split >= N && partial != nullptr, "diar lap: bad split");
  if (mfma)
    ZASR_LAUNCH((diar_lap_mfma_kernel<false>), dim3(tiles, split), dim3(kT), 0, st, M, deg, N, V1,
                V0, out, alpha, c, beta, chunk, partial);
  else
    ZASR_LAUNCH((diar_lap_kernel<false>), dim3(tiles, split), dim3(kT), 0, st, M, deg, N, V1, V0,
                out, alpha, c, beta, chunk, partial);
  ZASR_LAUNCH(diar_lap_reduce_kernel, dim3((unsigned)cdivl((long)N * kDiarB, kT)), dim3(kT), 0, st,
              partial, split, deg, N, V1, V0, out, alpha, c, beta);
}

void launch_diar_gram(const double* A, const double* B, int N, double* partial, double* G,
                      hipStream_t st) {
  const int nblk = cdiv(N, kDiarGramRows);
  ZASR_LAUNCH(diar_gram_partial_kernel, dim3(nblk), dim3(kT), 0, st, A, B, N, partial);
  ZASR_LAUNCH(diar_gram_reduce_kernel, dim3(1024 / kT), dim3(kT), 0, st, partial, nblk, G);
}

void launch_diar_block_mul(const double* A, const double* RA, const double* B, const double* RB,
                           int N, double* out, hipStream_t st) {
  ZASR_LAUNCH(diar_block_mul_kernel, dim3(cdiv(N, 8)), dim3(kT), 0, st, A, RA, B, RB, N, out);
}

}  // namespace zasr
