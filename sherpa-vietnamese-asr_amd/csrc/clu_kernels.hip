// Kernels of the centroid-linkage clustering (clu.h): the float64 pairwise distances, the
// nearest-neighbour cache and the merge loop.  Minima only, every tie broken by a fixed rule
// (the lowest index, except as noted in the merge loop): no sum whose order could vary, no
// floating-point atomics.  The object is built with
// -ffp-contract=off so that the Lance-Williams update rounds as scipy's C code does.
#include <climits>

#include "clu.h"
#include "common.h"

namespace zasr {

namespace {

constexpr int kT = 256;
constexpr int kTile = 32;  // outputs per side of one pairwise workgroup

__device__ __forceinline__ double clu_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// (d, i) <- the smaller of the wave's pairs, the lowest index among equal distances
__device__ __forceinline__ void wave_argmin(double& d, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(d, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (od < d || (od == d && oi < i)) {
      d = od;
      i = oi;
    }
  }
}

// one 32 x 32 tile of Dm per workgroup, 2 x 2 outputs per thread; the sum over the columns runs
// in column order for both (i, j) and (j, i), so Dm is symmetric to the bit
__global__ __launch_bounds__(kT) void clu_pairwise_kernel(const float* __restrict__ Xn, int N,
                                                          int D, int ldn,
                                                          double* __restrict__ Dm) {
  __shared__ float As[kTile][kTile + 1];
  __shared__ float Bs[kTile][kTile + 1];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
  for (int k0 = 0; k0 < D; k0 += kTile) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + kT * q;
      const int r = e >> 5, c = e & 31;
      const int k = k0 + c;
      As[r][c] = (i0 + r < N && k < D) ? Xn[(size_t)(i0 + r) * ldn + k] : 0.f;
      Bs[r][c] = (j0 + r < N && k < D) ? Xn[(size_t)(j0 + r) * ldn + k] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < kTile; ++kk) {
      const double a0 = As[ty][kk], a1 = As[ty + 16][kk];
      const double b0 = Bs[tx][kk], b1 = Bs[tx + 16][kk];
      double d;
      d = a0 - b0; acc[0][0] = fma(d, d, acc[0][0]);
      d = a0 - b1; acc[0][1] = fma(d, d, acc[0][1]);
      d = a1 - b0; acc[1][0] = fma(d, d, acc[1][0]);
      d = a1 - b1; acc[1][1] = fma(d, d, acc[1][1]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
      if (i < N && j < N) Dm[(size_t)i * N + j] = i == j ? clu_inf() : sqrt(acc[u][v]);
    }
}

// the minimum of row `row` of Dm over all columns, one wave; dead columns and the diagonal
// hold +inf.  idx = -1 when the row has no finite entry.
__device__ __forceinline__ void clu_row_min(const double* Dm, int N, int row, int lane, double& d,
                                            int& idx) {
  const double* p = Dm + (size_t)row * N;
  d = clu_inf();
  idx = INT_MAX;
  for (int c = lane; c < N; c += kWave) {
    const double v = p[c];
    if (v < d) {
      d = v;
      idx = c;
    }
  }
  wave_argmin(d, idx);
  if (idx == INT_MAX) idx = -1;
}

__global__ __launch_bounds__(kT) void clu_nn_init_kernel(const double* __restrict__ Dm, int N,
                                                         double* __restrict__ nn_dist,
                                                         int* __restrict__ nn_idx,
                                                         int* __restrict__ size,
                                                         int* __restrict__ parent,
                                                         long long* __restrict__ stats) {
  const int row = blockIdx.x * (kT / kWave) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x < 2) stats[threadIdx.x] = 0;
  if (row >= N) return;
  double d;
  int idx;
  clu_row_min(Dm, N, row, lane, d, idx);
  if (lane == 0) {
    nn_dist[row] = d;
    nn_idx[row] = idx;
    size[row] = 1;
    parent[row] = -1;
  }
}

constexpr int kCluStale = -2;  // nn_idx of a live row whose nn_dist is only a lower bound

// (d, i) <- the workgroup's smallest pair, in every thread.  One barrier inside; the caller
// keeps another barrier between two uses of the same s_d / s_i.
template <int W>
__device__ __forceinline__ void block_argmin(double& d, int& i, double* s_d, int* s_i, int lane,
                                             int wave) {
  wave_argmin(d, i);
  if (lane == 0) {
    s_d[wave] = d;
    s_i[wave] = i;
  }
  __syncthreads();
  d = s_d[0];
  i = s_i[0];
#pragma unroll
  for (int w = 1; w < W; ++w) {
    const double od = s_d[w];
    const int oi = s_i[w];
    if (od < d || (od == d && oi < i)) {
      d = od;
      i = oi;
    }
  }
}

// the smallest exact row minimum: rows with nn_idx >= 0 (dead rows hold -1 and +inf)
template <int T>
__device__ __forceinline__ void clu_fresh_min(const double* nn_dist, const int* nn_idx, int N,
                                              int tid, double& bd, int& bi) {
  bd = clu_inf();
  bi = INT_MAX;
  for (int k = tid; k < N; k += T) {
    const double d = nn_dist[k];
    if (nn_idx[k] >= 0 && d < bd) {
      bd = d;
      bi = k;
    }
  }
}

// The merge loop in ONE workgroup of T threads: four to six workgroup barriers per merge, no
// inter-workgroup communication.  Global memory written by one wave is read by another only
// across a __syncthreads() (workgroup-scope release / acquire; the waves share the CU's L1).
//
// Row minima are kept lazily, as scipy's own nearest-neighbour candidates are: when a row's
// nearest neighbour is merged away and the new cluster is farther than the old minimum, the old
// minimum stays as a lower bound (every other entry of the row is unchanged and was no smaller)
// and the row is marked stale.  A stale row is rescanned only when its bound could win: when it
// is not above the smallest exact minimum.
template <int T>
__global__ __launch_bounds__(T) void clu_merge_kernel(double* Dm, int N, double threshold,
                                                      double* nn_dist, int* nn_idx, int* size,
                                                      int* parent, long long* stats) {
  constexpr int W = T / kWave;
  __shared__ double s_d[W], s_d2[W];
  __shared__ int s_i[W], s_i2[W];
  __shared__ unsigned short s_list[kCluMaxN];  // rows to rescan this step (N <= 16384 < 65536)
  __shared__ int s_count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double inf = clu_inf();
  long long merges = 0, rescans = 0;
  for (int step = 0; step < N - 1; ++step) {
    // 1. the globally closest live pair: the smallest exact row minimum, after the stale rows
    // whose bound does not exceed it have been rescanned (one wave per row)
    double bd;
    int bi;
    if (tid == 0) s_count = 0;
    clu_fresh_min<T>(nn_dist, nn_idx, N, tid, bd, bi);
    block_argmin<W>(bd, bi, s_d, s_i, lane, wave);
    for (int k = tid; k < N; k += T)
      if (nn_idx[k] == kCluStale && nn_dist[k] <= bd) s_list[atomicAdd(&s_count, 1)] = (unsigned short)k;
    __syncthreads();
    const int cnt = s_count;
    if (cnt > 0) {  // uniform
      for (int r = wave; r < cnt; r += W) {
        const int k = s_list[r];
        double d;
        int idx;
        clu_row_min(Dm, N, k, lane, d, idx);
        if (lane == 0) {
          nn_dist[k] = d;
          nn_idx[k] = idx;
        }
      }
      rescans += cnt;
      __syncthreads();
      clu_fresh_min<T>(nn_dist, nn_idx, N, tid, bd, bi);
      block_argmin<W>(bd, bi, s_d, s_i, lane, wave);
    }
    if (bi == INT_MAX || !(bd <= threshold)) break;  // uniform: every thread reduced the same pairs
    const int other = nn_idx[bi];
    if (other < 0 || other >= N) break;  // cannot happen for finite rows; keeps every index in range
    const int i = bi < other ? bi : other, j = bi < other ? other : bi;
    const double ni = (double)size[i], nj = (double)size[j], nij = ni + nj;
    const double dij = bd;
    double* rowi = Dm + (size_t)i * N;
    double* rowj = Dm + (size_t)j * N;

    // 2. slot i becomes the merged cluster, slot j dies
    double nd = inf;
    int nk = INT_MAX;
    for (int k = tid; k < N; k += T) {
      const double dki = rowi[k];
      if (k == j || dki == inf) continue;  // the partner, the diagonal and dead columns
      const double dkj = rowj[k];
      // scipy _hierarchy _centroid, on plain distances
      double v = (((ni * dki * dki) + (nj * dkj * dkj)) - (ni * nj * dij * dij) / nij) / nij;
      v = sqrt(v > 0.0 ? v : 0.0);
      rowi[k] = v;
      Dm[(size_t)k * N + i] = v;
      rowj[k] = inf;
      Dm[(size_t)k * N + j] = inf;
      const int nb = nn_idx[k];
      const double cur = nn_dist[k];
      if (nb == i || nb == j || nb == kCluStale) {
        // every other entry of row k is at least cur: v <= cur is the new minimum exactly,
        // otherwise cur stays as a lower bound.  At v == cur a lower column may hold the same
        // value: the neighbour becomes i, not the lowest tied column -- a fixed rule all the
        // same, so the result does not depend on the route or the run
        if (v <= cur) {
          nn_dist[k] = v;
          nn_idx[k] = i;
        } else {
          nn_idx[k] = kCluStale;
        }
      } else if (v < cur || (v == cur && i < nb)) {
        nn_dist[k] = v;
        nn_idx[k] = i;
      }
      if (v < nd) {
        nd = v;
        nk = k;
      }
    }
    block_argmin<W>(nd, nk, s_d2, s_i2, lane, wave);
    if (tid == 0) {
      nn_dist[i] = nd;
      nn_idx[i] = nk == INT_MAX ? -1 : nk;
      nn_dist[j] = inf;
      nn_idx[j] = -1;
      size[i] = (int)nij;
      size[j] = 0;
      parent[j] = i;
      rowi[j] = inf;
      rowj[i] = inf;
    }
    ++merges;
    __syncthreads();
  }
  if (tid == 0) {
    stats[0] = merges;
    stats[1] = rescans;
  }
}

}  // namespace

void launch_clu_pairwise(const float* Xn, int N, int D, int ldn, double* Dm, hipStream_t st) {
  ZASR_LAUNCH(clu_pairwise_kernel, dim3(cdiv(N, kTile), cdiv(N, kTile)), dim3(kT), 0, st, Xn, N, D,
              ldn, Dm);
}

void launch_clu_nn_init(const double* Dm, int N, double* nn_dist, int* nn_idx, int* size,
                        int* parent, long long* stats, hipStream_t st) {
  ZASR_LAUNCH(clu_nn_init_kernel, dim3(cdiv(N, kT / kWave)), dim3(kT), 0, st, Dm, N, nn_dist,
              nn_idx, size, parent, stats);
}

void launch_clu_merge(double* Dm, int N, double threshold, double* nn_dist, int* nn_idx, int* size,
                      int* parent, long long* stats, int route, hipStream_t st) {
  ZASR_REQUIRE(N >= kCluMinN && N <= kCluMaxN, "clu merge: N outside [2, 16384]");
  ZASR_REQUIRE(route >= 0 && route < kCluRoutes, "clu merge: unknown route");
  if (route == 0)
    ZASR_LAUNCH(clu_merge_kernel<1024>, dim3(1), dim3(1024), 0, st, Dm, N, threshold, nn_dist,
                nn_idx, size, parent, stats);
  else
    ZASR_LAUNCH(clu_merge_kernel<256>, dim3(1), dim3(256), 0, st, Dm, N, threshold, nn_dist, nn_idx,
                size, parent, stats);
}

}  // namespace zasr
