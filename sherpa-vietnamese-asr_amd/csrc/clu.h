// Centroid-linkage agglomerative clustering on the device: the flat clustering of
//   fcluster(linkage(Xn, "centroid", "euclidean"), threshold, "distance")
// of the community-1 diarizer (core/speaker_diarization_pure_ort.py:918-921).  DESIGN.md 4j has
// the algorithm and the argument for the stopping rule.
//
//   normalise  Xn = X / (|X|_2 + 1e-10) row-wise in float32 (:918)
//   pairwise   Dm[i][j] = |Xn_i - Xn_j|_2 from float64 differences, +inf on the diagonal
//   nn         per row the nearest live column (lowest column on ties)
//   merge      one workgroup, workgroup barriers only: the globally closest live pair (i < j)
//              merges into slot i by scipy's Lance-Williams centroid update on plain distances,
//              column j dies (+inf).  A row whose nearest neighbour was i or j keeps its old
//              minimum as a lower bound when the new cluster is farther, and is rescanned (one
//              wave per row) only once that bound could be the global minimum.  The loop ends
//              at the first minimum above the threshold.
//
// A cluster lives in the slot of its lowest member row, so the labels number the clusters by
// lowest member.  No floating-point atomics; every minimum breaks ties by a fixed rule (the
// lowest index in every scan; a cached minimum met exactly by the new cluster moves to it), so
// the labels are bit-identical from run to run and between the two workgroup sizes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "device_mem.h"

namespace zasr {

constexpr int kCluMinN = 2, kCluMaxN = 16384, kCluMaxD = 512;
constexpr int kCluStages = 4;  // upload + normalise, pairwise, nearest neighbours, merge loop
constexpr int kCluRoutes = 2;  // merge loop in a workgroup of 1024 (route 0) or 256 threads

// ---- kernels (clu_kernels.hip) ----
// Dm [N][N] float64 from Xn [N][ldn] (columns past D are zero, ldn % 4 == 0)
void launch_clu_pairwise(const float* Xn, int N, int D, int ldn, double* Dm, hipStream_t st);
// nn_dist / nn_idx [N]: the row minima of Dm; size[i] = 1, parent[i] = -1, stats[0..1] = 0
void launch_clu_nn_init(const double* Dm, int N, double* nn_dist, int* nn_idx, int* size,
                        int* parent, long long* stats, hipStream_t st);
// the merge loop; parent[j] = the slot j merged into (lower than j), -1 for a live cluster;
// stats[0] = merges, stats[1] = rows rescanned
void launch_clu_merge(double* Dm, int N, double threshold, double* nn_dist, int* nn_idx, int* size,
                      int* parent, long long* stats, int route, hipStream_t st);

class CluEngine {
 public:
  explicit CluEngine(int device);
  // labels [N] on the host; synchronises `st`
  void ahc(const float* X, bool x_on_device, int N, int D, double threshold, int32_t* labels,
           hipStream_t st);
  void set_profile(bool on) { profile_ = on; }
  const float* stage_ms() const { return ms_; }
  void set_route(int route) { route_ = route; }
  long long last_merges = 0, last_rescans = 0;
  std::mutex mu;

 private:
  int device_ = 0;
  int route_ = 0;
  bool profile_ = false;
  float ms_[kCluStages] = {0, 0, 0, 0};
  Workspace ws_;
};

}  // namespace zasr
