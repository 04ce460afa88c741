// Host driver of the centroid-linkage clustering (clu.h).
#include "clu.h"

#include <vector>

#include "diar.h"

namespace zasr {

namespace {

// the stage events of one profiled call, destroyed on every way out of it (create() runs on
// the finished object, so a failed create frees the events made before it as well)
struct StageEvents {
  hipEvent_t ev[kCluStages + 1] = {};
  bool on = false;
  StageEvents() = default;
  StageEvents(const StageEvents&) = delete;
  StageEvents& operator=(const StageEvents&) = delete;
  void create() {
    on = true;
    for (auto& e : ev) ZASR_HIP_CHECK(hipEventCreate(&e));
  }
  ~StageEvents() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

CluEngine::CluEngine(int device) : device_(device) {
  int n = 0;
  ZASR_HIP_CHECK(hipGetDeviceCount(&n));
  ZASR_REQUIRE(device >= 0 && device < n, "clu: device id out of range");
  ZASR_HIP_CHECK(hipSetDevice(device));
}

void CluEngine::ahc(const float* X, bool x_on_device, int N, int D, double threshold,
                    int32_t* labels, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_REQUIRE(N >= kCluMinN && N <= kCluMaxN && D >= 1 && D <= kCluMaxD, "clu ahc: shape");
  StageEvents events;
  if (profile_) events.create();
  auto mark = [&](int i) {
    if (events.on) ZASR_HIP_CHECK(hipEventRecord(events.ev[i], st));
  };
  mark(0);
  const float* dX = X;
  if (!x_on_device) {
    float* up = ws_.get<float>("x", (size_t)N * D, &st);
    ZASR_HIP_CHECK(hipMemcpyAsync(up, X, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipStreamSynchronize(st));  // the caller's buffer is free on return
    dX = up;
  }
  const int ldn = cdiv(D, 4) * 4;
  float* xn = ws_.get<float>("xn", (size_t)N * ldn, &st);
  double* dm = ws_.get<double>("dm", (size_t)N * N, &st);
  double* nn_dist = ws_.get<double>("nn_dist", (size_t)N, &st);
  int* nn_idx = ws_.get<int>("nn_idx", (size_t)N, &st);
  int* size = ws_.get<int>("size", (size_t)N, &st);
  int* parent = ws_.get<int>("parent", (size_t)N, &st);
  long long* stats = ws_.get<long long>("stats", 2, &st);
  launch_diar_normalise(dX, N, D, xn, ldn, st);  // :918, the same float32 rule as §4f's
  mark(1);
  launch_clu_pairwise(xn, N, D, ldn, dm, st);
  mark(2);
  launch_clu_nn_init(dm, N, nn_dist, nn_idx, size, parent, stats, st);
  mark(3);
  launch_clu_merge(dm, N, threshold, nn_dist, nn_idx, size, parent, stats, route_, st);
  mark(4);
  std::vector<int> hparent(N);
  long long hstats[2] = {0, 0};
  ZASR_HIP_CHECK(hipMemcpyAsync(hparent.data(), parent, (size_t)N * sizeof(int),
                                hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipMemcpyAsync(hstats, stats, sizeof(hstats), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  if (events.on)
    for (int i = 0; i < kCluStages; ++i)
      ZASR_HIP_CHECK(hipEventElapsedTime(&ms_[i], events.ev[i], events.ev[i + 1]));
  last_merges = hstats[0];
  last_rescans = hstats[1];
  // a slot merges into a lower one, so one ascending pass finds every root; the clusters are
  // numbered by their root, which is their lowest member row
  int next = 0;
  for (int k = 0; k < N; ++k) {
    const int p = hparent[k];
    ZASR_REQUIRE(p < k, "clu ahc: a merge into a higher slot");
    labels[k] = p < 0 ? next++ : labels[p];
  }
}

}  // namespace zasr
