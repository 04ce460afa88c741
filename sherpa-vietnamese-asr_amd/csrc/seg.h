// PyanNet segmentation engine: the pyannote powerset segmentation network the
// reference's diarizer runs as its first stage through onnxruntime on the CPU
// (core/speaker_diarization_senko_campp_optimized.py:411-437: 10 s chunks every 5 s, 589 frames
// x 7 classes each), batched on MI355X.  Every chunk of a file is cut from the 16 kHz signal
// already in HBM; the sinc convolution, its pooling and the LSTM recurrence are kernels of
// their own (seg_kernels.hip), the other convolutions and every projection run on the exact-f32
// MFMA GEMM.  Decoding the class maps into speech / overlap regions stays host logic
// (zasr/segmentation.py).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace zasr {

// ---- kernels (seg_kernels.hip) ----
constexpr int kSegC0 = 80, kSegTaps = 251, kSegStride0 = 10;  // the sinc filter bank
constexpr int kSegH = 128, kSegClasses = 7;
constexpr int kSegMaxGroup = 16;  // sequences one recurrence workgroup can carry

// per-chunk mean and 1 / sqrt(var + eps) of the T samples at starts[k] (zeros past `total`),
// float64 sums in a fixed order -> stats[k] = (mean, rstd)
void launch_seg_chunk_stats(const float* audio, long total, const long* starts, int n, int T,
                            float2* stats, hipStream_t st);
struct SegFrontArgs {
  const float* audio;   // the 16 kHz signal
  long total;           // its length
  const long* starts;   // [n] first sample of each chunk
  const float2* stats;  // [n] (mean, rstd) of each chunk
  float in_w, in_b;     // the input InstanceNorm's affine
  const float* w0t;     // [251][80] sinc filter bank, tap-major
  float* out;           // [n][F1][80] max_3 |conv|
  int T, F1;
};
void launch_seg_front(const SegFrontArgs& a, int n, hipStream_t st);
// out[n][p][c] = max(x[n][3p .. 3p + 2][c]),  x [n][L][C], out [n][Fp][C], C % 4 == 0
// (max_blocks > 0 caps the grid of the grid-stride kernels; 0 = one thread per float4 up to 65536
// blocks, what the engine launches)
void launch_seg_pool3(const float* x, int n, int L, int C, int Fp, float* out, hipStream_t st,
                      int max_blocks = 0);
// InstanceNorm statistics over the F frames of x [n][F][C] (C <= 128): stats[n][c] = (mean, rstd)
void launch_seg_frame_stats(const float* x, int n, int F, int C, float2* stats, hipStream_t st);
// x = leaky_relu(((x - mean) * rstd) * w[c] + b[c]) in place
void launch_seg_norm_act(float* x, int n, int F, int C, const float2* stats, const float* w,
                         const float* b, hipStream_t st, int max_blocks = 0);
struct SegLstmArgs {
  const float* gx;   // [n * F][1024] x W_ih^T + b_ih + b_hh, forward gates | backward gates
  const float* whh;  // [2][512][128]
  float* out;        // [n * F][256] forward h | backward h
  int n, F;
};
// one layer, both directions; `group` sequences of one direction per workgroup
// (1, 2, 4, 8 or 16); a sequence's result does not depend on the group or its place in it
void launch_seg_lstm(const SegLstmArgs& a, int group, hipStream_t st);
// classifier + log_softmax + argmax (lowest index on ties) of x [rows][128]
void launch_seg_head(const float* x, long rows, const float* w, const float* b, float* logits,
                     unsigned char* classes, hipStream_t st);

// the kernels above alone, one launch function per entry on host operands (selftest.cpp;
// include/zasr.h zasr_selftest_seg_*): every output in / out, guarded
void selftest_seg_chunk_stats(long total, int n, int T, const float* audio, const long* starts,
                              float* stats);
void selftest_seg_front(long total, int n, int T, const float* audio, const long* starts,
                        const float* stats, float in_w, float in_b, const float* w0t, float* out);
void selftest_seg_pool3(int n, int L, int C, int Fp, int max_blocks, const float* x, float* out);
void selftest_seg_frame_stats(int n, int F, int C, const float* x, float* stats);
void selftest_seg_norm_act(int n, int F, int C, int max_blocks, const float* stats, const float* w,
                           const float* b, float* x);
void selftest_seg_lstm(int n, int F, int group, const float* gx, const float* whh, float* out);
void selftest_seg_head(long rows, const float* x, const float* w, const float* b, float* logits,
                       unsigned char* classes);

class SegEngine {
 public:
  SegEngine(const std::string& model_dir, int device);
  ~SegEngine();
  // frames the network gives for T samples (589 at 160000); 0 when T is too short
  static int num_frames(long T);
  static constexpr int kMinSamples = 1261;  // num_frames >= 2
  // chunk starts of a file (reference :418-424)
  static std::vector<long> chunk_starts(long total, long chunk, long step);
  // the ORT session's surface: batch [n][T] (host) -> logits [n][F][7] (host)
  void logits_host(const float* batch, int n, int T, float* logits);
  // every chunk of the signal d_audio[0, total): classes (host) [n_chunks][F]; d_logits
  // (device, [n_chunks][F][7]) may be null.  Ordered after user_stream's work when given;
  // synchronises before returning (classes are host memory).
  void classes_device(const float* d_audio, long total, int chunk, int step,
                      unsigned char* classes, float* d_logits, hipStream_t user_stream);
  // release the activation workspace (it otherwise stays as large as the longest file seen)
  void trim();
  // diagnostics: the recurrence group size of the last launch; a forced one (0 = automatic)
  int last_group() const { return last_group_; }
  void set_group(int g) { forced_group_ = g; }
  // diagnostics: with profiling on, every call times its stages on HIP events (front, convs,
  // projections, recurrence, head: ms summed over the call's launch groups)
  void set_profile(bool on) { profile_ = on; }
  const float* stage_ms() const { return stage_ms_; }
  static constexpr int kStages = 5;
  std::mutex mu;

 private:
  struct Lin {
    float* w = nullptr;
    float* b = nullptr;
    int N = 0, K = 0;
  };
  struct Norm {
    float* w = nullptr;
    float* b = nullptr;
  };
  template <class T>
  T* ws(const std::string& name, size_t count) {
    return ws_.get<T>(name, count, &st_);
  }
  // chunks starts[k0, k0 + ng) of the signal -> d_logits / d_classes rows of those chunks
  void run_group(const float* d_audio, long total, const long* d_starts, int ng, int T,
                 float* d_logits, unsigned char* d_classes);
  void run(const float* d_audio, long total, const std::vector<long>& starts, int T,
           float* d_logits, unsigned char* d_classes);
  int pick_group(int n) const;
  void mark(int stage);  // the stream's work since the previous mark belongs to `stage`
  void collect_marks();
  static size_t chunk_bytes(int T);

  int device_ = 0, cus_ = 256, last_group_ = 0, forced_group_ = 0;
  hipStream_t st_ = nullptr;
  bool profile_ = false;
  float stage_ms_[kStages] = {0.f, 0.f, 0.f, 0.f, 0.f};
  std::vector<std::pair<hipEvent_t, int>> marks_;
  float in_w_ = 1.f, in_b_ = 0.f;
  float* w0t_ = nullptr;
  Norm norm_[3];
  Lin conv_[2];
  Lin ih_[4];
  float* whh_[4] = {nullptr, nullptr, nullptr, nullptr};
  Lin lin_[2], cls_;
  DeviceStore store_;
  Workspace ws_;
};

}  // namespace zasr
