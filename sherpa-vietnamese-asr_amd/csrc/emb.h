// Community-1 speaker-embedding engine: the stage the reference's production
// diarizer runs through onnxruntime (core/speaker_diarization_pure_ort.py:769-879 and :681-707)
// -- kaldi fbank of the whole signal, a 998-frame window and CMVN per 10 s chunk, the WeSpeaker
// ResNet34 encoder, masked statistics pooling per (chunk, local speaker) and the 5120 -> 256
// projection -- on MI355X, from the signal in HBM to embeddings [chunks][3][256].  Clustering
// (AHC, PLDA, VBx) and the reconstruction stay with the caller.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace zasr {

// ---- kernels (emb_kernels.hip) ----
// One convolution on channels-last activations: y[n][Fo][To][Co] = epi(conv(x[n][Fi][Ti][Ci])),
// w [Co][(r ks + q) Ci + ci] (r over F, q over T), pad 1 (ks 3) or 0 (ks 1), the same stride on
// both axes, epi: + bias[co], then + res (nullable, the output's shape), then ReLU when relu.
struct EmbConv2d {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;
  float* y;
  int n, Fi, Ti, Ci, Fo, To, Co, ks, stride, relu;
};
// routes that take Co channels: 1 (32 channels per block), 2 (64, Co >= 64)
int emb_conv2d_routes(int Co);
// route 0: the engine's pick (the widest the layer takes)
void launch_emb_conv2d(const EmbConv2d& a, int route, hipStream_t st);
// the stem: Conv2d(1, Co, 3, pad 1) + bias + ReLU on x [n][T][F] -> y [n][F][T][Co], w [Co][9]
void launch_emb_stem(const float* x, const float* w, const float* bias, int n, int T, int F,
                     int Co, float* y, hipStream_t st);
// stats [n S][2 C F] = [mean | std] of x [n][F][T][C] under mask [n][S][nseg] (uint8), feature
// j = c F + f; pop: unmasked, population variance (mask ignored)
void launch_emb_pool(const float* x, const unsigned char* mask, int n, int F, int T, int C, int S,
                     int nseg, bool pop, float* stats, hipStream_t st);
// out [n][C F][T] (feature c F + f) of x [n][F][T][C]
void launch_emb_to_cft(const float* x, int n, int F, int T, int C, float* out, hipStream_t st);

// kernel self-tests on host operands (selftest.cpp; zasr_selftest_emb_*)
void selftest_emb_conv2d(int ks, int stride, int ci, int co, int n, int fi, int ti, int relu,
                         int route, const float* x, const float* w, const float* bias,
                         const float* res, float* y, int* n_routes);
void selftest_emb_pool(int n, int F, int T, int C, int S, int nseg, int pop, const float* x,
                       const unsigned char* mask, float* stats);

class EmbEngine {
 public:
  EmbEngine(const std::string& model_dir, int device);
  ~EmbEngine();
  static constexpr int kStages = 8;  // fbank + windows, stem, layer1 .. layer4, pooling, projection
  static constexpr int kSpeakers = 3;      // MAX_SPEAKERS_PER_CHUNK
  static constexpr int kChunkFrames = 998; // :801
  static constexpr int kTail = 160000;     // the zeros appended to the signal (:812)
  static constexpr int kMaxGroup = 128;
  int embed_dim() const { return emb_; }
  int feat_dim() const { return feat_; }
  int stat_dim() const { return 2 * 8 * m_ * bins_out(); }
  int bins_out() const { return down3(feat_); }
  static int down3(int n) { return (((n - 1) / 2 + 1 - 1) / 2 + 1 - 1) / 2 + 1; }
  int num_feat_frames(int T) const { return T >= 1 ? down3(T) : 0; }
  static long fbank_rows(long n, long tail) { return n + tail >= 400 ? 1 + (n + tail - 400) / 160 : 0; }
  // multiply-adds x 2 of the encoder on n inputs of T frames
  double encoder_flops(int T) const;
  // fbank rows (no CMVN) of wav[0, n) followed by `tail` zeros, host in / out
  void fbank_host(const float* wav, long n, long tail, float* out);
  // feats [n][T][feat] (host) -> frame features [n][C F][T'] (host)
  void encode_host(const float* feats, int n, int T, float* out);
  // chunks at starts[c] of the signal d_wav[0, total) in HBM, masks uint8 [n][3][nseg] (host)
  // -> out [n][3][embed] (host).  Ordered after user_stream's work when given.
  void chunks_device(const float* d_wav, long total, const long* starts, int n_chunks,
                     const unsigned char* masks, int nseg, float* out, hipStream_t user_stream);
  // one segment (host samples): its own fbank + CMVN, the encoder at that T, unmasked pooling,
  // the projection; false ("too short") under 9 fbank frames; at most 2^20 frames (2.9 h)
  bool segment_host(const float* wav, long n, float* out);
  void trim();
  void set_group(int g) { group_ = g; }
  int last_group() const { return last_group_; }
  void set_profile(bool on) { profile_ = on; }
  const float* stage_ms() const { return stage_ms_; }
  // activation bytes of one input of T frames in a launch group
  size_t input_bytes(int T) const;
  std::mutex mu;

 private:
  struct Conv {
    float* w = nullptr;
    float* b = nullptr;
    int ci = 0, co = 0, ks = 3, stride = 1;
  };
  struct Block {
    Conv a, b, sc;
    bool has_sc = false;
    int layer = 0;  // 0 .. 3: the stage the block belongs to
  };
  template <class T>
  T* ws(const std::string& name, size_t count) {
    return ws_.get<T>(name, count, &st_);
  }
  // feats [n][T][feat] on the device -> the last layer's output [n][F'][T'][C] (workspace)
  const float* encode(const float* d_feats, int n, int T);
  void fbank_device(const float* d_wav, long n, long rows, float* d_rows);
  int pick_group(int n, int T) const;
  void mark(int stage);
  void collect_marks();
  void wait_for(hipStream_t user_stream);

  int device_ = 0;
  hipStream_t st_ = nullptr;
  bool profile_ = false;
  float stage_ms_[kStages] = {};
  std::vector<std::pair<hipEvent_t, int>> marks_;
  int group_ = 0, last_group_ = 0;
  int feat_ = 80, m_ = 32, emb_ = 256;
  std::vector<int> num_blocks_;
  Conv stem_;
  std::vector<Block> blocks_;
  float *seg_w_ = nullptr, *seg_b_ = nullptr;
  long fb_off_h_ = 0;             // host sources of fbank_device's asynchronous uploads
  int fb_meta_h_[3] = {0, 0, 0};
  double* d_twiddle_ = nullptr;
  float* d_window_ = nullptr;
  int* d_mel_meta_ = nullptr;
  float* d_mel_w_ = nullptr;
  DeviceStore store_;
  Workspace ws_;
};

}  // namespace zasr
