// Conv-TasNet overlap separation engine: the two-speaker separation network the
// reference runs once per overlap region, batch 1, through onnxruntime on the CPU
// (core/overlap_separator.py:281-296), batched on MI355X.  The regions of a call are
// concatenated raggedly in a time-major [frames][channels] layout, so every 1x1 convolution
// (and the encoder and decoder filter banks) is one exact-f32 MFMA GEMM over all regions'
// frames; the global layer norms and the dilated depthwise convolution, the only operators that
// see region boundaries, are kernels of their own (sep_kernels.hip).  Matching streams to
// speakers, the context audio and the second decode stay host logic (zasr/overlap.py).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "device_mem.h"

namespace zasr {

// ---- kernels (sep_kernels.hip) ----
constexpr int kSepTile = 32;  // frames of one tile: the unit of the norms' partial sums

// one tile of at most kSepTile frames of one region; tiles never straddle regions
struct SepTile {
  int row0;    // first row of the tile in the ragged [sum F][.] buffers
  int f0;      // its frame within the region
  int F;       // frames of the region
  int region;  // its region, numbered over the whole call (not within the launch group)
};
struct SepRegion {
  long sig_off;  // first sample of the region in the signal
  long out_off;  // first element of its [2][T] output
  int T, F;
  int row0;      // first row of the region
  int tile0;     // first tile of the region
};

// a launch group: consecutive regions of a call, their tiles and rows
struct SepGroup {
  int region0 = 0, n_regions = 0, tile0 = 0, n_tiles = 0, max_T = 0;
  long rows = 0;
};
// The tables of the launch group regions[r0, r0 + ng) (T and F given): sets every region's row0
// and tile0, both relative to the group, and appends the group's tiles to `tiles` (a tile's
// `region` is the index in `regions`, its row0 relative to the group).  The group's tiles start
// at tiles[tile0]: groups are appended in call order.  sep.cpp.
SepGroup sep_fill_group(std::vector<SepRegion>& regions, int r0, int ng, std::vector<SepTile>& tiles);

// frames[row][k] = signal[sig_off + 16 f + k], k < 32: the encoder GEMM's A rows
void launch_sep_frames(const float* signal, const SepRegion* regions, const SepTile* tiles,
                       int n_tiles, int win, int hop, float* frames, hipStream_t st);
// per-tile float64 (sum, sum of squares) of x [rows][C] (row stride C, C % 4 == 0)
void launch_sep_tile_sums(const float* x, int C, const SepTile* tiles, int n_tiles,
                          double2* partial, hipStream_t st);
// per-region (mean, rstd) from its tiles' partial sums, added in tile order
void launch_sep_region_stats(const double2* partial, const SepRegion* regions, int n_regions, int C,
                             float2* stats, hipStream_t st);
// dst = (src - mean) * rstd * gamma[c] + beta[c]  (dst may be src)
void launch_sep_gln_apply(const float* src, float* dst, int C, const SepTile* tiles, int n_tiles,
                          const float2* stats, const float* gamma, const float* beta,
                          hipStream_t st);
struct SepMidArgs {
  const float* h;       // [rows][C] the 1x1 convolution's output after its PReLU
  float* y;             // [rows][C] PReLU(depthwise(gLN(h)) + bias)
  const float2* stats;  // [regions] (mean, rstd) of h
  const float* gamma;   // [C] the first gLN's affine
  const float* beta;
  const float* w;       // [3][C] depthwise taps, tap-major
  const float* bias;    // [C]
  float slope;          // the second PReLU
  int C, dil;
  double2* partial;     // [tiles] (sum, sum of squares) of y: the second gLN's statistics
};
void launch_sep_mid(const SepMidArgs& a, const SepTile* tiles, int n_tiles, hipStream_t st);
// x[row][c] = prelu(x[row][c]) for c < C, row stride ld (C % 4 == 0, ld % 4 == 0); max_blocks > 0
// caps the grid-stride launch (0 = one thread per float4 up to 65536 blocks, the engine's)
void launch_sep_prelu(float* x, long rows, int C, int ld, float slope, hipStream_t st,
                      int max_blocks = 0);
// overlap-add of the decoder GEMMs' [rows][win] frames (win = 2 hop, at most 65535 regions):
// out[r][s][t], exact zeros past the last frame's end
void launch_sep_overlap_add(const float* dec0, const float* dec1, const SepRegion* regions,
                            int n_regions, int max_T, int win, int hop, float* out,
                            hipStream_t st);

// the kernels above alone, one launch function per entry on host operands (selftest.cpp;
// include/zasr.h zasr_selftest_sep_*): every output in / out, guarded.  A call's regions are given
// as (sig_off, T) each, F = (T - win) / hop + 1; the entry runs the launch group [r0, r0 + ng) on
// the tables sep_fill_group makes for the groups [0, r0) and [r0, r0 + ng).
struct SepSelftestCall {
  int n_regions;
  const long* sig_off;
  const int* T;
  int r0, ng, win, hop;
};
void selftest_sep_frames(const SepSelftestCall& c, long n_signal, const float* signal, float* frames);
void selftest_sep_tile_sums(const SepSelftestCall& c, int C, const float* x, double* partial);
void selftest_sep_region_stats(const SepSelftestCall& c, int C, const double* partial, float* stats);
void selftest_sep_gln_apply(const SepSelftestCall& c, int C, int in_place, const float* stats,
                            const float* gamma, const float* beta, const float* src, float* dst);
void selftest_sep_mid(const SepSelftestCall& c, int C, int dil, float slope, const float* stats,
                      const float* gamma, const float* beta, const float* w, const float* bias,
                      const float* h, float* y, double* partial);
void selftest_sep_prelu(long rows, int C, int ld, int col0, float slope, int max_blocks, float* x);
void selftest_sep_overlap_add(const SepSelftestCall& c, const long* out_off, long n_out,
                              const float* dec0, const float* dec1, float* out);

class SepEngine {
 public:
  SepEngine(const std::string& model_dir, int device);
  ~SepEngine();
  static constexpr int kStages = 4;  // encoder, 1x1 GEMMs, norms + depthwise, mask + decoder
  int min_samples() const { return win_; }
  int num_frames(long T) const { return T < win_ ? 0 : (int)((T - win_) / hop_ + 1); }
  // n host mixtures (concatenated samples, offsets, lengths) -> out (host): [2][T_r] per region,
  // concatenated in region order
  void separate_host(const float* samples, long total, const long* offsets, const long* lengths,
                     int n, float* out);
  // regions [starts[r], starts[r] + lengths[r]) of the signal d_audio[0, total) already in HBM;
  // out as above, device memory when out_on_device.  Ordered after user_stream's work when
  // given; synchronises before returning.
  void separate_device(const float* d_audio, long total, const long* starts, const long* lengths,
                       int n, float* out, bool out_on_device, hipStream_t user_stream);
  void trim();
  // activation bytes a launch group may take (a region longer than that runs alone)
  void set_budget(size_t bytes) { budget_ = bytes; }
  int last_groups() const { return last_groups_; }
  void set_profile(bool on) { profile_ = on; }
  const float* stage_ms() const { return stage_ms_; }
  std::mutex mu;

 private:
  struct Lin {
    float* w = nullptr;
    float* b = nullptr;
    int N = 0, K = 0;
  };
  struct Block {
    Lin in;                  // bn_chan -> hid_chan
    float slope1 = 0.f;      // PReLU after it
    float *g1 = nullptr, *b1 = nullptr;  // first gLN
    float *dw = nullptr, *dwb = nullptr; // depthwise taps [3][hid], bias
    float slope2 = 0.f;
    float *g2 = nullptr, *b2 = nullptr;  // second gLN
    Lin out;                 // hid_chan -> res | skip (bn_chan + skip_chan rows)
    int dil = 1;
  };
  template <class T>
  T* ws(const std::string& name, size_t count) {
    return ws_.get<T>(name, count, &st_);
  }
  void run(const float* d_signal, const std::vector<SepRegion>& regions, float* d_out);
  void run_group(const float* d_signal, const SepGroup& g, float* d_out);
  void mark(int stage);
  void collect_marks();
  size_t frame_bytes() const;

  int device_ = 0;
  hipStream_t st_ = nullptr;
  bool profile_ = false;
  float stage_ms_[kStages] = {0.f, 0.f, 0.f, 0.f};
  std::vector<std::pair<hipEvent_t, int>> marks_;
  size_t budget_ = (size_t)4 << 30;
  int last_groups_ = 0;
  int nf_ = 512, win_ = 32, hop_ = 16, bn_ = 128, hid_ = 512, skip_ = 128;
  Lin enc_, bott_, mask_[2], dec_;
  float *bg_ = nullptr, *bb_ = nullptr;  // the bottleneck's gLN
  float mask_slope_ = 0.f;
  std::vector<Block> blocks_;
  // the running call's region and tile tables (host copies outlive their upload)
  std::vector<SepRegion> h_regions_;
  std::vector<SepTile> h_tiles_;
  SepRegion* d_regions_ = nullptr;
  SepTile* d_tiles_ = nullptr;
  float2* d_stats_ = nullptr;
  DeviceStore store_;
  Workspace ws_;
};

}  // namespace zasr
