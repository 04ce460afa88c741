// WPE dereverberation on device: the reference's apply_wpe_dereverberation
// (core/audio_preprocessing.py:157-216: nara-wpe's stft, wpe_v6 and istft in numpy, one chunk
// per call on the CPU) as three kernels over a ragged batch of chunks of one HBM signal: the
// Blackman STFT, one weighted-prediction-error iteration per (chunk, frequency bin) with its
// correlation sums and Cholesky solve in float64, and the biorthogonal inverse STFT in gather
// form.  The definitions in DESIGN §4k are the contract: the documented per-frequency algorithm.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "device_mem.h"

namespace zasr {

constexpr int kWpeFft = 512, kWpeHop = 128, kWpeBins = 257, kWpeFade = 384;
constexpr int kWpeMaxTaps = 16, kWpeMaxDelay = 16, kWpeMaxIters = 8;
constexpr long kWpeMaxSamples = 60L * 16000;  // one bin's series then fits a workgroup's LDS
constexpr int kWpeStftTile = 16;   // frames of one wpe_stft workgroup
constexpr int kWpeIstftTile = 16;  // frames one wpe_istft workgroup transforms
constexpr int kWpeIstftOut = 13;   // the output blocks of 128 samples they complete

// frames of a chunk of n samples: 384 zeros at both ends, then zeros to a whole frame
inline long wpe_frames(long n) { return (n + 2 * kWpeFade - kWpeFft + kWpeHop - 1) / kWpeHop + 1; }

struct WpeChunk {
  long sig_off;   // first sample of the chunk in the signal
  long n;         // its samples
  long out_off;   // first sample of its output in the packed output
  long spec_off;  // first complex element of its [257][T] (and [T][257]) spectra in the group
  int T;
  int index;      // the chunk within the group (its slots of the maxima and of g)
};

struct WpeTables {
  const float* window;    // [512] periodic Blackman
  const float* synth;     // [512] w[n] / sum_m w[n mod 128 + 128 m]^2
  const float2* twiddle;  // [256] exp(-2 pi i u / 512)
};

// ---- kernels (wpe_kernels.hip) ----
// Y[spec_off + bin * T + t] = rfft(x_pad[128 t : 128 t + 512] * window)[bin];
// max_bits[index * stride] = bits(max |Y|^2) of the chunk (an integer max: order independent)
void launch_wpe_stft(const float* signal, const WpeChunk* chunks, int n_chunks, int max_T,
                     const WpeTables& tabs, float2* Y, unsigned* max_bits, int max_stride,
                     hipStream_t st);
// One iteration for every (chunk, bin): x = y - g_prev^H ytilde (x = y when g_prev is null),
// lambda = max(|x|^2, 1e-10 max_bits[index * stride + it]), R and p in float64, g = R^-1 p by
// Cholesky with the pivot rule; g[(index * 257 + bin) * taps + k]; max |x_new|^2 folded into
// max_bits[index * stride + it + 1]; X[spec_off + t * 257 + bin] = x_new when X is given.
void launch_wpe_iter(const float2* Y, const WpeChunk* chunks, int n_chunks, int max_T, int taps,
                     int delay, int it, const double2* g_prev, double2* g, unsigned* max_bits,
                     int max_stride, float2* X, hipStream_t st);
size_t wpe_iter_lds_bytes(int T, int taps);
// out[out_off + n] = the overlap-add of irfft(X[t]) * synth, 384 samples dropped, n < chunk.n
void launch_wpe_istft(const float2* X, const WpeChunk* chunks, int n_chunks, long max_n,
                      const WpeTables& tabs, float* out, hipStream_t st);

class WpeEngine {
 public:
  explicit WpeEngine(int device);
  ~WpeEngine();
  static constexpr int kStages = 3;  // stft, iterations, istft
  // chunks [offsets[c], offsets[c] + lens[c]) of d_audio[0, total) -> d_out + out_offsets[c]
  // (device); a chunk under 2 * 512 samples is copied unchanged.  Ordered after user_stream's
  // work when given; synchronises before returning.
  void run_device(const float* d_audio, long total, const long* offsets, const long* lens,
                  int count, int taps, int delay, int iterations, float* d_out,
                  const long* out_offsets, hipStream_t user_stream);
  // the same on host memory: out is host memory too
  void run_host(const float* audio, long total, const long* offsets, const long* lens, int count,
                int taps, int delay, int iterations, float* out, const long* out_offsets);
  void trim();
  // spectrum bytes a launch group may take (a chunk beyond that runs alone)
  void set_budget(size_t bytes) { budget_ = bytes; }
  int last_groups() const { return last_groups_; }
  void set_profile(bool on) { profile_ = on; }
  const float* stage_ms() const { return stage_ms_; }
  // the kernels alone on host operands of one chunk (include/zasr.h zasr_selftest_wpe_*)
  void selftest_stft(const float* signal, long n, float* Y, float* max_sq);
  void selftest_iter(const float* Y, int T, int taps, int delay, float max_sq, const double* g_prev,
                     double* g, float* X, float* next_max_sq);
  void selftest_istft(const float* X, int T, long n, float* out);
  std::mutex mu;

 private:
  template <class T>
  T* ws(const std::string& name, size_t count) {
    return ws_.get<T>(name, count, &st_);
  }
  void run_group(const float* d_signal, const std::vector<WpeChunk>& chunks, int taps, int delay,
                 int iterations, float* d_out, hipStream_t st);
  WpeTables tables() const { return WpeTables{d_window_, d_synth_, d_twiddle_}; }

  int device_ = 0;
  hipStream_t st_ = nullptr;
  bool profile_ = false;
  float stage_ms_[kStages] = {0.f, 0.f, 0.f};
  size_t budget_ = (size_t)2 << 30;
  int last_groups_ = 0;
  float *d_window_ = nullptr, *d_synth_ = nullptr;
  float2* d_twiddle_ = nullptr;
  DeviceStore store_;
  Workspace ws_;
};

}  // namespace zasr
