// Device audio front end: raw PCM (f32 / int16, 1-8 interleaved channels, 4-384 kHz, host or
// device) -> the 16 kHz mono f32 HBM signal every other stage consumes, and the reference's
// level conditioning on that signal (core/asr_engine.py:495-516 load_audio's downmix and
// quiet-file boost; core/audio_preprocessing.py:46-140, 226-243 per-segment RMS normalisation
// and the peak limiter).  DESIGN.md "Audio front end" has the definition and the layout.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

namespace zasr {

constexpr int kAudioOutRate = 16000;
constexpr int kAudioMinRate = 4000, kAudioMaxRate = 384000, kAudioMaxChannels = 8;
enum { kAudioF32 = 0, kAudioI16 = 1 };

// The polyphase form of the Hann-windowed sinc (sherpa-onnx LinearResample's definition):
// output m = q P + p reads input frames q Q + lo[p] + t, t < taps, with weights
// w[p][t] = h((lo[p] + t - p Q / P) / fin) / fin.  Built in float64 / integers on the host.
struct ResampleTable {
  int rate = 0, P = 0, Q = 0, taps = 0;
  int out_tile = 0;  // outputs one workgroup makes per tile
  int span = 0;      // input frames a tile reads at most
  std::vector<int> lo;   // [P]
  std::vector<float> w;  // [P][taps]
  int in_tile() const { return (int)(((long)out_tile * Q + P - 1) / P); }
};
ResampleTable make_resample_table(int rate);  // host only; throws on a rate out of range
long audio_out_len(int rate, long n_frames);  // ceil(n_frames * 16000 / rate)

// ---- kernels (audio_kernels.hip) ----
struct ResampleArgs {
  const void* src;     // raw window: frames [w0, w1) of the signal, interleaved
  long w0, w1;
  float* out;          // the whole 16 kHz signal
  long m_begin, m_end; // outputs this launch writes; m_begin is a multiple of out_tile
  int P, Q, taps, out_tile, span;
  const int* lo;       // device [P]
  const float* w;      // device [P][taps]
  int table_in_lds;    // the whole table fits beside the input tile
  int vec_ok;          // src is 16-byte aligned
};
size_t resample_lds_bytes(const ResampleArgs& a);
void launch_resample(const ResampleArgs& a, int format, int channels, hipStream_t st);
// rate == 16000: convert + downmix alone, frames [0, n) of src -> out
void launch_downmix(const void* src, int format, int channels, long n, float* out, bool vec_ok,
                    hipStream_t st);
// *d_peak_bits = max(*d_peak_bits, bits(max |x|))  (an integer max: order independent)
void launch_peak(const float* x, long n, unsigned* d_peak_bits, hipStream_t st);
// x = (x / divisor) * multiplier, two f32 roundings
void launch_scale(float* x, long n, float divisor, float multiplier, hipStream_t st);
// partial[b] = f64 sum of squares of chunk b (kAudioChunk samples of one segment), then
// out[s] = the partials of segment s added in chunk order
constexpr int kAudioChunk = 4096;
void launch_segment_sumsq(const float* x, const long* seg_begin, const long* seg_end,
                          const long* blk_off, int n_seg, long n_blocks, double* partial,
                          double* out, hipStream_t st);
// x[i] *= gain(i): pieces [pb, pe) sorted and disjoint, gain pg (po < 0) or vals[po + i - pb];
// 1 elsewhere; the peak of the result as launch_peak
void launch_apply_gain(float* x, long n, const long* pb, const long* pe, const float* pg,
                       const long* po, int n_pieces, const float* vals, unsigned* d_peak_bits,
                       hipStream_t st);

class AudioFrontEnd {
 public:
  explicit AudioFrontEnd(int device);
  ~AudioFrontEnd();
  long to_16k(const void* src, int format, int channels, int rate, long n_frames,
              bool src_on_device, float* d_out, long cap, hipStream_t st);
  float peak(const float* d_wav, long n, hipStream_t st);
  void scale(float* d_wav, long n, float divisor, float multiplier, hipStream_t st);
  void segment_sumsq(const float* d_wav, const long* seg_begin, const long* seg_end, int n_seg,
                     double* out, hipStream_t st);
  float apply_gain(float* d_wav, long n, const long* pb, const long* pe, const float* pg,
                   const long* po, int n_pieces, const float* vals, long n_vals, hipStream_t st);
  std::mutex mu;

 private:
  struct DevTable {
    ResampleTable t;
    int* lo = nullptr;
    float* w = nullptr;
  };
  const DevTable& table(int rate);
  void* scratch(int slot, size_t bytes);  // grow-only device scratch

  int device_ = 0;
  std::map<int, DevTable> tables_;
  // host sources: two pinned staging pieces and their device twins, filled on copy_ while the
  // kernel of the previous piece runs
  static constexpr size_t kPieceBytes = size_t(8) << 20;
  hipStream_t copy_ = nullptr;
  void* pinned_[2] = {nullptr, nullptr};
  void* raw_[2] = {nullptr, nullptr};
  hipEvent_t up_[2] = {nullptr, nullptr};    // piece uploaded
  hipEvent_t used_[2] = {nullptr, nullptr};  // piece's kernel done
  unsigned* d_peak_ = nullptr;
  void* scr_[8] = {};
  size_t scr_bytes_[8] = {};
};

}  // namespace zasr
