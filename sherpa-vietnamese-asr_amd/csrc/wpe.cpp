// Host side of the WPE engine (wpe.h): the float64 tables, the launch groups under the spectrum
// budget, and the one-kernel entries of the selftests.
#include "wpe.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"

namespace zasr {

namespace {

// Y and X (complex64) of one chunk
size_t spectrum_bytes(int T) { return (size_t)2 * kWpeBins * (size_t)T * sizeof(float2); }

struct StageTimer {  // HIP-event time of one stage, when profiling
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t st;
  bool on;
  StageTimer(bool on_, hipStream_t st_) : st(st_), on(on_) {
    if (!on) return;
    ZASR_HIP_CHECK(hipEventCreate(&a));
    ZASR_HIP_CHECK(hipEventCreate(&b));
    ZASR_HIP_CHECK(hipEventRecord(a, st));
  }
  void stop() {
    if (on) ZASR_HIP_CHECK(hipEventRecord(b, st));
  }
  float ms() {  // after the stream was synchronised
    float v = 0.f;
    if (on) ZASR_HIP_CHECK(hipEventElapsedTime(&v, a, b));
    return v;
  }
  ~StageTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

WpeEngine::WpeEngine(int device) : device_(device) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
  // periodic Blackman (scipy.signal.windows.blackman(512, sym=False)) and its biorthogonal
  // synthesis window at hop 128, in float64, rounded once
  const double pi = 3.14159265358979323846;
  std::vector<double> w(kWpeFft);
  for (int n = 0; n < kWpeFft; ++n)
    w[n] = 0.42 - 0.5 * std::cos(2.0 * pi * n / kWpeFft) + 0.08 * std::cos(4.0 * pi * n / kWpeFft);
  std::vector<float> win(kWpeFft), syn(kWpeFft);
  for (int n = 0; n < kWpeFft; ++n) {
    double den = 0.0;
    for (int m = n % kWpeHop; m < kWpeFft; m += kWpeHop) den += w[m] * w[m];
    win[n] = (float)w[n];
    syn[n] = (float)(w[n] / den);
  }
  std::vector<float2> tw(256);
  for (int u = 0; u < 256; ++u)
    tw[u] = make_float2((float)std::cos(2.0 * pi * u / 512.0), (float)-std::sin(2.0 * pi * u / 512.0));
  d_window_ = store_.upload(win);
  d_synth_ = store_.upload(syn);
  d_twiddle_ = store_.upload(tw);
}

WpeEngine::~WpeEngine() {
  (void)hipSetDevice(device_);
  if (st_) {
    (void)hipStreamSynchronize(st_);
    (void)hipStreamDestroy(st_);
  }
}

void WpeEngine::trim() {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  ws_.clear();
}

void WpeEngine::run_group(const float* d_signal, const std::vector<WpeChunk>& chunks, int taps,
                          int delay, int iterations, float* d_out, hipStream_t st) {
  const int nc = (int)chunks.size();
  if (nc == 0) return;
  long spec = 0, max_n = 0;
  int max_T = 0;
  for (const WpeChunk& c : chunks) {
    spec += (long)kWpeBins * c.T;
    max_T = std::max(max_T, c.T);
    max_n = std::max(max_n, c.n);
  }
  const int stride = iterations + 1;
  WpeChunk* d_chunks = ws<WpeChunk>("chunks", (size_t)nc);
  float2* d_Y = ws<float2>("Y", (size_t)spec);
  float2* d_X = ws<float2>("X", (size_t)spec);
  double2* d_g[2] = {ws<double2>("g0", (size_t)nc * kWpeBins * taps),
                     ws<double2>("g1", (size_t)nc * kWpeBins * taps)};
  unsigned* d_max = ws<unsigned>("max", (size_t)nc * stride);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), (size_t)nc * sizeof(WpeChunk),
                                hipMemcpyHostToDevice, st));
  ZASR_HIP_CHECK(hipMemsetAsync(d_max, 0, (size_t)nc * stride * sizeof(unsigned), st));
  const WpeTables tabs = tables();
  StageTimer t0(profile_, st);
  launch_wpe_stft(d_signal, d_chunks, nc, max_T, tabs, d_Y, d_max, stride, st);
  t0.stop();
  StageTimer t1(profile_, st);
  for (int it = 0; it < iterations; ++it)
    launch_wpe_iter(d_Y, d_chunks, nc, max_T, taps, delay, it, it ? d_g[(it - 1) & 1] : nullptr,
                    d_g[it & 1], d_max, stride, it == iterations - 1 ? d_X : nullptr, st);
  t1.stop();
  StageTimer t2(profile_, st);
  launch_wpe_istft(d_X, d_chunks, nc, max_n, tabs, d_out, st);
  t2.stop();
  // the chunk table is read from this call's vector: it must outlive the upload
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  stage_ms_[0] += t0.ms();
  stage_ms_[1] += t1.ms();
  stage_ms_[2] += t2.ms();
}

void WpeEngine::run_device(const float* d_audio, long total, const long* offsets, const long* lens,
                           int count, int taps, int delay, int iterations, float* d_out,
                           const long* out_offsets, hipStream_t user_stream) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_REQUIRE(taps >= 1 && taps <= kWpeMaxTaps, "WPE: taps must be in 1..16");
  ZASR_REQUIRE(delay >= 1 && delay <= kWpeMaxDelay, "WPE: delay must be in 1..16");
  ZASR_REQUIRE(iterations >= 1 && iterations <= kWpeMaxIters, "WPE: iterations must be in 1..8");
  for (int c = 0; c < count; ++c) {
    ZASR_REQUIRE(lens[c] >= 0 && offsets[c] >= 0 && lens[c] <= total && offsets[c] <= total - lens[c],
                 "WPE: chunk outside the signal");
    ZASR_REQUIRE(lens[c] <= kWpeMaxSamples, "WPE: a chunk is at most 60 s");
    ZASR_REQUIRE(out_offsets[c] >= 0, "WPE: negative output offset");
  }
  if (user_stream) {  // order after the caller's producer of d_audio
    hipEvent_t ev;
    ZASR_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZASR_HIP_CHECK(hipEventRecord(ev, user_stream));
    ZASR_HIP_CHECK(hipStreamWaitEvent(st_, ev, 0));
    ZASR_HIP_CHECK(hipEventDestroy(ev));
  }
  std::fill(stage_ms_, stage_ms_ + kStages, 0.f);
  last_groups_ = 0;
  std::vector<WpeChunk> group;
  size_t bytes = 0;
  long spec = 0;
  auto flush = [&]() {
    if (group.empty()) return;
    run_group(d_audio, group, taps, delay, iterations, d_out, st_);
    ++last_groups_;
    group.clear();
    bytes = 0;
    spec = 0;
  };
  for (int c = 0; c < count; ++c) {
    if (lens[c] < 2 * kWpeFft) {  // the reference's guard: returned unchanged
      if (lens[c] > 0)
        ZASR_HIP_CHECK(hipMemcpyAsync(d_out + out_offsets[c], d_audio + offsets[c],
                                      (size_t)lens[c] * sizeof(float), hipMemcpyDeviceToDevice, st_));
      continue;
    }
    const int T = (int)wpe_frames(lens[c]);
    const size_t need = spectrum_bytes(T);
    if (!group.empty() && (bytes + need > budget_ || group.size() >= 65535)) flush();
    group.push_back(WpeChunk{offsets[c], lens[c], out_offsets[c], spec, T, (int)group.size()});
    bytes += need;
    spec += (long)kWpeBins * T;
  }
  flush();
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void WpeEngine::run_host(const float* audio, long total, const long* offsets, const long* lens,
                         int count, int taps, int delay, int iterations, float* out,
                         const long* out_offsets) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  long out_total = 0;
  for (int c = 0; c < count; ++c) {
    ZASR_REQUIRE(lens[c] >= 0 && out_offsets[c] >= 0, "WPE: negative length or output offset");
    out_total = std::max(out_total, out_offsets[c] + lens[c]);
  }
  float* d_in = ws<float>("host_in", (size_t)std::max(total, 1L));
  float* d_out = ws<float>("host_out", (size_t)std::max(out_total, 1L));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_in, audio, (size_t)total * sizeof(float), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)out_total * sizeof(float), st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  run_device(d_in, total, offsets, lens, count, taps, delay, iterations, d_out, out_offsets, nullptr);
  ZASR_HIP_CHECK(hipMemcpy(out, d_out, (size_t)out_total * sizeof(float), hipMemcpyDeviceToHost));
}

// ---- the kernels alone ----
void WpeEngine::selftest_stft(const float* signal, long n, float* Y, float* max_sq) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_REQUIRE(n >= 1 && n <= kWpeMaxSamples, "WPE selftest: n must be in 1..960000");
  const int T = (int)wpe_frames(n);
  const size_t spec = (size_t)kWpeBins * T;
  float* d_sig = ws<float>("t_sig", (size_t)n);
  float2* d_Y = ws<float2>("t_Y", spec);
  unsigned* d_max = ws<unsigned>("t_max", 2);
  WpeChunk* d_c = ws<WpeChunk>("t_chunk", 1);
  const WpeChunk c{0, n, 0, 0, T, 0};
  ZASR_HIP_CHECK(hipMemcpyAsync(d_sig, signal, (size_t)n * 4, hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_c, &c, sizeof(c), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_max, 0, 2 * sizeof(unsigned), st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_Y, 0xff, spec * sizeof(float2), st_));  // NaN where not written
  launch_wpe_stft(d_sig, d_c, 1, T, tables(), d_Y, d_max, 2, st_);
  ZASR_HIP_CHECK(hipMemcpyAsync(Y, d_Y, spec * sizeof(float2), hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(max_sq, d_max, sizeof(float), hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void WpeEngine::selftest_iter(const float* Y, int T, int taps, int delay, float max_sq,
                              const double* g_prev, double* g, float* X, float* next_max_sq) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_REQUIRE(T >= 1 && T <= wpe_frames(kWpeMaxSamples), "WPE selftest: T out of range");
  const size_t spec = (size_t)kWpeBins * T, ng = (size_t)kWpeBins * taps;
  float2* d_Y = ws<float2>("t_Y", spec);
  float2* d_X = ws<float2>("t_X", spec);
  double2* d_gp = ws<double2>("t_gp", ng);
  double2* d_g = ws<double2>("t_g", ng);
  unsigned* d_max = ws<unsigned>("t_max", 2);
  WpeChunk* d_c = ws<WpeChunk>("t_chunk", 1);
  const WpeChunk c{0, 0, 0, 0, T, 0};
  unsigned bits[2] = {0, 0};
  std::memcpy(&bits[0], &max_sq, 4);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_Y, Y, spec * sizeof(float2), hipMemcpyHostToDevice, st_));
  if (g_prev) ZASR_HIP_CHECK(hipMemcpyAsync(d_gp, g_prev, ng * sizeof(double2), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_c, &c, sizeof(c), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_max, bits, sizeof(bits), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_g, 0xff, ng * sizeof(double2), st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_X, 0xff, spec * sizeof(float2), st_));
  launch_wpe_iter(d_Y, d_c, 1, T, taps, delay, 0, g_prev ? d_gp : nullptr, d_g, d_max, 2,
                  X ? d_X : nullptr, st_);
  ZASR_HIP_CHECK(hipMemcpyAsync(g, d_g, ng * sizeof(double2), hipMemcpyDeviceToHost, st_));
  if (X) ZASR_HIP_CHECK(hipMemcpyAsync(X, d_X, spec * sizeof(float2), hipMemcpyDeviceToHost, st_));
  if (next_max_sq)
    ZASR_HIP_CHECK(hipMemcpyAsync(next_max_sq, d_max + 1, sizeof(float), hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void WpeEngine::selftest_istft(const float* X, int T, long n, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_REQUIRE(n >= 1 && n <= kWpeMaxSamples && T == wpe_frames(n),
               "WPE selftest: T must be the frame count of n");
  const size_t spec = (size_t)kWpeBins * T;
  float2* d_X = ws<float2>("t_X", spec);
  float* d_out = ws<float>("t_out", (size_t)n);
  WpeChunk* d_c = ws<WpeChunk>("t_chunk", 1);
  const WpeChunk c{0, n, 0, 0, T, 0};
  ZASR_HIP_CHECK(hipMemcpyAsync(d_X, X, spec * sizeof(float2), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_c, &c, sizeof(c), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemsetAsync(d_out, 0xff, (size_t)n * 4, st_));
  launch_wpe_istft(d_X, d_c, 1, n, tables(), d_out, st_);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

}  // namespace zasr
