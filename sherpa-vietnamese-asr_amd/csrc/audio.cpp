// Host side of the device audio front end (audio.h): the polyphase table in float64, the
// piecewise upload of host sources, and the small synchronising wrappers of the level passes.
#include "audio.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

#include "common.h"

namespace zasr {

long audio_out_len(int rate, long n_frames) {
  const long g = std::gcd((long)rate, (long)kAudioOutRate);
  const long P = kAudioOutRate / g, Q = rate / g;
  return (n_frames * P + Q - 1) / Q;
}

namespace {

long floor_div(long a, long b) {  // b > 0
  const long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// LDS budget of a tile in floats: the input tile, and the table when it fits beside it
constexpr int kTileFloats = 4096, kTableFloats = 9216, kMaxOutTile = 2048;

}  // namespace

ResampleTable make_resample_table(int rate) {
  ZASR_REQUIRE(rate >= kAudioMinRate && rate <= kAudioMaxRate, "sample rate must be in 4000..384000");
  ResampleTable t;
  const long fin = rate, fout = kAudioOutRate, g = std::gcd(fin, fout);
  const long P = fout / g, Q = fin / g, mn = std::min(fin, fout);
  t.rate = rate;
  t.P = (int)P;
  t.Q = (int)Q;
  // support |n / fin - m / fout| < ww = Z / (2 c), c = 0.99 * 0.5 * min(fin, fout), Z = 6: in
  // input frames, |n - q Q - p Q / P| < W = 200 fin / (33 mn).  Integer arithmetic:
  // lo[p] = the smallest n - q Q above p Q / P - W, hi[p] = the largest below p Q / P + W.
  const long den = 33 * mn * P;
  t.lo.resize(P);
  std::vector<long> hi(P);
  int taps = 0;
  for (long p = 0; p < P; ++p) {
    const long c = p * Q * 33 * mn, w = 200 * fin * P;  // p Q / P and W over den
    t.lo[p] = (int)(floor_div(c - w, den) + 1);
    hi[p] = -floor_div(-(c + w), den) - 1;
    taps = std::max(taps, (int)(hi[p] - t.lo[p] + 1));
  }
  t.taps = taps;
  const double pi = 3.14159265358979323846;
  const double c = 0.99 * 0.5 * (double)mn, Z = 6.0, ww = Z / (2.0 * c);
  t.w.assign((size_t)P * taps, 0.f);
  for (long p = 0; p < P; ++p)
    for (int k = 0; k < taps; ++k) {
      const double tt = ((double)(t.lo[p] + k) - (double)(p * Q) / (double)P) / (double)fin;
      double h = 0.0;
      if (std::fabs(tt) < ww) {
        const double s = tt == 0.0 ? 2.0 * c : std::sin(2.0 * pi * c * tt) / (pi * tt);
        h = 0.5 * (1.0 + std::cos(2.0 * pi * c * tt / Z)) * s;
      }
      t.w[(size_t)p * taps + k] = (float)(h / (double)fin);
    }
  // tile: as many outputs as keep the input tile inside its LDS budget, a multiple of 64
  long ot = ((long)(kTileFloats - taps) * P / Q) / 64 * 64;
  t.out_tile = (int)std::max(64L, std::min(ot, (long)kMaxOutTile));
  int span = 0;
  for (long p0 = 0; p0 < P; ++p0) {
    const long d = p0 + t.out_tile - 1, dq = d / P;
    span = std::max(span, (int)(dq * Q + t.lo[d - dq * P] - t.lo[p0] + taps));
  }
  t.span = span;
  return t;
}

AudioFrontEnd::AudioFrontEnd(int device) : device_(device) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamCreateWithFlags(&copy_, hipStreamNonBlocking));
  ZASR_HIP_CHECK(hipMalloc(&d_peak_, sizeof(unsigned)));
  for (int i = 0; i < 2; ++i) {
    ZASR_HIP_CHECK(hipEventCreateWithFlags(&up_[i], hipEventDisableTiming));
    ZASR_HIP_CHECK(hipEventCreateWithFlags(&used_[i], hipEventDisableTiming));
  }
}

AudioFrontEnd::~AudioFrontEnd() {
  (void)hipSetDevice(device_);
  (void)hipDeviceSynchronize();
  for (auto& kv : tables_) {
    (void)hipFree(kv.second.lo);
    (void)hipFree(kv.second.w);
  }
  for (int i = 0; i < 2; ++i) {
    if (pinned_[i]) (void)hipHostFree(pinned_[i]);
    if (raw_[i]) (void)hipFree(raw_[i]);
    if (up_[i]) (void)hipEventDestroy(up_[i]);
    if (used_[i]) (void)hipEventDestroy(used_[i]);
  }
  for (void* p : scr_)
    if (p) (void)hipFree(p);
  if (d_peak_) (void)hipFree(d_peak_);
  if (copy_) (void)hipStreamDestroy(copy_);
}

const AudioFrontEnd::DevTable& AudioFrontEnd::table(int rate) {
  auto it = tables_.find(rate);
  if (it != tables_.end()) return it->second;
  DevTable d;
  d.t = make_resample_table(rate);
  ZASR_HIP_CHECK(hipMalloc(&d.lo, d.t.lo.size() * sizeof(int)));
  ZASR_HIP_CHECK(hipMalloc(&d.w, d.t.w.size() * sizeof(float)));
  ZASR_HIP_CHECK(hipMemcpy(d.lo, d.t.lo.data(), d.t.lo.size() * sizeof(int), hipMemcpyHostToDevice));
  ZASR_HIP_CHECK(hipMemcpy(d.w, d.t.w.data(), d.t.w.size() * sizeof(float), hipMemcpyHostToDevice));
  return tables_.emplace(rate, std::move(d)).first->second;
}

void* AudioFrontEnd::scratch(int slot, size_t bytes) {
  if (scr_bytes_[slot] < bytes) {
    if (scr_[slot]) {
      ZASR_HIP_CHECK(hipDeviceSynchronize());  // an earlier call's kernels may still read it
      ZASR_HIP_CHECK(hipFree(scr_[slot]));
      scr_[slot] = nullptr;
      scr_bytes_[slot] = 0;
    }
    const size_t cap = std::max(bytes, size_t(4096));
    ZASR_HIP_CHECK(hipMalloc(&scr_[slot], cap));
    scr_bytes_[slot] = cap;
  }
  return scr_[slot];
}

long AudioFrontEnd::to_16k(const void* src, int format, int channels, int rate, long n_frames,
                           bool src_on_device, float* d_out, long cap, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const long n_out = audio_out_len(rate, n_frames);
  ZASR_REQUIRE(n_out <= cap, "output buffer too small");
  if (n_frames == 0) return 0;
  const size_t es = format == kAudioF32 ? 4 : 2, fb = es * channels;
  const bool pass = rate == kAudioOutRate;
  const DevTable* dt = pass ? nullptr : &table(rate);
  ResampleArgs a{};
  if (!pass) {
    const ResampleTable& t = dt->t;
    a.out = d_out;
    a.P = t.P;
    a.Q = t.Q;
    a.taps = t.taps;
    a.out_tile = t.out_tile;
    a.span = t.span;
    a.lo = dt->lo;
    a.w = dt->w;
    a.table_in_lds = (long)t.P + (long)t.P * (t.taps | 1) <= kTableFloats;
  }
  if (src_on_device) {
    const bool vec_ok = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    if (pass) {
      if (format == kAudioF32 && channels == 1)
        ZASR_HIP_CHECK(hipMemcpyAsync(d_out, src, n_frames * 4, hipMemcpyDeviceToDevice, st));
      else
        launch_downmix(src, format, channels, n_frames, d_out, vec_ok, st);
    } else {
      a.src = src;
      a.w0 = 0;
      a.w1 = n_frames;
      a.m_begin = 0;
      a.m_end = n_out;
      a.vec_ok = vec_ok;
      launch_resample(a, format, channels, st);
    }
    return n_out;
  }
  // Host source: frames go up in pieces of at most kPieceBytes on the copy stream into two
  // device buffers; piece k's kernel (on st) waits for its upload only, so piece k + 1's
  // upload runs under it.  A piece is a whole number of output tiles and holds every frame
  // their outputs read.  Pageable memory is staged through two pinned buffers of the same
  // size; memory the caller has pinned already is read by the copy engine where it lies.
  hipPointerAttribute_t attr{};
  const bool src_pinned = hipPointerGetAttributes(&attr, src) == hipSuccess &&
                          attr.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // an unregistered pointer is reported as an error: not one here
  for (int i = 0; i < 2; ++i) {
    if (!src_pinned && !pinned_[i])
      ZASR_HIP_CHECK(hipHostMalloc(&pinned_[i], kPieceBytes, hipHostMallocDefault));
    if (!raw_[i]) ZASR_HIP_CHECK(hipMalloc(&raw_[i], kPieceBytes));
  }
  const long piece_frames = (long)(kPieceBytes / fb);
  long tiles_per_piece = 0;
  if (!pass)  // outputs whose frames, with a tile's reach on both sides, fit one piece
    tiles_per_piece = std::max(1L, (piece_frames - 2L * dt->t.span) * a.P / a.Q / a.out_tile - 1);
  const unsigned char* h = static_cast<const unsigned char*>(src);
  const long total = pass ? n_frames : n_out;
  long done = 0;  // outputs (frames when nothing is resampled) finished
  for (int k = 0; done < total; ++k) {
    const int b = k & 1;
    long w0, w1, m1;
    if (pass) {
      w0 = done;
      w1 = m1 = std::min(n_frames, w0 + piece_frames);
    } else {
      m1 = std::min(n_out, done + tiles_per_piece * a.out_tile);
      const long q0 = done / a.P, p0 = done % a.P, ql = (m1 - 1) / a.P, pl = (m1 - 1) % a.P;
      w0 = std::min(n_frames, std::max(0L, q0 * a.Q + dt->t.lo[p0]));
      w1 = std::max(w0, std::min(n_frames, ql * a.Q + dt->t.lo[pl] + a.taps));
      ZASR_REQUIRE((size_t)(w1 - w0) * fb <= kPieceBytes, "audio piece exceeds its staging buffer");
    }
    const size_t bytes = (size_t)(w1 - w0) * fb;
    ZASR_HIP_CHECK(hipEventSynchronize(used_[b]));  // the kernel that read this buffer is done
    if (bytes) {
      const void* from = h + (size_t)w0 * fb;
      if (!src_pinned) from = std::memcpy(pinned_[b], from, bytes);
      ZASR_HIP_CHECK(hipMemcpyAsync(raw_[b], from, bytes, hipMemcpyHostToDevice, copy_));
    }
    ZASR_HIP_CHECK(hipEventRecord(up_[b], copy_));
    ZASR_HIP_CHECK(hipStreamWaitEvent(st, up_[b], 0));
    if (pass) {
      launch_downmix(raw_[b], format, channels, w1 - w0, d_out + w0, true, st);
    } else {
      a.src = raw_[b];
      a.w0 = w0;
      a.w1 = w1;
      a.m_begin = done;
      a.m_end = m1;
      a.vec_ok = 1;
      launch_resample(a, format, channels, st);
    }
    ZASR_HIP_CHECK(hipEventRecord(used_[b], st));
    done = m1;
  }
  // the caller's buffer is read during the call only
  if (src_pinned) ZASR_HIP_CHECK(hipStreamSynchronize(copy_));
  return n_out;
}

float AudioFrontEnd::peak(const float* d_wav, long n, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  unsigned bits = 0;
  ZASR_HIP_CHECK(hipMemsetAsync(d_peak_, 0, sizeof(unsigned), st));
  launch_peak(d_wav, n, d_peak_, st);
  ZASR_HIP_CHECK(hipMemcpyAsync(&bits, d_peak_, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  float v;
  std::memcpy(&v, &bits, 4);
  return v;
}

void AudioFrontEnd::scale(float* d_wav, long n, float divisor, float multiplier, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  launch_scale(d_wav, n, divisor, multiplier, st);
}

void AudioFrontEnd::segment_sumsq(const float* d_wav, const long* seg_begin, const long* seg_end,
                                  int n_seg, double* out, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  if (n_seg <= 0) return;
  // [begin | end | first block] of every segment, one upload
  std::vector<long> meta(3 * (size_t)n_seg + 1);
  long blocks = 0;
  for (int s = 0; s < n_seg; ++s) {
    meta[s] = seg_begin[s];
    meta[n_seg + s] = seg_end[s];
    meta[2 * (size_t)n_seg + s] = blocks;
    blocks += (std::max(0L, seg_end[s] - seg_begin[s]) + kAudioChunk - 1) / kAudioChunk;
  }
  meta[3 * (size_t)n_seg] = blocks;
  ZASR_REQUIRE(blocks < (1L << 31), "too many sum-of-squares chunks");
  long* d_meta = static_cast<long*>(scratch(0, meta.size() * sizeof(long)));
  double* d_part = static_cast<double*>(scratch(1, (size_t)(blocks + n_seg) * sizeof(double)));
  double* d_out = d_part + blocks;
  ZASR_HIP_CHECK(hipMemcpyAsync(d_meta, meta.data(), meta.size() * sizeof(long),
                                hipMemcpyHostToDevice, st));
  launch_segment_sumsq(d_wav, d_meta, d_meta + n_seg, d_meta + 2 * (size_t)n_seg, n_seg, blocks,
                       d_part, d_out, st);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)n_seg * sizeof(double), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
}

float AudioFrontEnd::apply_gain(float* d_wav, long n, const long* pb, const long* pe,
                                const float* pg, const long* po, int n_pieces, const float* vals,
                                long n_vals, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const size_t np = (size_t)std::max(n_pieces, 0);
  long* d_l = static_cast<long*>(scratch(2, (3 * np + 1) * sizeof(long)));
  float* d_f = static_cast<float*>(scratch(3, (np + (size_t)std::max(n_vals, 0L) + 1) * sizeof(float)));
  if (np) {
    ZASR_HIP_CHECK(hipMemcpyAsync(d_l, pb, np * sizeof(long), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipMemcpyAsync(d_l + np, pe, np * sizeof(long), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipMemcpyAsync(d_l + 2 * np, po, np * sizeof(long), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipMemcpyAsync(d_f, pg, np * sizeof(float), hipMemcpyHostToDevice, st));
    if (n_vals > 0)
      ZASR_HIP_CHECK(hipMemcpyAsync(d_f + np, vals, (size_t)n_vals * sizeof(float),
                                    hipMemcpyHostToDevice, st));
  }
  unsigned bits = 0;
  ZASR_HIP_CHECK(hipMemsetAsync(d_peak_, 0, sizeof(unsigned), st));
  launch_apply_gain(d_wav, n, d_l, d_l + np, d_f, d_l + 2 * np, (int)np, d_f + np, d_peak_, st);
  ZASR_HIP_CHECK(hipMemcpyAsync(&bits, d_peak_, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  float v;
  std::memcpy(&v, &bits, 4);
  return v;
}

}  // namespace zasr
