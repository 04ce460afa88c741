// Community-1 speaker-embedding engine: BatchNorm folding and weight layout at load, the fbank
// image, chunk windows, the ResNet34 forward in launch groups, pooling and projection.
#include "emb.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "dense_gemm.h"
#include "engine.h"
#include "host_io.h"
#include "kernels.h"

namespace zasr {

namespace {
constexpr int kStFront = 0, kStStem = 1, kStLayer1 = 2, kStPool = 6, kStProj = 7;
}  // namespace

EmbEngine::EmbEngine(const std::string& dir, int device) : device_(device) {
  const std::string cfg = dir + "/config.json", stf = dir + "/model.safetensors";
  if (!file_exists(cfg) || !file_exists(stf))
    throw std::invalid_argument("missing embedding model files in " + dir +
                                " (config.json + model.safetensors)");
  const Json j = Json::parse(read_file(cfg));
  feat_ = (int)j.at("feat_dim").as_int();
  m_ = (int)j.at("m_channels").as_int();
  emb_ = (int)j.at("embed_dim").as_int();
  num_blocks_ = j.at("num_blocks").as_int_vec();
  const double eps = j.at("bn_eps").num;
  ZASR_REQUIRE(feat_ == 80 && m_ == 32 && num_blocks_.size() == 4 && emb_ >= 1 && emb_ <= 4096,
               "embedding: feat_dim 80, m_channels 32, four stages");
  for (int nb : num_blocks_) ZASR_REQUIRE(nb >= 1 && nb <= 64, "embedding: 1-64 blocks per stage");
  SafeTensors W;
  W.load(stf);
  ZASR_HIP_CHECK(hipSetDevice(device_));
  // conv [co][ci][r][q] with the BatchNorm after it folded in float64, rounded to f32:
  // w' [co][(r ks + q) ci_n + ci] = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)
  auto conv = [&](const std::string& wn, const std::string& bn, int ci, int co, int ks, int stride) {
    const HostTensor& t = W.get(wn);
    ZASR_REQUIRE(t.numel == (size_t)co * ci * ks * ks, "embedding: bad size of " + wn);
    const float* g = W.get(bn + ".weight").data;
    const float* be = W.get(bn + ".bias").data;
    const float* mu_ = W.get(bn + ".running_mean").data;
    const float* var = W.get(bn + ".running_var").data;
    ZASR_REQUIRE(W.get(bn + ".weight").numel == (size_t)co && W.get(bn + ".bias").numel == (size_t)co &&
                     W.get(bn + ".running_mean").numel == (size_t)co &&
                     W.get(bn + ".running_var").numel == (size_t)co,
                 "embedding: bad size of " + bn);
    std::vector<float> w((size_t)co * ci * ks * ks), b((size_t)co);
    for (int o = 0; o < co; ++o) {
      const double sc = (double)g[o] / std::sqrt((double)var[o] + eps);
      b[o] = (float)((double)be[o] - (double)mu_[o] * sc);
      for (int c = 0; c < ci; ++c)
        for (int r = 0; r < ks; ++r)
          for (int q = 0; q < ks; ++q)
            w[(size_t)o * ci * ks * ks + (size_t)(r * ks + q) * ci + c] =
                (float)((double)t.data[(((size_t)o * ci + c) * ks + r) * ks + q] * sc);
    }
    Conv cv;
    cv.w = store_.upload(w);
    cv.b = store_.upload(b);
    cv.ci = ci;
    cv.co = co;
    cv.ks = ks;
    cv.stride = stride;
    return cv;
  };
  stem_ = conv("resnet.conv1.weight", "resnet.bn1", 1, m_, 3, 1);
  int in_planes = m_;
  for (int li = 0; li < 4; ++li) {
    const int planes = m_ << li;
    for (int bi = 0; bi < num_blocks_[li]; ++bi) {
      const int stride = (bi == 0 && li > 0) ? 2 : 1;
      const std::string p = "resnet.layer" + std::to_string(li + 1) + "." + std::to_string(bi) + ".";
      Block b;
      b.layer = li;
      b.a = conv(p + "conv1.weight", p + "bn1", in_planes, planes, 3, stride);
      b.b = conv(p + "conv2.weight", p + "bn2", planes, planes, 3, 1);
      b.has_sc = stride != 1 || in_planes != planes;
      if (b.has_sc) b.sc = conv(p + "shortcut.0.weight", p + "shortcut.1", in_planes, planes, 1, stride);
      blocks_.push_back(b);
      in_planes = planes;
    }
  }
  {
    const HostTensor& w = W.get("resnet.seg_1.weight");
    const HostTensor& b = W.get("resnet.seg_1.bias");
    ZASR_REQUIRE(w.numel == (size_t)emb_ * stat_dim() && b.numel == (size_t)emb_,
                 "embedding: bad size of resnet.seg_1");
    seg_w_ = store_.upload(w.data, w.numel);
    seg_b_ = store_.upload(b.data, b.numel);
  }
  // ---- fbank tables: Hamming window, kaldi mel bank 20 Hz .. Nyquist ----
  {
    std::vector<double> tw(512);
    for (int i = 0; i < 256; ++i) {
      const double a = -2.0 * M_PI * i / 512.0;
      tw[2 * i] = std::cos(a);
      tw[2 * i + 1] = std::sin(a);
    }
    d_twiddle_ = store_.upload(tw);
    std::vector<float> win(400);
    for (int i = 0; i < 400; ++i) win[i] = (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * i / 399.0));
    d_window_ = store_.upload(win);
    auto mel = [](double f) { return 1127.0 * std::log(1.0 + f / 700.0); };
    const double mlo = mel(20.0), mhi = mel(8000.0), delta = (mhi - mlo) / 81.0;
    std::vector<float> banks(80 * 256, 0.f), wts;
    for (int b = 0; b < 80; ++b) {
      const double l = mlo + b * delta, ce = mlo + (b + 1) * delta, r = mlo + (b + 2) * delta;
      for (int i = 0; i < 256; ++i) {
        const double m = mel(31.25 * i);
        if (m > l && m < r)
          banks[b * 256 + i] = (float)(m <= ce ? (m - l) / (ce - l) : (r - m) / (r - ce));
      }
    }
    std::vector<int> meta;
    pack_mel_banks(banks.data(), 256, meta, wts);
    d_mel_meta_ = store_.upload(meta);
    d_mel_w_ = store_.upload(wts);
  }
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  // last: nothing after it can throw, so a failed construction leaks no stream
  ZASR_HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
}

EmbEngine::~EmbEngine() {
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(st_);
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  (void)hipStreamDestroy(st_);
}

void EmbEngine::trim() {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  ws_.clear();
}

void EmbEngine::mark(int stage) {
  if (!profile_) return;
  hipEvent_t ev;
  ZASR_HIP_CHECK(hipEventCreate(&ev));
  ZASR_HIP_CHECK(hipEventRecord(ev, st_));
  marks_.emplace_back(ev, stage);
}

void EmbEngine::collect_marks() {
  if (marks_.empty()) return;
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  for (float& v : stage_ms_) v = 0.f;
  for (size_t i = 1; i < marks_.size(); ++i) {
    float ms = 0.f;
    if (marks_[i].second >= 0) {
      ZASR_HIP_CHECK(hipEventElapsedTime(&ms, marks_[i - 1].first, marks_[i].first));
      stage_ms_[marks_[i].second] += ms;
    }
  }
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  marks_.clear();
}

void EmbEngine::wait_for(hipStream_t user_stream) {
  if (!user_stream) return;
  hipEvent_t ev;
  ZASR_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  ZASR_HIP_CHECK(hipEventRecord(ev, user_stream));
  ZASR_HIP_CHECK(hipStreamWaitEvent(st_, ev, 0));
  ZASR_HIP_CHECK(hipEventDestroy(ev));
}

double EmbEngine::encoder_flops(int T) const {
  double fl = 2.0 * 9 * m_ * (double)feat_ * T;
  int F = feat_, t = T;
  for (const Block& b : blocks_) {
    const int Fo = (F - 1) / b.a.stride + 1, To = (t - 1) / b.a.stride + 1;
    const double pos = (double)Fo * To;
    fl += 2.0 * pos * 9 * b.a.ci * b.a.co + 2.0 * pos * 9 * b.b.ci * b.b.co;
    if (b.has_sc) fl += 2.0 * pos * b.sc.ci * b.sc.co;
    F = Fo;
    t = To;
  }
  return fl;
}

// the three ping-pong activation buffers at layer1's size, and the input rows
size_t EmbEngine::input_bytes(int T) const {
  return 4 * ((size_t)3 * feat_ * T * m_ + (size_t)feat_ * T);
}

int EmbEngine::pick_group(int n, int T) const {
  if (group_ > 0) return std::min(group_, n);
  size_t free_b = 0, total_b = 0;
  ZASR_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  const size_t per = input_bytes(T);
  const size_t fit = std::max<size_t>(1, free_b / 2 / per);
  // int positions in a launch: n F T stays below 2^31 / 256 channels
  const size_t cap = std::max<size_t>(1, ((size_t)1 << 23) / ((size_t)feat_ * T));
  return (int)std::min<size_t>({(size_t)n, fit, cap, (size_t)kMaxGroup});
}

const float* EmbEngine::encode(const float* d_feats, int n, int T) {
  const size_t act = (size_t)n * feat_ * T * m_;
  float* buf[3] = {ws<float>("act0", act), ws<float>("act1", act), ws<float>("act2", act)};
  launch_emb_stem(d_feats, stem_.w, stem_.b, n, T, feat_, m_, buf[0], st_);
  mark(kStStem);
  int cur = 0, F = feat_, t = T;
  auto run = [&](const Conv& c, const float* x, int Fi, int Ti, const float* res, bool relu, float* y) {
    EmbConv2d a{};
    a.x = x;
    a.w = c.w;
    a.bias = c.b;
    a.res = res;
    a.y = y;
    a.n = n;
    a.Fi = Fi;
    a.Ti = Ti;
    a.Ci = c.ci;
    a.Fo = (Fi - 1) / c.stride + 1;
    a.To = (Ti - 1) / c.stride + 1;
    a.Co = c.co;
    a.ks = c.ks;
    a.stride = c.stride;
    a.relu = relu ? 1 : 0;
    launch_emb_conv2d(a, 0, st_);
  };
  for (size_t bi = 0; bi < blocks_.size(); ++bi) {
    const Block& b = blocks_[bi];
    if (bi > 0 && b.layer != blocks_[bi - 1].layer) mark(kStLayer1 + blocks_[bi - 1].layer);
    const int Fo = (F - 1) / b.a.stride + 1, To = (t - 1) / b.a.stride + 1;
    float* x = buf[cur];
    float* mid = buf[(cur + 1) % 3];
    float* o = buf[(cur + 2) % 3];
    run(b.a, x, F, t, nullptr, true, mid);
    if (b.has_sc) {
      run(b.sc, x, F, t, nullptr, false, o);
      run(b.b, mid, Fo, To, o, true, x);  // x is dead once the shortcut has read it
      // cur stays: the block's output is in x
    } else {
      run(b.b, mid, Fo, To, x, true, o);
      cur = (cur + 2) % 3;
    }
    F = Fo;
    t = To;
  }
  mark(kStLayer1 + blocks_.back().layer);
  return buf[cur];
}

void EmbEngine::fbank_device(const float* d_wav, long n, long rows, float* d_rows) {
  ZASR_REQUIRE(n <= INT32_MAX && rows <= INT32_MAX / 80, "embedding: signal too long");
  long* d_off = ws<long>("fb_off", 1);
  int* d_meta = ws<int>("fb_meta", 3);
  // the sources are members: the copies may still be in flight when this function returns
  fb_off_h_ = 0;
  fb_meta_h_[0] = (int)n;
  fb_meta_h_[1] = 0;
  fb_meta_h_[2] = (int)rows;
  ZASR_HIP_CHECK(hipMemcpyAsync(d_off, &fb_off_h_, sizeof(long), hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_meta, fb_meta_h_, sizeof(fb_meta_h_), hipMemcpyHostToDevice, st_));
  FbankTables t{d_twiddle_, d_window_, d_mel_meta_, d_mel_meta_ + 80, d_mel_meta_ + 160, d_mel_w_};
  launch_fbank(d_wav, d_off, d_meta, d_meta + 1, 1, (int)rows, t, d_rows, st_, FBANK_WESPEAKER);
}

void EmbEngine::fbank_host(const float* wav, long n, long tail, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const long rows = fbank_rows(n, tail);
  if (rows <= 0) return;
  float* d_wav = ws<float>("signal", (size_t)std::max<long>(n, 1));
  float* d_rows = ws<float>("fb_rows", (size_t)rows * 80);
  if (n > 0) ZASR_HIP_CHECK(hipMemcpyAsync(d_wav, wav, (size_t)n * 4, hipMemcpyHostToDevice, st_));
  fbank_device(d_wav, n, rows, d_rows);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_rows, (size_t)rows * 80 * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void EmbEngine::encode_host(const float* feats, int n, int T, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  marks_.clear();
  const int Fq = bins_out(), Tq = num_feat_frames(T), C = 8 * m_;
  const int G = pick_group(n, T);
  last_group_ = G;
  float* d_in = ws<float>("feats", (size_t)G * T * feat_);
  float* d_out = ws<float>("cft", (size_t)G * C * Fq * Tq);
  for (int g0 = 0; g0 < n; g0 += G) {
    const int g = std::min(G, n - g0);
    mark(-1);
    ZASR_HIP_CHECK(hipMemcpyAsync(d_in, feats + (size_t)g0 * T * feat_, (size_t)g * T * feat_ * 4,
                                  hipMemcpyHostToDevice, st_));
    mark(kStFront);
    const float* y = encode(d_in, g, T);
    launch_emb_to_cft(y, g, Fq, Tq, C, d_out, st_);
    ZASR_HIP_CHECK(hipMemcpyAsync(out + (size_t)g0 * C * Fq * Tq, d_out, (size_t)g * C * Fq * Tq * 4,
                                  hipMemcpyDeviceToHost, st_));
    mark(kStPool);
    // the next group's upload overwrites d_in only after this group's stem (stream order)
  }
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  collect_marks();
}

void EmbEngine::chunks_device(const float* d_wav, long total, const long* starts, int n_chunks,
                              const unsigned char* masks, int nseg, float* out,
                              hipStream_t user_stream) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  marks_.clear();
  const int T = kChunkFrames, Fq = bins_out(), Tq = num_feat_frames(T), C = 8 * m_, S = kSpeakers;
  const int D = stat_dim();
  const long rows = fbank_rows(total, kTail);
  ZASR_REQUIRE(rows >= 1, "embedding: empty fbank image");
  wait_for(user_stream);
  mark(-1);
  float* d_rows = ws<float>("fb_rows", (size_t)rows * 80);
  fbank_device(d_wav, total, rows, d_rows);
  // windows: rows [starts[c] / 160, + 998) of the image, zeros past its end (:831-838)
  std::vector<int> wrow((size_t)n_chunks), wn((size_t)n_chunks);
  for (int c = 0; c < n_chunks; ++c) {
    const long r0 = starts[c] / 160;
    wrow[c] = (int)std::min<long>(r0, rows);
    wn[c] = (int)std::max<long>(0, std::min<long>(T, rows - r0));
  }
  const int G = pick_group(n_chunks, T);
  last_group_ = G;
  std::vector<int> fo((size_t)G + 1);  // the CMVN offsets of one group: [0, T, 2 T, ...]
  for (int c = 0; c <= G; ++c) fo[c] = c * T;
  int* d_wrow = ws<int>("win_row", (size_t)n_chunks);
  int* d_wn = ws<int>("win_n", (size_t)n_chunks);
  int* d_fo = ws<int>("win_fo", (size_t)G + 1);
  unsigned char* d_mask = ws<unsigned char>("masks", (size_t)n_chunks * S * nseg);
  float* d_feats = ws<float>("feats", (size_t)G * T * feat_);
  float* d_stats = ws<float>("stats", (size_t)n_chunks * S * D);
  float* d_emb = ws<float>("emb", (size_t)n_chunks * S * emb_);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_wrow, wrow.data(), (size_t)n_chunks * 4, hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_wn, wn.data(), (size_t)n_chunks * 4, hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_fo, fo.data(), ((size_t)G + 1) * 4, hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_mask, masks, (size_t)n_chunks * S * nseg, hipMemcpyHostToDevice, st_));
  mark(kStFront);
  for (int g0 = 0; g0 < n_chunks; g0 += G) {
    const int g = std::min(G, n_chunks - g0);
    mark(-1);
    launch_campp_gather(d_rows, d_wrow + g0, d_wn + g0, g, T, d_feats, st_);
    launch_campp_cmvn(d_feats, d_fo, g, st_);  // over all 998 rows, the zero ones included (:839)
    mark(kStFront);
    const float* y = encode(d_feats, g, T);
    launch_emb_pool(y, d_mask + (size_t)g0 * S * nseg, g, Fq, Tq, C, S, nseg, false,
                    d_stats + (size_t)g0 * S * D, st_);
    mark(kStPool);
  }
  mark(-1);
  // every row of the projection is its own fmaf chain over the 5120 statistics
  GemmParams p = dense_gemm_params(seg_w_, seg_b_, emb_, D, d_stats, D, n_chunks * S, d_emb, emb_);
  gemm_f32(p, EPI_NONE, ALOAD_DENSE, false, st_);
  mark(kStProj);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_emb, (size_t)n_chunks * S * emb_ * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  collect_marks();
}

bool EmbEngine::segment_host(const float* wav, long n, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const long rows = fbank_rows(n, 0);
  if (rows < 9) return false;  // :690
  ZASR_REQUIRE(rows <= 1 << 20, "embedding: segment too long");
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  marks_.clear();
  const int T = (int)rows, Fq = bins_out(), Tq = num_feat_frames(T), C = 8 * m_, D = stat_dim();
  float* d_wav = ws<float>("signal", (size_t)n);
  float* d_rows = ws<float>("fb_rows", (size_t)rows * 80);
  int* d_fo = ws<int>("win_fo", 2);
  float* d_stats = ws<float>("stats", (size_t)D);
  float* d_emb = ws<float>("emb", (size_t)emb_);
  const int fo[2] = {0, T};
  ZASR_HIP_CHECK(hipMemcpyAsync(d_wav, wav, (size_t)n * 4, hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_fo, fo, sizeof(fo), hipMemcpyHostToDevice, st_));
  fbank_device(d_wav, n, rows, d_rows);
  launch_campp_cmvn(d_rows, d_fo, 1, st_);
  last_group_ = 1;
  const float* y = encode(d_rows, 1, T);
  launch_emb_pool(y, nullptr, 1, Fq, Tq, C, 1, 0, true, d_stats, st_);
  GemmParams p = dense_gemm_params(seg_w_, seg_b_, emb_, D, d_stats, D, 1, d_emb, emb_);
  gemm_f32(p, EPI_NONE, ALOAD_DENSE, false, st_);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_emb, (size_t)emb_ * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  collect_marks();
  return true;
}

}  // namespace zasr
