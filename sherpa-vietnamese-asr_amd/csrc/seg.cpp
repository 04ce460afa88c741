// PyanNet segmentation engine: weight layout for the GEMM formulation and the batched forward.
#include "seg.h"

#include <algorithm>
#include <cstring>

#include "common.h"
#include "dense_gemm.h"
#include "host_io.h"

namespace zasr {

namespace {
constexpr int SH = kSegH, SK = 5;  // LSTM width, conv_1 / conv_2 taps
constexpr int SC1 = 60;            // conv_1 / conv_2 channels
// launch groups of chunks are sized so the activations of one group stay within this bound:
// 8 GiB.  A 10 s chunk takes 8.6 MB (chunk_bytes: 1.70 MB of it the pooled stage-0 activation,
// 2.41 MB one layer's gate pre-activations), so an hour (720 chunks, 6.2 GB) is one group and
// its recurrence has all 1440 sequences to fill the CUs with; longer files run in groups of 998.
constexpr size_t kWorkspaceBound = (size_t)8 << 30;

int pooled(long frames) { return (int)(frames / 3); }
}  // namespace

int SegEngine::num_frames(long T) {
  if (T < kSegTaps) return 0;
  const long l0 = (T - kSegTaps) / kSegStride0 + 1;
  const long f1 = l0 / 3;
  if (f1 < SK) return 0;
  const long f2 = (f1 - SK + 1) / 3;
  if (f2 < SK) return 0;
  return pooled(f2 - SK + 1);
}

std::vector<long> SegEngine::chunk_starts(long total, long chunk, long step) {
  std::vector<long> starts;
  for (long s = 0; s < total; s += step) {
    starts.push_back(s);
    if (s + chunk >= total) break;
  }
  return starts;
}

// activation bytes of one chunk: pooled stage 0 (the big one), conv_1 / conv_2 outputs and
// their pooled forms, one layer's gate pre-activations, the two layer outputs, the linears
size_t SegEngine::chunk_bytes(int T) {
  const size_t f1 = ((size_t)(T - kSegTaps) / kSegStride0 + 1) / 3, l1 = f1 - SK + 1, f2 = l1 / 3,
               l2 = f2 - SK + 1, f3 = l2 / 3;
  return 4 * (f1 * kSegC0 + (l1 + f2 + l2 + f3) * SC1 + f3 * (8 * SH + 4 * SH + 2 * SH));
}

SegEngine::SegEngine(const std::string& dir, int device) : device_(device) {
  const std::string cfg = dir + "/config.json", st = dir + "/model.safetensors";
  if (!file_exists(cfg) || !file_exists(st))
    throw std::invalid_argument("missing segmentation model files in " + dir +
                                " (config.json + model.safetensors)");
  const Json j = Json::parse(read_file(cfg));
  const std::vector<int> cc = j.at("conv_channels").as_int_vec(), lw = j.at("linear").as_int_vec();
  ZASR_REQUIRE(j.at("sinc_filters").as_int() == kSegC0 && j.at("sinc_taps").as_int() == kSegTaps &&
                   j.at("sinc_stride").as_int() == kSegStride0 && cc == std::vector<int>({SC1, SC1}) &&
                   j.at("conv_kernel").as_int() == SK && j.at("lstm_hidden").as_int() == SH &&
                   j.at("lstm_layers").as_int() == 4 && lw == std::vector<int>({SH, SH}) &&
                   j.at("classes").as_int() == kSegClasses,
               "segmentation: only the PyanNet shape (sinc 80 x 251 / 10, convs 60 x 5, LSTM 4 x 128 "
               "bidirectional, linears 128, 7 classes)");
  SafeTensors W;
  W.load(st);
  ZASR_HIP_CHECK(hipSetDevice(device_));
  {
    hipDeviceProp_t prop;
    ZASR_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
    cus_ = std::max(1, prop.multiProcessorCount);
  }
  auto get = [&](const std::string& n, size_t numel) {
    const HostTensor& t = W.get(n);
    ZASR_REQUIRE(t.numel == numel, "segmentation: bad size of " + n);
    return t.data;
  };
  in_w_ = get("sincnet.wav_norm1d.weight", 1)[0];
  in_b_ = get("sincnet.wav_norm1d.bias", 1)[0];
  {  // [80][1][251] -> tap-major [251][80]
    const float* src = get("sincnet.conv1d.0.weight", (size_t)kSegC0 * kSegTaps);
    std::vector<float> w((size_t)kSegTaps * kSegC0);
    for (int c = 0; c < kSegC0; ++c)
      for (int q = 0; q < kSegTaps; ++q) w[(size_t)q * kSegC0 + c] = src[(size_t)c * kSegTaps + q];
    w0t_ = store_.upload(w);
  }
  const int nc[3] = {kSegC0, SC1, SC1};
  for (int i = 0; i < 3; ++i) {
    const std::string p = "sincnet.norm1d." + std::to_string(i) + ".";
    norm_[i].w = store_.upload(get(p + "weight", nc[i]), nc[i]);
    norm_[i].b = store_.upload(get(p + "bias", nc[i]), nc[i]);
  }
  for (int i = 0; i < 2; ++i) {  // [co][ci][5] -> im2col GEMM weight [co][q * ci + c]
    const std::string p = "sincnet.conv1d." + std::to_string(i + 1) + ".";
    const int ci = nc[i], co = SC1, K = SK * ci;
    const float* src = get(p + "weight", (size_t)co * ci * SK);
    std::vector<float> w((size_t)co * K);
    for (int o = 0; o < co; ++o)
      for (int c = 0; c < ci; ++c)
        for (int q = 0; q < SK; ++q) w[(size_t)o * K + q * ci + c] = src[((size_t)o * ci + c) * SK + q];
    conv_[i].w = store_.upload(w);
    conv_[i].b = store_.upload(get(p + "bias", co), co);
    conv_[i].N = co;
    conv_[i].K = K;
  }
  for (int l = 0; l < 4; ++l) {  // both directions stacked: W_ih [1024][K], b_ih + b_hh, W_hh [2][512][128]
    const int K = l == 0 ? SC1 : 2 * SH;
    std::vector<float> wi((size_t)8 * SH * K), bi((size_t)8 * SH), wh((size_t)8 * SH * SH);
    for (int d = 0; d < 2; ++d) {
      const std::string sfx = "_l" + std::to_string(l) + (d ? "_reverse" : "");
      std::memcpy(&wi[(size_t)d * 4 * SH * K], get("lstm.weight_ih" + sfx, (size_t)4 * SH * K),
                  (size_t)4 * SH * K * 4);
      std::memcpy(&wh[(size_t)d * 4 * SH * SH], get("lstm.weight_hh" + sfx, (size_t)4 * SH * SH),
                  (size_t)4 * SH * SH * 4);
      const float* b1 = get("lstm.bias_ih" + sfx, 4 * SH);
      const float* b2 = get("lstm.bias_hh" + sfx, 4 * SH);
      for (int i = 0; i < 4 * SH; ++i) bi[(size_t)d * 4 * SH + i] = b1[i] + b2[i];
    }
    ih_[l].w = store_.upload(wi);
    ih_[l].b = store_.upload(bi);
    ih_[l].N = 8 * SH;
    ih_[l].K = K;
    whh_[l] = store_.upload(wh);
  }
  for (int i = 0; i < 2; ++i) {
    const std::string p = "linear." + std::to_string(i) + ".";
    const int K = i == 0 ? 2 * SH : SH;
    lin_[i].w = store_.upload(get(p + "weight", (size_t)SH * K), (size_t)SH * K);
    lin_[i].b = store_.upload(get(p + "bias", SH), SH);
    lin_[i].N = SH;
    lin_[i].K = K;
  }
  cls_.w = store_.upload(get("classifier.weight", (size_t)kSegClasses * SH), (size_t)kSegClasses * SH);
  cls_.b = store_.upload(get("classifier.bias", kSegClasses), kSegClasses);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  // last: nothing after it can throw, so a failed construction leaks no stream (the weights
  // above belong to store_, which is destroyed with the partly built object)
  ZASR_HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
}

// Frees the activation workspace (up to the 8 GiB bound after a long file); the next call
// allocates what it needs again.
void SegEngine::trim() {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  ws_.clear();
}

SegEngine::~SegEngine() {
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(st_);
  (void)hipStreamDestroy(st_);  // (store_ and ws_ free their buffers after this body)
}

// Sequences per recurrence workgroup: a launch of 2 ceil(n / B) workgroups (one per CU at a
// time: 128 weight registers per thread) takes ceil(workgroups / CUs) rounds, and a round's
// steps cost about (0.3 + B) units -- measured on an hour (719 chunks, 256 CUs,
// profiles/segmentation/): 2.1 / 4.1 / 7.3 / 13.8 / 26.8 ms per round at B = 1 / 2 / 4 / 8 / 16,
// so the barriers and the h broadcast shared by a group are a small part of a step and what B
// buys is fewer, fuller rounds.  The smallest B with the least rounds x cost: 1 for a short
// file, 2 for an hour (12.2 ms against 12.8 at B = 1 and 13.8 at B = 8).
int SegEngine::pick_group(int n) const {
  if (forced_group_ > 0) return forced_group_;
  int best = 1;
  long best_cost = -1;
  for (int B = 1; B <= kSegMaxGroup; B *= 2) {
    const long wgs = 2L * cdiv(n, B), cost = cdivl(wgs, cus_) * (3 + 10 * B);
    if (best_cost < 0 || cost < best_cost) {
      best = B;
      best_cost = cost;
    }
  }
  return best;
}

void SegEngine::mark(int stage) {
  if (!profile_) return;
  hipEvent_t ev;
  ZASR_HIP_CHECK(hipEventCreate(&ev));
  ZASR_HIP_CHECK(hipEventRecord(ev, st_));
  marks_.emplace_back(ev, stage);
}

void SegEngine::collect_marks() {
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

void SegEngine::run_group(const float* d_audio, long total, const long* d_starts, int ng, int T,
                          float* d_logits, unsigned char* d_classes) {
  const int l0 = (T - kSegTaps) / kSegStride0 + 1, f1 = l0 / 3, l1 = f1 - SK + 1, f2 = l1 / 3,
            l2 = f2 - SK + 1, F = l2 / 3;
  mark(-1);
  float2* cst = ws<float2>("chunk_stats", (size_t)ng);
  float2* fst = ws<float2>("frame_stats", (size_t)ng * kSegC0);
  launch_seg_chunk_stats(d_audio, total, d_starts, ng, T, cst, st_);
  float* P0 = ws<float>("p0", (size_t)ng * f1 * kSegC0);
  SegFrontArgs fa{};
  fa.audio = d_audio;
  fa.total = total;
  fa.starts = d_starts;
  fa.stats = cst;
  fa.in_w = in_w_;
  fa.in_b = in_b_;
  fa.w0t = w0t_;
  fa.out = P0;
  fa.T = T;
  fa.F1 = f1;
  launch_seg_front(fa, ng, st_);
  launch_seg_frame_stats(P0, ng, f1, kSegC0, fst, st_);
  launch_seg_norm_act(P0, ng, f1, kSegC0, fst, norm_[0].w, norm_[0].b, st_);
  mark(0);
  // conv_1 / conv_2: implicit-im2col GEMM, then pool, statistics, normalise + leaky_relu
  auto conv = [&](const Lin& l, const float* X, int Tin, int C, int Tout, int Fp, const Norm& nm,
                  const char* yname, const char* pname) {
    float* Y = ws<float>(yname, (size_t)ng * Tout * l.N);
    GemmParams p = dense_gemm_params(l.w, l.b, l.N, l.K, X, C, ng * Tout, Y, l.N);
    p.i2c.Tin = Tin;
    p.i2c.Tout = Tout;
    p.i2c.C = C;
    gemm_f32(p, EPI_NONE, ALOAD_IM2COL1D, false, st_);
    float* P = ws<float>(pname, (size_t)ng * Fp * l.N);
    launch_seg_pool3(Y, ng, Tout, l.N, Fp, P, st_);
    launch_seg_frame_stats(P, ng, Fp, l.N, fst, st_);
    launch_seg_norm_act(P, ng, Fp, l.N, fst, nm.w, nm.b, st_);
    return P;
  };
  const float* P1 = conv(conv_[0], P0, f1, kSegC0, l1, f2, norm_[1], "y1", "p1");
  const float* X = conv(conv_[1], P1, f2, SC1, l2, F, norm_[2], "y2", "p2");
  mark(1);
  const long rows = (long)ng * F;
  auto dense = [&](const Lin& l, const float* A, float* C, int epi) {
    const GemmParams p = dense_gemm_params(l.w, l.b, l.N, l.K, A, l.K, (int)rows, C, l.N);
    gemm_f32(p, epi, ALOAD_DENSE, false, st_);
  };
  float* GX = ws<float>("gx", (size_t)rows * 8 * SH);
  float* Hb[2] = {ws<float>("h0", (size_t)rows * 2 * SH), ws<float>("h1", (size_t)rows * 2 * SH)};
  last_group_ = pick_group(ng);
  for (int l = 0; l < 4; ++l) {
    dense(ih_[l], X, GX, EPI_NONE);
    mark(2);
    SegLstmArgs la{};
    la.gx = GX;
    la.whh = whh_[l];
    la.out = Hb[l & 1];
    la.n = ng;
    la.F = F;
    launch_seg_lstm(la, last_group_, st_);
    mark(3);
    X = Hb[l & 1];
  }
  float* L1 = ws<float>("lin1", (size_t)rows * SH);
  float* L2 = ws<float>("lin2", (size_t)rows * SH);
  dense(lin_[0], X, L1, EPI_LEAKY);
  dense(lin_[1], L1, L2, EPI_LEAKY);
  launch_seg_head(L2, rows, cls_.w, cls_.b, d_logits, d_classes, st_);
  mark(4);
}

void SegEngine::run(const float* d_audio, long total, const std::vector<long>& starts, int T,
                    float* d_logits, unsigned char* d_classes) {
  const int n = (int)starts.size(), F = num_frames(T);
  long* d_starts = ws<long>("starts", (size_t)n);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_starts, starts.data(), (size_t)n * 8, hipMemcpyHostToDevice, st_));
  const int per = (int)std::max<size_t>(1, std::min<size_t>(kWorkspaceBound / chunk_bytes(T), 32768));
  for (int k0 = 0; k0 < n; k0 += per) {
    const int ng = std::min(per, n - k0);
    run_group(d_audio, total, d_starts + k0, ng, T, d_logits + (size_t)k0 * F * kSegClasses,
              d_classes + (size_t)k0 * F);
  }
  collect_marks();
}

void SegEngine::logits_host(const float* batch, int n, int T, float* logits) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const int F = num_frames(T);
  ZASR_REQUIRE(n > 0 && T >= kMinSamples && F >= 2, "segmentation: bad batch shape");
  ZASR_REQUIRE((long)n * T < (1L << 40), "segmentation: batch too large");
  const long total = (long)n * T;
  float* d_audio = ws<float>("audio", (size_t)total);
  float* d_logits = ws<float>("logits", (size_t)n * F * kSegClasses);
  unsigned char* d_cls = ws<unsigned char>("classes", (size_t)n * F);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_audio, batch, (size_t)total * 4, hipMemcpyHostToDevice, st_));
  std::vector<long> starts(n);
  for (int k = 0; k < n; ++k) starts[k] = (long)k * T;
  run(d_audio, total, starts, T, d_logits, d_cls);
  ZASR_HIP_CHECK(hipMemcpyAsync(logits, d_logits, (size_t)n * F * kSegClasses * 4,
                                hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void SegEngine::classes_device(const float* d_audio, long total, int chunk, int step,
                               unsigned char* classes, float* d_logits, hipStream_t user_stream) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const int F = num_frames(chunk);
  ZASR_REQUIRE(chunk >= kMinSamples && F >= 2 && step > 0 && total >= 0,
               "segmentation: bad chunk geometry");
  const std::vector<long> starts = chunk_starts(total, chunk, step);
  if (starts.empty()) return;
  const size_t n = starts.size();
  if (user_stream) {  // order after the caller's producer of d_audio
    hipEvent_t ev;
    ZASR_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZASR_HIP_CHECK(hipEventRecord(ev, user_stream));
    ZASR_HIP_CHECK(hipStreamWaitEvent(st_, ev, 0));
    ZASR_HIP_CHECK(hipEventDestroy(ev));
  }
  float* dl = d_logits ? d_logits : ws<float>("logits", n * F * kSegClasses);
  unsigned char* d_cls = ws<unsigned char>("classes", n * F);
  run(d_audio, total, starts, chunk, dl, d_cls);
  ZASR_HIP_CHECK(hipMemcpyAsync(classes, d_cls, n * F, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

}  // namespace zasr
