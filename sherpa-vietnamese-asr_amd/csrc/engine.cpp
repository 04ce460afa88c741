// libzasr host runtime: construction, uploads and profiling, the linear building blocks, the
// fbank stage, the batch pipeline and the public entry points.  Model load, the encoder driver
// and the search driver are engine_load.cpp, engine_encoder.cpp and engine_search.cpp.
//
// Reference mapping:
//   load + session setup    core/asr_engine.py:903-1020 (create_recognizer)
//   fbank                   core/asr_engine.py:698-721
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <sstream>

#include "common.h"
#include "dense_gemm.h"
#include "host_io.h"
#include "onnx_io.h"

namespace zasr {

namespace {

ModelConfig parse_config(const std::string& text) {
  Json j = Json::parse(text);
  ModelConfig c;
  c.name = j.has("name") ? j.at("name").str : "zipformer";
  c.dims = j.at("encoder_dims").as_int_vec();
  c.layers = j.at("num_layers").as_int_vec();
  c.ff = j.at("ff_dims").as_int_vec();
  c.heads = j.at("num_heads").as_int_vec();
  c.ds = j.at("downsampling").as_int_vec();
  c.kernels = j.at("cnn_kernels").as_int_vec();
  c.qd = (int)j.at("query_head_dim").num;
  c.vd = (int)j.at("value_head_dim").num;
  c.pd = (int)j.at("pos_head_dim").num;
  c.pos_dim = (int)j.at("pos_dim").num;
  c.V = (int)j.at("vocab_size").num;
  c.dec_dim = (int)j.at("decoder_dim").num;
  c.joiner_dim = (int)j.at("joiner_dim").num;
  c.context = (int)j.at("context_size").num;
  if (j.has("layer1_channels")) c.c1 = (int)j.at("layer1_channels").num;
  if (j.has("layer2_channels")) c.c2 = (int)j.at("layer2_channels").num;
  if (j.has("layer3_channels")) c.c3 = (int)j.at("layer3_channels").num;
  ZASR_REQUIRE(c.qd == 32 && c.pd == 4, "kernels are specialised for query_head_dim 32, pos_head_dim 4");
  ZASR_REQUIRE(c.c1 == 8 && c.c2 == 32 && c.c3 == 128, "Conv2dSubsampling channels must be 8/32/128");
  ZASR_REQUIRE(c.context == 2, "decoder context_size must be 2");
  ZASR_REQUIRE(c.dec_dim == c.joiner_dim, "decoder_dim must equal joiner_dim");
  size_t ns = c.dims.size();
  ZASR_REQUIRE(c.layers.size() == ns && c.ff.size() == ns && c.heads.size() == ns &&
                   c.ds.size() == ns && c.kernels.size() == ns,
               "inconsistent stack config");
  for (size_t i = 0; i < ns; ++i) {
    ZASR_REQUIRE(c.dims[i] % 16 == 0, "encoder dims must be multiples of 16");
    ZASR_REQUIRE(c.ds[i] >= 1 && c.ds[i] <= 8, "downsampling factor must be 1..8");
  }
  return c;
}

}  // namespace

// ------------------------------------------------------------------------------------
// Engine
// ------------------------------------------------------------------------------------

void Engine::upload(void* dst, const void* src, size_t bytes) {
  // staged through the current pinned arena: a copy from pinned memory is truly
  // asynchronous, so enqueueing the next batch's encoder never waits for the stream (the
  // arena of a pipeline slot is reset only after that slot's previous batch has completed)
  PinArena& a = pin_[pin_cur_];
  const size_t need = (bytes + 255) & ~size_t(255);
  if (a.used + need <= a.cap) {
    char* h = a.p + a.used;
    a.used += need;
    std::memcpy(h, src, bytes);
    ZASR_HIP_CHECK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st_));
    return;
  }
  a.want += need;  // grown at the arena's next reset
  // pageable source: HIP stages the copy before returning, so `src` may be reused
  ZASR_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st_));
}

void Engine::pin_reset(int arena) {
  // callers guarantee every earlier copy out of this arena has executed
  PinArena& a = pin_[arena];
  const size_t want = std::max(a.want + a.used, a.cap);
  if (want > a.cap) {
    if (a.p) ZASR_HIP_CHECK(hipHostFree(a.p));
    a.cap = want + want / 4 + 4096;
    ZASR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&a.p), a.cap, hipHostMallocDefault));
  }
  a.used = 0;
  a.want = 0;
  pin_cur_ = arena;
}

Engine::Engine(const std::string& dir, int device, int beam, bool greedy,
               const std::vector<std::vector<int>>& hotwords, const std::vector<float>& hotword_scores,
               int precision)
    : device_(device), beam_(beam), greedy_(greedy) {
  ZASR_REQUIRE(precision >= 0 && precision <= 5,
               "precision must be 0 (fp32), 1 (bf16), 2 (bf16 encoder, f32 joiner + search), 3 "
               "(bf16x3: two-piece split-bf16 products), 4 (bf16x6: three-piece, f32 quality) or "
               "5 (f16x3: fp16 hi + scaled lo pieces, f32 quality)");
  prec_ = PrecisionFacts(static_cast<Precision>(precision));
  // host side first (no GPU state to unwind when the files are bad): config.json +
  // model.safetensors, or the reference's encoder-/decoder-/joiner-*.onnx (onnx_io.h;
  // core/asr_engine.py:913-928)
  SafeTensors W;
  model_.cfg = parse_config(load_model_dir(dir, W));
  hw_host_ = build_hotword_dfa(hotwords, hotword_scores, model_.cfg.V);
  ZASR_HIP_CHECK(hipSetDevice(device_));
  // ZASR_SEARCH_CUS = N > 0: the search stream runs on CUs [0, N) and the encoder streams on
  // the rest (CU-masked queues), so the latency-bound search chain never waits for CUs held
  // by the next batch's encoder blocks
  if (const char* e = getenv("ZASR_SEARCH_CUS")) search_cus_ = atoi(e);
  int ncu = 0;
  ZASR_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device_));
  if (search_cus_ > 0 && search_cus_ < ncu) {
    std::vector<uint32_t> ms((ncu + 31) / 32, 0u), me((ncu + 31) / 32, 0u);
    for (int c = 0; c < ncu; ++c) (c < search_cus_ ? ms : me)[c / 32] |= 1u << (c % 32);
    ZASR_HIP_CHECK(hipExtStreamCreateWithCUMask(&stream2_, (uint32_t)ms.size(), ms.data()));
    ZASR_HIP_CHECK(hipExtStreamCreateWithCUMask(&stream3_, (uint32_t)ms.size(), ms.data()));
    ZASR_HIP_CHECK(hipExtStreamCreateWithCUMask(&stream_, (uint32_t)me.size(), me.data()));
    for (auto& x : enc_extra_)
      ZASR_HIP_CHECK(hipExtStreamCreateWithCUMask(&x, (uint32_t)me.size(), me.data()));
  } else {
    search_cus_ = 0;
    ZASR_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    int least = 0, greatest = 0;
    ZASR_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    ZASR_HIP_CHECK(hipStreamCreateWithPriority(&stream2_, hipStreamNonBlocking, greatest));
    ZASR_HIP_CHECK(hipStreamCreateWithPriority(&stream3_, hipStreamNonBlocking, greatest));
    for (auto& x : enc_extra_) ZASR_HIP_CHECK(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
    // stream4_ (a third beam search in flight) is created on first use only: streams share
    // the process's hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order, and
    // one created ahead of the encoder streams put the second encoder stream on a shared
    // queue (greedy pipeline 107.5k -> 97.5k xRT, measured)
  }
  for (auto& e : part_ev_) ZASR_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  st_ = stream_;
  load_model(W);
  ZASR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h_pinned_), 64, hipHostMallocDefault));
  ZASR_HIP_CHECK(hipDeviceSynchronize());
}

// sparse rows: first nonzero bin, run length, offset into the packed weights
void pack_mel_banks(const float* banks, int n_bins, std::vector<int>& meta,
                    std::vector<float>& wts) {
  meta.assign(240, 0);
  wts.clear();
  for (int b = 0; b < 80; ++b) {
    const float* row = banks + (size_t)b * n_bins;
    int st = -1, en = -1;
    for (int i = 0; i < 256; ++i)
      if (row[i] != 0.f) {
        if (st < 0) st = i;
        en = i;
      }
    if (st < 0) st = en = 0;
    meta[b] = st;
    meta[80 + b] = en - st + 1;
    meta[160 + b] = (int)wts.size();
    for (int i = st; i <= en; ++i) wts.push_back(row[i]);
  }
}

void Engine::set_mel_banks(const float* banks, int n_bins) {
  ZASR_REQUIRE(n_bins == 256 || n_bins == 257, "mel banks: 256 or 257 bins per filter");
  for (int b = 0; n_bins == 257 && b < 80; ++b)
    ZASR_REQUIRE(banks[(size_t)b * 257 + 256] == 0.f, "mel banks: the Nyquist bin must carry no weight");
  std::vector<int> meta;
  std::vector<float> wts;
  pack_mel_banks(banks, n_bins, meta, wts);
  ZASR_HIP_CHECK(hipDeviceSynchronize());  // no fbank in flight reads the old tables
  if (!d_mel_meta_) ZASR_HIP_CHECK(hipMalloc(&d_mel_meta_, 240 * sizeof(int)));
  ZASR_HIP_CHECK(hipMemcpy(d_mel_meta_, meta.data(), 240 * sizeof(int), hipMemcpyHostToDevice));
  if (d_mel_w_) ZASR_HIP_CHECK(hipFree(d_mel_w_));
  d_mel_w_ = nullptr;
  ZASR_HIP_CHECK(hipMalloc(&d_mel_w_, wts.size() * sizeof(float)));
  ZASR_HIP_CHECK(hipMemcpy(d_mel_w_, wts.data(), wts.size() * sizeof(float), hipMemcpyHostToDevice));
}

std::string Engine::routes_json() const {
  std::ostringstream os;
  os << "{\"precision\": " << (int)prec_.mode << ", \"ffn_fused_h3\": " << routes_.ffn_fused_h3
     << ", \"ffn_gemm_pair\": " << routes_.ffn_gemm_pair << ", \"gemm_h3r\": " << routes_.gemm_h3r
     << ", \"gemm_x3_range\": " << routes_.gemm_x3_range << ", \"cnx_ffn_h3\": " << routes_.cnx_ffn_h3
     << ", \"dec_table\": " << (model_.dec_table ? 1 : 0) << "}";
  return os.str();
}

Engine::~Engine() {
  // best-effort teardown: errors here cannot be reported to the caller
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(stream_);
  // (store_ and ws_ free their buffers after this body)
  for (auto& s : model_.stacks)
    for (auto& l : s.layers)
      if (l.pos_tab) (void)hipFree(l.pos_tab);
  if (d_mel_meta_) (void)hipFree(d_mel_meta_);
  if (d_mel_w_) (void)hipFree(d_mel_w_);
  for (auto e : event_pool_) (void)hipEventDestroy(e);
  for (auto& pe : prof_pending_) {
    (void)hipEventDestroy(pe.a);
    (void)hipEventDestroy(pe.b);
  }
  if (copy_st_) (void)hipStreamSynchronize(copy_st_);
  for (auto e : upload_ev_)
    if (e) (void)hipEventDestroy(e);
  if (copy_st_) (void)hipStreamDestroy(copy_st_);
  (void)hipStreamSynchronize(stream2_);
  (void)hipStreamSynchronize(stream3_);
  if (stream4_) (void)hipStreamSynchronize(stream4_);
  if (h_pinned_) (void)hipHostFree(h_pinned_);
  for (auto& r : res_pin_)
    if (r.p) (void)hipHostFree(r.p);
  for (auto& a : pin_)
    if (a.p) (void)hipHostFree(a.p);
  for (auto e : part_ev_) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(stream2_);
  (void)hipStreamDestroy(stream3_);
  if (stream4_) (void)hipStreamDestroy(stream4_);
  for (auto x : enc_extra_) {
    (void)hipStreamSynchronize(x);
    (void)hipStreamDestroy(x);
  }
  (void)hipStreamDestroy(stream_);
}

// CompactRelPositionalEncoding (icefall zipformer.py, 3P) folded through linear_pos:
// table[x + pmax - 1][n] = sum_c W_pos[n][c] * pe(x)[c]
void Engine::ensure_pos_tables(int need) {
  if (need <= model_.pmax) return;
  // the tables are shared by every encoder stream: replace them only on an idle device
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  int pmax = 1024;
  while (pmax < need) pmax *= 2;
  const int P = model_.cfg.pos_dim;
  const int rows = 2 * pmax - 1;
  std::vector<double> pe((size_t)rows * P);
  const double cl = std::sqrt((double)P);
  const double ls = P / (2.0 * M_PI);
  for (int r = 0; r < rows; ++r) {
    double x = (double)(r - (pmax - 1));
    double sgn = (x > 0) - (x < 0);
    double xc = cl * sgn * (std::log(std::fabs(x) + cl) - std::log(cl));
    double xa = std::atan(xc / ls);
    for (int i = 0; i < P / 2; ++i) {
      pe[(size_t)r * P + 2 * i] = std::cos(xa * (i + 1));
      pe[(size_t)r * P + 2 * i + 1] = std::sin(xa * (i + 1));
    }
    pe[(size_t)r * P + P - 1] = 1.0;
  }
  for (auto& s : model_.stacks) {
    const int n4 = 4 * s.h;
    for (auto& l : s.layers) {
      std::vector<float> tab((size_t)rows * n4);
      for (int r = 0; r < rows; ++r)
        for (int n = 0; n < n4; ++n) {
          double acc = 0;
          const double* pr = &pe[(size_t)r * P];
          const float* wr = &l.pos_w[(size_t)n * P];
          for (int c = 0; c < P; ++c) acc += (double)wr[c] * pr[c];
          tab[(size_t)r * n4 + n] = (float)acc;
        }
      if (l.pos_tab) {
        ZASR_HIP_CHECK(hipStreamSynchronize(st_));
        ZASR_HIP_CHECK(hipFree(l.pos_tab));
      }
      ZASR_HIP_CHECK(hipMalloc(&l.pos_tab, tab.size() * sizeof(float)));
      ZASR_HIP_CHECK(hipMemcpy(l.pos_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  model_.pmax = pmax;
}

// ------------------------------------------------------------------------------------
// profiling
// ------------------------------------------------------------------------------------
hipEvent_t Engine::take_event() {
  if (!event_pool_.empty()) {
    hipEvent_t e = event_pool_.back();
    event_pool_.pop_back();
    return e;
  }
  hipEvent_t e;
  ZASR_HIP_CHECK(hipEventCreate(&e));
  return e;
}

void Engine::prof_begin(const char* name) { prof_begin(std::string(name)); }

void Engine::prof_begin(const std::string& name) {
  if (!prof_on_) return;
  ProfEvent pe{name, take_event(), take_event()};
  ZASR_HIP_CHECK(hipEventRecord(pe.a, st_));
  prof_pending_.push_back(pe);
}

void Engine::prof_end() {
  if (!prof_on_ || prof_pending_.empty()) return;
  ZASR_HIP_CHECK(hipEventRecord(prof_pending_.back().b, st_));
}

void Engine::profile_reset() {
  prof_acc_.clear();
  for (auto& pe : prof_pending_) {
    event_pool_.push_back(pe.a);
    event_pool_.push_back(pe.b);
  }
  prof_pending_.clear();
}

std::string Engine::profile_report() {
  for (auto& pe : prof_pending_) {
    ZASR_HIP_CHECK(hipEventSynchronize(pe.b));
    float ms = 0.f;
    ZASR_HIP_CHECK(hipEventElapsedTime(&ms, pe.a, pe.b));
    auto& acc = prof_acc_[pe.name];
    acc.first += 1;
    acc.second += ms;
    event_pool_.push_back(pe.a);
    event_pool_.push_back(pe.b);
  }
  prof_pending_.clear();
  std::ostringstream os;
  for (auto& kv : prof_acc_) os << kv.first << " " << kv.second.first << " " << kv.second.second << "\n";
  return os.str();
}

// per-shape GEMM class names (profile mode 2): "<class>|M|K|N|w16|a16|c16|epi", parsed by
// bench.py into the per-shape roofline table
std::string Engine::shape_key(const char* cls, int M, int K, int N, bool w16, bool a16, bool c16,
                              int epi) {
  std::ostringstream os;
  os << cls << "|" << M << "|" << K << "|" << N << "|" << (int)w16 << "|" << (int)a16 << "|"
     << (int)c16 << "|" << epi;
  return os.str();
}

// ------------------------------------------------------------------------------------
// building blocks
// ------------------------------------------------------------------------------------
void Engine::linear(const DLin& l, const float* A, int lda, int M, float* C, int ldc, int epi,
                    const char* cls, const float* byp_orig, const float* byp_scale) {
  ZASR_REQUIRE(byp_orig == nullptr || l.wx, "bypass epilogue: split-mode weights only");
  GemmParams p = dense_gemm_params(l.w, l.b, l.N, l.K, A, lda, M, C, ldc);
  p.byp_orig = byp_orig;
  p.byp_scale = byp_scale;
  if (prof_shapes_ && prof_on_)
    prof_begin(shape_key(cls, M, l.K, l.N, l.wh != nullptr, false, false, epi));
  else
    prof_begin(cls);
  if (l.wr && lda == l.K && byp_orig == nullptr && gemm_h3r_supported(l.K, l.N, epi))
    gemm_h3r(A, l.wr, l.b, C, ldc, M, l.N, l.K, epi, st_);
  else if (l.wx)
    gemm_x3(p, l.wx, (long)l.N * l.K, epi, ALOAD_DENSE, st_, prec_.pieces);
  else if (l.wh)
    gemm_bf16(p, l.wh, epi, ALOAD_DENSE, st_);
  else
    gemm_f32(p, epi, ALOAD_DENSE, false, st_);
  prof_end();
}

void Engine::linear_h(const DLin& l, const void* A, bool a_bf16, int lda, int M, void* C,
                      bool c_bf16, int ldc, int epi, const float* byp_orig,
                      const float* byp_scale) {
  ZASR_REQUIRE(l.wh != nullptr, "linear_h needs bf16 weights");
  GemmParams p = dense_gemm_params(l.w, l.bh ? l.bh : l.b, l.N, l.K, A, lda, M, C, ldc);
  p.byp_orig = byp_orig;
  p.byp_scale = byp_scale;
  if (prof_shapes_ && prof_on_)
    prof_begin(shape_key("enc_gemm", M, l.K, l.N, true, a_bf16, c_bf16, epi));
  else
    prof_begin("enc_gemm");
  gemm_bf16(p, l.wh, epi, ALOAD_DENSE, st_, a_bf16, c_bf16);
  prof_end();
}

void Engine::run_fbank(const float* d_wav, const std::vector<long>& wav_off,
                       const std::vector<long>& n, float* d_feats, std::vector<int>& frames) {
  const int B = (int)n.size();
  std::vector<long> off(B);
  std::vector<int> ns(B), fo(B + 1, 0);
  frames.resize(B);
  for (int b = 0; b < B; ++b) {
    off[b] = wav_off[b];
    ns[b] = (int)n[b];
    frames[b] = n[b] > 0 ? (int)((n[b] + 80) / 160) : 0;
    fo[b + 1] = fo[b] + frames[b];
  }
  long* d_off = ws<long>("fb_wavoff", B);
  int* d_meta = ws<int>("fb_meta", 2 * B + 1);
  std::vector<int> meta(ns);
  meta.insert(meta.end(), fo.begin(), fo.end());
  upload(d_off, off.data(), B * sizeof(long));
  upload(d_meta, meta.data(), meta.size() * sizeof(int));
  FbankTables t{d_twiddle_, d_window_, d_mel_meta_, d_mel_meta_ + 80, d_mel_meta_ + 160, d_mel_w_};
  prof_begin("fbank");
  launch_fbank(d_wav, d_off, d_meta, d_meta + B, B, fo[B], t, d_feats, st_);
  prof_end();
}


// ------------------------------------------------------------------------------------
// public entry points
// ------------------------------------------------------------------------------------
void Engine::encode_stage(const float* d_wav, const std::vector<long>& wav_off,
                          const std::vector<long>& n, int out_slot, int ws_slot,
                          hipStream_t stream, Pending& pd) {
  st_ = stream;
  pin_reset(out_slot);
  ws_tag_ = ws_slot ? "w" + std::to_string(ws_slot) + "/" : "";
  const int B = (int)n.size();
  pd = Pending{};
  pd.B = B;
  pd.ready = part_ev_[out_slot];
  std::vector<int> frames;
  long total_frames = 0;
  for (int b = 0; b < B; ++b) total_frames += n[b] > 0 ? (n[b] + 80) / 160 : 0;
  float* feats = ws<float>("feats", (size_t)std::max<long>(total_frames, 1) * 80);
  std::vector<long> off_dev(wav_off);
  if (host_wav_) {
    // this batch's span of the host signal -> the output slot's device buffer, on the copy
    // stream; the slot's previous batch has been searched, so its fbank is done with the buffer
    long lo = -1, hi = 0;
    for (int b = 0; b < B; ++b)
      if (n[b] > 0) {
        lo = lo < 0 ? wav_off[b] : std::min(lo, wav_off[b]);
        hi = std::max(hi, wav_off[b] + n[b]);
      }
    if (lo >= 0) {
      float* buf = ws<float>("wav_in" + std::to_string(out_slot), (size_t)(hi - lo));
      if (!copy_st_) ZASR_HIP_CHECK(hipStreamCreateWithFlags(&copy_st_, hipStreamNonBlocking));
      if (!upload_ev_[out_slot])
        ZASR_HIP_CHECK(hipEventCreateWithFlags(&upload_ev_[out_slot], hipEventDisableTiming));
      ZASR_HIP_CHECK(hipMemcpyAsync(buf, host_wav_ + lo, (size_t)(hi - lo) * sizeof(float),
                                    hipMemcpyHostToDevice, copy_st_));
      ZASR_HIP_CHECK(hipEventRecord(upload_ev_[out_slot], copy_st_));
      ZASR_HIP_CHECK(hipStreamWaitEvent(st_, upload_ev_[out_slot], 0));
      for (int b = 0; b < B; ++b) off_dev[b] = n[b] > 0 ? wav_off[b] - lo : 0;
      d_wav = buf;
    }
  }
  run_fbank(d_wav, off_dev, n, feats, frames);
  // chunks too short for the encoder produce empty results (T' = 0)
  std::vector<int> T;
  std::vector<long> foff(B + 1, 0);
  for (int b = 0; b < B; ++b) foff[b + 1] = foff[b] + frames[b];
  for (int b = 0; b < B; ++b)
    if (frames[b] >= 9) {
      pd.valid.push_back(b);
      T.push_back(frames[b]);
    }
  if (pd.valid.empty()) {
    ws_tag_.clear();
    return;
  }
  const float* fptr = feats;
  if ((int)pd.valid.size() != B) {  // compact valid chunks' features
    float* cf = ws<float>("feats_compact", (size_t)total_frames * 80);
    long pos = 0;
    for (int b : pd.valid) {
      ZASR_HIP_CHECK(hipMemcpyAsync(cf + pos * 80, feats + foff[b] * 80, (size_t)frames[b] * 80 * 4,
                                    hipMemcpyDeviceToDevice, st_));
      pos += frames[b];
    }
    fptr = cf;
  }
  long tot_out = 0;
  for (int t : T) tot_out += ((t - 7) / 2 + 1) / 2;
  // the encoder output is the only buffer the search reads: one per pipeline slot
  pd.enc = ws<float>("enc_out" + std::to_string(out_slot),
                     (size_t)std::max<long>(tot_out, 1) * model_.cfg.joiner_dim);
  run_encoder(fptr, T, pd.enc, pd.t_out);
  ZASR_HIP_CHECK(hipEventRecord(pd.ready, st_));
  ws_tag_.clear();
}

std::vector<TokenResult> Engine::search_stage(Pending& pd, int beam) {
  std::vector<TokenResult> out(pd.B);
  if (pd.valid.empty()) return out;
  hipStream_t main_st = st_;
  st_ = stream2_;
  ZASR_HIP_CHECK(hipStreamWaitEvent(stream2_, pd.ready, 0));
  std::vector<TokenResult> r = run_search(pd.enc, pd.t_out, beam);
  for (size_t i = 0; i < pd.valid.size(); ++i) out[pd.valid[i]] = std::move(r[i]);
  // the call's stream sees the search complete (its results are already on the host)
  ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 1], stream2_));
  ZASR_HIP_CHECK(hipStreamWaitEvent(main_st, part_ev_[kMaxEnc + 1], 0));
  st_ = main_st;
  return out;
}

std::vector<TokenResult> Engine::decode_device(const float* d_wav, const std::vector<long>& wav_off,
                                               const std::vector<long>& n, int beam,
                                               hipStream_t st) {
  return decode_device_batches(d_wav, wav_off, n, {(int)n.size()}, beam, st);
}

std::vector<TokenResult> Engine::decode_host_batches(const float* h_wav,
                                                     const std::vector<long>& wav_off,
                                                     const std::vector<long>& n,
                                                     const std::vector<int>& batch_sizes,
                                                     int beam, hipStream_t st) {
  struct Reset {
    const float** p;
    ~Reset() { *p = nullptr; }
  } reset{&host_wav_};
  host_wav_ = h_wav;
  return decode_device_batches(nullptr, wav_off, n, batch_sizes, beam, st);
}

std::vector<TokenResult> Engine::decode_device_batches(const float* d_wav,
                                                       const std::vector<long>& wav_off,
                                                       const std::vector<long>& n,
                                                       const std::vector<int>& batch_sizes,
                                                       int beam, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  long total = 0;
  for (int c : batch_sizes) {
    ZASR_REQUIRE(c >= 0, "negative batch size");
    total += c;
  }
  ZASR_REQUIRE(total == (long)n.size() && wav_off.size() == n.size(),
               "batch sizes must sum to the chunk count");
  hipStream_t main_st = st ? st : stream_;
  st_ = main_st;
  std::vector<TokenResult> out;
  out.reserve(n.size());
  // E encoder streams; L (= E + 1 by default, below) batches' encoders are enqueued ahead of
  // the search in flight.
  // Batch k: encoder output / event / pinned arena slot k % (L + 1), stream + workspace set
  // k % E.  When batch k + L is enqueued, the previous user of its output slot (batch k - 1)
  // has been searched (the search returns on the host), and its stream's previous batch
  // (k + L - E) is ordered before it on the same stream.
  // Greedy: the encoder is the critical path, a second encoder stream fills its kernel tails
  // (98.4k vs 95.3k xRT).  Beam search: the search is the critical path and a second encoder
  // stream only adds contention for it (69.9k vs 68.3k xRT at beam 8 + 20 hotwords).
  static const int env_e = getenv("ZASR_ENC_STREAMS") ? atoi(getenv("ZASR_ENC_STREAMS")) : 0;
  const int nb = (int)batch_sizes.size();
  // Beam search: several batches' searches in flight (ZASR_SEARCH_JOBS, default 2).  Each
  // batch's frame chain is latency-bound (joiner -> search step per frame, a few hundred
  // blocks), so further chains on the other search streams run beside it at nearly the same
  // per-frame latency.
  static const int env_jobs = getenv("ZASR_SEARCH_JOBS") ? atoi(getenv("ZASR_SEARCH_JOBS")) : 2;
  if (beam > 1 && env_jobs >= 2 && nb >= 2 && search_cus_ == 0)
    return decode_batches_two_searches(d_wav, wav_off, n, batch_sizes, beam, main_st);
  const int want_e = env_e ? env_e : (beam > 1 ? 1 : 2);
  const int E = std::max(1, std::min({want_e, (int)kMaxEnc, nb - 1}));
  // a second encoder stream: the persistent kernels leave 1/8 of the CUs to it (common.h)
  const PersistShare share(E > 1);
  // L: batches whose encoders are queued ahead of the search in flight, one more than the
  // encoder streams (at most kMaxEnc: L + 1 output slots): 111.8-113.1k -> 113.5-114.3k xRT
  // on one box (profiles/r03/enc_ahead/)
  const int L = std::max(E, std::min({E + 1, (int)kMaxEnc, nb}));
  // encoder stream 0 is the caller's stream, or (CU-partitioned) the engine's masked stream
  hipStream_t enc_st[kMaxEnc] = {search_cus_ > 0 ? stream_ : main_st};
  for (int e = 1; e < kMaxEnc; ++e) enc_st[e] = enc_extra_[e - 1];
  if (E > 1 || enc_st[0] != main_st) {  // the encoder streams start after the caller's prior work
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 2], main_st));
    for (int e = 0; e < E; ++e)
      if (enc_st[e] != main_st) ZASR_HIP_CHECK(hipStreamWaitEvent(enc_st[e], part_ev_[kMaxEnc + 2], 0));
  }
  std::vector<long> first(nb + 1, 0);
  for (int k = 0; k < nb; ++k) first[k + 1] = first[k] + batch_sizes[k];
  Pending pd[kMaxEnc + 1];
  auto enqueue = [&](int k) {
    std::vector<long> o(wav_off.begin() + first[k], wav_off.begin() + first[k + 1]);
    std::vector<long> l(n.begin() + first[k], n.begin() + first[k + 1]);
    encode_stage(d_wav, o, l, k % (L + 1), k % E, enc_st[k % E], pd[k % (L + 1)]);
    st_ = main_st;
  };
  for (int k = 0; k < std::min(L, nb); ++k) enqueue(k);
  for (int k = 0; k < nb; ++k) {
    if (k + L < nb) enqueue(k + L);
    std::vector<TokenResult> r = search_stage(pd[k % (L + 1)], beam);
    for (auto& x : r) out.push_back(std::move(x));
  }
  order_after_encoders(enc_st, E, main_st);
  st_ = stream_;
  return out;
}

void Engine::order_after_encoders(const hipStream_t* enc_st, int E, hipStream_t main_st) {
  // the caller's stream must not run ahead of an encoder stream that read its audio: a batch
  // without valid chunks is never searched, so nothing else orders its fbank / encoder work
  // (on a CU-masked stream_ or a second encoder stream) before the caller reuses the buffer
  for (int e = 0; e < E; ++e) {
    if (enc_st[e] == main_st) continue;
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 2], enc_st[e]));
    ZASR_HIP_CHECK(hipStreamWaitEvent(main_st, part_ev_[kMaxEnc + 2], 0));
  }
}

std::vector<TokenResult> Engine::decode_batches_two_searches(const float* d_wav,
                                                             const std::vector<long>& wav_off,
                                                             const std::vector<long>& n,
                                                             const std::vector<int>& batch_sizes,
                                                             int beam, hipStream_t main_st) {
  // J searches in flight (ZASR_SEARCH_JOBS, 2 or 3), L encoders enqueued ahead on E encoder
  // streams (ZASR_ENC_STREAMS, 1 or 2; default 1), J + L encoder output slots.  Batch k:
  // output slot / pinned arena k % (J + L), encoder stream and workspace set k % E, search job
  // set k % J on its own high-priority stream.  Per iteration k: start batch k's search,
  // collect batch k - J + 1's, enqueue batch k + L's encoder -- its slot was last used by
  // batch k - J (collected in iteration k - 1), its stream's previous batch k + L - E is
  // ordered before it on that stream, and job set k % J was last used by batch k - J.
  static const int env_jobs = getenv("ZASR_SEARCH_JOBS") ? atoi(getenv("ZASR_SEARCH_JOBS")) : 2;
  static const int env_e = getenv("ZASR_ENC_STREAMS") ? atoi(getenv("ZASR_ENC_STREAMS")) : 1;
  const int nb = (int)batch_sizes.size();
  const int J = std::max(2, std::min(env_jobs, (int)kMaxJobs));
  const int L = std::max(1, kMaxEnc + 1 - J);
  const int E = std::max(1, std::min(env_e, 2));
  // J searches beside the encoder: the persistent kernels leave 1/8 of the CUs to them
  // (config 3 in f16x3 58.5k -> 59.2k xRT, the drop-in phase within noise: 36.8k / 36.7k,
  // three interleaved pairs each, profiles/r06/persist_ab/beam_share.txt)
  const PersistShare share(true);
  const int NS = J + L;
  ZASR_REQUIRE(NS <= kMaxEnc + 1, "pipeline slots");
  hipStream_t enc_st[2] = {main_st, enc_extra_[0]};
  if (E > 1) {  // the second encoder stream starts after the caller's prior work
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 2], main_st));
    ZASR_HIP_CHECK(hipStreamWaitEvent(enc_st[1], part_ev_[kMaxEnc + 2], 0));
  }
  std::vector<long> first(nb + 1, 0);
  for (int k = 0; k < nb; ++k) first[k + 1] = first[k] + batch_sizes[k];
  Pending pd[kMaxEnc + 1];
  auto enqueue = [&](int k) {
    std::vector<long> o(wav_off.begin() + first[k], wav_off.begin() + first[k + 1]);
    std::vector<long> l(n.begin() + first[k], n.begin() + first[k + 1]);
    encode_stage(d_wav, o, l, k % NS, k % E, enc_st[k % E], pd[k % NS]);
    st_ = main_st;
  };
  struct Job {
    int B = 0;
    std::vector<int> valid;
    SearchJob sj;
    bool launched = false;
  } jobs[kMaxJobs];
  if (J > 2 && stream4_ == nullptr) {
    int least = 0, greatest = 0;
    ZASR_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    ZASR_HIP_CHECK(hipStreamCreateWithPriority(&stream4_, hipStreamNonBlocking, greatest));
  }
  const hipStream_t sst[kMaxJobs] = {stream2_, stream3_, stream4_};
  auto start = [&](int k) {
    Pending& p = pd[k % NS];
    Job& j = jobs[k % J];
    j.B = p.B;
    j.valid = p.valid;
    j.launched = !p.valid.empty();
    if (!j.launched) return;
    ZASR_HIP_CHECK(hipStreamWaitEvent(sst[k % J], p.ready, 0));
    launch_search(p.enc, p.t_out, beam, k % J, sst[k % J], false, j.sj);
  };
  std::vector<TokenResult> out;
  out.reserve(n.size());
  auto finish = [&](int k) {
    Job& j = jobs[k % J];
    std::vector<TokenResult> o(j.B);
    if (j.launched) {
      std::vector<TokenResult> r = collect_search(j.sj);
      for (size_t i = 0; i < j.valid.size(); ++i) o[j.valid[i]] = std::move(r[i]);
    }
    for (auto& x : o) out.push_back(std::move(x));
  };
  for (int k = 0; k < std::min(L, nb); ++k) enqueue(k);
  for (int k = 0; k < nb; ++k) {
    start(k);
    if (k - J + 1 >= 0) finish(k - J + 1);
    if (k + L < nb) enqueue(k + L);
  }
  for (int k = std::max(0, nb - J + 1); k < nb; ++k) finish(k);
  // the call's stream sees every search and encoder complete (results are on the host)
  for (int s = 0; s < J; ++s) {
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 1], sst[s]));
    ZASR_HIP_CHECK(hipStreamWaitEvent(main_st, part_ev_[kMaxEnc + 1], 0));
  }
  if (E > 1) {
    ZASR_HIP_CHECK(hipEventRecord(part_ev_[kMaxEnc + 1], enc_st[1]));
    ZASR_HIP_CHECK(hipStreamWaitEvent(main_st, part_ev_[kMaxEnc + 1], 0));
  }
  st_ = stream_;
  return out;
}

float* Engine::upload_rows(const char* name, const std::vector<const float*>& rows,
                           const std::vector<long>& row_len, int width, long min_len) {
  long tot = 0;
  for (long n : row_len) tot += n >= min_len ? n : 0;
  float* d = ws<float>(name, (size_t)std::max<long>(tot, 1) * width);
  long pos = 0;
  for (size_t b = 0; b < rows.size(); ++b) {
    if (row_len[b] < min_len) continue;
    ZASR_HIP_CHECK(hipMemcpyAsync(d + pos * width, rows[b], (size_t)row_len[b] * width * 4,
                                  hipMemcpyHostToDevice, st_));
    pos += row_len[b];
  }
  return d;
}

std::vector<TokenResult> Engine::decode_features(const std::vector<const float*>& feats,
                                                 const std::vector<long>& frames, int beam) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  st_ = stream_;
  pin_reset(0);
  const int B = (int)feats.size();
  std::vector<int> valid, T;
  long tot_out = 0;
  for (int b = 0; b < B; ++b)
    if (frames[b] >= 9) {
      valid.push_back(b);
      T.push_back((int)frames[b]);
      tot_out += ((frames[b] - 7) / 2 + 1) / 2;
    }
  std::vector<TokenResult> out(B);
  if (valid.empty()) return out;
  float* d = upload_rows("feats", feats, frames, 80, 9);
  float* enc = ws<float>("enc_out", (size_t)tot_out * model_.cfg.joiner_dim);
  std::vector<int> t_out;
  run_encoder(d, T, enc, t_out);
  std::vector<TokenResult> r = run_search(enc, t_out, beam);
  for (size_t i = 0; i < valid.size(); ++i) out[valid[i]] = std::move(r[i]);
  return out;
}

void Engine::fbank_host(const float* wav, long n, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  st_ = stream_;
  pin_reset(0);
  const long frames = n > 0 ? (n + 80) / 160 : 0;
  if (frames == 0) return;
  float* dw = ws<float>("fbh_wav", n);
  float* df = ws<float>("fbh_out", (size_t)frames * 80);
  ZASR_HIP_CHECK(hipMemcpyAsync(dw, wav, n * 4, hipMemcpyHostToDevice, st_));
  std::vector<int> fr;
  run_fbank(dw, {0}, {n}, df, fr);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, df, (size_t)frames * 80 * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void Engine::encode_host(const std::vector<const float*>& feats, const std::vector<long>& frames,
                         std::vector<float>& out, std::vector<int>& t_out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  st_ = stream_;
  pin_reset(0);
  const int B = (int)feats.size();
  std::vector<int> T(B);
  long tot_out = 0;
  for (int b = 0; b < B; ++b) {
    ZASR_REQUIRE(frames[b] >= 9, "encoder needs >= 9 fbank frames per chunk");
    T[b] = (int)frames[b];
    tot_out += ((frames[b] - 7) / 2 + 1) / 2;
  }
  float* d = upload_rows("feats", feats, frames, 80, 9);
  float* enc = ws<float>("enc_out", (size_t)tot_out * model_.cfg.joiner_dim);
  run_encoder(d, T, enc, t_out);
  out.resize((size_t)tot_out * model_.cfg.joiner_dim);
  ZASR_HIP_CHECK(hipMemcpyAsync(out.data(), enc, out.size() * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

std::vector<TokenResult> Engine::search_host(const std::vector<const float*>& enc,
                                             const std::vector<long>& t_out, int beam) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  st_ = stream_;
  pin_reset(0);
  float* d = upload_rows("enc_in", enc, t_out, model_.cfg.joiner_dim, 1);
  const std::vector<int> to(t_out.begin(), t_out.end());
  return run_search(d, to, beam);
}

}  // namespace zasr
