// Conv-TasNet separation engine: weight layout for the GEMM formulation and the ragged forward.
#include "sep.h"

#include <algorithm>
#include <cstring>

#include "common.h"
#include "dense_gemm.h"
#include "host_io.h"

namespace zasr {

namespace {
constexpr int kStEncoder = 0, kStGemm = 1, kStNorm = 2, kStDecoder = 3;
constexpr long kMaxGroupRows = 1L << 20;  // int row arithmetic in the GEMM and the tile tables
constexpr int kMaxGroupRegions = 32768;   // the overlap-add's grid.y
}  // namespace

// activation bytes of one frame: the framed signal, the encoder output, the block's two
// hid_chan-wide buffers (which later hold the two masked encodings), o | skip, the decoder rows
size_t SepEngine::frame_bytes() const {
  return 4 * ((size_t)win_ + nf_ + 2 * (size_t)std::max(hid_, nf_) + bn_ + skip_ + 2 * (size_t)win_);
}

SepEngine::SepEngine(const std::string& dir, int device) : device_(device) {
  const std::string cfg = dir + "/config.json", st = dir + "/model.safetensors";
  if (!file_exists(cfg) || !file_exists(st))
    throw std::invalid_argument("missing separation model files in " + dir +
                                " (config.json + model.safetensors)");
  const Json j = Json::parse(read_file(cfg));
  nf_ = j.at("n_filters").as_int();
  win_ = j.at("kernel_size").as_int();
  hop_ = j.at("stride").as_int();
  bn_ = j.at("bn_chan").as_int();
  hid_ = j.at("hid_chan").as_int();
  skip_ = j.at("skip_chan").as_int();
  const int n_blocks = j.at("n_blocks").as_int(), n_repeats = j.at("n_repeats").as_int();
  const int hq = hid_ / 4;
  ZASR_REQUIRE(j.at("n_src").as_int() == 2 && j.at("conv_kernel_size").as_int() == 3 &&
                   j.at("norm_type").str == "gLN" && j.at("mask_act").str == "relu",
               "separation: only n_src 2, conv_kernel_size 3, gLN, relu masks");
  ZASR_REQUIRE(win_ == 2 * hop_ && win_ % 4 == 0 && win_ >= 4 && nf_ % 4 == 0 && nf_ > 0 &&
                   bn_ % 4 == 0 && bn_ > 0 && skip_ % 4 == 0 && skip_ > 0 && hid_ % 4 == 0 &&
                   hid_ > 0 && (hq % 256 == 0 || 256 % hq == 0) && n_blocks >= 1 &&
                   n_blocks <= 12 && n_repeats >= 1,
               "separation: kernel_size = 2 stride; channel counts multiples of 4; hid_chan / 4 "
               "a divisor or multiple of 256; 1-12 blocks per repeat");
  SafeTensors W;
  W.load(st);
  ZASR_HIP_CHECK(hipSetDevice(device_));
  auto get = [&](const std::string& n, size_t numel) {
    const HostTensor& t = W.get(n);
    ZASR_REQUIRE(t.numel == numel, "separation: bad size of " + n);
    return t.data;
  };
  auto up = [&](const std::string& n, size_t numel) { return store_.upload(get(n, numel), numel); };
  enc_.w = up("encoder.filterbank._filters", (size_t)nf_ * win_);  // [nf][1][win] = W [N][K]
  enc_.N = nf_;
  enc_.K = win_;
  bg_ = up("masker.bottleneck.0.gamma", nf_);
  bb_ = up("masker.bottleneck.0.beta", nf_);
  bott_.w = up("masker.bottleneck.1.weight", (size_t)bn_ * nf_);
  bott_.b = up("masker.bottleneck.1.bias", bn_);
  bott_.N = bn_;
  bott_.K = nf_;
  blocks_.resize((size_t)n_blocks * n_repeats);
  for (size_t i = 0; i < blocks_.size(); ++i) {
    Block& b = blocks_[i];
    const std::string p = "masker.TCN." + std::to_string(i) + ".", s = p + "shared_block.";
    b.dil = 1 << (i % n_blocks);
    b.in.w = up(s + "0.weight", (size_t)hid_ * bn_);
    b.in.b = up(s + "0.bias", hid_);
    b.in.N = hid_;
    b.in.K = bn_;
    b.slope1 = get(s + "1.weight", 1)[0];
    b.g1 = up(s + "2.gamma", hid_);
    b.b1 = up(s + "2.beta", hid_);
    {  // [hid][1][3] -> tap-major [3][hid]
      const float* src = get(s + "3.weight", (size_t)hid_ * 3);
      std::vector<float> w((size_t)3 * hid_);
      for (int c = 0; c < hid_; ++c)
        for (int q = 0; q < 3; ++q) w[(size_t)q * hid_ + c] = src[(size_t)c * 3 + q];
      b.dw = store_.upload(w);
    }
    b.dwb = up(s + "3.bias", hid_);
    b.slope2 = get(s + "4.weight", 1)[0];
    b.g2 = up(s + "5.gamma", hid_);
    b.b2 = up(s + "5.beta", hid_);
    {  // res_conv rows, then skip_conv rows: one GEMM adds into o | skip
      std::vector<float> w((size_t)(bn_ + skip_) * hid_), bias((size_t)bn_ + skip_);
      std::memcpy(w.data(), get(p + "res_conv.weight", (size_t)bn_ * hid_), (size_t)bn_ * hid_ * 4);
      std::memcpy(w.data() + (size_t)bn_ * hid_, get(p + "skip_conv.weight", (size_t)skip_ * hid_),
                  (size_t)skip_ * hid_ * 4);
      std::memcpy(bias.data(), get(p + "res_conv.bias", bn_), (size_t)bn_ * 4);
      std::memcpy(bias.data() + bn_, get(p + "skip_conv.bias", skip_), (size_t)skip_ * 4);
      b.out.w = store_.upload(w);
      b.out.b = store_.upload(bias);
      b.out.N = bn_ + skip_;
      b.out.K = hid_;
    }
  }
  mask_slope_ = get("masker.mask_net.0.weight", 1)[0];
  {
    float* w = up("masker.mask_net.1.weight", (size_t)2 * nf_ * skip_);
    float* b = up("masker.mask_net.1.bias", (size_t)2 * nf_);
    for (int s = 0; s < 2; ++s) {
      mask_[s].w = w + (size_t)s * nf_ * skip_;
      mask_[s].b = b + (size_t)s * nf_;
      mask_[s].N = nf_;
      mask_[s].K = skip_;
    }
  }
  {  // ConvTranspose1d weight [nf][1][win] -> W [win][nf]
    const float* src = get("decoder.filterbank._filters", (size_t)nf_ * win_);
    std::vector<float> w((size_t)win_ * nf_);
    for (int c = 0; c < nf_; ++c)
      for (int k = 0; k < win_; ++k) w[(size_t)k * nf_ + c] = src[(size_t)c * win_ + k];
    dec_.w = store_.upload(w);
    dec_.N = win_;
    dec_.K = nf_;
  }
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  // last: nothing after it can throw, so a failed construction leaks no stream
  ZASR_HIP_CHECK(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
}

void SepEngine::trim() {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
  ws_.clear();
}

SepEngine::~SepEngine() {
  (void)hipSetDevice(device_);
  (void)hipStreamSynchronize(st_);
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  (void)hipStreamDestroy(st_);
}

void SepEngine::mark(int stage) {
  if (!profile_) return;
  hipEvent_t ev;
  ZASR_HIP_CHECK(hipEventCreate(&ev));
  ZASR_HIP_CHECK(hipEventRecord(ev, st_));
  marks_.emplace_back(ev, stage);
}

void SepEngine::collect_marks() {
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

// One launch group: regions d_regions_[k0, k0 + ng), their tiles d_tiles_[t0, t0 + nt), M rows.
void SepEngine::run_group(const float* d_signal, const SepGroup& g, float* d_out) {
  const long M = g.rows;
  const int nt = g.n_tiles, ng = g.n_regions, os = bn_ + skip_, wide = std::max(hid_, nf_);
  const SepTile* tiles = d_tiles_ + g.tile0;
  const SepRegion* regions = d_regions_ + g.region0;
  float2* stats = d_stats_;  // indexed by the call's region number
  auto gemm = [&](const Lin& l, const float* A, int lda, float* C, int ldc, int epi, float slope,
                  const float* aux, int ldaux) {
    GemmParams p = dense_gemm_params(l.w, l.b, l.N, l.K, A, lda, (int)M, C, ldc);
    p.slope = slope;
    p.aux = aux;
    p.ldaux = ldaux;
    gemm_f32(p, epi, ALOAD_DENSE, false, st_);
  };
  auto region_stats = [&](const double2* partial, int C) {
    launch_sep_region_stats(partial, regions, ng, C, stats + g.region0, st_);
  };
  mark(-1);
  float* X = ws<float>("frames", (size_t)M * win_);
  float* TF = ws<float>("tf", (size_t)M * nf_);
  float* H = ws<float>("h", (size_t)M * wide);
  float* Y = ws<float>("y", (size_t)M * wide);
  float* OS = ws<float>("o_skip", (size_t)M * os);
  float* D0 = ws<float>("dec0", (size_t)M * win_);
  float* D1 = ws<float>("dec1", (size_t)M * win_);
  double2* P = ws<double2>("partial", (size_t)nt);
  launch_sep_frames(d_signal, d_regions_, tiles, nt, win_, hop_, X, st_);
  gemm(enc_, X, win_, TF, nf_, EPI_NONE, 0.f, nullptr, 0);
  mark(kStEncoder);
  launch_sep_tile_sums(TF, nf_, tiles, nt, P, st_);
  region_stats(P, nf_);
  launch_sep_gln_apply(TF, H, nf_, tiles, nt, stats, bg_, bb_, st_);
  mark(kStNorm);
  ZASR_HIP_CHECK(hipMemsetAsync(OS, 0, (size_t)M * os * 4, st_));  // skip starts at 0
  gemm(bott_, H, nf_, OS, os, EPI_NONE, 0.f, nullptr, 0);
  for (const Block& b : blocks_) {
    gemm(b.in, OS, os, H, hid_, EPI_PRELU, b.slope1, nullptr, 0);
    mark(kStGemm);
    launch_sep_tile_sums(H, hid_, tiles, nt, P, st_);
    region_stats(P, hid_);
    SepMidArgs ma{};
    ma.h = H;
    ma.y = Y;
    ma.stats = stats;
    ma.gamma = b.g1;
    ma.beta = b.b1;
    ma.w = b.dw;
    ma.bias = b.dwb;
    ma.slope = b.slope2;
    ma.C = hid_;
    ma.dil = b.dil;
    ma.partial = P;
    launch_sep_mid(ma, tiles, nt, st_);
    region_stats(P, hid_);
    // the second gLN is applied in place; the res | skip GEMM then reads plain rows
    launch_sep_gln_apply(Y, Y, hid_, tiles, nt, stats, b.g2, b.b2, st_);
    mark(kStNorm);
    gemm(b.out, Y, hid_, OS, os, EPI_RESADD, 0.f, nullptr, 0);
  }
  mark(kStGemm);
  launch_sep_prelu(OS + bn_, M, skip_, os, mask_slope_, st_);
  float* masked[2] = {H, Y};
  float* dec[2] = {D0, D1};
  for (int s = 0; s < 2; ++s) {
    gemm(mask_[s], OS + bn_, os, masked[s], nf_, EPI_RELUMUL, 0.f, TF, nf_);
    gemm(dec_, masked[s], nf_, dec[s], win_, EPI_NONE, 0.f, nullptr, 0);
  }
  launch_sep_overlap_add(D0, D1, regions, ng, g.max_T, win_, hop_, d_out, st_);
  mark(kStDecoder);
}

SepGroup sep_fill_group(std::vector<SepRegion>& regions, int r0, int ng, std::vector<SepTile>& tiles) {
  ZASR_REQUIRE(r0 >= 0 && ng >= 0 && (size_t)r0 + (size_t)ng <= regions.size(),
               "separation: launch group outside the call's regions");
  SepGroup g{};
  g.region0 = r0;
  g.tile0 = (int)tiles.size();
  for (int r = r0; r < r0 + ng; ++r) {
    SepRegion& rg = regions[(size_t)r];
    rg.row0 = (int)g.rows;
    rg.tile0 = g.n_tiles;
    for (int f0 = 0; f0 < rg.F; f0 += kSepTile) {
      tiles.push_back(SepTile{rg.row0 + f0, f0, rg.F, r});
      ++g.n_tiles;
    }
    g.rows += rg.F;
    g.n_regions += 1;
    g.max_T = std::max(g.max_T, rg.T);
  }
  return g;
}

void SepEngine::run(const float* d_signal, const std::vector<SepRegion>& in, float* d_out) {
  const size_t n = in.size();
  // events a call that threw left behind must not count into this call's stage times
  for (auto& m : marks_) (void)hipEventDestroy(m.first);
  marks_.clear();
  h_regions_ = in;
  h_tiles_.clear();
  std::vector<SepGroup> groups;
  const long per = std::max<long>(1, std::min<long>((long)(budget_ / frame_bytes()), kMaxGroupRows));
  for (size_t r0 = 0; r0 < n;) {  // a group takes regions while its rows fit (one at least)
    int ng = 0;
    long rows = 0;
    while (r0 + ng < n) {
      const SepRegion& rg = h_regions_[r0 + ng];
      ZASR_REQUIRE(rg.F <= kMaxGroupRows, "separation: region too long");
      if (ng > 0 && (rows + rg.F > per || ng >= kMaxGroupRegions)) break;
      rows += rg.F;
      ++ng;
    }
    groups.push_back(sep_fill_group(h_regions_, (int)r0, ng, h_tiles_));
    r0 += (size_t)ng;
  }
  last_groups_ = (int)groups.size();
  d_regions_ = ws<SepRegion>("regions", n);
  d_tiles_ = ws<SepTile>("tiles", h_tiles_.size());
  d_stats_ = ws<float2>("stats", n);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_regions_, h_regions_.data(), n * sizeof(SepRegion),
                                hipMemcpyHostToDevice, st_));
  ZASR_HIP_CHECK(hipMemcpyAsync(d_tiles_, h_tiles_.data(), h_tiles_.size() * sizeof(SepTile),
                                hipMemcpyHostToDevice, st_));
  for (const SepGroup& gs : groups) run_group(d_signal, gs, d_out);
  collect_marks();
}

namespace {
std::vector<SepRegion> make_regions(const long* starts, const long* lengths, int n, long total,
                                    int win, int hop, long* out_total) {
  ZASR_REQUIRE(n > 0 && starts && lengths, "separation: no regions");
  std::vector<SepRegion> v((size_t)n);
  long out_off = 0;
  for (int r = 0; r < n; ++r) {
    ZASR_REQUIRE(lengths[r] >= win, "separation: a region needs at least kernel_size samples");
    ZASR_REQUIRE(lengths[r] < (1L << 30), "separation: region too long");
    ZASR_REQUIRE(starts[r] >= 0 && starts[r] + lengths[r] <= total,
                 "separation: region outside the signal");
    SepRegion& rg = v[(size_t)r];
    rg.sig_off = starts[r];
    rg.out_off = out_off;
    rg.T = (int)lengths[r];
    rg.F = (int)((lengths[r] - win) / hop + 1);
    rg.row0 = rg.tile0 = 0;
    out_off += 2 * lengths[r];
  }
  *out_total = out_off;
  return v;
}
}  // namespace

void SepEngine::separate_host(const float* samples, long total, const long* offsets,
                              const long* lengths, int n, float* out) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  long out_total = 0;
  const std::vector<SepRegion> regions = make_regions(offsets, lengths, n, total, win_, hop_, &out_total);
  float* d_sig = ws<float>("signal", (size_t)total);
  float* d_out = ws<float>("out", (size_t)out_total);
  ZASR_HIP_CHECK(hipMemcpyAsync(d_sig, samples, (size_t)total * 4, hipMemcpyHostToDevice, st_));
  run(d_sig, regions, d_out);
  ZASR_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)out_total * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

void SepEngine::separate_device(const float* d_audio, long total, const long* starts,
                                const long* lengths, int n, float* out, bool out_on_device,
                                hipStream_t user_stream) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  long out_total = 0;
  const std::vector<SepRegion> regions = make_regions(starts, lengths, n, total, win_, hop_, &out_total);
  if (user_stream) {  // order after the caller's producer of d_audio
    hipEvent_t ev;
    ZASR_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ZASR_HIP_CHECK(hipEventRecord(ev, user_stream));
    ZASR_HIP_CHECK(hipStreamWaitEvent(st_, ev, 0));
    ZASR_HIP_CHECK(hipEventDestroy(ev));
  }
  float* d_out = out_on_device ? out : ws<float>("out", (size_t)out_total);
  run(d_audio, regions, d_out);
  if (!out_on_device)
    ZASR_HIP_CHECK(hipMemcpyAsync(out, d_out, (size_t)out_total * 4, hipMemcpyDeviceToHost, st_));
  ZASR_HIP_CHECK(hipStreamSynchronize(st_));
}

}  // namespace zasr
