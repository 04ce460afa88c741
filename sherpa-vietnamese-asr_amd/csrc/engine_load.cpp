// libzasr model load: the weights of config.json + model.safetensors (or the reference's ONNX
// files) onto the device, the operands each precision mode adds, and the tables.
//
// Reference mapping:
//   load + session setup    core/asr_engine.py:903-1020 (create_recognizer)
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "engine.h"
#include "host_io.h"

namespace zasr {

namespace {

const HostTensor& tensor(const SafeTensors& W, const std::string& name,
                         std::initializer_list<int64_t> shape) {
  const HostTensor& t = W.get(name);
  ZASR_REQUIRE(t.shape == std::vector<int64_t>(shape), "shape mismatch for " + name);
  return t;
}

float scalar(const SafeTensors& W, const std::string& name) {
  const HostTensor& t = W.get(name);
  ZASR_REQUIRE(t.numel == 1, name + " must be a scalar");
  return t.data[0];
}

// softmax of a SimpleDownsample's bias: the weights of its `n` taps
void downsample_weights(const float* bias, int n, float* out) {
  double mx = -1e30, sum = 0;
  for (int u = 0; u < n; ++u) mx = std::max(mx, (double)bias[u]);
  std::vector<double> e(n);
  for (int u = 0; u < n; ++u) sum += (e[u] = std::exp((double)bias[u] - mx));
  for (int u = 0; u < n; ++u) out[u] = (float)(e[u] / sum);
}

// f32 -> bf16, round to nearest even: what convert_to_bf16 stores on the device
std::vector<__bf16> to_bf16_host(const float* w, size_t n) {
  std::vector<__bf16> h(n);
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, &w[i], 4);
    const uint16_t r = (u & 0x7fffffffu) > 0x7f800000u
                           ? (uint16_t)((u >> 16) | 0x40)
                           : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    std::memcpy(&h[i], &r, 2);
  }
  return h;
}

// a layer's projections: attention and NonlinAttention, then self-attention and conv modules,
// then (with_ffn) the feed-forward modules
std::vector<DLin*> layer_lins(DLayer& L, bool with_ffn) {
  std::vector<DLin*> v{&L.attn_in, &L.na_in, &L.na_out};
  for (int a = 0; a < 2; ++a)
    for (DLin* l : {&L.sa_in[a], &L.sa_out[a], &L.cv_in[a], &L.cv_out[a]}) v.push_back(l);
  if (with_ffn)
    for (int a = 0; a < 3; ++a)
      for (DLin* l : {&L.ff_in[a], &L.ff_out[a]}) v.push_back(l);
  return v;
}

}  // namespace

DLin Engine::load_linear(const SafeTensors& W, const std::string& pre, int N, int K) {
  DLin l;
  l.N = N;
  l.K = K;
  l.hw = tensor(W, pre + ".weight", {N, K}).data;
  if (prec_.f16x3) {
    // f16x3 splits every weight into fp16 pieces: a magnitude at or beyond the fp16 range
    // would become inf, so such a model is refused here (use bf16x6: same quality)
    for (size_t i = 0; i < (size_t)N * K; ++i)
      ZASR_REQUIRE(std::fabs(l.hw[i]) < 65504.f,
                   "precision f16x3: weight " + pre + " exceeds the fp16 range; use bf16x6");
  }
  l.hb = tensor(W, pre + ".bias", {N}).data;
  l.w = store_.upload(l.hw, (size_t)N * K);
  l.b = store_.upload(l.hb, N);
  return l;
}

void Engine::load_model(const SafeTensors& W) {
  std::vector<std::vector<float>> host_images;  // host weight images the tensors do not hold
  load_frontend(W);
  load_stacks(W, host_images);
  load_decoder(W);
  ensure_pos_tables(2048);
  if (prec_.pieces > 0) load_split_operands();
  if (prec_.bf16_act) load_bf16_operands();
  build_dec_table();
  load_fbank_tables();
  load_hotword_tables();
  // the host images go away with W and host_images
  for (DLin* l : {&model_.conv4, &model_.conv7, &model_.pw1, &model_.pw2, &model_.out,
                  &model_.enc_proj, &model_.dec_proj, &model_.joiner})
    l->hw = l->hb = nullptr;
  for (auto& s : model_.stacks)
    for (auto& L : s.layers)
      for (DLin* l : layer_lins(L, true)) l->hw = l->hb = nullptr;
}

// ---- Conv2dSubsampling ----
void Engine::load_frontend(const SafeTensors& W) {
  auto vec = [&](const std::string& name, int n) {
    return store_.upload(tensor(W, name, {n}).data, n);
  };
  // a 3x3 conv [O][C][3][3] as the implicit-im2col GEMM's weight [o][(kt*3+kf)*C + c]
  auto conv3x3 = [&](const std::string& pre, int O, int C) {
    const HostTensor& w = tensor(W, pre + ".weight", {O, C, 3, 3});
    std::vector<float> p((size_t)O * C * 9);
    for (int o = 0; o < O; ++o)
      for (int c = 0; c < C; ++c)
        for (int kk = 0; kk < 9; ++kk) p[(size_t)o * C * 9 + kk * C + c] = w.data[(o * C + c) * 9 + kk];
    return DLin{store_.upload(p), vec(pre + ".bias", O), O, C * 9};
  };
  auto pointwise = [&](const std::string& pre, int O, int C) {
    DLin l{nullptr, vec(pre + ".bias", O), O, C};
    l.hw = tensor(W, pre + ".weight", {O, C, 1, 1}).data;
    l.w = store_.upload(l.hw, (size_t)O * C);
    return l;
  };
  model_.conv0_w = store_.upload(tensor(W, "encoder_embed.conv.0.weight", {8, 1, 3, 3}).data, 72);
  model_.conv0_b = vec("encoder_embed.conv.0.bias", 8);
  model_.conv4 = conv3x3("encoder_embed.conv.4", 32, 8);
  model_.conv7 = conv3x3("encoder_embed.conv.7", 128, 32);
  model_.dw_w = store_.upload(
      tensor(W, "encoder_embed.convnext.depthwise_conv.weight", {128, 1, 7, 7}).data, 128 * 49);
  model_.dw_b = vec("encoder_embed.convnext.depthwise_conv.bias", 128);
  model_.pw1 = pointwise("encoder_embed.convnext.pointwise_conv1", 384, 128);
  model_.pw2 = pointwise("encoder_embed.convnext.pointwise_conv2", 128, 384);
  // out: input index c*19 + f  ->  f*128 + c  (our [L][19][128] layout)
  const int d0 = model_.cfg.dims[0];
  const HostTensor& wo = tensor(W, "encoder_embed.out.weight", {d0, 128 * 19});
  std::vector<float> po((size_t)d0 * 2432);
  for (int n = 0; n < d0; ++n)
    for (int c = 0; c < 128; ++c)
      for (int f = 0; f < 19; ++f) po[(size_t)n * 2432 + f * 128 + c] = wo.data[(size_t)n * 2432 + c * 19 + f];
  model_.out = DLin{store_.upload(po), vec("encoder_embed.out.bias", d0), d0, 2432};
  model_.out_norm_b = vec("encoder_embed.out_norm.bias", d0);
  model_.out_norm_ls = scalar(W, "encoder_embed.out_norm.log_scale");
}

// ---- Zipformer stacks ----
void Engine::load_stacks(const SafeTensors& W, std::vector<std::vector<float>>& host_images) {
  const ModelConfig& cfg = model_.cfg;
  const int qd = cfg.qd, vd = cfg.vd, pd = cfg.pd;
  auto vec = [&](const std::string& name, int n) {
    return store_.upload(tensor(W, name, {n}).data, n);
  };
  // every mode but fp32 applies the conv modules' GLU in the in_proj GEMM's epilogue (EPI_GLU):
  // weight rows and bias interleaved (a_c, s_c).  The interleaved host image is the one
  // uploaded, and the one every later packing reads.
  const bool glu = prec_.bf16_act || prec_.pieces > 0;
  auto conv_in_proj = [&](const std::string& pre, int d) {
    if (!glu) return load_linear(W, pre, 2 * d, d);
    DLin l;
    l.N = 2 * d;
    l.K = d;
    l.glu = true;
    const float* w = tensor(W, pre + ".weight", {2 * d, d}).data;
    const float* b = tensor(W, pre + ".bias", {2 * d}).data;
    std::vector<float> wi((size_t)l.N * d), bi(l.N);
    for (int c = 0; c < d; ++c)
      for (int h = 0; h < 2; ++h) {
        std::memcpy(&wi[(size_t)(2 * c + h) * d], &w[(size_t)(h * d + c) * d], (size_t)d * 4);
        bi[2 * c + h] = b[h * d + c];
      }
    if (prec_.f16x3)
      for (float v : wi)
        ZASR_REQUIRE(std::fabs(v) < 65504.f,
                     "precision f16x3: weight " + pre + " exceeds the fp16 range; use bf16x6");
    l.w = store_.upload(wi);
    l.b = store_.upload(bi);
    host_images.push_back(std::move(wi));
    l.hw = host_images.back().data();
    host_images.push_back(std::move(bi));
    l.hb = host_images.back().data();
    return l;
  };
  for (size_t i = 0; i < cfg.dims.size(); ++i) {
    DStack s;
    s.d = cfg.dims[i];
    s.F = cfg.ff[i];
    s.h = cfg.heads[i];
    s.ds = cfg.ds[i];
    s.K = cfg.kernels[i];
    const int d = s.d, F = s.F, h = s.h;
    std::string pre = "encoder.encoders." + std::to_string(i) + ".";
    if (s.ds != 1) {
      downsample_weights(tensor(W, pre + "downsample.bias", {s.ds}).data, s.ds, s.ds_w);
      s.comb = vec(pre + "out_combiner.bypass_scale", d);
      pre += "encoder.";
    }
    for (int j = 0; j < cfg.layers[i]; ++j) {
      DLayer L;
      std::string p = pre + "layers." + std::to_string(j) + ".";
      L.bypass = vec(p + "bypass.bypass_scale", d);
      L.bypass_mid = vec(p + "bypass_mid.bypass_scale", d);
      L.attn_in = load_linear(W, p + "self_attn_weights.in_proj", (2 * qd + pd) * h, d);
      const HostTensor& pw = tensor(W, p + "self_attn_weights.linear_pos.weight", {pd * h, cfg.pos_dim});
      L.pos_w.assign(pw.data, pw.data + pw.numel);
      for (int a = 0; a < 2; ++a) {
        std::string n = p + "self_attn" + std::to_string(a + 1);
        L.sa_in[a] = load_linear(W, n + ".in_proj", vd * h, d);
        L.sa_out[a] = load_linear(W, n + ".out_proj", d, vd * h);
      }
      const int fdims[3] = {(F * 3) / 4, F, (F * 5) / 4};
      for (int a = 0; a < 3; ++a) {
        std::string n = p + "feed_forward" + std::to_string(a + 1);
        L.ff_in[a] = load_linear(W, n + ".in_proj", fdims[a], d);
        L.ff_out[a] = load_linear(W, n + ".out_proj", d, fdims[a]);
      }
      const int hid = 3 * d / 4;
      L.na_in = load_linear(W, p + "nonlin_attention.in_proj", 3 * hid, d);
      L.na_out = load_linear(W, p + "nonlin_attention.out_proj", d, hid);
      for (int a = 0; a < 2; ++a) {
        std::string n = p + "conv_module" + std::to_string(a + 1);
        L.cv_in[a] = conv_in_proj(n + ".in_proj", d);
        L.cv_out[a] = load_linear(W, n + ".out_proj", d, d);
        L.cv_dw_w[a] = store_.upload(tensor(W, n + ".depthwise_conv.weight", {d, 1, s.K}).data,
                                     (size_t)d * s.K);
        L.cv_dw_b[a] = vec(n + ".depthwise_conv.bias", d);
      }
      L.norm_b = vec(p + "norm.bias", d);
      L.norm_ls = scalar(W, p + "norm.log_scale");
      s.layers.push_back(std::move(L));
    }
    model_.stacks.push_back(std::move(s));
  }
  downsample_weights(tensor(W, "encoder.downsample_output.bias", {2}).data, 2, model_.out_ds_w);
}

// ---- encoder_proj, decoder, joiner ----
void Engine::load_decoder(const SafeTensors& W) {
  const ModelConfig& cfg = model_.cfg;
  const int D = cfg.dec_dim;
  model_.enc_proj = load_linear(W, "encoder_proj", cfg.joiner_dim, cfg.max_dim());
  const HostTensor& E = tensor(W, "decoder.embedding.weight", {cfg.V, D});
  const HostTensor& Wc = tensor(W, "decoder.conv.weight", {D, 4, 2});
  model_.dec_emb = store_.upload(E.data, (size_t)cfg.V * D);
  model_.dec_conv = store_.upload(Wc.data, (size_t)D * 8);
  // decoder conv taps per vocabulary entry: tap_k[v][c] = sum_ci W[c][ci][k] E[v][4(c/4)+ci]
  std::vector<float> t0((size_t)cfg.V * D), t1((size_t)cfg.V * D);
  for (int v = 0; v < cfg.V; ++v)
    for (int c = 0; c < D; ++c) {
      const float* e = E.data + (size_t)v * D + (c & ~3);
      const float* w = Wc.data + (size_t)c * 8;
      float a0 = 0.f, a1 = 0.f;
      for (int ci = 0; ci < 4; ++ci) {
        a0 = std::fma(w[ci * 2 + 0], e[ci], a0);
        a1 = std::fma(w[ci * 2 + 1], e[ci], a1);
      }
      t0[(size_t)v * D + c] = a0;
      t1[(size_t)v * D + c] = a1;
    }
  model_.dec_tap0 = store_.upload(t0);
  model_.dec_tap1 = store_.upload(t1);
  model_.dec_proj = load_linear(W, "decoder_proj", cfg.joiner_dim, D);
  model_.joiner = load_linear(W, "joiner.output_linear", cfg.V, cfg.joiner_dim);
}

// ---- bf16x3 / bf16x6 / f16x3: split pieces of every projection weight ----
void Engine::load_split_operands() {
  const ModelConfig& cfg = model_.cfg;
  const int np = prec_.pieces, stored = stored_pieces(np);
  auto split = [&](DLin& l) {
    l.wx = store_.alloc((size_t)l.N * l.K * 2 * stored);
    split_to_bf16(l.w, l.wx, (long)l.N * l.K, np, stream_);
  };
  // both fp16 pieces of W in ffn_pack_h3_host's fragment order (every |w| < 31)
  auto pack_h3 = [&](const DLin& l) {
    return upload_packed(2 * (size_t)l.N * l.K,
                         [&](__bf16* out) { ffn_pack_h3_host(l.hw, l.N, l.K, out); });
  };
  auto range_ok = [](const DLin& l) { return ffn_h3_weights_ok(l.hw, (long)l.N * l.K); };
  for (DLin* l : {&model_.conv4, &model_.conv7, &model_.pw1, &model_.pw2, &model_.out,
                  &model_.enc_proj, &model_.joiner})
    split(*l);
  if (cfg.joiner_dim == 256 || cfg.joiner_dim == 512) {
    // the joiner's W pieces in MFMA-fragment order (one packed image per piece) for
    // joiner_split_packed_kernel; J is written in the same order, already split, by store_j4
    const long pe = gemm_rp_packed_elems(cfg.V, cfg.joiner_dim);
    void* p = store_.alloc((size_t)pe * 2 * stored);
    for (int t = 0; t < stored; ++t)
      gemm_rp_pack_weights(reinterpret_cast<const __bf16*>(model_.joiner.wx) + (long)t * cfg.V * cfg.joiner_dim,
                           cfg.V, cfg.joiner_dim, reinterpret_cast<__bf16*>(p) + t * pe, stream_);
    model_.joiner_packed = p;
    model_.joiner_plane = pe;
  }
  for (auto& s : model_.stacks)
    for (auto& L : s.layers)
      for (DLin* l : layer_lins(L, true)) split(*l);
  ZASR_HIP_CHECK(hipStreamSynchronize(stream_));
  if (!prec_.f16x3) return;
  // the fused f16x3 ConvNeXt MLP reads pw1 / pw2 as fp16 piece images in MFMA-fragment
  // order (pack_frag32_host per piece, the same split as split_to_bf16)
  for (DLin* l : {&model_.pw1, &model_.pw2}) {
    const size_t n = (size_t)l->N * l->K;
    l->wp = upload_packed(2 * n, [&](__bf16* out) {
      std::vector<__bf16> piece(n);
      for (int t = 0; t < 2; ++t) {
        for (size_t i = 0; i < n; ++i) {
          const _Float16 hi = (_Float16)l->hw[i];
          const _Float16 v = t == 0 ? hi : (_Float16)((l->hw[i] - (float)hi) * 2048.f);
          std::memcpy(&piece[i], &v, 2);
        }
        pack_frag32_host(piece.data(), l->N, l->K, out + t * n);
      }
    });
  }
  // the fused f16x3 FFN (model dims 256..512) reads W1 / W2 as fp16 piece images in
  // MFMA-fragment order; a layer whose weights reach 31 in magnitude keeps the GEMM pair
  for (auto& s : model_.stacks)
    for (auto& L : s.layers)
      for (int a = 0; a < 3; ++a) {
        DLin &w1 = L.ff_in[a], &w2 = L.ff_out[a];
        if (!ffn_h3_supported(w1.K, w1.N)) continue;
        if (!range_ok(w1) || !range_ok(w2)) {
          ++routes_.ffn_gemm_pair;
          continue;
        }
        ++routes_.ffn_fused_h3;
        w1.wp = pack_h3(w1);
        w2.wp = pack_h3(w2);
      }
  // the layer projections the row-resident f16x3 GEMM takes (K, N within its shapes and
  // every |w| < 31; the others keep gemm_x3)
  for (auto& s : model_.stacks)
    for (auto& L : s.layers)
      for (DLin* l : layer_lins(L, false)) {
        if (!gemm_h3r_supported(l->K, l->N, EPI_NONE)) continue;
        if (!range_ok(*l)) {
          ++routes_.gemm_x3_range;
          continue;
        }
        ++routes_.gemm_h3r;
        l->wr = pack_h3(*l);
      }
  // the ConvNeXt MLP (pw1 [384][128], pw2 [128][384]) as the fused f16x3 FFN
  if (model_.pw1.K == 128 && model_.pw2.N == 128 && ffn_h3_supported(128, model_.pw1.N)) {
    const bool ok = range_ok(model_.pw1) && range_ok(model_.pw2);
    routes_.cnx_ffn_h3 = ok ? 1 : 0;
    if (ok)
      for (DLin* l : {&model_.pw1, &model_.pw2}) l->wr = pack_h3(*l);
  }
}

// ---- bf16 modes: bf16 copies of every dense projection weight ----
void Engine::load_bf16_operands() {
  const ModelConfig& cfg = model_.cfg;
  auto to_bf16 = [&](DLin& l) {
    l.wh = store_.alloc((size_t)l.N * l.K * 2);
    convert_to_bf16(l.w, l.wh, (long)l.N * l.K, stream_);
  };
  // the bf16 weights (what convert_to_bf16 wrote) in a kernel's fragment order
  auto pack_bf16 = [&](const DLin& l, void (*pack)(const __bf16*, int, int, __bf16*)) {
    return upload_packed((size_t)l.N * l.K, [&](__bf16* out) {
      pack(to_bf16_host(l.hw, (size_t)l.N * l.K).data(), l.N, l.K, out);
    });
  };
  for (DLin* l : {&model_.conv4, &model_.conv7, &model_.pw1, &model_.pw2, &model_.out,
                  &model_.enc_proj})
    to_bf16(*l);
  // f32_search keeps the joiner (and with it J, the logits and the search) in f32
  if (!prec_.f32_search) {
    to_bf16(model_.joiner);
    if (cfg.joiner_dim == 256 || cfg.joiner_dim == 512) {  // speculative-greedy joiner operand
      model_.joiner_packed = store_.alloc((size_t)gemm_rp_packed_elems(cfg.V, cfg.joiner_dim) * 2);
      gemm_rp_pack_weights(model_.joiner.wh, cfg.V, cfg.joiner_dim, model_.joiner_packed, stream_);
    }
  }
  for (auto& s : model_.stacks)
    for (auto& L : s.layers) {
      // attn_in: the query and positional-query rows carry log2(e) in the bf16 path (the
      // flash attention works in the log2 domain), folded before the single rounding
      DLin& ai = L.attn_in;
      std::vector<float> rs(ai.N, 1.f), bias(ai.N);
      const float kLog2e = 1.4426950408889634f;
      for (int r = 0; r < ai.N; ++r)
        if (r < 32 * s.h || r >= 64 * s.h) rs[r] = kLog2e;
      for (int r = 0; r < ai.N; ++r) bias[r] = ai.hb[r] * rs[r];
      float* d_rs = store_.upload(rs);
      ai.bh = store_.upload(bias);
      ai.wh = store_.alloc((size_t)ai.N * ai.K * 2);
      convert_rows_to_bf16(ai.w, d_rs, ai.wh, ai.N, ai.K, stream_);
      for (DLin* l : layer_lins(L, true))
        if (l != &ai) to_bf16(*l);
    }
  ZASR_HIP_CHECK(hipStreamSynchronize(stream_));
  // the ConvNeXt MLP reads pw1 / pw2 in MFMA-fragment order
  for (DLin* l : {&model_.pw1, &model_.pw2}) l->wp = pack_bf16(*l, pack_frag32_host);
  // the wide fused FFN (model dims 256..512) reads W1 / W2 in MFMA-fragment order
  for (auto& s : model_.stacks)
    for (auto& L : s.layers)
      for (int a = 0; a < 3; ++a) {
        const int F = L.ff_in[a].N, d = L.ff_in[a].K;
        if (d < 256 || !ffn_fused_supported(d) || F % 32 != 0 || F > 2048) continue;
        for (DLin* l : {&L.ff_in[a], &L.ff_out[a]}) l->wp = pack_bf16(*l, ffn_pack_host);
      }
}

// ---- decoder-context table (kernels.h, DecTable): V^2 x D f32, built once ----
void Engine::build_dec_table() {
  const ModelConfig& cfg = model_.cfg;
  const double gb = (double)cfg.V * cfg.V * cfg.joiner_dim * 4.0 / 1e9;
  double max_gb = 24.0;
  if (const char* e = getenv("ZASR_DEC_TABLE_MAX_GB")) max_gb = atof(e);
  if (gb > max_gb) return;
  model_.dec_table = reinterpret_cast<float*>(
      store_.alloc((size_t)cfg.V * cfg.V * cfg.joiner_dim * sizeof(float)));
  DecoderW dw{model_.dec_tap0, model_.dec_tap1, model_.dec_proj.b, cfg.joiner_dim};
  launch_dec_table(dw, model_.dec_proj.w, cfg.V, model_.dec_table, stream_);
  ZASR_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Engine::load_fbank_tables() {
  std::vector<double> tw(512);
  for (int j = 0; j < 256; ++j) {
    double a = -2.0 * M_PI * j / 512.0;
    tw[2 * j] = std::cos(a);
    tw[2 * j + 1] = std::sin(a);
  }
  d_twiddle_ = store_.upload(tw);
  std::vector<float> win(400);
  for (int i = 0; i < 400; ++i)
    win[i] = (float)std::pow(0.5 - 0.5 * std::cos(2.0 * M_PI / 399.0 * i), 0.85);
  d_window_ = store_.upload(win);
  // knf's triangles: mel-linear between 20 Hz and 7600 Hz over the bins 0 .. 255
  auto mel = [](float f) { return 1127.0f * logf(1.0f + f / 700.0f); };
  const float mlo = mel(20.0f), mhi = mel(7600.0f);
  const float delta = (mhi - mlo) / 81.0f;
  std::vector<float> banks(80 * 256, 0.f);
  for (int b = 0; b < 80; ++b) {
    float left = mlo + (float)b * delta, center = mlo + (float)(b + 1) * delta,
          right = mlo + (float)(b + 2) * delta;
    for (int i = 0; i < 256; ++i) {
      float m = mel(31.25f * (float)i);
      if (m > left && m < right)
        banks[b * 256 + i] = (m <= center) ? (m - left) / (center - left) : (right - m) / (right - center);
    }
  }
  set_mel_banks(banks.data(), 256);
}

void Engine::load_hotword_tables() {
  hw_.num_states = hw_host_.num_states;
  hw_.num_cls = hw_host_.num_cls;
  if (hw_host_.num_states == 0) return;
  hw_.tok2cls = store_.upload(hw_host_.tok2cls);
  hw_.next = store_.upload(hw_host_.next);
  hw_.delta = store_.upload(hw_host_.delta);
  hw_.node_score = store_.upload(hw_host_.node_score);
}

}  // namespace zasr
