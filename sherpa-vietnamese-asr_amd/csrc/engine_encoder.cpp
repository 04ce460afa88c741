// libzasr encoder driver: Conv2dSubsampling, the Zipformer2 stacks and their seams, encoder_proj.
//
// Reference mapping:
//   encoder run             core/asr_engine.py:1045-1049 (Zipformer2 graph, icefall 3P)
#include <algorithm>
#include <cstring>

#include "common.h"
#include "engine.h"

namespace zasr {

namespace {
struct LevelMeta {
  std::vector<int> len;  // per sequence
  std::vector<int> off;  // B + 1
  int total = 0, maxlen = 0;
};
LevelMeta make_level(const std::vector<int>& len) {
  LevelMeta m;
  m.len = len;
  m.off.assign(len.size() + 1, 0);
  for (size_t b = 0; b < len.size(); ++b) {
    m.off[b + 1] = m.off[b] + len[b];
    m.maxlen = std::max(m.maxlen, len[b]);
  }
  m.total = m.off.back();
  return m;
}
struct MetaPack {
  std::vector<char> bytes;
  size_t add(const void* p, size_t n) {
    size_t at = (bytes.size() + 15) & ~size_t(15);
    bytes.resize(at + n);
    if (n) std::memcpy(bytes.data() + at, p, n);
    return at;
  }
};
}  // namespace

// feed_forward1 on a fused kernel (feed_forward's routes below): it can run out of place
bool Engine::ff1_fused(const DStack& S, const DLayer& Ly) const {
  const DLin& fi = Ly.ff_in[0];
  if (fi.wh) return ffn_fused_supported(S.d) && (S.d < 256 || fi.wp);
  return fi.wp && prec_.f16x3 && ffn_h3_oop_ok(S.d);
}

void Engine::project(const DLin& l, const void* A, bool a16, int lda, int M, void* C, bool c16,
                     int ldc, int epi) {
  if (prec_.bf16_act)
    linear_h(l, A, a16, lda, M, C, c16, ldc, epi);
  else
    linear(l, reinterpret_cast<const float*>(A), lda, M, reinterpret_cast<float*>(C), ldc, epi);
}

// attention weights (shared by nonlin_attention, self_attn1, self_attn2)
Engine::LayerAttn Engine::attention_weights(const StackCtx& c, const DLayer& Ly, const float* X) {
  const int d = c.stk->d, h = c.stk->h, R = c.R;
  LayerAttn at;
  if (prec_.bf16_act) {
    // flash-style attention on bf16 q / k / v (attn_kernels.hip): every head's statistics come
    // from self_attn1; head 0's weights are consumed inside the fused NonlinAttention kernel
    __bf16* qkp16 = ws<__bf16>("ly_qkp_h", (size_t)R * 68 * h);
    linear_h(Ly.attn_in, X, false, d, R, qkp16, true, 68 * h, EPI_NONE);
    __bf16* A16 = ws<__bf16>("ly_attn_h", 1);  // sized by the caller
    at.stats = ws<float>("ly_attn_stats", (size_t)R * h);
    at.fa = AttnFlashArgs{qkp16, h, Ly.pos_tab, model_.pmax, c.off, c.a_off, c.B, c.maxL, A16,
                          nullptr, nullptr, at.stats, at.stats};
  } else if (prec_.pieces) {
    // split modes: the same flash kernels on f32 q / k / v, every MFMA product split into
    // pieces per operand; head 0's weights in f32 (L8 row stride)
    at.qkp = ws<float>("ly_qkp", (size_t)R * 68 * h);
    linear(Ly.attn_in, X, d, R, at.qkp, 68 * h, EPI_NONE);
    at.A = ws<float>("ly_attn", 1);  // sized by the caller
    at.stats = ws<float>("ly_attn_stats", (size_t)R * h);
    at.fa = AttnFlashArgs{at.qkp, h, Ly.pos_tab, model_.pmax, c.off, c.a_off, c.B, c.maxL, at.A,
                          nullptr, nullptr, at.stats, at.stats, prec_.pieces};
    if (!prec_.nonlin_fused) {  // f16x3: consumed in the fused NonlinAttention kernel
      AttnFlashArgs a = at.fa;
      a.map = c.bm.head0;
      a.map_len = c.bm.n_head0;
      prof_begin("attn_softmax");
      launch_attn_flash(a, 0, st_);
      prof_end();
    }
  } else {
    // head 0 only: its normalised weights feed nonlin_attention; every head's statistics
    // come from self_attn1's online softmax
    at.qkp = ws<float>("ly_qkp", (size_t)R * 68 * h);
    linear(Ly.attn_in, X, d, R, at.qkp, 68 * h, EPI_NONE);
    at.A = ws<float>("ly_attn", 1);  // sized by the caller
    at.stats = ws<float>("ly_attn_stats", (size_t)R * h * 2);
    AttnArgs a{at.qkp, h, Ly.pos_tab, model_.pmax, c.off, c.a_off, c.B, c.maxL, at.A, at.stats, 1};
    prof_begin("attn_softmax");
    launch_attn_softmax(a, st_);
    prof_end();
  }
  return at;
}

// bf16 mode: feed_forward2's residual epilogue also applies bypass_mid (same formula as
// launch_bypass, one pass over X fewer)
void Engine::feed_forward(const StackCtx& c, const DLayer& Ly, int k, float* X, const float* O,
                          const float* src) {
  const int d = c.stk->d, R = c.R;
  const DLin &fi = Ly.ff_in[k], &fo = Ly.ff_out[k];
  const float* bo = (prec_.bf16_act && k == 1) ? O : nullptr;
  const float* bs = (prec_.bf16_act && k == 1) ? Ly.bypass_mid : nullptr;
  if (fi.wh && ffn_fused_supported(d) && (d < 256 || fi.wp)) {
    // bf16 mode: in_proj -> SwooshL -> out_proj + residual in one kernel, hidden on chip
    // (d >= 256: the fragment-packed weights of ffn_wide_kernel)
    prof_begin("ffn_fused");
    launch_ffn_fused(X, R, d, fi.N, d < 256 ? fi.wh : fi.wp, fi.b, d < 256 ? fo.wh : fo.wp, fo.b,
                     st_, bo, bs, src);
    prof_end();
    return;
  }
  ZASR_REQUIRE(src == nullptr || (!fi.wh && fi.wp && prec_.f16x3),
               "feed-forward: only the fused kernels run out of place");
  if (fi.wh) {  // bf16 mode: the hidden activation crosses HBM in bf16
    __bf16* H = ws<__bf16>("ly_hid_h", (size_t)R * fi.N);
    linear_h(fi, X, false, d, R, H, true, fi.N, EPI_SWOOSHL);
    linear_h(fo, H, true, fi.N, R, X, false, d, EPI_RESADD, bo, bs);
  } else if (fi.wp && prec_.f16x3) {
    // f16x3 mode: the same fusion at f32 quality, the hidden layer on chip as fp16 pieces;
    // feed_forward2 folds bypass_mid as the GEMM pair's residual epilogue does
    prof_begin("ffn_fused");
    launch_ffn_fused_h3(X, R, d, fi.N, fi.wp, fi.b, fo.wp, fo.b, st_, k == 1 ? O : nullptr,
                        k == 1 ? Ly.bypass_mid : nullptr, nullptr, src);
    prof_end();
  } else {
    // split modes: feed_forward2's epilogue applies bypass_mid too (fp32: launch_bypass)
    const bool byp = k == 1 && fo.wx != nullptr;
    float* H = ws<float>("ly_hid", (size_t)R * fi.N);
    linear(fi, X, d, R, H, fi.N, EPI_SWOOSHL);
    linear(fo, H, fi.N, R, X, d, EPI_RESADD, "enc_gemm", byp ? O : nullptr,
           byp ? Ly.bypass_mid : nullptr);
  }
}

// the bf16 modes keep the value projection and the attention output in bf16 (ly_*_h)
void Engine::self_attention(const StackCtx& c, const DLayer& Ly, int k, float* X,
                            const LayerAttn& at) {
  const int d = c.stk->d, h = c.stk->h, R = c.R;
  const bool h16 = prec_.bf16_act;
  const size_t n = (size_t)R * 12 * h;
  // (bf16: the flash kernels' V staging reads 4 elements past the last row, kernels.h)
  void* vv = h16 ? (void*)ws<__bf16>("ly_vv_h", n + 4) : (void*)ws<float>("ly_vv", n);
  void* oa = h16 ? (void*)ws<__bf16>("ly_oa_h", n) : (void*)ws<float>("ly_oa", n);
  project(Ly.sa_in[k], X, false, d, R, vv, h16, 12 * h, EPI_NONE);
  prof_begin("attn_apply");
  if (prec_.flash) {
    AttnFlashArgs a = at.fa;
    a.v = vv;
    a.out = oa;
    a.map = c.bm.heads;
    a.map_len = c.bm.n_heads;
    launch_attn_flash(a, k == 0 ? 1 : 2, st_);
  } else {
    AttnSAArgs sa{at.qkp, h, Ly.pos_tab, model_.pmax, c.off, c.B, c.maxL, at.stats,
                  reinterpret_cast<const float*>(vv), reinterpret_cast<float*>(oa), at.stats};
    launch_attn_sa(sa, k == 0, false, st_);
  }
  prof_end();
  project(Ly.sa_out[k], oa, h16, 12 * h, R, X, false, d, EPI_RESADD);
}

// the bf16 modes keep the in_proj output and the out_proj input in bf16 (ly_*_h)
void Engine::conv_module(const StackCtx& c, const DLayer& Ly, int k, float* X) {
  const int d = c.stk->d, R = c.R, K = c.stk->K;
  const DLin& in = Ly.cv_in[k];
  const bool h16 = in.wh != nullptr;
  const size_t n = (size_t)R * d;
  void* dc = h16 ? (void*)ws<__bf16>("ly_dc_h", n) : (void*)ws<float>("ly_dc", n);
  if (in.glu) {  // the GLU in the in_proj epilogue (f32; bf16 modes: then bf16), d columns out
    void* g = h16 ? (void*)ws<__bf16>("ly_glu_h", n) : (void*)ws<float>("ly_glu", n);
    project(in, X, false, d, R, g, h16, d, EPI_GLU);
    prof_begin("dwconv1d");
    if (h16)
      launch_dwconv1d_post_glu_bf16(reinterpret_cast<__bf16*>(g), c.off, c.map, R, d, K,
                                    Ly.cv_dw_w[k], Ly.cv_dw_b[k], reinterpret_cast<__bf16*>(dc), st_);
    else
      launch_dwconv1d_post_glu(reinterpret_cast<float*>(g), c.off, c.map, R, d, K, Ly.cv_dw_w[k],
                               Ly.cv_dw_b[k], reinterpret_cast<float*>(dc), st_);
  } else {  // fp32 only (the loader interleaves the in_proj for every other mode): f32 throughout
    ZASR_REQUIRE(!h16, "conv module: a bf16 in_proj carries the GLU epilogue");
    float* g2 = ws<float>("ly_g2", 2 * n);
    project(in, X, false, d, R, g2, false, 2 * d, EPI_NONE);
    prof_begin("dwconv1d");
    launch_glu_dwconv1d(g2, c.off, c.map, R, d, K, Ly.cv_dw_w[k], Ly.cv_dw_b[k],
                        reinterpret_cast<float*>(dc), st_);
  }
  prof_end();
  project(Ly.cv_out[k], dc, h16, d, R, X, false, d, EPI_RESADD);
}

// z = (A0 @ t1) * y in the flash kernel (mode 3): head 0's weights never reach HBM
void Engine::launch_nonlin_flash(const StackCtx& c, const LayerAttn& at, const void* t1t, int hid,
                                 const void* y, void* z) {
  AttnFlashArgs a = at.fa;
  a.t1t = t1t;
  a.o8 = c.o8;
  a.ldt = c.R8;
  a.hid = hid;
  a.y = y;
  a.ldy = 3 * hid;
  a.z = z;
  a.map = c.bm.head0;
  a.map_len = c.bm.n_head0;
  prof_begin("attn_nonlin");
  launch_attn_flash(a, 3, st_);
  prof_end();
}

// nonlin_attention (attention head 0 only)
void Engine::nonlin_attention(const StackCtx& c, const DLayer& Ly, float* X, const LayerAttn& at) {
  const int d = c.stk->d, R = c.R, R8 = c.R8;
  const int hid = 3 * d / 4;
  const int np = prec_.pieces;
  if (prec_.bf16_act) {
    // z = (A0 @ t1) * y with t1^T [hid][R8] bf16, z bf16; (s, x, y) = chunk(in_proj(src), 3)
    // in bf16: s, x read by the transpose kernel, y by the fused kernel's epilogue
    __bf16* h3 = ws<__bf16>("ly_h3_h", (size_t)R * 3 * hid);
    __bf16* t1t = ws<__bf16>("ly_t1t", (size_t)hid * R8);
    __bf16* z = ws<__bf16>("ly_z_h", (size_t)R * hid);
    linear_h(Ly.na_in, X, false, d, R, h3, true, 3 * hid, EPI_NONE);
    prof_begin("elementwise");
    launch_nonlin_prep_t(h3, true, c.off, c.o8, c.map, R, hid, R8, t1t, st_);
    prof_end();
    launch_nonlin_flash(c, at, t1t, hid, h3 + 2 * hid, z);
    linear_h(Ly.na_out, z, true, hid, R, X, false, d, EPI_RESADD);
    return;
  }
  float* h3 = ws<float>("ly_h3", (size_t)R * 3 * hid);
  // z = (A0 @ t1) * y as a per-sequence GEMM on head 0's weights (fp32, bf16x3, bf16x6)
  GemmParams p{};
  p.A = at.A;
  p.sbk = 1;
  p.sbn = R8;
  p.ldc = hid;
  p.N = hid;
  p.aux = h3 + 2 * hid;
  p.ldaux = 3 * hid;
  p.slices = c.nl_slices;
  p.num_slices = c.B;
  p.max_M = c.maxL;
  if (np) {
    // A0 [L][L8] f32 (split while staging), t1^T as np pieces [np][hid][R8] (the weight
    // layout), y f32 in the epilogue
    __bf16* t1t = ws<__bf16>("ly_t1t_x", (size_t)stored_pieces(np) * hid * R8);
    float* z = ws<float>("ly_z", (size_t)R * hid);
    linear(Ly.na_in, X, d, R, h3, 3 * hid, EPI_NONE);
    prof_begin("elementwise");
    launch_nonlin_prep_t(h3, false, c.off, c.o8, c.map, R, hid, R8, t1t, st_, np);
    prof_end();
    if (prec_.nonlin_fused) {  // f16x3: fp16 pieces of P and t1 in the flash kernel
      launch_nonlin_flash(c, at, t1t, hid, h3 + 2 * hid, z);
    } else {
      p.C = z;
      prof_begin("attn_nonlin");
      gemm_x3(p, t1t, (long)hid * R8, EPI_MULAUX, ALOAD_DENSE, st_, np);
      prof_end();
    }
    linear(Ly.na_out, z, hid, R, X, d, EPI_RESADD);
  } else {
    float* t1 = ws<float>("ly_t1", (size_t)R * hid);
    float* z = ws<float>("ly_z", (size_t)R * hid);
    linear(Ly.na_in, X, d, R, h3, 3 * hid, EPI_NONE);
    prof_begin("elementwise");
    launch_nonlin_prep(h3, t1, R, hid, st_);
    prof_end();
    p.B = t1;
    p.sbk = hid;
    p.sbn = 1;
    p.C = z;
    prof_begin("attn_nonlin");
    gemm_f32(p, EPI_MULAUX, ALOAD_DENSE, true, st_);
    prof_end();
    linear(Ly.na_out, z, hid, R, X, d, EPI_RESADD);
  }
}

float* Engine::layer_forward(const StackCtx& c, const DLayer& Ly, float* X, float* Xalt,
                             bool orig_ready, bool copy_for_next) {
  const int d = c.stk->d, R = c.R;
  // O = the layer's input (src of bypass_mid and the final bypass).  A fused feed_forward1
  // reads it from X and writes Xalt, where the rest of the layer runs in place: X itself stays
  // as O.  The GEMM-pair routes update X in place, so they keep a copy.
  const bool oop = ff1_fused(*c.stk, Ly);
  float* O = X;
  if (!oop) {
    O = ws<float>("ly_orig", (size_t)R * d);
    if (!orig_ready)  // else the previous layer's BiasNorm already wrote src here
      ZASR_HIP_CHECK(hipMemcpyAsync(O, X, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, st_));
  }
  const LayerAttn at = attention_weights(c, Ly, X);
  // 1. feed_forward1 (fused: O -> Xalt, the layer's X from here on)
  if (oop) {
    X = Xalt;
    feed_forward(c, Ly, 0, X, O, O);
  } else {
    feed_forward(c, Ly, 0, X, O);
  }
  // 2. nonlin_attention, self_attn1, conv_module1, feed_forward2
  nonlin_attention(c, Ly, X, at);
  self_attention(c, Ly, 0, X, at);
  conv_module(c, Ly, 0, X);
  feed_forward(c, Ly, 1, X, O);
  // 3. bypass_mid (bf16 and split modes: folded into feed_forward2's epilogue)
  if (!prec_.bf16_act && Ly.ff_out[1].wx == nullptr) {
    prof_begin("elementwise");
    launch_bypass(X, O, Ly.bypass_mid, R, d, st_);
    prof_end();
  }
  // 4. self_attn2, conv_module2, feed_forward3
  self_attention(c, Ly, 1, X, at);
  conv_module(c, Ly, 1, X);
  feed_forward(c, Ly, 2, X, O);
  // 5. BiasNorm + bypass (folding it into feed_forward3's fused epilogue -- the row's sums of
  // squares reduced across the block's waves, X read twice -- measured slower: ffn_fused
  // +1.26 ms, elementwise -0.78 ms per hour)
  prof_begin("elementwise");
  // (copy_for_next: the next layer's feed_forward1 is a GEMM pair and takes its copy of src
  // from here; written over `orig` where that is the copy, which the same lane has read)
  launch_bias_norm(X, R, d, Ly.norm_b, Ly.norm_ls, O, Ly.bypass, st_,
                   copy_for_next ? ws<float>("ly_orig", (size_t)R * d) : nullptr);
  prof_end();
  return X;
}

ConvGemmRoute frontend_conv_route(const DLin& l, bool a_bf16, bool c_bf16) {
  if (l.wh && (a_bf16 || c_bf16)) return CONV_GEMM_BF16;
  if (l.wx) return CONV_GEMM_X3;
  return l.wh ? CONV_GEMM_BF16 : CONV_GEMM_F32;
}

void launch_frontend_conv_gemm(GemmParams& p, const DLin& l, int aload, bool a_bf16, bool c_bf16,
                               int pieces, hipStream_t st) {
  p.B = l.w;
  p.sbk = 1;
  p.sbn = l.K;
  p.ldc = l.N;
  p.bias = l.b;
  p.N = l.N;
  switch (frontend_conv_route(l, a_bf16, c_bf16)) {
    case CONV_GEMM_BF16: return gemm_bf16(p, l.wh, EPI_SWOOSHR, aload, st, a_bf16, c_bf16);
    case CONV_GEMM_X3: return gemm_x3(p, l.wx, (long)l.N * l.K, EPI_SWOOSHR, aload, st, pieces);
    case CONV_GEMM_F32: return gemm_f32(p, EPI_SWOOSHR, aload, false, st);
  }
}

FrontendConvSlices frontend_conv_slices(const int* T, int nseq) {
  FrontendConvSlices y;
  y.c2.resize(nseq);
  y.c3.resize(nseq);
  for (int b = 0; b < nseq; ++b) {
    const int t1 = T[b] - 2, l2 = (T[b] - 3) / 2, L = (T[b] - 7) / 2;
    y.c2[b] = GemmSlice{y.rows_c1 * 640, 0, y.rows_c2 * 39 * 32, 0, l2 * 39, 72, 0, 0};
    y.c3[b] = GemmSlice{y.rows_c2 * 39 * 32, 0, y.rows_L * 19 * 128, 0, L * 19, 288, 0, 0};
    y.max_M2 = std::max(y.max_M2, l2 * 39);
    y.max_M3 = std::max(y.max_M3, L * 19);
    y.rows_c1 += t1;
    y.rows_c2 += l2;
    y.rows_L += L;
  }
  return y;
}

void Engine::frontend_conv_gemm(GemmParams& p, const DLin& l, int aload, bool a_bf16, bool c_bf16) {
  prof_begin("frontend_conv");
  launch_frontend_conv_gemm(p, l, aload, a_bf16, c_bf16, prec_.pieces, st_);
  prof_end();
}

void Engine::run_encoder(const float* d_feats, const std::vector<int>& T, float* d_enc,
                         std::vector<int>& t_out) {
  const ModelConfig& cfg = model_.cfg;
  const int B = (int)T.size();
  std::vector<int> t1(B), l2(B), L(B), tout(B);
  for (int b = 0; b < B; ++b) {
    ZASR_REQUIRE(T[b] >= 9, "encoder needs >= 9 fbank frames per chunk");
    t1[b] = T[b] - 2;
    l2[b] = (T[b] - 3) / 2;
    L[b] = (T[b] - 7) / 2;
    tout[b] = (L[b] + 1) / 2;
  }
  t_out = tout;
  LevelMeta mfb = make_level(T), mc1 = make_level(t1), mc2 = make_level(l2), mL = make_level(L),
            mout = make_level(tout);
  const int ns = (int)model_.stacks.size();
  std::vector<LevelMeta> mst(ns);
  std::vector<std::vector<long>> aoff(ns);
  std::vector<std::vector<GemmSlice>> sl_nl(ns);
  std::vector<std::vector<int>> o8(ns);
  std::vector<int> R8(ns, 0);
  // the flash attention path (every mode but fp32): head-0 weights with L32 rows ("L8" / "o8" /
  // "R8" below: 32-padded), NonlinAttention's B operand as t1^T columns
  const bool flash = prec_.flash;
  size_t attn_floats = 0;
  int maxL_all = 0;
  for (int i = 0; i < ns; ++i) {
    const DStack& s = model_.stacks[i];
    std::vector<int> len(B);
    for (int b = 0; b < B; ++b) len[b] = (L[b] + s.ds - 1) / s.ds;
    mst[i] = make_level(len);
    maxL_all = std::max(maxL_all, mst[i].maxlen);
    const int hid = 3 * s.d / 4;
    // head 0's weight blocks and the t1^T columns (kernels.h attn_head0_layout, which the
    // attention self-tests share)
    AttnHead0Layout lay = attn_head0_layout(len.data(), B, flash);
    for (int b = 0; b < B; ++b) {
      const int Lb = len[b], L8 = (Lb + 31) & ~31;
      GemmSlice g{};
      g.a_off = lay.a_off[b];  // head 0 block of this sequence
      g.b_off = flash ? (long)lay.o32[b] : (long)mst[i].off[b] * hid;  // flash: column of t1^T
      g.c_off = (long)mst[i].off[b] * hid;
      g.aux_off = (long)mst[i].off[b] * 3 * hid;
      g.M = Lb;
      g.K = flash ? L8 : Lb;
      // weight row stride (flash: the GEMM's K padding, 32 for the LDS-DMA nonlin GEMM)
      g.lda = AttnHead0Layout::stride(Lb, flash);
      sl_nl[i].push_back(g);
    }
    R8[i] = lay.R32;
    attn_floats = std::max(attn_floats, lay.elems);
    aoff[i] = std::move(lay.a_off);
    o8[i] = std::move(lay.o32);
  }
  ensure_pos_tables(maxL_all + 192);  // the bf16 attention stages rows up to L + 160
  // frontend conv slices
  const FrontendConvSlices fcs = frontend_conv_slices(T.data(), B);
  const std::vector<GemmSlice>&sl_c2 = fcs.c2, &sl_c3 = fcs.c3;
  // one metadata upload
  MetaPack mp;
  size_t o_fb = mp.add(mfb.off.data(), (B + 1) * 4), o_c1 = mp.add(mc1.off.data(), (B + 1) * 4),
         o_L = mp.add(mL.off.data(), (B + 1) * 4), o_out = mp.add(mout.off.data(), (B + 1) * 4);
  size_t o_c2s = mp.add(sl_c2.data(), B * sizeof(GemmSlice)),
         o_c3s = mp.add(sl_c3.data(), B * sizeof(GemmSlice));
  std::vector<size_t> o_st(ns), o_ao(ns), o_sn(ns), o_o8(ns), o_bmh(ns), o_bm0(ns);
  // the flash kernels' block maps (kernels.h build_attn_block_map), per stack: every head's
  // (modes 1 / 2), and head 0's by z-chunk of the fused NonlinAttention (mode 3: the bf16 and
  // f16x3 modes) or alone (mode 0: bf16x3 / bf16x6)
  std::vector<int> n_bmh(ns, 0), n_bm0(ns, 0);
  std::vector<unsigned> bmap;
  for (int i = 0; i < ns; ++i) {
    o_st[i] = mp.add(mst[i].off.data(), (B + 1) * 4);
    o_o8[i] = mp.add(o8[i].data(), (B + 1) * 4);
    o_ao[i] = mp.add(aoff[i].data(), B * sizeof(long));
    o_sn[i] = mp.add(sl_nl[i].data(), sl_nl[i].size() * sizeof(GemmSlice));
    if (flash) {
      const DStack& s = model_.stacks[i];
      n_bmh[i] = build_attn_block_map(mst[i].len.data(), B, s.h, 0, bmap);
      o_bmh[i] = mp.add(bmap.data(), bmap.size() * sizeof(unsigned));
      const int chunks = prec_.nonlin_fused
                             ? attn_nonlin_chunks(3 * s.d / 4, prec_.bf16_act ? 1 : prec_.pieces)
                             : 1;
      n_bm0[i] = build_attn_block_map(mst[i].len.data(), B, chunks, 0, bmap);
      o_bm0[i] = mp.add(bmap.data(), bmap.size() * sizeof(unsigned));
    }
  }
  char* d_meta = ws<char>("enc_meta", mp.bytes.size());
  upload(d_meta, mp.bytes.data(), mp.bytes.size());
  auto I = [&](size_t o) { return reinterpret_cast<const int*>(d_meta + o); };
  // row -> sequence maps of every resolution used by per-row kernels
  int* c1_map = ws<int>("map_c1", mc1.total);
  int* L_map = ws<int>("map_L", mL.total);
  int* out_map = ws<int>("map_out", mout.total);
  launch_row2seq(I(o_c1), B, mc1.total, c1_map, st_);
  launch_row2seq(I(o_L), B, mL.total, L_map, st_);
  launch_row2seq(I(o_out), B, mout.total, out_map, st_);
  std::vector<int*> st_map(ns);
  for (int i = 0; i < ns; ++i) {
    st_map[i] = ws<int>("map_st" + std::to_string(i), mst[i].total);
    launch_row2seq(I(o_st[i]), B, mst[i].total, st_map[i], st_);
  }

  // ---------------- Conv2dSubsampling ----------------
  // bf16 mode: conv.0 and conv.4 outputs in bf16 (read back through the GEMM's bf16
  // implicit-im2col loaders)
  const bool fe16 = model_.conv4.wh != nullptr && model_.conv7.wh != nullptr;
  void* c1 = fe16 ? (void*)ws<__bf16>("fe_c1_h", (size_t)mc1.total * 640)
                  : (void*)ws<float>("fe_c1", (size_t)mc1.total * 640);
  prof_begin("frontend_conv");
  launch_conv1(d_feats, I(o_fb), I(o_c1), c1_map, mc1.total, model_.conv0_w, model_.conv0_b, c1,
               fe16, st_, prec_.f16x3);
  prof_end();
  void* c2 = fe16 ? (void*)ws<__bf16>("fe_c2_h", (size_t)mc2.total * 39 * 32)
                  : (void*)ws<float>("fe_c2", (size_t)mc2.total * 39 * 32);
  {
    GemmParams p{};
    p.A = reinterpret_cast<const float*>(c1);
    p.C = reinterpret_cast<float*>(c2);
    p.slices = reinterpret_cast<const GemmSlice*>(d_meta + o_c2s);
    p.num_slices = B;
    p.max_M = fcs.max_M2;
    frontend_conv_gemm(p, model_.conv4, ALOAD_CONV2, fe16, fe16);
  }
  const int d0 = cfg.dims[0];
  float* e0 = ws<float>("fe_e0", (size_t)mL.total * d0);
  {
    GemmParams p{};
    p.A = reinterpret_cast<const float*>(c2);
    p.slices = reinterpret_cast<const GemmSlice*>(d_meta + o_c3s);
    p.num_slices = B;
    p.max_M = fcs.max_M3;
    if (model_.pw1.wh) {
      // bf16 mode: conv.7 output, the ConvNeXt block and its output stay bf16
      __bf16* x3 = ws<__bf16>("fe_x3_h", (size_t)mL.total * 19 * 128);
      __bf16* y3 = ws<__bf16>("fe_y3_h", (size_t)mL.total * 19 * 128);
      __bf16* x4 = ws<__bf16>("fe_x4_h", (size_t)mL.total * 19 * 128);
      p.C = reinterpret_cast<float*>(x3);
      frontend_conv_gemm(p, model_.conv7, ALOAD_CONV3, fe16, true);
      prof_begin("frontend_conv");
      launch_convnext_bf16(x3, I(o_L), L_map, mL.total, model_.dw_w, model_.dw_b, model_.pw1.wp,
                           model_.pw1.b, model_.pw2.wp, model_.pw2.b, y3, x4, st_);
      prof_end();
      linear_h(model_.out, x4, true, 2432, mL.total, e0, false, d0, EPI_NONE);
    } else {
      float* x3 = ws<float>("fe_x3", (size_t)mL.total * 19 * 128);
      p.C = x3;
      frontend_conv_gemm(p, model_.conv7, ALOAD_CONV3, false, false);
      float* y3 = ws<float>("fe_y3", (size_t)mL.total * 19 * 128);
      prof_begin("frontend_conv");
      launch_dwconv2d_tiled(x3, I(o_L), L_map, mL.total, model_.dw_w, model_.dw_b, y3, st_);
      prof_end();
      if (model_.pw1.wr && model_.pw2.wr) {
        // f16x3: the ConvNeXt MLP as the fused f16x3 FFN (d = 128, pw1.N hidden): x3 += MLP(y3)
        prof_begin("frontend_conv");
        launch_ffn_fused_h3(x3, mL.total * 19, 128, model_.pw1.N, model_.pw1.wr, model_.pw1.b,
                            model_.pw2.wr, model_.pw2.b, st_, nullptr, nullptr, y3);
        prof_end();
      } else if (model_.pw1.wp && model_.pw2.wp && prec_.f16x3) {
        // f16x3: pw1 -> SwooshL -> pw2 + residual in one kernel, the hidden layer on chip
        prof_begin("frontend_conv");
        launch_convnext_mlp_h3(y3, x3, (long)mL.total * 19, model_.pw1.wp, model_.pw1.b,
                               model_.pw2.wp, model_.pw2.b, x3, st_);
        prof_end();
      } else {
        float* hcn = ws<float>("fe_h", (size_t)mL.total * 19 * 384);
        linear(model_.pw1, y3, 128, mL.total * 19, hcn, 384, EPI_SWOOSHL);
        linear(model_.pw2, hcn, 384, mL.total * 19, x3, 128, EPI_RESADD);
      }
      linear(model_.out, x3, 2432, mL.total, e0, d0, EPI_NONE);
    }
  }
  prof_begin("elementwise");
  launch_bias_norm(e0, mL.total, d0, model_.out_norm_b, model_.out_norm_ls, nullptr, nullptr, st_);
  prof_end();

  // ---------------- encoder stacks ----------------
  if (prec_.bf16_act)  // (the fused NonlinAttention never materialises head 0's weights)
    ws<__bf16>("ly_attn_h", 1);
  else
    ws<float>("ly_attn", prec_.f16x3 ? 1 : std::max<size_t>(attn_floats, 1));
  const int Dm = cfg.max_dim();
  // the 25 Hz full-dim output: each column range is written by the seam of the latest stack
  // that has it
  float* fo = ws<float>("enc_ds", (size_t)mout.total * Dm);
  // stack i's input (50 Hz, width d_i): stack 0 takes the embed output (itself where the
  // widths agree), every later one is written by the previous seam
  float* orig = e0;
  if (d0 != model_.stacks[0].d) {
    orig = ws<float>("st_orig0", (size_t)mL.total * model_.stacks[0].d);
    prof_begin("elementwise");
    launch_copy_cols(e0, d0, 0, orig, model_.stacks[0].d, 0, std::min(d0, model_.stacks[0].d),
                     mL.total, true, model_.stacks[0].d, st_);
    prof_end();
  }
  // the running stack's second X buffer (layer_forward), sized for the largest stack
  size_t xalt_n = 1;
  for (int i = 0; i < ns; ++i) xalt_n = std::max(xalt_n, (size_t)mst[i].total * model_.stacks[i].d);
  float* xalt = ws<float>("st_xalt", xalt_n);
  // a downsampled stack's X (its own rate) is written by the seam ahead of it, which still
  // reads the previous stack's: st_x0 / st_x1 in turn
  float* Xds = nullptr;
  if (model_.stacks[0].ds > 1) {  // no seam ahead of stack 0
    const DStack& s = model_.stacks[0];
    Xds = ws<float>("st_x0", (size_t)mst[0].total * s.d);
    prof_begin("elementwise");
    launch_downsample(orig, I(o_L), I(o_st[0]), st_map[0], mst[0].total, s.d, s.ds, s.ds_w, Xds, st_);
    prof_end();
  }
  for (int i = 0; i < ns; ++i) {
    const DStack& s = model_.stacks[i];
    const int d = s.d;
    const StackCtx ctx{&s, mst[i].total, B, I(o_st[i]), st_map[i],
                       reinterpret_cast<const long*>(d_meta + o_ao[i]),
                       reinterpret_cast<const GemmSlice*>(d_meta + o_sn[i]), mst[i].maxlen,
                       I(o_o8[i]), R8[i],
                       AttnBlockMaps{reinterpret_cast<const unsigned*>(d_meta + o_bmh[i]), n_bmh[i],
                                     reinterpret_cast<const unsigned*>(d_meta + o_bm0[i]), n_bm0[i]}};
    // the stack's X and a second buffer: a layer whose feed_forward1 is fused leaves its
    // output in the other one, and the next layer swaps their roles
    float* X = s.ds == 1 ? orig : Xds;
    float* Xalt = xalt;
    bool orig_ready = false;
    for (size_t li = 0; li < s.layers.size(); ++li) {
      const bool copy_for_next = li + 1 < s.layers.size() && !ff1_fused(s, s.layers[li + 1]);
      float* Xo = layer_forward(ctx, s.layers[li], X, Xalt, orig_ready, copy_for_next);
      if (Xo != X) std::swap(X, Xalt);
      orig_ready = copy_for_next;
    }
    // seam (seam_kernel): upsample + bypass combine, written as stack i+1's 50 Hz input, as
    // its SimpleDownsample'd X, and, downsampled by 2, into the encoder output's channel range
    // [d_later_max, d) (the latest stack that has those channels)
    int later_max = 0;
    for (int j = i + 1; j < ns; ++j) later_max = std::max(later_max, model_.stacks[j].d);
    const bool more = i + 1 < ns;
    const int dn = more ? model_.stacks[i + 1].d : 0;
    const int dsn = more ? model_.stacks[i + 1].ds : 1;
    SeamDesc sd;
    sd.xd = X;
    sd.orig = s.ds == 1 ? X : orig;  // ds == 1: y is the stack's final X, whichever buffer
    sd.s = s.comb;
    sd.off_in = I(o_L);
    sd.off_ds = I(o_st[i]);
    sd.off_run = dsn > 1 ? I(o_st[i + 1]) : I(o_out);
    sd.map_run = dsn > 1 ? st_map[i + 1] : out_map;
    sd.runs = dsn > 1 ? mst[i + 1].total : mout.total;
    sd.rows = mL.total;
    sd.d = d;
    sd.ds = s.ds;
    sd.next = more ? ws<float>("st_orig" + std::to_string((i + 1) % 2), (size_t)mL.total * dn)
                   : nullptr;
    sd.dn = dn;
    sd.ds_next = dsn;
    if (dsn > 1) {
      sd.xnext = ws<float>("st_x" + std::to_string((i + 1) % 2), (size_t)mst[i + 1].total * dn);
      sd.wn_host8 = model_.stacks[i + 1].ds_w;
    }
    if (d > later_max) {
      sd.out = fo;
      sd.off_out = I(o_out);
      sd.wo_host2 = model_.out_ds_w;
      sd.ldo = Dm;
      sd.c0 = later_max;
    }
    prof_begin("elementwise");
    launch_seam(sd, st_);
    prof_end();
    orig = sd.next;
    Xds = sd.xnext;
  }
  // ---------------- encoder_proj ----------------
  linear(model_.enc_proj, fo, Dm, mout.total, d_enc, cfg.joiner_dim, EPI_NONE);
}

}  // namespace zasr
