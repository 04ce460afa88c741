// Kernel-level self-tests on host data (include/zasr.h zasr_selftest_*): the general GEMM entry
// points, the f16x3 one-accumulator kernels and the bf16 fused FFN run alone on caller-supplied
// operands, so the tests can sweep the shapes and row counts the decode only reaches
// incidentally (tail tiles, M < 16, every K / D and epilogue) against a float64 product on the
// host; the fused FFNs also out of place, the fused stack seam beside the kernels it
// replaces, and the convolution path's hand-written kernels (ConvolutionModule depthwise conv,
// conv.0, the ConvNeXt block) and BiasNorm on ragged batches given as per-sequence lengths, and
// the joiner kernels on row-major and on host-packed J, and the transducer search kernels (one
// frame, one greedy window, the final pick) on a caller-supplied search state, and the general
// GEMMs behind their implicit-im2col and BN-ReLU operand loaders (conv.4 / conv.7 over one
// z-slice per sequence as a decode launches them; the CAM++ projections of gemm_f32), and the
// CAM++, Silero VAD and ViBERT kernels, one launch function per entry, and the PyanNet and
// Conv-TasNet kernels likewise (each on a stream of its own).
// Device 0 of the process, its null stream, synchronous; nothing here is on the decode path.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/zasr.h"
#include "common.h"
#include "dense_gemm.h"
#include "emb.h"
#include "engine.h"
#include "gemm.h"
#include "kernels.h"
#include "seg.h"
#include "sep.h"

namespace zasr {
namespace {
struct DevBuf {
  void* p = nullptr;
  explicit DevBuf(size_t bytes) { ZASR_HIP_CHECK(hipMalloc(&p, bytes > 0 ? bytes : 4)); }
  ~DevBuf() { (void)hipFree(p); }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};
void up(DevBuf& d, const void* h, size_t bytes) {
  if (bytes) ZASR_HIP_CHECK(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
}
}  // namespace

void selftest_gemm_h3r(int M, int K, int N, int epi, const float* A, const float* W,
                       const float* bias, float* C) {
  ZASR_REQUIRE(M >= 1, "selftest gemm_h3r: M >= 1");
  ZASR_REQUIRE(gemm_h3r_supported(K, N, epi), "selftest gemm_h3r: unsupported K / N / epilogue");
  ZASR_REQUIRE(ffn_h3_weights_ok(W, (long)N * K), "selftest gemm_h3r: |w| must stay below 31");
  const int ncol = epi == EPI_GLU ? N / 2 : N;
  std::vector<__bf16> pk(2 * (size_t)N * K);
  ffn_pack_h3_host(W, N, K, pk.data());
  DevBuf dA((size_t)M * K * 4), dW(pk.size() * 2), dB((size_t)N * 4), dC((size_t)M * ncol * 4);
  up(dA, A, (size_t)M * K * 4);
  up(dW, pk.data(), pk.size() * 2);
  if (bias) up(dB, bias, (size_t)N * 4);
  up(dC, C, (size_t)M * ncol * 4);  // the RESADD operand (and what rows past M would keep)
  gemm_h3r(dA.as<float>(), dW.p, bias ? dB.as<float>() : nullptr, dC.as<float>(), ncol, M, N, K,
           epi, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ZASR_HIP_CHECK(hipMemcpy(C, dC.p, (size_t)M * ncol * 4, hipMemcpyDeviceToHost));
}

void selftest_gemm(int mode, int M, int K, int N, int epi, bool a_bf16, bool c_bf16,
                   const float* A, const float* W, const float* bias, const float* aux,
                   const float* byp_orig, const float* byp_scale, float* C) {
  const bool f32 = mode == ZASR_PRECISION_FP32, h16 = mode == ZASR_PRECISION_BF16;
  const int pieces = mode == ZASR_PRECISION_BF16X3   ? 2
                     : mode == ZASR_PRECISION_BF16X6 ? 3
                     : mode == ZASR_PRECISION_F16X3  ? kPiecesF16
                                                     : 0;
  ZASR_REQUIRE(f32 || h16 || pieces != 0,
               "selftest gemm: mode must be ZASR_PRECISION_FP32, _BF16, _BF16X3, _BF16X6 or _F16X3");
  ZASR_REQUIRE(M >= 1 && K >= 1 && N >= 1, "selftest gemm: M, K, N >= 1");
  ZASR_REQUIRE(h16 || (!a_bf16 && !c_bf16), "selftest gemm: bf16 A / C in the bf16 mode only");
  const bool mulaux = epi == EPI_MULAUX || epi == EPI_MULAUX16;
  ZASR_REQUIRE(!mulaux || aux != nullptr, "selftest gemm: EPI_MULAUX needs aux");
  ZASR_REQUIRE((byp_orig == nullptr) == (byp_scale == nullptr) &&
                   (byp_orig == nullptr || (epi == EPI_RESADD && !f32)),
               "selftest gemm: the bypass takes both operands, EPI_RESADD, not the fp32 mode");
  ZASR_REQUIRE(epi != EPI_GLU || N % 2 == 0, "selftest gemm: EPI_GLU needs an even N");
  const int ncol = epi == EPI_GLU ? N / 2 : N;
  const size_t na = (size_t)M * K, nw = (size_t)N * K, nc = (size_t)M * ncol, nx = (size_t)M * N;
  const size_t ea = a_bf16 ? 2 : 4, ec = c_bf16 ? 2 : 4, ex = epi == EPI_MULAUX16 ? 2 : 4;
  auto round16 = [](const float* s, size_t n) {
    std::vector<__bf16> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = (__bf16)s[i];
    return h;
  };
  DevBuf dA(na * ea), dW(nw * 4), dWx(nw * 2 * (pieces ? stored_pieces(pieces) : 1)), dB((size_t)N * 4),
      dC((nc + ncol) * ec), dX(aux ? nx * ex : 4), dbo(byp_orig ? nc * 4 : 4), dbs((size_t)N * 4);
  if (a_bf16) up(dA, round16(A, na).data(), na * 2);
  else up(dA, A, na * 4);
  up(dW, W, nw * 4);
  // the weights as the loader prepares them (engine_load.cpp)
  if (h16) convert_to_bf16(dW.as<float>(), dWx.p, (long)nw, nullptr);
  if (pieces) split_to_bf16(dW.as<float>(), dWx.p, (long)nw, pieces, nullptr);
  if (bias) up(dB, bias, (size_t)N * 4);
  if (c_bf16) up(dC, round16(C, nc).data(), nc * 2);  // the RESADD operand / what stays unwritten
  else up(dC, C, nc * 4);
  // one guard row behind C: a store past the row tail must not reach it
  const size_t gb = (size_t)ncol * ec;
  ZASR_HIP_CHECK(hipMemset(dC.as<unsigned char>() + nc * ec, 0x5a, gb));
  if (aux && epi == EPI_MULAUX16) up(dX, round16(aux, nx).data(), nx * 2);
  else if (aux) up(dX, aux, nx * 4);
  if (byp_orig) {
    up(dbo, byp_orig, nc * 4);
    up(dbs, byp_scale, (size_t)N * 4);
  }
  GemmParams p = dense_gemm_params(dW.as<float>(), bias ? dB.as<float>() : nullptr, N, K, dA.p, K, M,
                                   dC.p, ncol);
  if (aux) {
    p.aux = dX.as<float>();
    p.ldaux = N;
  }
  if (byp_orig) {
    p.byp_orig = dbo.as<float>();
    p.byp_scale = dbs.as<float>();
  }
  if (f32) gemm_f32(p, epi, ALOAD_DENSE, false, nullptr);
  else if (h16) gemm_bf16(p, dWx.p, epi, ALOAD_DENSE, nullptr, a_bf16, c_bf16);
  else gemm_x3(p, dWx.p, (long)nw, epi, ALOAD_DENSE, nullptr, pieces);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  std::vector<unsigned char> guard(gb);
  ZASR_HIP_CHECK(hipMemcpy(guard.data(), dC.as<unsigned char>() + nc * ec, gb, hipMemcpyDeviceToHost));
  for (unsigned char g : guard) ZASR_REQUIRE(g == 0x5a, "selftest gemm: the kernel wrote past row M of C");
  if (c_bf16) {
    std::vector<__bf16> h(nc);
    ZASR_HIP_CHECK(hipMemcpy(h.data(), dC.p, nc * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nc; ++i) C[i] = (float)h[i];
  } else {
    ZASR_HIP_CHECK(hipMemcpy(C, dC.p, nc * 4, hipMemcpyDeviceToHost));
  }
}

void selftest_ffn_h3(int R, int D, int F, const float* Y, const float* W1, const float* b1,
                     const float* W2, const float* b2, const float* byp_orig,
                     const float* byp_scale, float* X, float* Xout) {
  ZASR_REQUIRE(R >= 1, "selftest ffn_h3: R >= 1");
  ZASR_REQUIRE(Xout == nullptr || Y == nullptr, "selftest ffn_h3: out of place reads X");
  ZASR_REQUIRE(ffn_h3_supported(D, F), "selftest ffn_h3: unsupported model / feed-forward dim");
  ZASR_REQUIRE(ffn_h3_weights_ok(W1, (long)F * D) && ffn_h3_weights_ok(W2, (long)F * D),
               "selftest ffn_h3: |w| must stay below 31");
  std::vector<__bf16> p1(2 * (size_t)F * D), p2(p1.size());
  ffn_pack_h3_host(W1, F, D, p1.data());
  ffn_pack_h3_host(W2, D, F, p2.data());
  const size_t xb = (size_t)R * D * 4;
  DevBuf dY(xb), dX(xb), d1(p1.size() * 2), d2(p2.size() * 2), db1((size_t)F * 4),
      db2((size_t)D * 4), dbo(byp_orig ? xb : 4), dbs((size_t)D * 4), dO(Xout ? xb : 4);
  if (Y) up(dY, Y, xb);
  up(dX, X, xb);
  if (Xout) up(dO, Xout, xb);  // what the kernel must overwrite
  up(d1, p1.data(), p1.size() * 2);
  up(d2, p2.data(), p2.size() * 2);
  up(db1, b1, (size_t)F * 4);
  up(db2, b2, (size_t)D * 4);
  if (byp_orig) {
    ZASR_REQUIRE(byp_scale != nullptr, "selftest ffn_h3: bypass needs its scale");
    up(dbo, byp_orig, xb);
    up(dbs, byp_scale, (size_t)D * 4);
  }
  launch_ffn_fused_h3(Xout ? dO.as<float>() : dX.as<float>(), R, D, F, d1.p, db1.as<float>(), d2.p,
                      db2.as<float>(), nullptr, byp_orig ? dbo.as<float>() : nullptr,
                      byp_orig ? dbs.as<float>() : nullptr, Y ? dY.as<float>() : nullptr,
                      Xout ? dX.as<float>() : nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ZASR_HIP_CHECK(hipMemcpy(X, dX.p, xb, hipMemcpyDeviceToHost));
  if (Xout) ZASR_HIP_CHECK(hipMemcpy(Xout, dO.p, xb, hipMemcpyDeviceToHost));
}

void selftest_ffn_bf16(int R, int D, int F, const float* W1, const float* b1, const float* W2,
                       const float* b2, const float* byp_orig, const float* byp_scale, float* X,
                       int form, float* Xout) {
  ZASR_REQUIRE(form == 0 || form == 1, "selftest ffn_bf16: form 0 (default route) or 1 (rows form)");
  ZASR_REQUIRE(R >= 1, "selftest ffn_bf16: R >= 1");
  ZASR_REQUIRE(ffn_fused_supported(D), "selftest ffn_bf16: unsupported model dim");
  // W1 [F][D] and W2 [D][F] in bf16; d >= 256 in MFMA-fragment order (the engine's wp)
  std::vector<__bf16> h1((size_t)F * D), h2((size_t)D * F);
  for (size_t i = 0; i < h1.size(); ++i) h1[i] = (__bf16)W1[i];
  for (size_t i = 0; i < h2.size(); ++i) h2[i] = (__bf16)W2[i];
  if (D >= 256) {
    std::vector<__bf16> p1(h1.size()), p2(h2.size());
    ffn_pack_host(h1.data(), F, D, p1.data());
    ffn_pack_host(h2.data(), D, F, p2.data());
    h1.swap(p1);
    h2.swap(p2);
  }
  const size_t xb = (size_t)R * D * 4;
  DevBuf dX(xb), d1(h1.size() * 2), d2(h2.size() * 2), db1((size_t)F * 4), db2((size_t)D * 4),
      dbo(byp_orig ? xb : 4), dbs((size_t)D * 4), dO(Xout ? xb : 4);
  up(dX, X, xb);
  if (Xout) up(dO, Xout, xb);  // what the kernel must overwrite
  up(d1, h1.data(), h1.size() * 2);
  up(d2, h2.data(), h2.size() * 2);
  up(db1, b1, (size_t)F * 4);
  up(db2, b2, (size_t)D * 4);
  if (byp_orig) {
    ZASR_REQUIRE(byp_scale != nullptr, "selftest ffn_bf16: bypass needs its scale");
    up(dbo, byp_orig, xb);
    up(dbs, byp_scale, (size_t)D * 4);
  }
  const int saved = ffn_rows_on();
  ffn_set_rows(form);
  try {
    launch_ffn_fused(Xout ? dO.as<float>() : dX.as<float>(), R, D, F, d1.p, db1.as<float>(), d2.p,
                     db2.as<float>(), nullptr, byp_orig ? dbo.as<float>() : nullptr,
                     byp_orig ? dbs.as<float>() : nullptr, Xout ? dX.as<float>() : nullptr);
  } catch (...) {
    ffn_set_rows(saved);
    throw;
  }
  ffn_set_rows(saved);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ZASR_HIP_CHECK(hipMemcpy(X, dX.p, xb, hipMemcpyDeviceToHost));
  if (Xout) ZASR_HIP_CHECK(hipMemcpy(Xout, dO.p, xb, hipMemcpyDeviceToHost));
}

void selftest_seam(int nseq, const int* L, int d, int ds, int dn, int ds_next, int c0, int ldo,
                   const float* xd, const float* orig, const float* s, const float* wn8,
                   const float* wo2, float* next, float* xnext, float* out, float* next_ref,
                   float* xnext_ref, float* out_ref) {
  ZASR_REQUIRE(nseq >= 1 && d >= 4 && dn >= 0 && ds >= 1 && ds_next >= 1 && c0 >= 0,
               "selftest seam: sizes");
  ZASR_REQUIRE(ldo % 4 == 0 && ldo >= d, "selftest seam: output row stride >= d, a multiple of 4");
  const bool has_x = ds_next > 1 && dn > 0, has_out = c0 < d;
  // the levels the engine forms: 50 Hz, the stack's own, the next stack's, the 25 Hz output
  auto level = [&](int f, std::vector<int>& off) {
    off.assign(nseq + 1, 0);
    for (int b = 0; b < nseq; ++b) {
      ZASR_REQUIRE(L[b] >= 1, "selftest seam: every sequence needs a frame");
      off[b + 1] = off[b] + (L[b] + f - 1) / f;
    }
    return off[nseq];
  };
  std::vector<int> oL, oS, oN, oO;
  const int rows = level(1, oL), rs = level(ds, oS), rn = level(ds_next, oN), ro = level(2, oO);
  const size_t ib = (size_t)(nseq + 1) * 4;
  DevBuf dL(ib), dS(ib), dN(ib), dO(ib), mL((size_t)rows * 4), mN((size_t)rn * 4),
      mO((size_t)ro * 4);
  up(dL, oL.data(), ib);
  up(dS, oS.data(), ib);
  up(dN, oN.data(), ib);
  up(dO, oO.data(), ib);
  launch_row2seq(dL.as<int>(), nseq, rows, mL.as<int>(), nullptr);
  launch_row2seq(dN.as<int>(), nseq, rn, mN.as<int>(), nullptr);
  launch_row2seq(dO.as<int>(), nseq, ro, mO.as<int>(), nullptr);
  const size_t bo = (size_t)rows * d * 4, bx = (size_t)rs * d * 4, bn = (size_t)rows * dn * 4,
               bxn = (size_t)rn * dn * 4, bout = (size_t)ro * ldo * 4, bfull = (size_t)rows * ldo * 4;
  DevBuf dorig(bo), dxd(bx), ds_(d * 4), dnext(bn), dxn(bxn), dout(bout), dnext_r(bn), dxn_r(bxn),
      dout_r(bout), dfull(bfull);
  up(dorig, orig, bo);
  if (ds > 1) {
    up(dxd, xd, bx);
    up(ds_, s, (size_t)d * 4);
  }
  // both sides start from the caller's images, so what a kernel leaves alone shows
  up(dnext, next, bn);
  up(dnext_r, next, bn);
  if (has_x) {
    up(dxn, xnext, bxn);
    up(dxn_r, xnext, bxn);
  }
  up(dout, out, bout);
  up(dout_r, out, bout);
  ZASR_HIP_CHECK(hipMemset(dfull.p, 0, bfull > 0 ? bfull : 4));
  SeamDesc sd;
  sd.xd = dxd.as<float>();
  sd.orig = dorig.as<float>();
  sd.s = ds_.as<float>();
  sd.off_in = dL.as<int>();
  sd.off_ds = dS.as<int>();
  sd.off_run = ds_next > 1 ? dN.as<int>() : dO.as<int>();
  sd.map_run = ds_next > 1 ? mN.as<int>() : mO.as<int>();
  sd.runs = ds_next > 1 ? rn : ro;
  sd.rows = rows;
  sd.d = d;
  sd.ds = ds;
  sd.next = dn > 0 ? dnext.as<float>() : nullptr;
  sd.dn = dn;
  sd.ds_next = ds_next;
  if (has_x) {
    sd.xnext = dxn.as<float>();
    sd.wn_host8 = wn8;
  }
  if (has_out) {
    sd.out = dout.as<float>();
    sd.off_out = dO.as<int>();
    sd.wo_host2 = wo2;
    sd.ldo = ldo;
    sd.c0 = c0;
  }
  launch_seam(sd, nullptr);
  // the composition it replaces: glue -> downsample(next) -> downsample(full, 2)
  launch_stack_glue(dxd.as<float>(), dorig.as<float>(), dL.as<int>(), dS.as<int>(), mL.as<int>(),
                    rows, d, ds, ds_.as<float>(), dn > 0 ? dnext_r.as<float>() : nullptr, dn,
                    has_out ? dfull.as<float>() : nullptr, ldo, c0, nullptr);
  if (has_x)
    launch_downsample(dnext_r.as<float>(), dL.as<int>(), dN.as<int>(), mN.as<int>(), rn, dn,
                      ds_next, wn8, dxn_r.as<float>(), nullptr);
  if (has_out)
    launch_downsample(dfull.as<float>(), dL.as<int>(), dO.as<int>(), mO.as<int>(), ro, ldo, 2, wo2,
                      dout_r.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  auto down = [](void* h, const DevBuf& dv, size_t bytes) {
    if (bytes) ZASR_HIP_CHECK(hipMemcpy(h, dv.p, bytes, hipMemcpyDeviceToHost));
  };
  down(next, dnext, bn);
  down(next_ref, dnext_r, bn);
  if (has_x) {
    down(xnext, dxn, bxn);
    down(xnext_ref, dxn_r, bxn);
  }
  down(out, dout, bout);
  down(out_ref, dout_r, bout);
}

// ---- the convolution path's kernels and BiasNorm ----
namespace {
std::vector<__bf16> round16(const float* s, size_t n) {
  std::vector<__bf16> h(n);
  for (size_t i = 0; i < n; ++i) h[i] = (__bf16)s[i];
  return h;
}

// one ragged level as the engine forms it: offsets from the per-sequence lengths (each less
// `cut` frames), the row -> sequence map from launch_row2seq
struct Level {
  std::vector<int> off;
  int rows;
  DevBuf d_off, d_map;
  Level(int nseq, const int* len, int cut)
      : off(offsets(nseq, len, cut)), rows(off.back()), d_off(off.size() * 4),
        d_map((size_t)rows * 4) {
    up(d_off, off.data(), off.size() * 4);
    launch_row2seq(d_off.as<int>(), nseq, rows, d_map.as<int>(), nullptr);
  }
  static std::vector<int> offsets(int nseq, const int* len, int cut) {
    ZASR_REQUIRE(nseq >= 1 && len != nullptr, "selftest: at least one sequence");
    std::vector<int> o(nseq + 1, 0);
    for (int b = 0; b < nseq; ++b) {
      ZASR_REQUIRE(len[b] - cut >= 1, "selftest: every sequence needs a frame at every level");
      o[b + 1] = o[b] + len[b] - cut;
    }
    return o;
  }
};

// an output image of n elements (f32, or bf16: rounded to nearest even on upload, widened on
// return) that starts as the caller's, with one guard row of `row` elements behind it
struct OutBuf {
  size_t n, row, eb;
  DevBuf d;
  OutBuf(const float* init, size_t n_, size_t row_, bool h16)
      : n(n_), row(row_), eb(h16 ? 2 : 4), d((n_ + row_) * (h16 ? 2 : 4)) {
    if (h16) up(d, round16(init, n).data(), n * 2);
    else up(d, init, n * 4);
    ZASR_HIP_CHECK(hipMemset(d.as<unsigned char>() + n * eb, 0x5a, row * eb));
  }
  template <class T>
  T* as() const { return d.as<T>(); }
  // after the kernel: the guard row intact, then the image back to the caller
  void down(float* out, const char* what) const {
    std::vector<unsigned char> guard(row * eb);
    ZASR_HIP_CHECK(hipMemcpy(guard.data(), d.as<unsigned char>() + n * eb, guard.size(),
                             hipMemcpyDeviceToHost));
    for (unsigned char g : guard)
      ZASR_REQUIRE(g == 0x5a, std::string("selftest ") + what + ": the kernel wrote past the last row");
    if (n == 0) return;
    if (eb == 2) {
      std::vector<__bf16> h(n);
      ZASR_HIP_CHECK(hipMemcpy(h.data(), d.p, n * 2, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
    } else {
      ZASR_HIP_CHECK(hipMemcpy(out, d.p, n * 4, hipMemcpyDeviceToHost));
    }
  }
};

void up16(DevBuf& d, const float* h, size_t n, bool h16) {
  if (h16) up(d, round16(h, n).data(), n * 2);
  else up(d, h, n * 4);
}
}  // namespace

void selftest_dwconv1d(int nseq, const int* L, int d, int K, bool glu, bool bf16, const float* x,
                       const float* w, const float* b, float* out) {
  ZASR_REQUIRE(!(glu && bf16), "selftest dwconv1d: the GLU form is f32 only");
  ZASR_REQUIRE(d >= 4 && d % 4 == 0, "selftest dwconv1d: d a positive multiple of 4");
  ZASR_REQUIRE(K >= 1 && K <= 31 && (K & 1), "selftest dwconv1d: K odd, at most 31");
  Level lv(nseq, L, 0);
  const size_t nx = (size_t)lv.rows * (glu ? 2 * d : d), no = (size_t)lv.rows * d;
  DevBuf dX(nx * (bf16 ? 2 : 4)), dW((size_t)d * K * 4), dB((size_t)d * 4);
  up16(dX, x, nx, bf16);
  up(dW, w, (size_t)d * K * 4);
  up(dB, b, (size_t)d * 4);
  OutBuf o(out, no, d, bf16);
  if (glu)
    launch_glu_dwconv1d(dX.as<float>(), lv.d_off.as<int>(), lv.d_map.as<int>(), lv.rows, d, K,
                        dW.as<float>(), dB.as<float>(), o.as<float>(), nullptr);
  else if (bf16)
    launch_dwconv1d_post_glu_bf16(dX.p, lv.d_off.as<int>(), lv.d_map.as<int>(), lv.rows, d, K,
                                  dW.as<float>(), dB.as<float>(), o.d.p, nullptr);
  else
    launch_dwconv1d_post_glu(dX.as<float>(), lv.d_off.as<int>(), lv.d_map.as<int>(), lv.rows, d, K,
                             dW.as<float>(), dB.as<float>(), o.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(out, "dwconv1d");
}

void selftest_conv1(int nseq, const int* T, int form, const float* fb, const float* w,
                    const float* b, float* out) {
  ZASR_REQUIRE(form >= 0 && form <= 2, "selftest conv1: form 0 (libm), 1 (fast) or 2 (bf16 out)");
  Level lf(nseq, T, 0), lc(nseq, T, 2);  // fbank rows, conv.0 rows (T - 2 per sequence)
  DevBuf dF((size_t)lf.rows * 80 * 4), dW(8 * 9 * 4), dB(8 * 4);
  up(dF, fb, (size_t)lf.rows * 80 * 4);
  up(dW, w, 8 * 9 * 4);
  up(dB, b, 8 * 4);
  OutBuf o(out, (size_t)lc.rows * 640, 640, form == 2);
  launch_conv1(dF.as<float>(), lf.d_off.as<int>(), lc.d_off.as<int>(), lc.d_map.as<int>(), lc.rows,
               dW.as<float>(), dB.as<float>(), o.d.p, form == 2, nullptr, form == 1);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(out, "conv1");
}

void selftest_convnext(int nseq, const int* L, int form, const float* x, const float* dw_w,
                       const float* dw_b, const float* w1, const float* b1, const float* w2,
                       const float* b2, float* y, float* out) {
  ZASR_REQUIRE(form >= 0 && form <= 2,
               "selftest convnext: form 0 (depthwise f32), 1 (bf16 block) or 2 (f16x3 block)");
  ZASR_REQUIRE(form == 0 || (w1 && b1 && w2 && b2 && out), "selftest convnext: the MLP's operands");
  Level lv(nseq, L, 0);
  constexpr size_t kRow = 19 * 128, kW = 384 * 128;
  const size_t n = (size_t)lv.rows * kRow;
  const bool h16 = form == 1;
  DevBuf dWd(128 * 49 * 4), dBd(128 * 4), d1(2 * kW * 2), d2(2 * kW * 2), db1(384 * 4), db2(128 * 4);
  up(dWd, dw_w, 128 * 49 * 4);
  up(dBd, dw_b, 128 * 4);
  OutBuf oy(y, n, kRow, h16);
  const int *off = lv.d_off.as<int>(), *map = lv.d_map.as<int>();
  if (form == 0) {
    DevBuf dX(n * 4);
    up(dX, x, n * 4);
    launch_dwconv2d_tiled(dX.as<float>(), off, map, lv.rows, dWd.as<float>(), dBd.as<float>(),
                          oy.as<float>(), nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    oy.down(y, "convnext");
    return;
  }
  up(db1, b1, 384 * 4);
  up(db2, b2, 128 * 4);
  // pw1 [384][128] / pw2 [128][384] as the loader prepares them (engine_load.cpp): bf16, or the
  // two fp16 pieces (hi, (w - hi) * 2^11), every image in MFMA-fragment order
  auto pack = [&](const float* wsrc, int rows, int cols, DevBuf& dst) {
    std::vector<__bf16> img(2 * kW), piece(kW);
    if (h16) {
      pack_frag32_host(round16(wsrc, kW).data(), rows, cols, img.data());
    } else {
      for (int t = 0; t < 2; ++t) {
        for (size_t i = 0; i < kW; ++i) {
          const _Float16 hi = (_Float16)wsrc[i];
          const _Float16 v = t == 0 ? hi : (_Float16)((wsrc[i] - (float)hi) * 2048.f);
          std::memcpy(&piece[i], &v, 2);
        }
        pack_frag32_host(piece.data(), rows, cols, img.data() + t * kW);
      }
    }
    up(dst, img.data(), (h16 ? 1 : 2) * kW * 2);
  };
  pack(w1, 384, 128, d1);
  pack(w2, 128, 384, d2);
  if (h16) {
    DevBuf dX(n * 2);
    up16(dX, x, n, true);
    OutBuf oo(out, n, kRow, true);
    launch_convnext_bf16(dX.p, off, map, lv.rows, dWd.as<float>(), dBd.as<float>(), d1.p,
                         db1.as<float>(), d2.p, db2.as<float>(), oy.d.p, oo.d.p, nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    oy.down(y, "convnext");
    oo.down(out, "convnext");
    return;
  }
  // f16x3: the engine's pair of calls, the MLP in place over x (its residual and its output)
  OutBuf ox(x, n, kRow, false);
  launch_dwconv2d_tiled(ox.as<float>(), off, map, lv.rows, dWd.as<float>(), dBd.as<float>(),
                        oy.as<float>(), nullptr);
  launch_convnext_mlp_h3(oy.as<float>(), ox.as<float>(), (long)lv.rows * 19, d1.p, db1.as<float>(),
                         d2.p, db2.as<float>(), ox.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  oy.down(y, "convnext");
  ox.down(out, "convnext");
}

void selftest_bias_norm(int rows, int d, const float* bias, float log_scale, float* orig,
                        const float* bscale, int copy_mode, float* x, float* copy_out) {
  ZASR_REQUIRE(rows >= 1 && d >= 4, "selftest bias_norm: rows >= 1, d >= 4");
  ZASR_REQUIRE((orig == nullptr) == (bscale == nullptr), "selftest bias_norm: the blend takes both operands");
  ZASR_REQUIRE(copy_mode >= 0 && copy_mode <= 2 && (copy_mode != 1 || copy_out != nullptr) &&
                   (copy_mode != 2 || orig != nullptr),
               "selftest bias_norm: copy_mode 0 (none), 1 (copy_out) or 2 (over orig)");
  const size_t n = (size_t)rows * d;
  DevBuf dB((size_t)d * 4), dS((size_t)d * 4);
  up(dB, bias, (size_t)d * 4);
  if (bscale) up(dS, bscale, (size_t)d * 4);
  OutBuf ox(x, n, d, false);
  std::unique_ptr<OutBuf> oo, oc;
  if (orig) oo.reset(new OutBuf(orig, n, d, false));
  if (copy_mode == 1) oc.reset(new OutBuf(copy_out, n, d, false));
  float* co = copy_mode == 1 ? oc->as<float>() : copy_mode == 2 ? oo->as<float>() : nullptr;
  launch_bias_norm(ox.as<float>(), rows, d, dB.as<float>(), log_scale,
                   orig ? oo->as<float>() : nullptr, bscale ? dS.as<float>() : nullptr, nullptr, co);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ox.down(x, "bias_norm");
  if (oo) oo->down(orig, "bias_norm");
  if (oc) oc->down(copy_out, "bias_norm");
}

// ---- the joiner kernels ----
namespace {
// J [M][D] as the search kernels leave it for the packed joiner (kernels.h JoinerArgs; written
// here from that description, not with the device packer): element (row, k) of an image at
// ((row / 32 * (D / 16) + k / 16) * 64 + row % 32 + 32 * (k / 8 % 2)) * 8 + k % 8, `rows` rows a
// multiple of 64, one image per stored piece.  Pieces as store_j4 writes them: bf16 (pieces 0),
// successive bf16 residuals, or the fp16 hi piece and (x - hi) * 2^11.  Rows past M hold `pad`.
std::vector<__bf16> pack_j_host(const float* J, int M, int D, long rows, int pieces, float pad) {
  const int np = pieces ? stored_pieces(pieces) : 1;
  const size_t plane = (size_t)rows * D;
  std::vector<__bf16> img(plane * np);
  for (long row = 0; row < rows; ++row)
    for (int k = 0; k < D; ++k) {
      const size_t at = ((size_t)((row / 32) * (D / 16) + k / 16) * 64 + row % 32 + 32 * (k / 8 % 2)) * 8 + k % 8;
      float x = row < M ? J[(size_t)row * D + k] : pad;
      if (pieces == kPiecesF16) {
        const _Float16 hi = (_Float16)x, lo = (_Float16)((x - (float)hi) * 2048.f);
        std::memcpy(&img[at], &hi, 2);
        std::memcpy(&img[plane + at], &lo, 2);
        continue;
      }
      for (int t = 0; t < np; ++t) {
        const __bf16 v = (__bf16)x;
        img[t * plane + at] = v;
        x -= (float)v;
      }
    }
  return img;
}
}  // namespace

void selftest_joiner(int mode, int layout, int M, int V, int D, const float* J, const float* W,
                     const float* bias, const int* live_t, const int* live_len, int live_f,
                     float* out) {
  const bool f32 = mode == ZASR_PRECISION_FP32, h16 = mode == ZASR_PRECISION_BF16;
  const int pieces = mode == ZASR_PRECISION_BF16X3   ? 2
                     : mode == ZASR_PRECISION_BF16X6 ? 3
                     : mode == ZASR_PRECISION_F16X3  ? kPiecesF16
                                                     : 0;
  ZASR_REQUIRE(f32 || h16 || pieces != 0,
               "selftest joiner: mode must be ZASR_PRECISION_FP32, _BF16, _BF16X3, _BF16X6 or _F16X3");
  ZASR_REQUIRE(layout == 0 || (layout == 1 && !f32), "selftest joiner: layout 0, or 1 outside fp32");
  ZASR_REQUIRE(M >= 1 && V >= 1 && D >= 16 && D % 16 == 0, "selftest joiner: M, V >= 1, D % 16 == 0");
  const int np = pieces ? stored_pieces(pieces) : 1;
  const size_t nj = (size_t)M * D, nw = (size_t)V * D;
  // W as the loader prepares it (engine_load.cpp): bf16, or the split pieces; layout 1: every
  // piece in fragment order
  const size_t pe = layout == 1 ? (size_t)gemm_rp_packed_elems(V, D) : 0;
  DevBuf dW(nw * 4), dWx(nw * 2 * np), dWp(pe * 2 * np), dB((size_t)V * 4);
  up(dW, W, nw * 4);
  up(dB, bias, (size_t)V * 4);
  if (h16) convert_to_bf16(dW.as<float>(), dWx.p, (long)nw, nullptr);
  if (pieces) split_to_bf16(dW.as<float>(), dWx.p, (long)nw, pieces, nullptr);
  for (int t = 0; layout == 1 && t < np; ++t)
    gemm_rp_pack_weights(dWx.as<__bf16>() + t * nw, V, D, dWp.as<__bf16>() + t * pe, nullptr);
  // J as its producers leave it (decjoin_kernel row-major, store_j4 packed)
  const long jrows = joiner_packed_rows(M);
  DevBuf dJ(layout == 1 ? (size_t)jrows * D * 2 * np : nj * 4);
  if (layout == 1) {
    const std::vector<__bf16> img = pack_j_host(J, M, D, jrows, pieces, 0.75f);
    up(dJ, img.data(), img.size() * 2);
  } else if (h16) {
    up(dJ, round16(J, nj).data(), nj * 2);
  } else {
    up(dJ, J, nj * 4);
  }
  const int ns = live_t ? (M + live_f - 1) / live_f : 0;
  DevBuf dT((size_t)ns * 4), dL((size_t)ns * 4);
  if (live_t) {
    up(dT, live_t, (size_t)ns * 4);
    up(dL, live_len, (size_t)ns * 4);
  }
  OutBuf o(out, (size_t)M * V, V, false);  // a skipped tile keeps the caller's values
  JoinerArgs ja{dJ.p, layout == 1 ? dWp.p : f32 ? dW.p : dWx.p, dB.as<float>(), o.as<float>(), M, V, D};
  ja.layout = layout == 1 ? JOINER_PACKED : h16 ? JOINER_BF16 : JOINER_F32;
  ja.pieces = pieces;
  ja.j_plane = jrows * D;
  ja.w_plane = layout == 1 ? (long)pe : (long)nw;
  ja.live_t = live_t ? dT.as<int>() : nullptr;
  ja.live_len = live_t ? dL.as<int>() : nullptr;
  ja.live_f = live_t ? live_f : 0;
  launch_joiner(ja, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(out, "joiner");
}

// ---- the attention kernels ----
namespace {
constexpr size_t kAttnGuard = 1024;  // guard bytes behind every attention output

// an output of `bytes` bytes that starts as the caller's image, kAttnGuard guard bytes behind it
struct GuardedOut {
  size_t bytes;
  DevBuf d;
  GuardedOut(const void* init, size_t bytes_) : bytes(bytes_), d(bytes_ + kAttnGuard) {
    up(d, init, bytes);
    ZASR_HIP_CHECK(hipMemset(d.as<unsigned char>() + bytes, 0x5a, kAttnGuard));
  }
  void down(void* out, const char* what) const {
    unsigned char guard[kAttnGuard];
    ZASR_HIP_CHECK(hipMemcpy(guard, d.as<unsigned char>() + bytes, kAttnGuard, hipMemcpyDeviceToHost));
    for (unsigned char g : guard)
      ZASR_REQUIRE(g == 0x5a, std::string("selftest ") + what + ": the kernel wrote past its output");
    if (bytes) ZASR_HIP_CHECK(hipMemcpy(out, d.p, bytes, hipMemcpyDeviceToHost));
  }
};
// the same for an output the mode stores in f32 or in bf16 (rounded on upload, widened on return)
struct GuardedOut16 {
  size_t n;
  bool h16;
  std::unique_ptr<GuardedOut> g;
  GuardedOut16(const float* init, size_t n_, bool h16_) : n(n_), h16(h16_) {
    if (h16) g.reset(new GuardedOut(round16(init, n).data(), n * 2));
    else g.reset(new GuardedOut(init, n * 4));
  }
  void* p() const { return g->d.p; }
  void down(float* out, const char* what) const {
    if (!h16) return g->down(out, what);
    std::vector<__bf16> h(n);
    g->down(h.data(), what);
    for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
  }
};

// one ragged attention problem on the device as a decode prepares it: the packed-row offsets,
// head 0's weight offsets and the t1^T columns (attn_head0_layout), qkp [R][68 H] and the
// positional table [2 pmax - 1][4 H].  Every shape the kernels cannot take is refused here,
// before anything is launched.
struct AttnProblem {
  bool f32, h16, flash;
  int pieces, H, nseq, pmax, R = 0, maxL = 0;
  std::vector<int> len, off;
  AttnHead0Layout lay;
  std::unique_ptr<DevBuf> d_off, d_aoff, d_o32, d_qkp, d_pos, d_map;

  AttnProblem(const char* what, int mode, int H_, int nseq_, const int* L, int pmax_,
              const float* qkp, const float* pos_tab)
      : H(H_), nseq(nseq_), pmax(pmax_) {
    const std::string w = std::string("selftest ") + what + ": ";
    f32 = mode == ZASR_PRECISION_FP32;
    h16 = mode == ZASR_PRECISION_BF16;
    pieces = mode == ZASR_PRECISION_BF16X3   ? 2
             : mode == ZASR_PRECISION_BF16X6 ? 3
             : mode == ZASR_PRECISION_F16X3  ? kPiecesF16
                                             : 0;
    flash = !f32;
    ZASR_REQUIRE(f32 || h16 || pieces != 0,
                 w + "mode must be ZASR_PRECISION_FP32, _BF16, _BF16X3, _BF16X6 or _F16X3");
    ZASR_REQUIRE(nseq >= 1 && nseq <= kAttnMapMaxSeq && L != nullptr, w + "at least one sequence");
    ZASR_REQUIRE(H >= 1 && (!flash || (H % 2 == 0 && H <= kAttnMapMaxUnits)),
                 w + "the flash kernels take an even head count of at most 16");
    off.assign(nseq + 1, 0);
    for (int b = 0; b < nseq; ++b) {
      ZASR_REQUIRE(L[b] >= 0 && L[b] <= 128 * kAttnMapMaxTiles, w + "sequence length out of range");
      len.push_back(L[b]);
      off[b + 1] = off[b] + L[b];
      maxL = std::max(maxL, L[b]);
    }
    R = off[nseq];
    ZASR_REQUIRE(R >= 1, w + "at least one frame");
    // the flash kernels clamp the positional rows; the fp32 kernels read rows j - i for every
    // (query, key) of their 32 x 32 tiles unclamped, |j - i| < max(L) rounded up to 32
    ZASR_REQUIRE(pmax >= (flash ? maxL : (maxL + 31) / 32 * 32),
                 w + "pmax below the longest sequence (fp32: rounded up to 32)");
    lay = attn_head0_layout(len.data(), nseq, flash);
    const size_t nq = (size_t)R * 68 * H, np = (size_t)(2 * pmax - 1) * 4 * H;
    d_off.reset(new DevBuf(off.size() * 4));
    d_aoff.reset(new DevBuf(lay.a_off.size() * sizeof(long)));
    d_o32.reset(new DevBuf(lay.o32.size() * 4));
    d_qkp.reset(new DevBuf(nq * (h16 ? 2 : 4)));
    d_pos.reset(new DevBuf(np * 4));
    d_map.reset(new DevBuf((size_t)R * 4));
    up(*d_off, off.data(), off.size() * 4);
    up(*d_aoff, lay.a_off.data(), lay.a_off.size() * sizeof(long));
    up(*d_o32, lay.o32.data(), lay.o32.size() * 4);
    up16(*d_qkp, qkp, nq, h16);
    up(*d_pos, pos_tab, np * 4);
  }
  // the flash arguments the engine's attention_weights forms
  AttnFlashArgs flash_args() const {
    AttnFlashArgs a{};
    a.qkp = d_qkp->p;
    a.H = H;
    a.pos_tab = d_pos->as<float>();
    a.pmax = pmax;
    a.row_off = d_off->as<int>();
    a.a_off = d_aoff->as<long>();
    a.nseq = nseq;
    a.max_len = maxL;
    a.pieces = h16 ? 1 : pieces;
    return a;
  }
};

// one block map in the engine's order 0, on the device
struct AttnMap {
  std::vector<unsigned> host;
  int n;
  DevBuf d;
  static std::vector<unsigned> make(const std::vector<int>& len, int units) {
    std::vector<unsigned> m;
    build_attn_block_map(len.data(), (int)len.size(), units, 0, m);
    return m;
  }
  AttnMap(const std::vector<int>& len, int units)
      : host(make(len, units)), n((int)host.size()), d(host.size() * 4) {
    up(d, host.data(), host.size() * 4);
  }
};
}  // namespace

void selftest_attn_weights(int mode, int H, int nseq, const int* L, int pmax, const float* qkp,
                           const float* pos_tab, float* A0) {
  AttnProblem c("attn_weights", mode, H, nseq, L, pmax, qkp, pos_tab);
  ZASR_REQUIRE(c.f32 || c.pieces == 2 || c.pieces == 3,
               "selftest attn_weights: head 0's weights are materialised in the fp32, bf16x3 and "
               "bf16x6 modes only (bf16 and f16x3 consume them inside flash mode 3)");
  GuardedOut o(A0, c.lay.elems * 4);
  if (c.f32) {
    GuardedOut st(std::vector<float>((size_t)c.R * H * 2, 0.f).data(), (size_t)c.R * H * 2 * 4);
    AttnArgs a{c.d_qkp->as<float>(), H, c.d_pos->as<float>(), pmax, c.d_off->as<int>(),
               c.d_aoff->as<long>(), nseq, c.maxL, o.d.as<float>(), st.d.as<float>(), 1};
    launch_attn_softmax(a, nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> sink((size_t)c.R * H * 2);
    st.down(sink.data(), "attn_weights");
  } else {
    const AttnMap m(c.len, 1);
    AttnFlashArgs a = c.flash_args();
    a.attn = o.d.p;
    a.map = m.d.as<unsigned>();
    a.map_len = m.n;
    launch_attn_flash(a, 0, nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
  }
  o.down(A0, "attn_weights");
}

void selftest_attn_sa(int mode, int H, int nseq, const int* L, int pmax, const float* qkp,
                      const float* pos_tab, const float* v1, const float* v2, float* out1,
                      float* stats, float* out2) {
  AttnProblem c("attn_sa", mode, H, nseq, L, pmax, qkp, pos_tab);
  const size_t n = (size_t)c.R * 12 * H, ns = (size_t)c.R * H * (c.f32 ? 2 : 1);
  // bf16: 4 readable elements behind v, the flash kernels' read contract (kernels.h)
  const size_t vb = c.h16 ? (n + 4) * 2 : n * 4;
  DevBuf dv1(vb), dv2(vb);
  ZASR_HIP_CHECK(hipMemset(dv1.p, 0, vb));
  ZASR_HIP_CHECK(hipMemset(dv2.p, 0, vb));
  up16(dv1, v1, n, c.h16);
  up16(dv2, v2, n, c.h16);
  GuardedOut16 o1(out1, n, c.h16), o2(out2, n, c.h16);
  GuardedOut st(stats, ns * 4);
  if (c.flash) {
    const AttnMap m(c.len, H);
    AttnFlashArgs a = c.flash_args();
    a.map = m.d.as<unsigned>();
    a.map_len = m.n;
    a.stats_in = st.d.as<float>();
    a.stats_out = st.d.as<float>();
    a.v = dv1.p;
    a.out = o1.p();
    launch_attn_flash(a, 1, nullptr);
    a.v = dv2.p;
    a.out = o2.p();
    launch_attn_flash(a, 2, nullptr);
  } else {
    AttnSAArgs sa{c.d_qkp->as<float>(), H, c.d_pos->as<float>(), pmax, c.d_off->as<int>(), nseq,
                  c.maxL, st.d.as<float>(), dv1.as<float>(), reinterpret_cast<float*>(o1.p()),
                  st.d.as<float>()};
    launch_attn_sa(sa, true, false, nullptr);
    sa.v = dv2.as<float>();
    sa.out = reinterpret_cast<float*>(o2.p());
    launch_attn_sa(sa, false, false, nullptr);
  }
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o1.down(out1, "attn_sa");
  st.down(stats, "attn_sa");
  o2.down(out2, "attn_sa");
}

void selftest_nonlin(int mode, int H, int nseq, const int* L, int pmax, int hid, const float* qkp,
                     const float* pos_tab, const float* h3, unsigned short* t1t, float* z) {
  AttnProblem c("nonlin", mode, H, nseq, L, pmax, qkp, pos_tab);
  ZASR_REQUIRE(!c.f32, "selftest nonlin: the fp32 route (row-major t1) is not covered");
  ZASR_REQUIRE(hid >= 4 && hid % 4 == 0, "selftest nonlin: hid a positive multiple of 4");
  const bool fused = c.h16 || c.pieces == kPiecesF16;  // flash mode 3 follows the transpose
  ZASR_REQUIRE(!fused || z != nullptr, "selftest nonlin: z");
  const int np = c.h16 ? 1 : c.pieces, R32 = c.lay.R32;
  const size_t nh = (size_t)c.R * 3 * hid, nt = (size_t)stored_pieces(np) * hid * R32,
               nz = (size_t)c.R * hid;
  DevBuf dh(nh * (c.h16 ? 2 : 4));
  up16(dh, h3, nh, c.h16);
  launch_row2seq(c.d_off->as<int>(), nseq, c.R, c.d_map->as<int>(), nullptr);
  GuardedOut ot(t1t, nt * 2);
  launch_nonlin_prep_t(dh.p, c.h16, c.d_off->as<int>(), c.d_o32->as<int>(), c.d_map->as<int>(), c.R,
                       hid, R32, ot.d.p, nullptr, np);
  if (!fused) {
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    ot.down(t1t, "nonlin");
    return;
  }
  GuardedOut16 oz(z, nz, c.h16);
  const AttnMap m(c.len, attn_nonlin_chunks(hid, np));
  AttnFlashArgs a = c.flash_args();
  a.t1t = ot.d.p;
  a.o8 = c.d_o32->as<int>();
  a.ldt = R32;
  a.hid = hid;
  a.y = c.h16 ? (const void*)(dh.as<__bf16>() + 2 * hid) : (const void*)(dh.as<float>() + 2 * hid);
  a.ldy = 3 * hid;
  a.z = oz.p();
  a.map = m.d.as<unsigned>();
  a.map_len = m.n;
  launch_attn_flash(a, 3, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ot.down(t1t, "nonlin");
  oz.down(z, "nonlin");
}

// ---- the transducer search kernels ----
namespace {
constexpr size_t kSearchGuard = 256;  // guard bytes before the first and behind every array

// every array of one call in one device allocation, one upload and one download: array i starts
// 256-aligned, the bytes up to the next array (at least kSearchGuard) are guard bytes
struct SearchArena {
  struct Seg {
    size_t off, bytes;
    const void* src;
    void* dst;  // null: an input
  };
  std::vector<Seg> segs;
  size_t total = kSearchGuard;
  std::unique_ptr<DevBuf> d;
  size_t add(const void* src, size_t bytes, void* dst = nullptr) {
    segs.push_back(Seg{total, bytes, src, dst});
    total += (bytes + 255) / 256 * 256 + kSearchGuard;
    return segs.size() - 1;
  }
  template <class T>
  size_t io(T* p, size_t n) { return add(p, n * sizeof(T), p); }
  template <class T>
  size_t in(const T* p, size_t n) { return add(p, n * sizeof(T)); }
  void upload() {
    std::vector<unsigned char> img(total, 0x5a);
    for (const Seg& g : segs)
      if (g.bytes) std::memcpy(img.data() + g.off, g.src, g.bytes);
    d.reset(new DevBuf(total));
    up(*d, img.data(), total);
  }
  template <class T>
  T* at(size_t i) const { return reinterpret_cast<T*>(d->as<unsigned char>() + segs[i].off); }
  // the guard bytes intact, then every in / out array back to the caller
  void download(const char* what) const {
    std::vector<unsigned char> img(total);
    ZASR_HIP_CHECK(hipMemcpy(img.data(), d->p, total, hipMemcpyDeviceToHost));
    size_t pos = 0;
    for (size_t i = 0; i <= segs.size(); ++i) {
      const size_t end = i < segs.size() ? segs[i].off : total;
      for (; pos < end; ++pos)
        ZASR_REQUIRE(img[pos] == 0x5a,
                     std::string("selftest ") + what + ": the kernel wrote outside its arrays");
      if (i < segs.size()) pos = segs[i].off + segs[i].bytes;
    }
    for (const Seg& g : segs)
      if (g.dst && g.bytes) std::memcpy(g.dst, img.data() + g.off, g.bytes);
  }
};

HotwordDFA search_dfa(const std::string& w, const zasr_st_hotwords& hw, int V) {
  ZASR_REQUIRE(hw.n >= 0, w + "negative phrase count");
  std::vector<std::vector<int>> phrases;
  std::vector<float> scores;
  const int* tp = hw.tokens;
  for (int p = 0; p < hw.n; ++p) {
    ZASR_REQUIRE(hw.tokens && hw.lens && hw.scores, w + "phrases need tokens, lens and scores");
    ZASR_REQUIRE(hw.lens[p] >= 1, w + "an empty hotword phrase");
    phrases.emplace_back(tp, tp + hw.lens[p]);
    for (int tk : phrases.back()) ZASR_REQUIRE(tk >= 0 && tk < V, w + "hotword token id out of range");
    tp += hw.lens[p];
    scores.push_back(hw.scores[p]);
  }
  return build_hotword_dfa(phrases, scores, V);
}

struct SearchHw {
  HotwordDFA dfa;
  size_t i_cls = 0, i_next = 0, i_delta = 0, i_score = 0;
  void add(SearchArena& ar) {
    if (dfa.num_states == 0) return;
    i_cls = ar.in(dfa.tok2cls.data(), dfa.tok2cls.size());
    i_next = ar.in(dfa.next.data(), dfa.next.size());
    i_delta = ar.in(dfa.delta.data(), dfa.delta.size());
    i_score = ar.in(dfa.node_score.data(), dfa.node_score.size());
  }
  HotwordTables tables(const SearchArena& ar) const {
    HotwordTables t{};
    if (dfa.num_states == 0) return t;
    t.num_states = dfa.num_states;
    t.num_cls = dfa.num_cls;
    t.tok2cls = ar.at<int>(i_cls);
    t.next = ar.at<int>(i_next);
    t.delta = ar.at<double>(i_delta);
    t.node_score = ar.at<double>(i_score);
    return t;
  }
};

// the state arrays checked against what the kernels index with them, then laid into the arena
struct SearchSt {
  size_t i[15];
  static void check(const std::string& w, const zasr_st_state& st, int V, int max_nh, int room,
                    int num_states, bool parents) {
    ZASR_REQUIRE(st.S >= 1 && st.S <= 4096, w + "1 <= S <= 4096");
    ZASR_REQUIRE(st.Hmax >= 1 && st.Hmax <= 16, w + "1 <= Hmax <= 16");
    ZASR_REQUIRE(st.node_cap >= 1 && st.node_cap <= (1 << 24), w + "node_cap out of range");
    ZASR_REQUIRE(st.lp && st.lpf && st.hash && st.len && st.y1 && st.y2 && st.hw && st.node &&
                     st.nh && st.node_tok && st.node_frame && st.node_parent && st.node_lp &&
                     st.node_stats && st.node_count,
                 w + "null state array");
    for (int s = 0; s < st.S; ++s) {
      const int nc = st.node_count[s];
      ZASR_REQUIRE(nc >= 0 && (long)nc + room <= st.node_cap,
                   w + "node_cap too small for node_count and the nodes one call can add");
      ZASR_REQUIRE(st.nh[s] >= 0 && st.nh[s] <= max_nh, w + "nh out of range");
      for (int h = 0; h < st.Hmax; ++h) {
        const int o = s * st.Hmax + h;
        const bool live = h < st.nh[s] || h == 0;  // the final pick reads slot 0 of an empty stream
        if (!live) continue;
        ZASR_REQUIRE(st.y1[o] >= 0 && st.y1[o] < V && st.y2[o] >= 0 && st.y2[o] < V,
                     w + "context token out of range");
        ZASR_REQUIRE(st.hw[o] >= 0 && st.hw[o] < (num_states > 0 ? num_states : 1),
                     w + "hotword state out of range");
        ZASR_REQUIRE(st.node[o] >= -1 && st.node[o] < nc, w + "node out of range");
        ZASR_REQUIRE(st.len[o] >= 0 && st.len[o] < (1 << 30), w + "len out of range");
      }
      if (parents)
        for (int n = 0; n < nc; ++n) {
          const int pr = st.node_parent[(size_t)s * st.node_cap + n];
          ZASR_REQUIRE(pr >= -1 && pr < n, w + "node_parent must lie in [-1, own index)");
        }
    }
  }
  void add(SearchArena& ar, const zasr_st_state& st) {
    const size_t sl = (size_t)st.S * st.Hmax, nn = (size_t)st.S * st.node_cap;
    i[0] = ar.io(st.lp, sl);
    i[1] = ar.io(st.lpf, sl);
    i[2] = ar.io(st.hash, sl);
    i[3] = ar.io(st.len, sl);
    i[4] = ar.io(st.y1, sl);
    i[5] = ar.io(st.y2, sl);
    i[6] = ar.io(st.hw, sl);
    i[7] = ar.io(st.node, sl);
    i[8] = ar.io(st.nh, (size_t)st.S);
    i[9] = ar.io(st.node_tok, nn);
    i[10] = ar.io(st.node_frame, nn);
    i[11] = ar.io(st.node_parent, nn);
    i[12] = ar.io(st.node_lp, nn);
    i[13] = ar.io(st.node_stats, nn * 4);
    i[14] = ar.io(st.node_count, (size_t)st.S);
  }
  SearchState dev(const SearchArena& ar, int node_cap) const {
    SearchState d{};
    d.lp = ar.at<double>(i[0]);
    d.lpf = ar.at<int>(i[1]);
    d.hash = ar.at<unsigned long long>(i[2]);
    d.len = ar.at<int>(i[3]);
    d.y1 = ar.at<int>(i[4]);
    d.y2 = ar.at<int>(i[5]);
    d.hw = ar.at<int>(i[6]);
    d.node = ar.at<int>(i[7]);
    d.nh = ar.at<int>(i[8]);
    d.node_tok = ar.at<int>(i[9]);
    d.node_frame = ar.at<int>(i[10]);
    d.node_parent = ar.at<int>(i[11]);
    d.node_lp = ar.at<double>(i[12]);
    d.node_stats = ar.at<float4>(i[13]);
    d.node_count = ar.at<int>(i[14]);
    d.node_cap = node_cap;
    return d;
  }
};

// the full decoder-context table of the last (V, D, a, b), kept on the device between calls (a
// chain passes the same table every frame)
struct SearchTableCache {
  int V = 0, D = 0;
  std::vector<float> a, b;
  std::unique_ptr<DevBuf> d;
  const float* get(int V_, int D_, const float* a_, const float* b_) {
    const size_t n = (size_t)V_ * D_;
    if (d && V == V_ && D == D_ && std::memcmp(a.data(), a_, n * 4) == 0 &&
        std::memcmp(b.data(), b_, n * 4) == 0)
      return d->as<float>();
    d.reset();
    std::vector<float> tab((size_t)V_ * n);
    for (int y2 = 0; y2 < V_; ++y2)
      for (int y1 = 0; y1 < V_; ++y1) {
        float* row = tab.data() + ((size_t)y2 * V_ + y1) * D_;
        for (int k = 0; k < D_; ++k) row[k] = a_[(size_t)y2 * D_ + k] + b_[(size_t)y1 * D_ + k];
      }
    d.reset(new DevBuf(tab.size() * 4));
    up(*d, tab.data(), tab.size() * 4);
    V = V_;
    D = D_;
    a.assign(a_, a_ + n);
    b.assign(b_, b_ + n);
    return d->as<float>();
  }
};
SearchTableCache& search_table_cache() {
  static SearchTableCache* c = new SearchTableCache;  // outlives the HIP runtime's teardown
  return *c;
}

struct SearchTab {
  size_t i_enc = 0, i_off = 0, i_J = 0;
  long jrows = 0;
  static void check(const std::string& w, const zasr_st_table& tb, int V, int S, const int* enc_len,
                    long rows) {
    ZASR_REQUIRE(tb.D >= 4 && tb.D % 4 == 0 && tb.D <= 512, w + "joiner dim must be a multiple of 4, <= 512");
    ZASR_REQUIRE(tb.jfmt >= 0 && tb.jfmt <= 5, w + "J format 0 .. 5");
    ZASR_REQUIRE(tb.jfmt < 2 || tb.D == 256 || tb.D == 512, w + "fragment-order J: joiner dim 256 or 512");
    ZASR_REQUIRE((size_t)V * V * tb.D <= ((size_t)1 << 27), w + "decoder table beyond 2^27 floats");
    ZASR_REQUIRE(tb.a && tb.b && tb.enc && tb.enc_off && tb.J, w + "null table argument");
    ZASR_REQUIRE(tb.enc_rows >= 1, w + "enc_rows >= 1");
    for (int s = 0; s < S; ++s)
      ZASR_REQUIRE(tb.enc_off[s] >= 0 && (long)tb.enc_off[s] + enc_len[s] <= tb.enc_rows,
                   w + "enc_off + enc_len beyond enc_rows");
    ZASR_REQUIRE(tb.j_bytes == (long)bytes(tb, rows), w + "j_bytes is not the J format's size");
  }
  static int images(int jfmt) { return jfmt == 4 ? 3 : jfmt == 3 || jfmt == 5 ? 2 : 1; }
  static size_t bytes(const zasr_st_table& tb, long rows) {
    if (tb.jfmt == 0) return (size_t)rows * tb.D * 4;
    if (tb.jfmt == 1) return (size_t)rows * tb.D * 2;
    return (size_t)joiner_packed_rows(rows) * tb.D * 2 * images(tb.jfmt);
  }
  void add(SearchArena& ar, const zasr_st_table& tb, int S, long rows) {
    jrows = joiner_packed_rows(rows);
    i_enc = ar.in(tb.enc, (size_t)tb.enc_rows * tb.D);
    i_off = ar.in(tb.enc_off, (size_t)S);
    i_J = ar.add(tb.J, bytes(tb, rows), tb.J);
  }
  DecTable dev(const SearchArena& ar, const zasr_st_table& tb, int V, const int* d_enc_len) const {
    DecTable dt{search_table_cache().get(V, tb.D, tb.a, tb.b), V, ar.at<float>(i_enc),
                ar.at<int>(i_off), d_enc_len, ar.at<void>(i_J), tb.D,
                tb.jfmt == 1 || tb.jfmt == 2 ? 1 : 0};
    dt.j_packed = tb.jfmt >= 2 ? 1 : 0;
    dt.j_pieces = tb.jfmt == 3 ? 2 : tb.jfmt == 4 ? 3 : tb.jfmt == 5 ? kPiecesF16 : 0;
    dt.j_plane = jrows * tb.D;
    return dt;
  }
};

void check_search_common(const std::string& w, int V, int S, const int* enc_len) {
  ZASR_REQUIRE(V >= 4 && V % 4 == 0 && V <= 4096, w + "vocabulary size must be a multiple of 4, <= 4096");
  for (int s = 0; s < S; ++s)
    ZASR_REQUIRE(enc_len[s] >= 0 && enc_len[s] <= (1 << 24), w + "enc_len out of range");
}
}  // namespace

void selftest_hotword_dfa(int V, const zasr_st_hotwords& hw, int cap, int* num_states,
                          int* num_cls, int* tok2cls, int* next, double* delta, double* node_score) {
  const std::string w = "selftest hotword_dfa: ";
  ZASR_REQUIRE(V >= 1, w + "V >= 1");
  const HotwordDFA dfa = search_dfa(w, hw, V);
  *num_states = dfa.num_states;
  *num_cls = dfa.num_cls;
  for (int v = 0; v < V; ++v) tok2cls[v] = dfa.num_states ? dfa.tok2cls[v] : -1;
  ZASR_REQUIRE((long)dfa.num_states * dfa.num_cls <= cap && dfa.num_states <= cap,
               w + "cap too small for the automaton");
  std::copy(dfa.next.begin(), dfa.next.end(), next);
  std::copy(dfa.delta.begin(), dfa.delta.end(), delta);
  std::copy(dfa.node_score.begin(), dfa.node_score.end(), node_score);
}

void selftest_search_step(int V, int beam, int t, const int* enc_len, const zasr_st_state& st,
                          const float* logits, const zasr_st_hotwords& hw, const zasr_st_table* tab) {
  const std::string w = "selftest search_step: ";
  ZASR_REQUIRE(st.S >= 1 && st.S <= 4096, w + "1 <= S <= 4096");
  check_search_common(w, V, st.S, enc_len);
  ZASR_REQUIRE(beam >= 1 && beam <= 16 && beam <= st.Hmax, w + "beam out of range");
  SearchHw h;
  h.dfa = search_dfa(w, hw, V);
  const bool init = t < 0;
  if (init) {
    ZASR_REQUIRE(st.Hmax >= 1 && st.Hmax <= 16 && st.node_cap >= beam, w + "Hmax / node_cap out of range");
    ZASR_REQUIRE(st.lp && st.lpf && st.hash && st.len && st.y1 && st.y2 && st.hw && st.node &&
                     st.nh && st.node_tok && st.node_frame && st.node_parent && st.node_lp &&
                     st.node_stats && st.node_count,
                 w + "null state array");
  } else {
    SearchSt::check(w, st, V, beam, beam, h.dfa.num_states, false);
    ZASR_REQUIRE(logits != nullptr, w + "null logits");
  }
  const long rows = (long)st.S * st.Hmax;
  if (tab) SearchTab::check(w, *tab, V, st.S, enc_len, rows);
  SearchArena ar;
  SearchSt ss;
  SearchTab tb;
  ss.add(ar, st);
  h.add(ar);
  const size_t i_len = ar.in(enc_len, (size_t)st.S);
  const size_t i_lg = init ? 0 : ar.in(logits, (size_t)rows * V);
  if (tab) tb.add(ar, *tab, st.S, rows);
  ar.upload();
  const SearchState ds = ss.dev(ar, st.node_cap);
  DecTable dt{};
  if (tab) dt = tb.dev(ar, *tab, V, ar.at<int>(i_len));
  if (init) {
    launch_search_init(ds, st.S, st.Hmax, nullptr);
    if (tab) launch_table_init(dt, st.S, st.Hmax, nullptr);
  } else {
    launch_search_step(ds, ar.at<float>(i_lg), V, st.S, st.Hmax, beam, t, ar.at<int>(i_len),
                       h.tables(ar), tab ? &dt : nullptr, nullptr);
  }
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ar.download("search_step");
}

void selftest_greedy_spec(int V, int F, int init, int parity, const int* enc_len, int* t_cur,
                          int* active, const zasr_st_state& st, const float* logits,
                          const zasr_st_hotwords& hw, const zasr_st_table& tab) {
  const std::string w = "selftest greedy_spec: ";
  ZASR_REQUIRE(st.S >= 1 && st.S <= 4096, w + "1 <= S <= 4096");
  check_search_common(w, V, st.S, enc_len);
  ZASR_REQUIRE(F == 4 || F == 8, w + "window must be 4 or 8 frames");
  ZASR_REQUIRE(init >= 0 && init <= 2 && (parity == 0 || parity == 1), w + "init 0 .. 2, parity 0 / 1");
  ZASR_REQUIRE(st.Hmax == 1, w + "beam 1: Hmax = 1");
  SearchHw h;
  h.dfa = search_dfa(w, hw, V);
  if (init == 0) {
    SearchSt::check(w, st, V, 1, 1, h.dfa.num_states, false);
    for (int s = 0; s < st.S; ++s) {
      ZASR_REQUIRE(t_cur[s] >= 0 && t_cur[s] <= (1 << 24), w + "t_cur out of range");
      ZASR_REQUIRE(st.nh[s] == 1, w + "nh = 1");
    }
  } else {
    ZASR_REQUIRE(st.node_cap >= 1 && st.node_cap <= (1 << 24), w + "node_cap out of range");
    ZASR_REQUIRE(st.lp && st.lpf && st.hash && st.len && st.y1 && st.y2 && st.hw && st.node &&
                     st.nh && st.node_tok && st.node_frame && st.node_parent && st.node_lp &&
                     st.node_stats && st.node_count,
                 w + "null state array");
  }
  ZASR_REQUIRE(init == 2 || logits != nullptr, w + "null logits");
  const long rows = (long)st.S * F;
  SearchTab::check(w, tab, V, st.S, enc_len, rows);
  SearchArena ar;
  SearchSt ss;
  SearchTab tb;
  ss.add(ar, st);
  h.add(ar);
  const size_t i_len = ar.in(enc_len, (size_t)st.S);
  const size_t i_t = ar.io(t_cur, (size_t)st.S);
  const size_t i_act = ar.io(active, 2);
  const size_t i_lg = init == 2 ? 0 : ar.in(logits, (size_t)rows * V);
  tb.add(ar, tab, st.S, rows);
  ar.upload();
  const SearchState ds = ss.dev(ar, st.node_cap);
  const DecTable dt = tb.dev(ar, tab, V, ar.at<int>(i_len));
  if (init != 0) {
    launch_search_init(ds, st.S, 1, nullptr);
    launch_greedy_spec_init(dt, st.S, F, ar.at<int>(i_t), ar.at<int>(i_act), nullptr);
  }
  if (init != 2)
    launch_greedy_spec(ds, ar.at<float>(i_lg), V, st.S, F, ar.at<int>(i_t), ar.at<int>(i_len),
                       h.tables(ar), dt, ar.at<int>(i_act), parity, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ar.download("greedy_spec");
}

void selftest_search_final(int V, const zasr_st_state& st, const zasr_st_hotwords& hw, int out_cap,
                           int* out_tok, int* out_frame, double* out_lp, float* out_stats,
                           int* out_count) {
  const std::string w = "selftest search_final: ";
  ZASR_REQUIRE(V >= 1 && V <= 4096, w + "V out of range");
  ZASR_REQUIRE(out_cap >= 1 && out_cap <= (1 << 24), w + "out_cap out of range");
  SearchHw h;
  h.dfa = search_dfa(w, hw, V);
  SearchSt::check(w, st, V, st.Hmax, 0, h.dfa.num_states, true);
  SearchArena ar;
  SearchSt ss;
  ss.add(ar, st);
  h.add(ar);
  const size_t n = (size_t)st.S * out_cap;
  const size_t i_tok = ar.io(out_tok, n), i_fr = ar.io(out_frame, n), i_lp = ar.io(out_lp, n),
               i_st = ar.io(out_stats, n * 4), i_cnt = ar.io(out_count, (size_t)st.S);
  ar.upload();
  launch_search_final(ss.dev(ar, st.node_cap), st.S, st.Hmax, h.tables(ar), out_cap,
                      ar.at<int>(i_tok), ar.at<int>(i_fr), ar.at<double>(i_lp),
                      ar.at<float4>(i_st), ar.at<int>(i_cnt), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  ar.download("search_final");
}

// ---- the GEMMs' implicit-im2col loaders and ragged z-slices ----
namespace {
// an output image of n elements (f32, or bf16 as OutBuf) that starts as the caller's, with
// `guard` elements of 0x5a before it and behind it (guard * element size a multiple of 16)
struct FramedOut {
  size_t n, guard, eb;
  DevBuf d;
  FramedOut(const float* init, size_t n_, size_t guard_, bool h16)
      : n(n_), guard(guard_), eb(h16 ? 2 : 4), d((n_ + 2 * guard_) * (h16 ? 2 : 4)) {
    ZASR_HIP_CHECK(hipMemset(d.p, 0x5a, (n + 2 * guard) * eb));
    if (n == 0) return;
    if (h16) ZASR_HIP_CHECK(hipMemcpy(image(), round16(init, n).data(), n * 2, hipMemcpyHostToDevice));
    else ZASR_HIP_CHECK(hipMemcpy(image(), init, n * 4, hipMemcpyHostToDevice));
  }
  unsigned char* image() const { return d.as<unsigned char>() + guard * eb; }
  void down(float* out, const char* what) const {
    std::vector<unsigned char> all((n + 2 * guard) * eb);
    ZASR_HIP_CHECK(hipMemcpy(all.data(), d.p, all.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < guard * eb; ++i) {
      ZASR_REQUIRE(all[i] == 0x5a, std::string("selftest ") + what + ": the kernel wrote before the first row");
      ZASR_REQUIRE(all[(guard + n) * eb + i] == 0x5a,
                   std::string("selftest ") + what + ": the kernel wrote past the last row");
    }
    if (n == 0) return;
    if (eb == 2) {
      const __bf16* h = reinterpret_cast<const __bf16*>(all.data() + guard * eb);
      for (size_t i = 0; i < n; ++i) out[i] = (float)h[i];
    } else {
      std::memcpy(out, all.data() + guard * eb, n * 4);
    }
  }
};
}  // namespace

void selftest_conv_gemm(int mode, int which, bool a_bf16, bool c_bf16, int nseq, const int* T,
                        const float* A, const float* W, const float* bias, float* C) {
  const bool f32 = mode == ZASR_PRECISION_FP32, h16 = mode == ZASR_PRECISION_BF16;
  const int pieces = mode == ZASR_PRECISION_BF16X3   ? 2
                     : mode == ZASR_PRECISION_BF16X6 ? 3
                     : mode == ZASR_PRECISION_F16X3  ? kPiecesF16
                                                     : 0;
  ZASR_REQUIRE(f32 || h16 || pieces != 0,
               "selftest conv_gemm: mode must be ZASR_PRECISION_FP32, _BF16, _BF16X3, _BF16X6 or _F16X3");
  ZASR_REQUIRE(which == 4 || which == 7, "selftest conv_gemm: which must be 4 (conv.4) or 7 (conv.7)");
  ZASR_REQUIRE(h16 || (!a_bf16 && !c_bf16), "selftest conv_gemm: bf16 A / C in the bf16 mode only");
  ZASR_REQUIRE(!a_bf16 || c_bf16, "selftest conv_gemm: bf16 A takes bf16 C");
  ZASR_REQUIRE(a_bf16 == c_bf16 || which == 7, "selftest conv_gemm: f32 A with bf16 C is conv.7's only");
  ZASR_REQUIRE(nseq >= 1 && nseq <= 65535, "selftest conv_gemm: 1 .. 65535 sequences");
  for (int b = 0; b < nseq; ++b)
    ZASR_REQUIRE(T[b] >= 9 && T[b] <= (1 << 20), "selftest conv_gemm: every T in [9, 2^20]");
  const FrontendConvSlices fcs = frontend_conv_slices(T, nseq);
  const bool c4 = which == 4;
  const int N = c4 ? 32 : 128, K = c4 ? 72 : 288;
  const size_t na = c4 ? (size_t)fcs.rows_c1 * 640 : (size_t)fcs.rows_c2 * 39 * 32;
  const size_t nc = c4 ? (size_t)fcs.rows_c2 * 39 * 32 : (size_t)fcs.rows_L * 19 * 128;
  ZASR_REQUIRE(na < ((size_t)1 << 31) && nc < ((size_t)1 << 31), "selftest conv_gemm: batch too large");
  const size_t nw = (size_t)N * K;
  DevBuf dA(na * (a_bf16 ? 2 : 4)), dW(nw * 4), dWx(nw * 2 * (pieces ? stored_pieces(pieces) : 1)),
      dB((size_t)N * 4), dS((size_t)nseq * sizeof(GemmSlice));
  up16(dA, A, na, a_bf16);
  up(dW, W, nw * 4);
  up(dB, bias, (size_t)N * 4);
  // the weight's images as the loader prepares them (engine_load.cpp)
  DLin l;
  l.w = dW.as<float>();
  l.b = dB.as<float>();
  l.N = N;
  l.K = K;
  if (h16) {
    convert_to_bf16(dW.as<float>(), dWx.p, (long)nw, nullptr);
    l.wh = dWx.p;
  }
  if (pieces) {
    split_to_bf16(dW.as<float>(), dWx.p, (long)nw, pieces, nullptr);
    l.wx = dWx.p;
  }
  const std::vector<GemmSlice>& sl = c4 ? fcs.c2 : fcs.c3;
  up(dS, sl.data(), (size_t)nseq * sizeof(GemmSlice));
  FramedOut o(C, nc, (size_t)(c4 ? 39 * 32 : 19 * 128), c_bf16);  // one frame either side
  GemmParams p{};
  p.A = dA.as<float>();
  p.C = reinterpret_cast<float*>(o.image());
  p.slices = dS.as<GemmSlice>();
  p.num_slices = nseq;
  p.max_M = c4 ? fcs.max_M2 : fcs.max_M3;
  launch_frontend_conv_gemm(p, l, c4 ? ALOAD_CONV2 : ALOAD_CONV3, a_bf16, c_bf16, pieces, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(C, "conv_gemm");
}

void selftest_gemm_aload(int aload, int M, int K, int N, int lda, int ldc, int c_col, int epi,
                         const float* A, const float* W, const float* bias, const float* a_scale,
                         const float* a_shift, int Tin, int Tout, int Cin, int stride, int dil,
                         int pad, const float* aux, int ldaux, float* C) {
  const GemmIm2col1d g{Tin, Tout, Cin, stride, dil, pad};
  const bool bn = aload == ALOAD_BNRELU;
  ZASR_REQUIRE(bn || aload == ALOAD_IM2COL1D,
               "selftest gemm_aload: aload must be ALOAD_BNRELU (4) or ALOAD_IM2COL1D (5)");
  ZASR_REQUIRE(M >= 1 && K >= 1 && N >= 1 && M <= (1 << 20) && K <= (1 << 16) && N <= (1 << 16),
               "selftest gemm_aload: M, K, N out of range");
  ZASR_REQUIRE(c_col >= 0 && ldc >= c_col + N && ldc <= (1 << 16),
               "selftest gemm_aload: columns [c_col, c_col + N) must lie inside ldc");
  ZASR_REQUIRE(!bn || (a_scale && a_shift), "selftest gemm_aload: ALOAD_BNRELU needs a_scale / a_shift");
  ZASR_REQUIRE(epi != EPI_MULAUX || (aux != nullptr && ldaux >= N && ldaux <= (1 << 16)),
               "selftest gemm_aload: EPI_MULAUX needs aux with ldaux >= N");
  long a_rows = M;
  if (bn) {
    ZASR_REQUIRE(lda >= K && lda <= (1 << 16), "selftest gemm_aload: lda >= K");
  } else {
    ZASR_REQUIRE(g.Tin >= 1 && g.Tout >= 1 && g.C >= 1 && g.stride >= 1 && g.dil >= 1 && g.pad >= 0 &&
                     g.Tin <= (1 << 20) && g.stride <= 64 && g.dil <= 64 && g.pad <= 4096,
                 "selftest gemm_aload: im2col fields out of range");
    ZASR_REQUIRE(lda >= g.C && lda <= (1 << 16), "selftest gemm_aload: lda >= C");
    a_rows = (long)cdiv(M, g.Tout) * g.Tin;
  }
  const size_t na = (size_t)a_rows * lda, nw = (size_t)N * K, nc = (size_t)M * ldc;
  ZASR_REQUIRE(na < ((size_t)1 << 31) && nc < ((size_t)1 << 31), "selftest gemm_aload: problem too large");
  const size_t nx = epi == EPI_MULAUX ? (size_t)M * ldaux : 0;
  DevBuf dA(na * 4), dW(nw * 4), dB((size_t)N * 4), dSc((size_t)K * 4), dSh((size_t)K * 4), dX(nx * 4);
  up(dA, A, na * 4);
  up(dW, W, nw * 4);
  if (bias) up(dB, bias, (size_t)N * 4);
  if (bn) {
    up(dSc, a_scale, (size_t)K * 4);
    up(dSh, a_shift, (size_t)K * 4);
  }
  if (nx) up(dX, aux, nx * 4);
  FramedOut o(C, nc, (size_t)((ldc + 3) & ~3), false);
  GemmParams p = dense_gemm_params(dW.as<float>(), bias ? dB.as<float>() : nullptr, N, K, dA.p, lda, M,
                                   reinterpret_cast<float*>(o.image()) + c_col, ldc);
  if (nx) {
    p.aux = dX.as<float>();
    p.ldaux = ldaux;
  }
  if (bn) {
    p.a_scale = dSc.as<float>();
    p.a_shift = dSh.as<float>();
  } else {
    p.i2c = g;
  }
  gemm_f32(p, epi, aload, false, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(C, "gemm_aload");
}

// ---- the CAM++, Silero VAD and ViBERT kernels ----
namespace {
constexpr size_t kAuxMax = (size_t)1 << 27;  // elements of any one array of these entries

// an input of n elements of T on the device (n = 0 or a null host pointer: a 4-byte allocation)
template <class T>
struct DevIn {
  DevBuf d;
  DevIn(const T* h, size_t n) : d(n * sizeof(T)) {
    if (h) up(d, h, n * sizeof(T));
  }
  const T* p() const { return d.as<T>(); }
};
}  // namespace

void selftest_campp_conv2d(int ks, int ci, int fi, int sf, int T, int n, int relu, int tdnn_out,
                           int in_tf, int use_mfma, int rb, const float* x, const float* w,
                           const float* scale, const float* shift, const float* res, float* y,
                           int* route, int* rb_used) {
  const std::string m = "selftest campp_conv2d: ";
  ZASR_REQUIRE(ks == 1 || ks == 3, m + "kernel 1 or 3");
  ZASR_REQUIRE(ci >= 1 && ci <= 1024, m + "Ci out of range");  // the launch refuses Ci > 32
  ZASR_REQUIRE(fi >= 1 && fi <= 1024 && T >= 1 && T <= 4096 && n >= 1 && n <= 65535 && sf >= 1 && sf <= 8,
               m + "sizes out of range");
  ZASR_REQUIRE(!in_tf || ci == 1, m + "the [n][T][fi] input form is the Ci = 1 convolution's");
  ZASR_REQUIRE(rb >= 0 && rb % 2 == 0, m + "rb 0 (the engine's pick) or even");
  ZASR_REQUIRE(!use_mfma || ci == 32, m + "the permuted weights are the Ci = 32 convolutions'");
  const int fo = (fi - 1) / sf + 1;
  const size_t nx = (size_t)n * ci * fi * T, nw = (size_t)32 * ci * ks * ks, ny = (size_t)n * 32 * fo * T;
  ZASR_REQUIRE(nx <= kAuxMax && ny <= kAuxMax, m + "problem too large");
  std::vector<float> pk(use_mfma ? nw : 0);
  if (use_mfma) campp_conv2d_permute_weights(w, ks, pk.data());
  DevIn<float> dX(x, nx), dW(w, nw), dK(pk.data(), pk.size()), dSc(scale, 32), dSh(shift, 32),
      dR(res, res ? ny : 0);
  GuardedOut o(y, ny * 4);
  CamppConv2d a{};
  a.x = dX.p();
  a.w = dW.p();
  a.scale = dSc.p();
  a.shift = dSh.p();
  a.res = res ? dR.p() : nullptr;
  a.y = o.d.as<float>();
  a.n = n;
  a.ci = ci;
  a.fi = fi;
  a.fo = fo;
  a.T = T;
  a.sf = sf;
  a.relu = relu;
  a.tdnn_out = tdnn_out;
  a.in_tf = in_tf;
  a.wk = use_mfma ? dK.p() : nullptr;
  const int used = launch_campp_conv2d(a, ks, rb ? rb : campp_conv2d_rows_per_block(fo, n), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(y, "campp_conv2d");
  *route = used ? 1 : 0;
  *rb_used = used;
}

void selftest_campp_cam_mask(int n, int T, int seg_len, const float* h, const float* w1,
                             const float* b1, const float* w2, const float* b2, float* mexp) {
  ZASR_REQUIRE(n >= 1 && n <= 65535 && T >= 1 && seg_len >= 1 && (size_t)n * T * 128 <= kAuxMax,
               "selftest campp_cam_mask: sizes out of range");
  DevIn<float> dH(h, (size_t)n * T * 128), d1(w1, 64 * 128), dB1(b1, 64), d2(w2, 32 * 64), dB2(b2, 32);
  GuardedOut o(mexp, (size_t)n * T * 32 * 4);
  CamppCamMask a{dH.p(), d1.p(), dB1.p(), d2.p(), dB2.p(), o.d.as<float>(), n, T, seg_len};
  launch_campp_cam_mask(a, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(mexp, "campp_cam_mask");
}

void selftest_campp_stats(int N, int T, int C, const float* x, const float* s, const float* b,
                          float* out) {
  ZASR_REQUIRE(N >= 1 && T >= 1 && C >= 1 && (size_t)N * T * C <= kAuxMax,
               "selftest campp_stats: sizes out of range");
  DevIn<float> dX(x, (size_t)N * T * C), dS(s, C), dB(b, C);
  GuardedOut o(out, (size_t)N * 2 * C * 4);
  launch_campp_stats(dX.p(), N, T, C, dS.p(), dB.p(), o.d.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(out, "campp_stats");
}

void selftest_campp_cmvn(int nseq, int rows, const int* fr_off, float* x) {
  const std::string m = "selftest campp_cmvn: ";
  ZASR_REQUIRE(nseq >= 1 && nseq <= 65535 && rows >= 0 && (size_t)rows * 80 <= kAuxMax, m + "sizes out of range");
  ZASR_REQUIRE(fr_off[0] >= 0 && fr_off[nseq] <= rows, m + "the sequences must lie inside the rows");
  for (int s = 0; s < nseq; ++s) ZASR_REQUIRE(fr_off[s] <= fr_off[s + 1], m + "offsets must not decrease");
  DevIn<int> dO(fr_off, (size_t)nseq + 1);
  GuardedOut o(x, (size_t)rows * 80 * 4);
  launch_campp_cmvn(o.d.as<float>(), dO.p(), nseq, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(x, "campp_cmvn");
}

void selftest_campp_gather(int nwin, int wf, int nrows, const float* rows, const int* win_row,
                           const int* win_n, float* out) {
  const std::string m = "selftest campp_gather: ";
  ZASR_REQUIRE(nwin >= 1 && wf >= 1 && nrows >= 1 && (size_t)nwin * wf * 80 <= kAuxMax &&
                   (size_t)nrows * 80 <= kAuxMax, m + "sizes out of range");
  for (int w = 0; w < nwin; ++w)
    ZASR_REQUIRE(win_row[w] >= 0 && win_n[w] >= 0 && win_n[w] <= wf && (long)win_row[w] + win_n[w] <= nrows,
                 m + "every window's rows must lie inside the packed rows, at most wf of them");
  DevIn<float> dR(rows, (size_t)nrows * 80);
  DevIn<int> dW(win_row, nwin), dN(win_n, nwin);
  GuardedOut o(out, (size_t)nwin * wf * 80 * 4);
  launch_campp_gather(dR.p(), dW.p(), dN.p(), nwin, wf, o.d.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(out, "campp_gather");
}

void selftest_vad_frames(int n_files, long n_windows, long n_samples, const float* audio,
                         const long* off, const long* win_start, const long* len,
                         const float* rows576, unsigned* maxabs, float* frames) {
  const std::string m = "selftest vad_frames: ";
  ZASR_REQUIRE(n_windows >= 1 && (size_t)n_windows * 1024 <= kAuxMax, m + "window count out of range");
  GuardedOut o(frames, (size_t)n_windows * 1024 * 4);
  VadFramesArgs a{};
  a.frames = o.d.as<float>();
  if (rows576) {
    DevIn<float> dR(rows576, (size_t)n_windows * 576);
    a.rows576 = dR.p();
    launch_vad_frames(a, n_windows, nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    o.down(frames, "vad_frames");
    return;
  }
  ZASR_REQUIRE(audio && off && win_start, m + "the file mode takes audio, off and win_start");
  ZASR_REQUIRE(n_files >= 1 && n_files <= 65535 && n_samples >= 1 && (size_t)n_samples <= kAuxMax,
               m + "sizes out of range");
  ZASR_REQUIRE((len == nullptr) == (maxabs == nullptr), m + "len and maxabs go together");
  ZASR_REQUIRE(win_start[0] == 0, m + "the first file starts at window 0");
  for (int f = 0; f < n_files; ++f) {
    const long next = f + 1 < n_files ? win_start[f + 1] : n_windows;
    ZASR_REQUIRE(next >= win_start[f] && next <= n_windows, m + "win_start must not decrease");
    ZASR_REQUIRE(off[f] >= 0 && off[f] + (next - win_start[f]) * 512 <= n_samples,
                 m + "every file's windows must lie inside the audio");
    ZASR_REQUIRE(!len || (len[f] >= 0 && off[f] + len[f] <= n_samples), m + "every file must lie inside the audio");
  }
  DevIn<float> dA(audio, (size_t)n_samples);
  DevIn<long> dO(off, n_files), dS(win_start, n_files), dL(len, len ? n_files : 0);
  GuardedOut mx(std::vector<unsigned>(n_files, 0u).data(), (size_t)n_files * 4);
  a.audio = dA.p();
  a.off = dO.p();
  a.win_start = dS.p();
  a.n_files = n_files;
  if (len) {
    launch_vad_maxabs(dA.p(), dO.p(), dL.p(), n_files, mx.d.as<unsigned>(), nullptr);
    a.maxabs = mx.d.as<unsigned>();
  }
  launch_vad_frames(a, n_windows, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(frames, "vad_frames");
  if (len) mx.down(maxabs, "vad_frames (maxabs)");
}

void selftest_vad_im2col(int which, long N, int T, int C, int stride, int ldS, int Kp,
                         const float* in, float* A) {
  const std::string m = "selftest vad_im2col: ";
  ZASR_REQUIRE(which == 0 || which == 1, m + "which 0 (mag_im2col) or 1 (im2col)");
  ZASR_REQUIRE(N >= 1 && N <= (1 << 20) && C >= 1 && C <= 4096, m + "sizes out of range");
  if (which == 0) {  // N windows of 4 STFT rows (re | im), C bins
    ZASR_REQUIRE(ldS >= 2 * C && ldS <= 16384 && Kp >= 1 && Kp <= 16384, m + "ldS >= 2 bins, Kp >= 1");
    ZASR_REQUIRE((size_t)N * 4 * ldS <= kAuxMax && (size_t)N * 4 * Kp <= kAuxMax, m + "problem too large");
    DevIn<float> dS(in, (size_t)N * 4 * ldS);
    GuardedOut o(A, (size_t)N * 4 * Kp * 4);
    launch_vad_mag_im2col(dS.p(), ldS, C, Kp, N, o.d.as<float>(), nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    o.down(A, "vad_im2col");
    return;
  }
  ZASR_REQUIRE(T >= 1 && T <= 4096 && stride >= 1 && stride <= 64, m + "T / stride out of range");
  const int Tout = (T - 1) / stride + 1;
  ZASR_REQUIRE((size_t)N * T * C <= kAuxMax && (size_t)N * Tout * 3 * C <= kAuxMax, m + "problem too large");
  DevIn<float> dY(in, (size_t)N * T * C);
  GuardedOut o(A, (size_t)N * Tout * 3 * C * 4);
  launch_vad_im2col(dY.p(), N, T, C, stride, Tout, o.d.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(A, "vad_im2col");
}

void selftest_vad_lstm(long windows, int nseg, const float* gx, const float* whh, const float* bhh,
                       const float* wd, float bd, const long* seg_start, const int* seg_count,
                       const int* seg_warm, const float* init, float* probs, float* s_out,
                       float* e_out) {
  const std::string m = "selftest vad_lstm: ";
  ZASR_REQUIRE(windows >= 1 && windows <= (1 << 16) && nseg >= 1 && nseg <= 4096, m + "sizes out of range");
  for (int s = 0; s < nseg; ++s) {
    const int warm = seg_warm ? seg_warm[s] : 0;
    ZASR_REQUIRE(warm >= 0 && seg_count[s] >= 0 && seg_start[s] - warm >= 0 &&
                     seg_start[s] + seg_count[s] <= windows,
                 m + "every segment, its warm-up included, must lie inside the windows");
  }
  const size_t ns = (size_t)nseg * 256;
  DevIn<float> dG(gx, (size_t)windows * 512), dW(whh, 512 * 128), dB(bhh, 512), dD(wd, 128),
      dI(init, init ? ns : 0);
  DevIn<long> dS(seg_start, nseg);
  DevIn<int> dC(seg_count, nseg), dWm(seg_warm, seg_warm ? nseg : 0);
  GuardedOut op(probs, (size_t)windows * 4);
  std::unique_ptr<GuardedOut> os, oe;
  if (s_out) os.reset(new GuardedOut(s_out, ns * 4));
  if (e_out) oe.reset(new GuardedOut(e_out, ns * 4));
  VadLstmArgs a{};
  a.gx = dG.p();
  a.whh = dW.p();
  a.bhh = dB.p();
  a.wd = dD.p();
  a.bd = bd;
  a.seg_start = dS.p();
  a.seg_count = dC.p();
  a.seg_warm = seg_warm ? dWm.p() : nullptr;
  a.init = init ? dI.p() : nullptr;
  a.s_out = os ? os->d.as<float>() : nullptr;
  a.e_out = oe ? oe->d.as<float>() : nullptr;
  a.probs = op.d.as<float>();
  launch_vad_lstm(a, nseg, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  op.down(probs, "vad_lstm");
  if (os) os->down(s_out, "vad_lstm");
  if (oe) oe->down(e_out, "vad_lstm");
}

void selftest_vibert_ln(long rows, int H, int L, const long* ids, const long* tt, int V, int P,
                        int TT, const float* word, const float* pos, const float* type,
                        const float* g, const float* b, float eps, float* x) {
  const std::string m = "selftest vibert_ln: ";
  ZASR_REQUIRE(rows >= 1 && rows <= (1 << 20) && H >= 1 && H <= (1 << 16) && (size_t)rows * H <= kAuxMax,
               m + "sizes out of range");
  DevIn<float> dG(g, H), dB(b, H);
  GuardedOut o(x, (size_t)rows * H * 4);
  if (!ids) {
    launch_vibert_layernorm(o.d.as<float>(), rows, H, dG.p(), dB.p(), eps, nullptr);
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    o.down(x, "vibert_ln");
    return;
  }
  ZASR_REQUIRE(tt && word && pos && type, m + "the embedding form takes ids, tt and the three tables");
  ZASR_REQUIRE(L >= 1 && V >= 1 && TT >= 1 && P >= L && (size_t)V * H <= kAuxMax && (size_t)P * H <= kAuxMax,
               m + "table sizes out of range (the position table needs L rows)");
  for (long r = 0; r < rows; ++r)
    ZASR_REQUIRE(ids[r] >= 0 && ids[r] < V && tt[r] >= 0 && tt[r] < TT, m + "ids / token types outside their tables");
  DevIn<long> dI(ids, rows), dT(tt, rows);
  DevIn<float> dW(word, (size_t)V * H), dP(pos, (size_t)P * H), dY(type, (size_t)TT * H);
  VibertEmbedArgs a{dI.p(), dT.p(), dW.p(), dP.p(), dY.p(), dG.p(), dB.p(), o.d.as<float>(), L, H, eps};
  launch_vibert_embed(a, rows, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(x, "vibert_ln");
}

void selftest_vibert_attn(int B, int L, int heads, int H, const float* qkv, const long* mask,
                          float* ctx) {
  const std::string m = "selftest vibert_attn: ";
  ZASR_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && L <= (1 << 16) && heads >= 1 && heads <= 1024 && H >= 1 &&
                   H <= (1 << 16) && (size_t)B * L * 3 * H <= kAuxMax, m + "sizes out of range");
  const size_t R = (size_t)B * L;
  DevIn<float> dQ(qkv, R * 3 * H);
  DevIn<long> dM(mask, R);
  GuardedOut o(ctx, R * H * 4);
  const int D = H / heads;
  VibertAttnArgs a{dQ.p(), dM.p(), o.d.as<float>(), L, H, 1.f / std::sqrt((float)(D > 0 ? D : 1))};
  launch_vibert_attention(a, B, heads, nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(ctx, "vibert_attn");
}

void selftest_vibert_gather(int B, int L, int W, int H, const float* x, const long* offsets,
                            float* g) {
  const std::string m = "selftest vibert_gather: ";
  ZASR_REQUIRE(B >= 1 && L >= 1 && W >= 1 && H >= 1 && (size_t)B * L * H <= kAuxMax &&
                   (size_t)B * W * H <= kAuxMax, m + "sizes out of range");
  for (long i = 0; i < (long)B * W; ++i)
    ZASR_REQUIRE(offsets[i] >= 0 && offsets[i] < L, m + "offsets must lie inside the sequence");
  DevIn<float> dX(x, (size_t)B * L * H);
  DevIn<long> dO(offsets, (size_t)B * W);
  GuardedOut o(g, (size_t)B * W * H * 4);
  launch_vibert_gather(dX.p(), dO.p(), B, L, W, H, o.d.as<float>(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(g, "vibert_gather");
}


// ---- the community-1 embedding kernels (emb_kernels.hip) ----
namespace {
// an output with guard bytes before and behind it, holding the caller's values where the kernel
// does not write
struct GuardedBoth {
  size_t bytes;
  DevBuf d;
  explicit GuardedBoth(const void* init, size_t bytes_) : bytes(bytes_), d(bytes_ + 2 * kAttnGuard) {
    ZASR_HIP_CHECK(hipMemset(d.p, 0x5a, bytes + 2 * kAttnGuard));
    if (bytes) ZASR_HIP_CHECK(hipMemcpy(p(), init, bytes, hipMemcpyHostToDevice));
  }
  float* p() const { return reinterpret_cast<float*>(d.as<unsigned char>() + kAttnGuard); }
  void down(void* out, const char* what) const {
    std::vector<unsigned char> all(bytes + 2 * kAttnGuard);
    ZASR_HIP_CHECK(hipMemcpy(all.data(), d.p, all.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < kAttnGuard; ++i)
      ZASR_REQUIRE(all[i] == 0x5a && all[kAttnGuard + bytes + i] == 0x5a,
                   std::string("selftest ") + what + ": the kernel wrote outside its output");
    std::memcpy(out, all.data() + kAttnGuard, bytes);
  }
};
}  // namespace

void selftest_emb_conv2d(int ks, int stride, int ci, int co, int n, int fi, int ti, int relu,
                         int route, const float* x, const float* w, const float* bias,
                         const float* res, float* y, int* n_routes) {
  const std::string m = "selftest emb_conv2d: ";
  auto okc = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  const bool stem = ci == 1;
  ZASR_REQUIRE(okc(co) && (stem || okc(ci)), m + "Ci, Co in {32, 64, 128, 256}, or Ci = 1 (the stem)");
  ZASR_REQUIRE((ks == 1 || ks == 3) && (stride == 1 || stride == 2), m + "kernel 1 | 3, stride 1 | 2");
  ZASR_REQUIRE(!stem || (ks == 3 && stride == 1 && relu && !res && route == 0),
               m + "the stem is 3x3, stride 1, ReLU, no residual, one route");
  ZASR_REQUIRE(n >= 1 && fi >= 1 && ti >= 1 && n <= 65535 && fi <= 4096 && ti <= (1 << 20), m + "sizes out of range");
  const int fo = (fi - 1) / stride + 1, to = (ti - 1) / stride + 1;
  const size_t nx = (size_t)n * fi * ti * ci, nw = (size_t)co * ks * ks * ci, ny = (size_t)n * fo * to * co;
  ZASR_REQUIRE(nx <= kAuxMax && ny <= kAuxMax, m + "problem too large");
  const int routes = stem ? 1 : emb_conv2d_routes(co);
  if (n_routes) *n_routes = routes;
  ZASR_REQUIRE(route >= 0 && route <= routes, m + "no such route for this layer");
  DevIn<float> dX(x, nx), dW(w, nw), dB(bias, co), dR(res, res ? ny : 0);
  GuardedBoth o(y, ny * 4);
  if (stem) {
    launch_emb_stem(dX.p(), dW.p(), dB.p(), n, ti, fi, co, o.p(), nullptr);
  } else {
    EmbConv2d a{};
    a.x = dX.p();
    a.w = dW.p();
    a.bias = dB.p();
    a.res = res ? dR.p() : nullptr;
    a.y = o.p();
    a.n = n;
    a.Fi = fi;
    a.Ti = ti;
    a.Ci = ci;
    a.Fo = fo;
    a.To = to;
    a.Co = co;
    a.ks = ks;
    a.stride = stride;
    a.relu = relu ? 1 : 0;
    launch_emb_conv2d(a, route, nullptr);
  }
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(y, "emb_conv2d");
}

void selftest_emb_pool(int n, int F, int T, int C, int S, int nseg, int pop, const float* x,
                       const unsigned char* mask, float* stats) {
  const std::string m = "selftest emb_pool: ";
  ZASR_REQUIRE(n >= 1 && F >= 1 && T >= 1 && C >= 1 && S >= 1 && S <= 4 && (pop || T <= 1024) &&
                   (size_t)n * F * T * C <= kAuxMax && (size_t)n * S * 2 * C * F <= kAuxMax,
               m + "sizes out of range");
  ZASR_REQUIRE(pop || (mask && nseg >= 1 && (size_t)n * S * nseg <= kAuxMax), m + "the masked form takes masks");
  DevIn<float> dX(x, (size_t)n * F * T * C);
  DevIn<unsigned char> dM(pop ? nullptr : mask, pop ? 0 : (size_t)n * S * nseg);
  GuardedBoth o(stats, (size_t)n * S * 2 * C * F * 4);
  launch_emb_pool(dX.p(), pop ? nullptr : dM.p(), n, F, T, C, S, nseg, pop != 0, o.p(), nullptr);
  ZASR_HIP_CHECK(hipDeviceSynchronize());
  o.down(stats, "emb_pool");
}

// ---- the PyanNet and Conv-TasNet kernels (seg_kernels.hip, sep_kernels.hip) ----
namespace {
// a stream of the entry's own; made after every buffer, so that the uploads and the guards'
// fills (null stream) are complete before anything runs on it
struct FreshStream {
  hipStream_t s = nullptr;
  FreshStream() {
    ZASR_HIP_CHECK(hipDeviceSynchronize());
    ZASR_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  }
  ~FreshStream() { (void)hipStreamDestroy(s); }
  void sync() const { ZASR_HIP_CHECK(hipStreamSynchronize(s)); }
};
}  // namespace

void selftest_seg_chunk_stats(long total, int n, int T, const float* audio, const long* starts,
                              float* stats) {
  const std::string m = "selftest seg_chunk_stats: ";
  ZASR_REQUIRE(total >= 1 && (size_t)total <= kAuxMax && n >= 1 && n <= 65535 && T >= 1 && T <= (1 << 24),
               m + "sizes out of range");
  for (int k = 0; k < n; ++k) ZASR_REQUIRE(starts[k] >= 0, m + "chunk starts must not be negative");
  DevIn<float> dA(audio, (size_t)total);
  DevIn<long> dS(starts, n);
  GuardedOut o(stats, (size_t)n * 8);
  FreshStream st;
  launch_seg_chunk_stats(dA.p(), total, dS.p(), n, T, o.d.as<float2>(), st.s);
  st.sync();
  o.down(stats, "seg_chunk_stats");
}

void selftest_seg_front(long total, int n, int T, const float* audio, const long* starts,
                        const float* stats, float in_w, float in_b, const float* w0t, float* out) {
  const std::string m = "selftest seg_front: ";
  ZASR_REQUIRE(total >= 1 && (size_t)total <= kAuxMax && n >= 1 && n <= (1 << 17) && T >= kSegTaps &&
                   T <= (1 << 24), m + "sizes out of range");
  const int F1 = ((T - kSegTaps) / kSegStride0 + 1) / 3;
  ZASR_REQUIRE(F1 >= 1 && (size_t)n * F1 * kSegC0 <= kAuxMax, m + "T must give at least one pooled frame");
  for (int k = 0; k < n; ++k) ZASR_REQUIRE(starts[k] >= 0, m + "chunk starts must not be negative");
  DevIn<float> dA(audio, (size_t)total), dSt(stats, (size_t)n * 2), dW(w0t, (size_t)kSegTaps * kSegC0);
  DevIn<long> dS(starts, n);
  GuardedOut o(out, (size_t)n * F1 * kSegC0 * 4);
  SegFrontArgs a{};
  a.audio = dA.p();
  a.total = total;
  a.starts = dS.p();
  a.stats = reinterpret_cast<const float2*>(dSt.p());
  a.in_w = in_w;
  a.in_b = in_b;
  a.w0t = dW.p();
  a.out = o.d.as<float>();
  a.T = T;
  a.F1 = F1;
  FreshStream st;
  launch_seg_front(a, n, st.s);
  st.sync();
  o.down(out, "seg_front");
}

void selftest_seg_pool3(int n, int L, int C, int Fp, int max_blocks, const float* x, float* out) {
  ZASR_REQUIRE(n >= 1 && L >= 1 && C >= 1 && Fp >= 1 && max_blocks >= 0 && (size_t)n * L * C <= kAuxMax &&
                   (size_t)n * Fp * C <= kAuxMax, "selftest seg_pool3: sizes out of range");
  DevIn<float> dX(x, (size_t)n * L * C);
  GuardedOut o(out, (size_t)n * Fp * C * 4);
  FreshStream st;
  launch_seg_pool3(dX.p(), n, L, C, Fp, o.d.as<float>(), st.s, max_blocks);
  st.sync();
  o.down(out, "seg_pool3");
}

void selftest_seg_frame_stats(int n, int F, int C, const float* x, float* stats) {
  ZASR_REQUIRE(n >= 1 && n <= 65535 && F >= 1 && C >= 1 && C <= 4096 && (size_t)n * F * C <= kAuxMax,
               "selftest seg_frame_stats: sizes out of range");
  DevIn<float> dX(x, (size_t)n * F * C);
  GuardedOut o(stats, (size_t)n * C * 8);
  FreshStream st;
  launch_seg_frame_stats(dX.p(), n, F, C, o.d.as<float2>(), st.s);
  st.sync();
  o.down(stats, "seg_frame_stats");
}

void selftest_seg_norm_act(int n, int F, int C, int max_blocks, const float* stats, const float* w,
                           const float* b, float* x) {
  ZASR_REQUIRE(n >= 1 && F >= 1 && C >= 1 && C <= 4096 && max_blocks >= 0 && (size_t)n * F * C <= kAuxMax,
               "selftest seg_norm_act: sizes out of range");
  DevIn<float> dS(stats, (size_t)n * C * 2), dW(w, C), dB(b, C);
  GuardedBoth o(x, (size_t)n * F * C * 4);
  FreshStream st;
  launch_seg_norm_act(o.p(), n, F, C, reinterpret_cast<const float2*>(dS.p()), dW.p(), dB.p(), st.s,
                      max_blocks);
  st.sync();
  o.down(x, "seg_norm_act");
}

void selftest_seg_lstm(int n, int F, int group, const float* gx, const float* whh, float* out) {
  ZASR_REQUIRE(n >= 1 && n <= 4096 && F >= 1 && F <= 4096 && group >= 1 && group <= 4096,
               "selftest seg_lstm: sizes out of range");
  DevIn<float> dG(gx, (size_t)n * F * 8 * kSegH), dW(whh, (size_t)2 * 4 * kSegH * kSegH);
  GuardedOut o(out, (size_t)n * F * 2 * kSegH * 4);
  SegLstmArgs a{dG.p(), dW.p(), o.d.as<float>(), n, F};
  FreshStream st;
  launch_seg_lstm(a, group, st.s);
  st.sync();
  o.down(out, "seg_lstm");
}

void selftest_seg_head(long rows, const float* x, const float* w, const float* b, float* logits,
                       unsigned char* classes) {
  ZASR_REQUIRE(rows >= 1 && rows <= (1 << 20), "selftest seg_head: rows out of range");
  DevIn<float> dX(x, (size_t)rows * kSegH), dW(w, (size_t)kSegClasses * kSegH), dB(b, kSegClasses);
  GuardedOut ol(logits, (size_t)rows * kSegClasses * 4), oc(classes, (size_t)rows);
  FreshStream st;
  launch_seg_head(dX.p(), rows, dW.p(), dB.p(), ol.d.as<float>(), oc.d.as<unsigned char>(), st.s);
  st.sync();
  ol.down(logits, "seg_head (logits)");
  oc.down(classes, "seg_head (classes)");
}

namespace {
// the region and tile tables of one call as the engine's own builder makes them, the launch
// groups [0, r0) and [r0, r0 + ng) appended in that order
struct SepTables {
  std::vector<SepRegion> regions;
  std::vector<SepTile> tiles;
  SepGroup g;
  SepTables(const SepSelftestCall& c, const long* out_off, const std::string& m) {
    ZASR_REQUIRE(c.n_regions >= 1 && c.n_regions <= (1 << 17) && c.r0 >= 0 && c.ng >= 1 &&
                     (long)c.r0 + c.ng <= c.n_regions, m + "the group must lie inside the call's regions");
    ZASR_REQUIRE(c.win >= 1 && c.win <= 4096 && c.hop >= 1 && c.hop <= c.win, m + "win / hop out of range");
    regions.resize((size_t)c.n_regions);
    for (int r = 0; r < c.n_regions; ++r) {
      ZASR_REQUIRE(c.T[r] >= c.win && c.T[r] <= (1 << 24) && c.sig_off[r] >= 0,
                   m + "every region needs win <= T <= 2^24 and sig_off >= 0");
      SepRegion& rg = regions[(size_t)r];
      rg.sig_off = c.sig_off[r];
      rg.out_off = out_off ? out_off[r] : 0;
      rg.T = c.T[r];
      rg.F = (c.T[r] - c.win) / c.hop + 1;
      rg.row0 = rg.tile0 = 0;
    }
    if (c.r0 > 0) sep_fill_group(regions, 0, c.r0, tiles);
    g = sep_fill_group(regions, c.r0, c.ng, tiles);
    ZASR_REQUIRE(g.rows >= 1 && g.rows <= (1 << 20), m + "the group's rows out of range");
  }
};
// the tables on the device
struct SepDevTables {
  DevIn<SepRegion> regions;
  DevIn<SepTile> tiles;
  explicit SepDevTables(const SepTables& t)
      : regions(t.regions.data(), t.regions.size()), tiles(t.tiles.data(), t.tiles.size()) {}
};
}  // namespace

void selftest_sep_frames(const SepSelftestCall& c, long n_signal, const float* signal, float* frames) {
  const std::string m = "selftest sep_frames: ";
  const SepTables t(c, nullptr, m);
  ZASR_REQUIRE(n_signal >= 1 && (size_t)n_signal <= kAuxMax, m + "signal length out of range");
  for (int r = c.r0; r < c.r0 + c.ng; ++r) {
    const SepRegion& rg = t.regions[(size_t)r];
    ZASR_REQUIRE(rg.sig_off + (long)(rg.F - 1) * c.hop + c.win <= n_signal, m + "region outside the signal");
  }
  DevIn<float> dS(signal, (size_t)n_signal);
  const SepDevTables d(t);
  GuardedBoth o(frames, (size_t)t.g.rows * c.win * 4);
  FreshStream st;
  launch_sep_frames(dS.p(), d.regions.p(), d.tiles.p() + t.g.tile0, t.g.n_tiles, c.win, c.hop, o.p(), st.s);
  st.sync();
  o.down(frames, "sep_frames");
}

void selftest_sep_tile_sums(const SepSelftestCall& c, int C, const float* x, double* partial) {
  const std::string m = "selftest sep_tile_sums: ";
  const SepTables t(c, nullptr, m);
  ZASR_REQUIRE(C >= 1 && C <= 4096, m + "C out of range");
  DevIn<float> dX(x, (size_t)t.g.rows * C);
  const SepDevTables d(t);
  GuardedBoth o(partial, (size_t)t.g.n_tiles * 16);
  FreshStream st;
  launch_sep_tile_sums(dX.p(), C, d.tiles.p() + t.g.tile0, t.g.n_tiles,
                       reinterpret_cast<double2*>(o.p()), st.s);
  st.sync();
  o.down(partial, "sep_tile_sums");
}

void selftest_sep_region_stats(const SepSelftestCall& c, int C, const double* partial, float* stats) {
  const std::string m = "selftest sep_region_stats: ";
  const SepTables t(c, nullptr, m);
  ZASR_REQUIRE(C >= 1 && C <= 4096, m + "C out of range");
  DevIn<double> dP(partial, (size_t)t.g.n_tiles * 2);
  const SepDevTables d(t);
  GuardedBoth o(stats, (size_t)c.n_regions * 8);
  FreshStream st;
  launch_sep_region_stats(reinterpret_cast<const double2*>(dP.p()), d.regions.p() + c.r0, c.ng, C,
                          reinterpret_cast<float2*>(o.p()) + c.r0, st.s);
  st.sync();
  o.down(stats, "sep_region_stats");
}

void selftest_sep_gln_apply(const SepSelftestCall& c, int C, int in_place, const float* stats,
                            const float* gamma, const float* beta, const float* src, float* dst) {
  const std::string m = "selftest sep_gln_apply: ";
  const SepTables t(c, nullptr, m);
  ZASR_REQUIRE(C >= 1 && C <= 4096, m + "C out of range");
  ZASR_REQUIRE(in_place || src, m + "out of place takes src");
  const size_t n = (size_t)t.g.rows * C;
  DevIn<float> dSt(stats, (size_t)c.n_regions * 2), dG(gamma, C), dB(beta, C), dX(in_place ? nullptr : src, in_place ? 0 : n);
  const SepDevTables d(t);
  GuardedBoth o(dst, n * 4);
  FreshStream st;
  launch_sep_gln_apply(in_place ? o.p() : dX.p(), o.p(), C, d.tiles.p() + t.g.tile0, t.g.n_tiles,
                       reinterpret_cast<const float2*>(dSt.p()), dG.p(), dB.p(), st.s);
  st.sync();
  o.down(dst, "sep_gln_apply");
}

void selftest_sep_mid(const SepSelftestCall& c, int C, int dil, float slope, const float* stats,
                      const float* gamma, const float* beta, const float* w, const float* bias,
                      const float* h, float* y, double* partial) {
  const std::string m = "selftest sep_mid: ";
  const SepTables t(c, nullptr, m);
  ZASR_REQUIRE(C >= 1 && C <= 4096 && dil >= 1 && dil <= (1 << 16), m + "C / dilation out of range");
  const size_t n = (size_t)t.g.rows * C;
  DevIn<float> dSt(stats, (size_t)c.n_regions * 2), dG(gamma, C), dB(beta, C), dW(w, (size_t)3 * C),
      dBi(bias, C), dH(h, n);
  const SepDevTables d(t);
  GuardedBoth oy(y, n * 4);
  GuardedBoth op(partial, (size_t)t.g.n_tiles * 16);
  SepMidArgs a{};
  a.h = dH.p();
  a.y = oy.p();
  a.stats = reinterpret_cast<const float2*>(dSt.p());
  a.gamma = dG.p();
  a.beta = dB.p();
  a.w = dW.p();
  a.bias = dBi.p();
  a.slope = slope;
  a.C = C;
  a.dil = dil;
  a.partial = reinterpret_cast<double2*>(op.p());
  FreshStream st;
  launch_sep_mid(a, d.tiles.p() + t.g.tile0, t.g.n_tiles, st.s);
  st.sync();
  oy.down(y, "sep_mid");
  op.down(partial, "sep_mid (partial sums)");
}

void selftest_sep_prelu(long rows, int C, int ld, int col0, float slope, int max_blocks, float* x) {
  const std::string m = "selftest sep_prelu: ";
  ZASR_REQUIRE(rows >= 1 && C >= 1 && ld >= 1 && ld <= (1 << 16) && max_blocks >= 0 &&
                   (size_t)rows * ld <= kAuxMax, m + "sizes out of range");
  ZASR_REQUIRE(col0 >= 0 && col0 % 4 == 0 && (long)col0 + C <= ld, m + "columns [col0, col0 + C) must lie inside ld");
  GuardedBoth o(x, (size_t)rows * ld * 4);
  FreshStream st;
  launch_sep_prelu(o.p() + col0, rows, C, ld, slope, st.s, max_blocks);
  st.sync();
  o.down(x, "sep_prelu");
}

void selftest_sep_overlap_add(const SepSelftestCall& c, const long* out_off, long n_out,
                              const float* dec0, const float* dec1, float* out) {
  const std::string m = "selftest sep_overlap_add: ";
  const SepTables t(c, out_off, m);
  ZASR_REQUIRE(n_out >= 1 && (size_t)n_out <= kAuxMax, m + "output length out of range");
  for (int r = c.r0; r < c.r0 + c.ng; ++r) {
    const SepRegion& rg = t.regions[(size_t)r];
    ZASR_REQUIRE(rg.out_off >= 0 && rg.out_off + 2L * rg.T <= n_out, m + "a region's [2][T] outside the output");
  }
  const size_t n = (size_t)t.g.rows * c.win;
  DevIn<float> d0(dec0, n), d1(dec1, n);
  const SepDevTables d(t);
  GuardedBoth o(out, (size_t)n_out * 4);
  FreshStream st;
  launch_sep_overlap_add(d0.p(), d1.p(), d.regions.p() + c.r0, c.ng, t.g.max_T, c.win, c.hop, o.p(), st.s);
  st.sync();
  o.down(out, "sep_overlap_add");
}

}  // namespace zasr
