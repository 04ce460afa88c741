// Host driver of the diarization clustering (diar.h): the stage entries and the
// Chebyshev-filtered subspace iteration for the smallest eigenpairs of L = diag(deg) - M.
#include "diar.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "dense_gemm.h"

namespace zasr {

namespace {

constexpr int B = kDiarB;

// counter-based start block: splitmix64 of the element index, uniform in [-1, 1)
double start_value(uint64_t idx) {
  uint64_t z = (idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

}  // namespace

int diar_prune_count(int N, double pval, int min_pnum) {
  // int() truncates toward zero, as the cast does; the product is the same IEEE double
  double t = (1.0 - pval) * (double)N;
  long n_elems = (long)t;
  n_elems = std::min<long>(n_elems, (long)N - min_pnum);
  n_elems = std::max<long>(n_elems, 0);
  return (int)std::min<long>(n_elems, N);
}

void jacobi_eigh(std::vector<double>& A, int n, std::vector<double>& w, std::vector<double>& Q) {
  // A stays symmetric: a rotation updates rows p and q (contiguous) and mirrors them into the
  // columns; Qt holds the eigenvectors as rows.  An off-diagonal entry too small to change
  // either diagonal entry is set to zero, so the sweeps end on an exactly diagonal matrix.
  std::vector<double> Qt((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) Qt[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    if (off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double* ap = &A[(size_t)p * n];
        double* aq = &A[(size_t)q * n];
        const double apq = ap[q];
        if (apq == 0.0) continue;
        const double app = ap[p], aqq = aq[q];
        const double g = 100.0 * std::fabs(apq);
        if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
          ap[q] = aq[p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = ap[k], akq = aq[k];
          ap[k] = c * akp - s * akq;
          aq[k] = s * akp + c * akq;
        }
        ap[p] = app - t * apq;
        aq[q] = aqq + t * apq;
        ap[q] = aq[p] = 0.0;
        for (int k = 0; k < n; ++k) {
          A[(size_t)k * n + p] = ap[k];
          A[(size_t)k * n + q] = aq[k];
        }
        double* qp = &Qt[(size_t)p * n];
        double* qq = &Qt[(size_t)q * n];
        for (int k = 0; k < n; ++k) {
          const double x = qp[k], y = qq[k];
          qp[k] = c * x - s * y;
          qq[k] = s * x + c * y;
        }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return A[(size_t)a * n + a] < A[(size_t)b * n + b]; });
  w.resize(n);
  Q.assign((size_t)n * n, 0.0);
  for (int c = 0; c < n; ++c) {
    w[c] = A[(size_t)order[c] * n + order[c]];
    for (int k = 0; k < n; ++k) Q[(size_t)k * n + c] = Qt[(size_t)order[c] * n + k];
  }
}

DiarEngine::DiarEngine(int device) : device_(device) {
  int n = 0;
  ZASR_HIP_CHECK(hipGetDeviceCount(&n));
  ZASR_REQUIRE(device >= 0 && device < n, "diar: device id out of range");
  ZASR_HIP_CHECK(hipSetDevice(device));
}

void DiarEngine::similarity(const float* d_X, int N, int D, float* d_M, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const int ldn = cdiv(D, 4) * 4;
  float* xn = ws_.get<float>("xn", (size_t)N * ldn, &st);
  launch_diar_normalise(d_X, N, D, xn, ldn, st);
  if (D % 4 == 0) {
    // the exact-f32 MFMA GEMM with W = Xn: no rounding below float32 ahead of the prune
    gemm_f32(dense_gemm_params(xn, nullptr, N, D, xn, ldn, N, d_M, N), EPI_NONE, ALOAD_DENSE, false,
             st);
  } else {
    launch_diar_similarity_plain(xn, N, D, ldn, d_M, st);
  }
}

void DiarEngine::prune(float* d_M, int N, double pval, int min_pnum, double* d_deg,
                       hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const int n_elems = diar_prune_count(N, pval, min_pnum);
  launch_diar_prune(d_M, N, std::max(1, N - n_elems), st);
  launch_diar_symmetrise(d_M, N, st);
  launch_diar_degree(d_M, N, d_deg, st);
}

int DiarEngine::eigs(const float* d_M, const double* d_deg, int N, int k, double* lambdas,
                     double* vecs, hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const int b = std::min(B, N);
  ZASR_REQUIRE(k >= 1 && k <= std::min(kDiarMaxK, N), "diar eigs: k outside [1, min(16, N)]");
  const size_t blk = (size_t)N * B;
  double* buf[5];
  for (int i = 0; i < 5; ++i) buf[i] = ws_.get<double>("blk" + std::to_string(i), blk, &st);
  const int split = diar_lap_split(N);
  double* lap_part = ws_.get<double>("lap_part", split > 1 ? blk * split : 1, &st);
  double* gram_part = ws_.get<double>("gram_part", (size_t)cdiv(N, kDiarGramRows) * 1024, &st);
  double* dG = ws_.get<double>("G", 1024, &st);
  double* dRA = ws_.get<double>("RA", 1024, &st);
  double* dRB = ws_.get<double>("RB", 1024, &st);

  std::vector<double> hdeg(N);
  ZASR_HIP_CHECK(hipMemcpyAsync(hdeg.data(), d_deg, N * sizeof(double), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  double ub = 1.01 * 2.0 * *std::max_element(hdeg.begin(), hdeg.end());  // Gershgorin
  if (!(ub > 0.0)) ub = 1.0;  // L = 0: any orthonormal block is an eigenbasis

  long apps = 0;
  auto lap = [&](const double* V1, const double* V0, double* out, double alpha, double c,
                 double beta) {
    launch_diar_lap_block(d_M, d_deg, N, V1, V0, out, alpha, c, beta, split, lap_part, st);
    ++apps;
  };
  std::vector<double> hG(1024), hR(1024);
  auto gram = [&](const double* A, const double* Bm) {
    launch_diar_gram(A, Bm, N, gram_part, dG, st);
    ZASR_HIP_CHECK(hipMemcpyAsync(hG.data(), dG, 1024 * sizeof(double), hipMemcpyDeviceToHost, st));
    ZASR_HIP_CHECK(hipStreamSynchronize(st));
  };
  // R [b][b] -> the device's [32][32] (zero outside), synchronously: hR is reused
  auto upload = [&](const std::vector<double>& R, double* d) {
    std::fill(hR.begin(), hR.end(), 0.0);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j) hR[(size_t)i * B + j] = R[(size_t)i * b + j];
    ZASR_HIP_CHECK(hipMemcpyAsync(d, hR.data(), 1024 * sizeof(double), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipStreamSynchronize(st));
  };

  int iv = 0;                 // buf[iv] is V
  auto free_buf = [&](std::initializer_list<int> used) {
    for (int i = 0; i < 5; ++i)
      if (std::find(used.begin(), used.end(), i) == used.end()) return i;
    return -1;
  };

  // max |V^T V - I| of the Gram matrix in hG
  auto gram_deviation = [&]() {
    double dev = 0.0;
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j)
        dev = std::max(dev, std::fabs(hG[(size_t)i * B + j] - (i == j ? 1.0 : 0.0)));
    return dev;
  };
  // one SVQB step from G = V^T V in hG: V <- V D U Lambda^-1/2 with D = diag(G)^-1/2 and
  // (U, Lambda) the eigenpairs of D G D, Lambda clipped at 1e-14 of its maximum
  std::vector<double> Gs, wg, U, R((size_t)b * b), d(b);
  auto svqb = [&]() {
    for (int i = 0; i < b; ++i) {
      const double g = hG[(size_t)i * B + i];
      d[i] = g > 0.0 ? 1.0 / std::sqrt(g) : 0.0;
    }
    Gs.assign((size_t)b * b, 0.0);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j)
        Gs[(size_t)i * b + j] = 0.5 * (hG[(size_t)i * B + j] + hG[(size_t)j * B + i]) * d[i] * d[j];
    jacobi_eigh(Gs, b, wg, U);
    const double floor = 1e-14 * std::max(wg[b - 1], 0.0);
    for (int j = 0; j < b; ++j) {
      const double lam = std::max(wg[j], floor);
      const double s = lam > 0.0 ? 1.0 / std::sqrt(lam) : 0.0;
      for (int i = 0; i < b; ++i) R[(size_t)i * b + j] = d[i] * U[(size_t)i * b + j] * s;
    }
    upload(R, dRA);
    const int o = free_buf({iv});
    launch_diar_block_mul(buf[iv], dRA, nullptr, nullptr, N, buf[o], st);
    iv = o;
  };
  // SVQB twice, then until |V^T V - I|_max <= 1e-10 (three more steps at most)
  auto orthonormalise = [&]() {
    for (int round = 0; round < 5; ++round) {
      gram(buf[iv], buf[iv]);
      if (round >= 2 && gram_deviation() <= 1e-10) return;
      svqb();
    }
    gram(buf[iv], buf[iv]);
    ZASR_REQUIRE(gram_deviation() <= 1e-10, "diar eigs: the block did not orthonormalise");
  };

  {
    std::vector<double> h(blk, 0.0);
    for (int i = 0; i < N; ++i)
      for (int c = 0; c < b; ++c) h[(size_t)i * B + c] = start_value((uint64_t)i * B + c);
    ZASR_HIP_CHECK(hipMemcpyAsync(buf[iv], h.data(), blk * sizeof(double), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipStreamSynchronize(st));
  }
  orthonormalise();

  std::vector<double> H, w, Q, QL((size_t)b * b);
  int pass = 0;
  bool done = false;
  while (pass < kDiarMaxPasses) {
    ++pass;
    // Rayleigh-Ritz: H = V^T (L V), V <- V Q, residual block R = (L V) Q - V Q diag(w)
    const int iw = free_buf({iv});
    lap(buf[iv], nullptr, buf[iw], 1.0, 0.0, 0.0);
    gram(buf[iv], buf[iw]);
    H.assign((size_t)b * b, 0.0);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j)
        H[(size_t)i * b + j] = 0.5 * (hG[(size_t)i * B + j] + hG[(size_t)j * B + i]);
    jacobi_eigh(H, b, w, Q);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j) QL[(size_t)i * b + j] = -Q[(size_t)i * b + j] * w[j];
    upload(Q, dRA);
    upload(QL, dRB);
    const int inew = free_buf({iv, iw}), ir = free_buf({iv, iw, inew});
    launch_diar_block_mul(buf[iv], dRA, nullptr, nullptr, N, buf[inew], st);
    launch_diar_block_mul(buf[iw], dRA, buf[iv], dRB, N, buf[ir], st);
    iv = inew;
    gram(buf[ir], buf[ir]);
    double worst = 0.0;
    for (int c = 0; c < k; ++c) worst = std::max(worst, std::sqrt(std::max(hG[(size_t)c * B + c], 0.0)));
    if (worst <= 1e-7 * ub) {
      done = true;
      break;
    }
    ZASR_REQUIRE(b < N, "diar eigs: the Rayleigh-Ritz of the whole space did not converge");
    // degree-m Chebyshev filter damping [lb, ub], scaled to 1 at a0 (Zhou & Saad's scaled
    // recurrence: the block stays in range without a separate rescaling pass)
    const double lb = w[b - 1];
    double a0 = w[0];
    if (lb - a0 < 1e-6 * ub) a0 = lb - 1e-6 * ub;
    const double e = 0.5 * (ub - lb), c = 0.5 * (ub + lb);
    double sigma = e / (a0 - c);
    const double tau = 2.0 / sigma;
    int ip = iv, ic = free_buf({iv});
    lap(buf[ip], nullptr, buf[ic], sigma / e, c, 0.0);
    for (int d = 2; d <= kDiarChebDegree; ++d) {
      const double sn = 1.0 / (tau - sigma);
      const int in = free_buf({ip, ic});
      lap(buf[ic], buf[ip], buf[in], 2.0 * sn / e, c, sigma * sn);
      ip = ic;
      ic = in;
      sigma = sn;
    }
    iv = ic;
    orthonormalise();
  }
  last_applications = apps;
  ZASR_REQUIRE(done, "diar eigs: no convergence in " + std::to_string(kDiarMaxPasses) +
                         " passes (residual above 1e-7 of the spectral bound)");
  std::vector<double> hV(blk);
  ZASR_HIP_CHECK(hipMemcpyAsync(hV.data(), buf[iv], blk * sizeof(double), hipMemcpyDeviceToHost, st));
  ZASR_HIP_CHECK(hipStreamSynchronize(st));
  for (int c = 0; c < k; ++c) lambdas[c] = w[c];
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < k; ++c) vecs[(size_t)i * k + c] = hV[(size_t)i * B + c];
  return pass;
}

int DiarEngine::spectral_embed(const float* X, bool x_on_device, int N, int D, double pval,
                               int min_pnum, int k, double* lambdas, double* vecs,
                               hipStream_t st) {
  ZASR_HIP_CHECK(hipSetDevice(device_));
  const float* dX = X;
  if (!x_on_device) {
    float* up = ws_.get<float>("x", (size_t)N * D, &st);
    ZASR_HIP_CHECK(hipMemcpyAsync(up, X, (size_t)N * D * sizeof(float), hipMemcpyHostToDevice, st));
    ZASR_HIP_CHECK(hipStreamSynchronize(st));  // the caller's buffer is free on return
    dX = up;
  }
  float* dM = ws_.get<float>("M", (size_t)N * N, &st);
  double* ddeg = ws_.get<double>("deg", (size_t)N, &st);
  similarity(dX, N, D, dM, st);
  prune(dM, N, pval, min_pnum, ddeg, st);
  return eigs(dM, ddeg, N, k, lambdas, vecs, st);
}

}  // namespace zasr
