// WPE dereverberation kernels (wpe.h) for gfx950: wpe_stft, wpe_iter, wpe_istft
// over a ragged batch of chunks.  Nothing here adds floating-point values with atomics: the
// only atomics are integer maxima of non-negative floats' bit patterns, so a chunk's result
// depends on that chunk alone, whatever else shares the launch.
#include "wpe.h"

#include "common.h"

namespace zasr {

namespace {

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

__device__ __forceinline__ float norm2f(float2 v) {
  return __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y));
}

// 256-point complex FFT of one wave's image A (the fbank kernel's radix-4 Stockham scheme, in
// float32): four passes, one butterfly per lane per pass, ping-ponging A and B; the result is
// in A.  sTw[u] = exp(-2 pi i u / 512), u < 256.
__device__ __forceinline__ void fft256(float2* A, float2* B, const float2* sTw, int j) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float2* X = (s & 1) ? B : A;
    float2* Y = (s & 1) ? A : B;
    const int ns_log = 2 * s, Ns = 1 << ns_log;
    const int k = j & (Ns - 1);
    float2 v0 = X[j], v1 = X[j + 64], v2 = X[j + 128], v3 = X[j + 192];
    if (s > 0) {
      const int u = k << (7 - ns_log);
      const int u2 = 2 * u, u3 = 3 * u;
      const float2 t1 = sTw[u];
      const float2 t2 = u2 < 256 ? sTw[u2] : make_float2(-sTw[u2 - 256].x, -sTw[u2 - 256].y);
      const float2 t3 = u3 < 256 ? sTw[u3] : make_float2(-sTw[u3 - 256].x, -sTw[u3 - 256].y);
      v1 = cmulf(v1, t1);
      v2 = cmulf(v2, t2);
      v3 = cmulf(v3, t3);
    }
    const float2 a0 = make_float2(v0.x + v2.x, v0.y + v2.y);
    const float2 a1 = make_float2(v0.x - v2.x, v0.y - v2.y);
    const float2 a2 = make_float2(v1.x + v3.x, v1.y + v3.y);
    const float2 a3 = make_float2(v1.y - v3.y, v3.x - v1.x);  // (v1 - v3) * (-i)
    const int o = ((j >> ns_log) << (ns_log + 2)) + k;
    Y[o] = make_float2(a0.x + a2.x, a0.y + a2.y);
    Y[o + Ns] = make_float2(a1.x + a3.x, a1.y + a3.y);
    Y[o + 2 * Ns] = make_float2(a0.x - a2.x, a0.y - a2.y);
    Y[o + 3 * Ns] = make_float2(a1.x - a3.x, a1.y - a3.y);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// wpe_stft: block (tile of 16 frames, chunk); each wave transforms frames w, w + 4, ... of the
// tile: samples with the zero fading, window, 512-point real FFT as a 256-point complex one of
// z[n] = x[2n] + i x[2n+1] and the even / odd split.  The tile's spectra go through LDS so that
// the stores run along frames.  Every wave of the block runs the same number of frames (frames
// past T transform zeros and are not stored), so fft256's barriers are block-uniform.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wpe_stft_kernel(const float* __restrict__ signal,
                                                       const WpeChunk* __restrict__ chunks,
                                                       WpeTables tabs, float2* __restrict__ Y,
                                                       unsigned* __restrict__ max_bits,
                                                       int max_stride) {
  __shared__ float2 sTw[256];
  __shared__ float sWin[kWpeFft];
  __shared__ float2 sA[4][256], sB[4][256];
  __shared__ float2 sT[kWpeBins][kWpeStftTile + 1];
  const WpeChunk c = chunks[blockIdx.y];
  const int t0 = blockIdx.x * kWpeStftTile;
  if (t0 >= c.T) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  sTw[tid] = tabs.twiddle[tid];
  sWin[tid] = tabs.window[tid];
  sWin[tid + 256] = tabs.window[tid + 256];
  __syncthreads();
  const float* base = signal + c.sig_off;
  float2* A = sA[w];
  float2* B = sB[w];
  float m = 0.f;
  for (int fi = w; fi < kWpeStftTile; fi += 4) {
    const int t = t0 + fi;
    const bool live = t < c.T;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = lane + 64 * q;
      const long p = (long)kWpeHop * t + 2 * j - kWpeFade;
      const float x0 = (live && p >= 0 && p < c.n) ? base[p] : 0.f;
      const float x1 = (live && p + 1 >= 0 && p + 1 < c.n) ? base[p + 1] : 0.f;
      A[j] = make_float2(x0 * sWin[2 * j], x1 * sWin[2 * j + 1]);
    }
    __syncthreads();
    fft256(A, B, sTw, lane);
    // X[k] = E[k] + W512^k O[k], E = (Z_k + conj Z_-k) / 2, O = (Z_k - conj Z_-k) / 2i
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kb = lane + 64 * q;
      const float2 zk = A[kb], zm = A[(256 - kb) & 255];
      const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
      const float2 O = make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x));
      const float2 P = cmulf(O, sTw[kb]);
      const float2 X = make_float2(E.x + P.x, kb == 0 ? 0.f : E.y + P.y);
      sT[kb][fi] = X;
      m = fmaxf(m, norm2f(X));
    }
    if (lane == 0) {
      const float2 X = make_float2(A[0].x - A[0].y, 0.f);
      sT[256][fi] = X;
      m = fmaxf(m, norm2f(X));
    }
    __syncthreads();  // the next frame rewrites A and B
  }
  m = wave_max(m);
  if (lane == 0) atomicMax(&max_bits[(long)c.index * max_stride], __float_as_uint(m));
  // 16 bins x 16 frames per pass: a bin's frames are contiguous in Y
  const int f = tid & 15, t = t0 + f;
  if (t < c.T)
    for (int bin = tid >> 4; bin < kWpeBins; bin += 16)
      Y[c.spec_off + (long)bin * c.T + t] = sT[bin][f];
}

// ---------------------------------------------------------------------------------------
// wpe_iter: block (bin, chunk).  The bin's series y[0, T) and the weights' lambda live in LDS.
// Thread (slice s, entry e) adds its entry of R (lower triangle) or p over t = t_first + s,
// + S, ... in float64, S = 256 / E slices; the slices of an entry are then added in slice
// order.  Cholesky with the pivot rule, one column per step, rows across threads.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float2 wpe_predict(const float2* sY, int t, int delay, int K,
                                              const float2* g) {
  float2 x = sY[t];
  for (int k = 0; k < K; ++k) {
    const int tt = t - delay - k;
    if (tt < 0) break;
    const float2 y = sY[tt], gk = g[k];  // x -= conj(g_k) y
    x.x = fmaf(-gk.x, y.x, x.x);
    x.x = fmaf(-gk.y, y.y, x.x);
    x.y = fmaf(-gk.x, y.y, x.y);
    x.y = fmaf(gk.y, y.x, x.y);
  }
  return x;
}

__global__ __launch_bounds__(256) void wpe_iter_kernel(
    const float2* __restrict__ Y, const WpeChunk* __restrict__ chunks, int K, int delay, int it,
    const double2* __restrict__ g_prev, double2* __restrict__ g_out,
    unsigned* __restrict__ max_bits, int max_stride, float2* __restrict__ X) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wpe_lds[];
  __shared__ double2 sPart[256];
  __shared__ double2 sR[kWpeMaxTaps * kWpeMaxTaps];
  __shared__ double2 sP[kWpeMaxTaps], sG[kWpeMaxTaps];
  __shared__ double sDiag[kWpeMaxTaps];
  __shared__ float2 sG32[kWpeMaxTaps];
  const WpeChunk c = chunks[blockIdx.y];
  const int bin = blockIdx.x, T = c.T, tid = threadIdx.x;
  float2* sY = reinterpret_cast<float2*>(wpe_lds);
  float* sLam = reinterpret_cast<float*>(wpe_lds + (size_t)8 * T);
  const float2* y = Y + c.spec_off + (long)bin * T;
  for (int t = tid; t < T; t += 256) sY[t] = y[t];
  const long gi = ((long)c.index * kWpeBins + bin) * K;
  const bool have_prev = g_prev != nullptr;
  if (tid < K) {
    const double2 gp = have_prev ? g_prev[gi + tid] : make_double2(0.0, 0.0);
    sG32[tid] = make_float2((float)gp.x, (float)gp.y);
  }
  const float mx = __uint_as_float(max_bits[(long)c.index * max_stride + it]);
  const float eps = __fmul_rn(1e-10f, mx);
  __syncthreads();
  if (!(mx > 0.f)) {  // an all-zero chunk: g = 0, x = y = 0
    if (tid < K) g_out[gi + tid] = make_double2(0.0, 0.0);
    if (X)
      for (int t = tid; t < T; t += 256) X[c.spec_off + (long)t * kWpeBins + bin] = sY[t];
    return;
  }
  for (int t = tid; t < T; t += 256) {
    const float2 x = have_prev ? wpe_predict(sY, t, delay, K, sG32) : sY[t];
    sLam[t] = fmaxf(norm2f(x), eps);
  }
  __syncthreads();
  // entries: e < nR the lower triangle (i, j), j <= i, row by row; then p_k
  const int nR = K * (K + 1) / 2, E = nR + K, S = 256 / E;
  {
    const int s = tid / E, e = tid - s * E;
    double2 acc = make_double2(0.0, 0.0);
    if (s < S) {
      int i = 0, j = 0;
      const bool isR = e < nR;
      if (isR) {
        while ((i + 1) * (i + 2) / 2 <= e) ++i;
        j = e - i * (i + 1) / 2;
      } else {
        i = e - nR;
      }
      // R_ij = sum y[t - delay - i] conj(y[t - delay - j]) / lambda_t (t >= delay + i);
      // p_i = sum y[t - delay - i] conj(y[t]) / lambda_t
      for (int t = delay + i + s; t < T; t += S) {
        const float lam = sLam[t];
        const double wgt = lam > 0.f ? 1.0 / (double)lam : 0.0;
        const float2 a = sY[t - delay - i], b = isR ? sY[t - delay - j] : sY[t];
        const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
        acc.x += (ax * bx + ay * by) * wgt;
        acc.y += (ay * bx - ax * by) * wgt;
      }
      sPart[s * E + e] = acc;
    }
  }
  __syncthreads();
  if (tid < E) {
    double2 tot = sPart[tid];
    for (int s = 1; s < S; ++s) {
      tot.x += sPart[s * E + tid].x;
      tot.y += sPart[s * E + tid].y;
    }
    if (tid < nR) {
      int i = 0;
      while ((i + 1) * (i + 2) / 2 <= tid) ++i;
      const int j = tid - i * (i + 1) / 2;
      if (i == j) tot.y = 0.0;
      sR[i * K + j] = tot;
    } else {
      sP[tid - nR] = tot;
    }
  }
  __syncthreads();
  double maxdiag = 0.0;
  for (int k = 0; k < K; ++k) maxdiag = fmax(maxdiag, sR[k * K + k].x);
  const double tol = 1e-12 * maxdiag;
  // L overwrites R's strict lower triangle, its diagonal goes to sDiag; a rejected pivot
  // leaves a zero column (the tap is removed)
  for (int j = 0; j < K; ++j) {
    double d = sR[j * K + j].x;
    for (int k = 0; k < j; ++k) {
      const double2 l = sR[j * K + k];
      d -= l.x * l.x + l.y * l.y;
    }
    const bool ok = d > tol;
    const double dj = ok ? sqrt(d) : 0.0;
    if (tid > j && tid < K) {
      double2 v = sR[tid * K + j];
      for (int k = 0; k < j; ++k) {  // v -= L_ik conj(L_jk)
        const double2 a = sR[tid * K + k], b = sR[j * K + k];
        v.x -= a.x * b.x + a.y * b.y;
        v.y -= a.y * b.x - a.x * b.y;
      }
      sR[tid * K + j] = ok ? make_double2(v.x / dj, v.y / dj) : make_double2(0.0, 0.0);
    }
    if (tid == 0) sDiag[j] = dj;
    __syncthreads();
  }
  if (tid == 0) {
    // L z = p, then L^H g = z, over the kept taps
    for (int j = 0; j < K; ++j) {
      double2 v = sP[j];
      for (int k = 0; k < j; ++k) {
        const double2 l = sR[j * K + k], z = sG[k];
        v.x -= l.x * z.x - l.y * z.y;
        v.y -= l.x * z.y + l.y * z.x;
      }
      const double dj = sDiag[j];
      sG[j] = dj > 0.0 ? make_double2(v.x / dj, v.y / dj) : make_double2(0.0, 0.0);
    }
    for (int j = K - 1; j >= 0; --j) {
      double2 v = sG[j];
      for (int i = j + 1; i < K; ++i) {  // v -= conj(L_ij) g_i
        const double2 l = sR[i * K + j], gg = sG[i];
        v.x -= l.x * gg.x + l.y * gg.y;
        v.y -= l.x * gg.y - l.y * gg.x;
      }
      const double dj = sDiag[j];
      sG[j] = dj > 0.0 ? make_double2(v.x / dj, v.y / dj) : make_double2(0.0, 0.0);
    }
  }
  __syncthreads();
  if (tid < K) {
    const double2 gk = sG[tid];
    g_out[gi + tid] = gk;
    sG32[tid] = make_float2((float)gk.x, (float)gk.y);
  }
  __syncthreads();
  float m = 0.f;
  for (int t = tid; t < T; t += 256) {
    const float2 x = wpe_predict(sY, t, delay, K, sG32);
    m = fmaxf(m, norm2f(x));
    if (X) X[c.spec_off + (long)t * kWpeBins + bin] = x;
  }
  m = wave_max(m);
  if ((tid & 63) == 0)
    atomicMax(&max_bits[(long)c.index * max_stride + it + 1], __float_as_uint(m));
}

// ---------------------------------------------------------------------------------------
// wpe_istft: block (tile of 13 output blocks of 128 samples, chunk).  Output block ob (samples
// 128 ob ..) is the sum of frames ob .. ob + 3, so the tile inverts frames ob0 .. ob0 + 15 into
// LDS (times the synthesis window) and each output sample gathers its four frames in frame order.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wpe_istft_kernel(const float2* __restrict__ X,
                                                        const WpeChunk* __restrict__ chunks,
                                                        WpeTables tabs, float* __restrict__ out) {
  __shared__ float2 sTw[256];
  __shared__ float sSyn[kWpeFft];
  __shared__ float2 sA[4][256], sB[4][256];
  __shared__ float sF[kWpeIstftTile][kWpeFft];
  const WpeChunk c = chunks[blockIdx.y];
  const int ob0 = blockIdx.x * kWpeIstftOut;
  if ((long)ob0 * kWpeHop >= c.n) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  sTw[tid] = tabs.twiddle[tid];
  sSyn[tid] = tabs.synth[tid];
  sSyn[tid + 256] = tabs.synth[tid + 256];
  __syncthreads();
  float2* A = sA[w];
  float2* B = sB[w];
  for (int fi = w; fi < kWpeIstftTile; fi += 4) {
    const int t = ob0 + fi;
    const bool live = t < c.T;
    const float2* Xr = X + c.spec_off + (long)(live ? t : 0) * kWpeBins;
    // Z = E + i O with E = (X_k + conj X_{256-k}) / 2, O = (X_k - conj X_{256-k}) / 2 * conj W^k;
    // z = IFFT256(Z) = conj(FFT256(conj Z)) / 256, x[2n] = Re z[n], x[2n+1] = Im z[n]
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kb = lane + 64 * q;
      float2 xk = live ? Xr[kb] : make_float2(0.f, 0.f);
      float2 xm = live ? Xr[256 - kb] : make_float2(0.f, 0.f);
      if (kb == 0) xk.y = 0.f, xm.y = 0.f;  // irfft reads no imaginary part at DC and Nyquist
      xm.y = -xm.y;
      const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y + xm.y));
      const float2 D = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y - xm.y));
      const float2 tw = sTw[kb];
      const float2 O = cmulf(D, make_float2(tw.x, -tw.y));
      A[kb] = make_float2(E.x - O.y, -(E.y + O.x));
    }
    __syncthreads();
    fft256(A, B, sTw, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = lane + 64 * q;
      const float2 z = A[n];
      sF[fi][2 * n] = (z.x * (1.f / 256.f)) * sSyn[2 * n];
      sF[fi][2 * n + 1] = (-z.y * (1.f / 256.f)) * sSyn[2 * n + 1];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < kWpeIstftOut * kWpeHop; idx += 256) {
    const int ob = idx >> 7, r = idx & 127;
    const long n = (long)(ob0 + ob) * kWpeHop + r;
    if (n < c.n) {
      float v = sF[ob][384 + r];
      v = __fadd_rn(v, sF[ob + 1][256 + r]);
      v = __fadd_rn(v, sF[ob + 2][128 + r]);
      v = __fadd_rn(v, sF[ob + 3][r]);
      out[c.out_off + n] = v;
    }
  }
}

}  // namespace

void launch_wpe_stft(const float* signal, const WpeChunk* chunks, int n_chunks, int max_T,
                     const WpeTables& tabs, float2* Y, unsigned* max_bits, int max_stride,
                     hipStream_t st) {
  if (n_chunks <= 0 || max_T <= 0) return;
  ZASR_REQUIRE(n_chunks <= 65535, "WPE: at most 65535 chunks per launch group");
  ZASR_LAUNCH(wpe_stft_kernel, dim3(cdiv(max_T, kWpeStftTile), n_chunks), dim3(256), 0, st, signal,
              chunks, tabs, Y, max_bits, max_stride);
}

size_t wpe_iter_lds_bytes(int T, int /*taps*/) { return (size_t)12 * T; }

void launch_wpe_iter(const float2* Y, const WpeChunk* chunks, int n_chunks, int max_T, int taps,
                     int delay, int it, const double2* g_prev, double2* g, unsigned* max_bits,
                     int max_stride, float2* X, hipStream_t st) {
  if (n_chunks <= 0 || max_T <= 0) return;
  ZASR_REQUIRE(n_chunks <= 65535, "WPE: at most 65535 chunks per launch group");
  ZASR_REQUIRE(taps >= 1 && taps <= kWpeMaxTaps && delay >= 1 && delay <= kWpeMaxDelay,
               "WPE: taps and delay must be in 1..16");
  ZASR_REQUIRE(max_T <= wpe_frames(kWpeMaxSamples), "WPE: a chunk is at most 60 s");
  static bool attr = false;
  if (!attr) {  // 90 KB of dynamic LDS at the 60 s cap
    ZASR_HIP_CHECK(hipFuncSetAttribute((const void*)wpe_iter_kernel,
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)wpe_iter_lds_bytes((int)wpe_frames(kWpeMaxSamples), 0)));
    attr = true;
  }
  ZASR_LAUNCH(wpe_iter_kernel, dim3(kWpeBins, n_chunks), dim3(256), wpe_iter_lds_bytes(max_T, taps),
              st, Y, chunks, taps, delay, it, g_prev, g, max_bits, max_stride, X);
}

void launch_wpe_istft(const float2* X, const WpeChunk* chunks, int n_chunks, long max_n,
                      const WpeTables& tabs, float* out, hipStream_t st) {
  if (n_chunks <= 0 || max_n <= 0) return;
  ZASR_REQUIRE(n_chunks <= 65535, "WPE: at most 65535 chunks per launch group");
  const int tiles = (int)cdivl(max_n, (long)kWpeIstftOut * kWpeHop);
  ZASR_LAUNCH(wpe_istft_kernel, dim3(tiles, n_chunks), dim3(256), 0, st, X, chunks, tabs, out);
}

}  // namespace zasr
