// Kernels of the community-1 speaker-embedding stage: the WeSpeaker ResNet34's
// convolutions as implicit GEMMs on the exact-f32 MFMA, its stem, the masked statistics pooling
// and the frame-feature transpose of the API.  Activations are channels-last [n][F][T][C]
// (F = frequency bins, T = frames), so the K axis of a convolution, k = (r ks + q) Ci + ci, is
// contiguous in runs of Ci and a 32-wide K chunk never straddles a tap.
#include "common.h"
#include "emb.h"

namespace zasr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// =====================================================================================
// emb_conv2d_kernel: O^T[co][m] = sum_k W[co][k] X^T[k][m] on v_mfma_f32_16x16x4_f32, m the flat
// output position (n, fo, to).  A block of 4 waves owns 128 positions x BN = 16 NT channels; a
// wave 32 positions x BN channels as 2 x NT tiles of 16 x 16 (2 NT independent accumulators).
// Per 32-wide K chunk (one tap, 32 input channels) the block stages X rows [128][32] and W rows
// [BN][32] in LDS (row stride 36 floats: the b128 fragment reads of 16 rows hit 16 distinct
// 4-bank groups), double-buffered, the next chunk's global loads issued before the current
// chunk's MFMAs.  A lane reads float4 k = 4 (l >> 4) + j of a row and feeds element j to MFMA j
// of a group of four, so the chunk's k order is a fixed permutation, the same for both operands:
// every output is one fmaf chain over K whose order depends on nothing but the layer.
// The channels are the MFMA's rows, so a lane ends with 4 consecutive channels of one position:
// bias, residual and store are float4s.
// =====================================================================================
constexpr int kEmbBM = 128;     // positions per block
constexpr int kEmbKC = 32;      // K chunk
constexpr int kEmbLd = 36;      // LDS row stride (floats)

template <int NT>
__global__ __launch_bounds__(256) void emb_conv2d_kernel(EmbConv2d a) {
  constexpr int BN = 16 * NT;
  constexpr int WPT = BN / 32;  // weight float4s per thread and chunk
  __shared__ float sX[2][kEmbBM * kEmbLd];
  __shared__ float sW[2][BN * kEmbLd];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long M = (long)a.n * a.Fo * a.To;
  const long m0 = (long)blockIdx.x * kEmbBM;
  const int co0 = blockIdx.y * BN;
  const int pad = a.ks == 3 ? 1 : 0;
  // this thread's 4 staging positions (rows tid >> 3 + 32 i), column float4 tid & 7
  const int c4 = tid & 7;
  long xbase[4];
  int fi0[4], ti0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long m = m0 + (tid >> 3) + 32 * i;
    if (m < M) {
      const int to = (int)(m % a.To);
      const long r = m / a.To;
      const int fo = (int)(r % a.Fo);
      const long n = r / a.Fo;
      fi0[i] = fo * a.stride - pad;
      ti0[i] = to * a.stride - pad;
      xbase[i] = n * a.Fi * a.Ti;
    } else {
      fi0[i] = -(1 << 20);  // every tap out of range: zeros
      ti0[i] = 0;
      xbase[i] = 0;
    }
  }
  const int cpt = a.Ci / kEmbKC;           // chunks per tap
  const int nchunk = a.ks * a.ks * cpt;
  const int K = a.ks * a.ks * a.Ci;
  float4 rx[4], rw[WPT];
  auto gload = [&](int ch) {
    const int tap = ch / cpt, ci0 = (ch - tap * cpt) * kEmbKC;
    const int r = tap / a.ks, q = tap - r * a.ks;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int fi = fi0[i] + r, ti = ti0[i] + q;
      const bool ok = fi >= 0 && fi < a.Fi && ti >= 0 && ti < a.Ti;
      rx[i] = ok ? *reinterpret_cast<const float4*>(
                       a.x + ((xbase[i] + (long)fi * a.Ti + ti) * a.Ci + ci0 + c4 * 4))
                 : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int row = (tid >> 3) + 32 * i;  // < BN
      rw[i] = *reinterpret_cast<const float4*>(a.w + (long)(co0 + row) * K + (long)tap * a.Ci +
                                               ci0 + c4 * 4);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<float4*>(&sX[buf][((tid >> 3) + 32 * i) * kEmbLd + c4 * 4]) = rx[i];
#pragma unroll
    for (int i = 0; i < WPT; ++i)
      *reinterpret_cast<float4*>(&sW[buf][((tid >> 3) + 32 * i) * kEmbLd + c4 * 4]) = rw[i];
  };
  f32x4 acc[NT][2];
#pragma unroll
  for (int c = 0; c < NT; ++c)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};
  gload(0);
  lstore(0);
  __syncthreads();
  const int frow = lane & 15, fk = (lane >> 4) * 4;
  for (int ch = 0; ch < nchunk; ++ch) {
    const int buf = ch & 1;
    if (ch + 1 < nchunk) gload(ch + 1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // 16 k per half chunk
      float4 xf[2], wf[NT];
#pragma unroll
      for (int p = 0; p < 2; ++p)
        xf[p] = *reinterpret_cast<const float4*>(
            &sX[buf][(wv * 32 + p * 16 + frow) * kEmbLd + h * 16 + fk]);
#pragma unroll
      for (int c = 0; c < NT; ++c)
        wf[c] = *reinterpret_cast<const float4*>(&sW[buf][(c * 16 + frow) * kEmbLd + h * 16 + fk]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const float wj = j == 0 ? wf[c].x : j == 1 ? wf[c].y : j == 2 ? wf[c].z : wf[c].w;
            const float xj = j == 0 ? xf[p].x : j == 1 ? xf[p].y : j == 2 ? xf[p].z : xf[p].w;
            acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(wj, xj, acc[c][p], 0, 0, 0);
          }
    }
    if (ch + 1 < nchunk) {
      lstore(buf ^ 1);  // last read two iterations ago, before the previous barrier
      __syncthreads();
    }
  }
  // D[row = channel 4 (l >> 4) + reg][col = position l & 15]
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const long m = m0 + wv * 32 + p * 16 + (lane & 15);
    if (m >= M) continue;
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      const int co = co0 + c * 16 + (lane >> 4) * 4;
      const float4 b = *reinterpret_cast<const float4*>(a.bias + co);
      float4 v = make_float4(acc[c][p][0] + b.x, acc[c][p][1] + b.y, acc[c][p][2] + b.z,
                             acc[c][p][3] + b.w);
      if (a.res) {
        const float4 r = *reinterpret_cast<const float4*>(a.res + m * a.Co + co);
        v.x += r.x;
        v.y += r.y;
        v.z += r.z;
        v.w += r.w;
      }
      if (a.relu) {
        v.x = fmaxf(v.x, 0.f);
        v.y = fmaxf(v.y, 0.f);
        v.z = fmaxf(v.z, 0.f);
        v.w = fmaxf(v.w, 0.f);
      }
      *reinterpret_cast<float4*>(a.y + m * a.Co + co) = v;
    }
  }
}

int emb_conv2d_routes(int Co) { return Co >= 64 ? 2 : 1; }

void launch_emb_conv2d(const EmbConv2d& a, int route, hipStream_t st) {
  ZASR_REQUIRE(a.ks == 1 || a.ks == 3, "emb conv2d: kernel 1 or 3");
  ZASR_REQUIRE(a.stride == 1 || a.stride == 2, "emb conv2d: stride 1 or 2");
  auto okc = [](int c) { return c == 32 || c == 64 || c == 128 || c == 256; };
  ZASR_REQUIRE(okc(a.Ci) && okc(a.Co), "emb conv2d: Ci, Co in {32, 64, 128, 256}");
  ZASR_REQUIRE(a.n >= 1 && a.Fi >= 1 && a.Ti >= 1, "emb conv2d: empty input");
  ZASR_REQUIRE(a.Fo == (a.Fi - 1) / a.stride + 1 && a.To == (a.Ti - 1) / a.stride + 1,
               "emb conv2d: output size");
  ZASR_REQUIRE(route >= 0 && route <= emb_conv2d_routes(a.Co), "emb conv2d: no such route");
  const long M = (long)a.n * a.Fo * a.To;
  ZASR_REQUIRE(cdivl(M, kEmbBM) <= INT32_MAX, "emb conv2d: too many positions");
  // route 1: 32 channels per block; route 2: 64 (the X fragments feed twice the MFMAs)
  const int r = route ? route : emb_conv2d_routes(a.Co);
  const dim3 grid((unsigned)cdivl(M, kEmbBM), (unsigned)(a.Co / (r == 2 ? 64 : 32)));
  if (r == 2) ZASR_LAUNCH(emb_conv2d_kernel<4>, grid, dim3(256), 0, st, a);
  else ZASR_LAUNCH(emb_conv2d_kernel<2>, grid, dim3(256), 0, st, a);
}

// =====================================================================================
// The stem: Conv2d(1, Co, 3, pad 1) on x [n][T][F] (the fbank rows), output [n][F][T][Co], ReLU.
// One thread per (position, channel), channels fastest; the 9 taps in (r, q) order.
// =====================================================================================
__global__ __launch_bounds__(256) void emb_stem_kernel(const float* __restrict__ x,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ bias, int n,
                                                       int T, int F, int Co,
                                                       float* __restrict__ y) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)n * F * T * Co;
  if (i >= total) return;
  const int co = (int)(i % Co);
  long m = i / Co;
  const int t = (int)(m % T);
  m /= T;
  const int f = (int)(m % F);
  const long b = m / F;
  float acc = 0.f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int ff = f + r - 1, tt = t + q - 1;
      const float v = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? x[(b * T + tt) * F + ff] : 0.f;
      acc = fmaf(w[co * 9 + r * 3 + q], v, acc);
    }
  y[i] = fmaxf(acc + bias[co], 0.f);
}

void launch_emb_stem(const float* x, const float* w, const float* bias, int n, int T, int F,
                     int Co, float* y, hipStream_t st) {
  const long total = (long)n * F * T * Co;
  if (total <= 0) return;
  ZASR_REQUIRE(cdivl(total, 256) <= INT32_MAX, "emb stem: too many outputs");
  ZASR_LAUNCH(emb_stem_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, st, x, w, bias, n,
              T, F, Co, y);
}

// =====================================================================================
// Masked statistics pooling (core/speaker_diarization_pure_ort.py:856-871): one block per
// (sample, frequency bin), a thread per channel, the S speakers of the sample together so the
// features are read once per pass.  Sums over the frames in frame order in float64, every value
// numpy holds in float32 rounded to float32 where numpy rounds it.  pop: no mask, population
// variance (:701-705).  stats[(n S + s)][j] = mean, [D + j] = std, j = c F + f.
// =====================================================================================
constexpr int kPoolMaxS = 4;
constexpr int kPoolMaxT = 1024;

__global__ __launch_bounds__(256) void emb_pool_kernel(const float* __restrict__ x,
                                                       const unsigned char* __restrict__ mask,
                                                       int F, int T, int C, int S, int nseg,
                                                       int pop, float* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ float sWt[kPoolMaxS][kPoolMaxT];
  const int n = blockIdx.x / F, f = blockIdx.x % F;
  const int D = C * F;
  if (!pop) {  // the population form has no weights to stage, and so no bound on T
    for (int i = threadIdx.x; i < S * T; i += 256) {
      const int s = i / T, t = i - s * T;
      long idx = (long)t * nseg / T;
      if (idx > nseg - 1) idx = nseg - 1;
      sWt[s][t] = (float)mask[((long)n * S + s) * nseg + idx];
    }
  }
  __syncthreads();
  const float* xr = x + ((long)n * F + f) * T * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    double sw[kPoolMaxS], sw2[kPoolMaxS], sx[kPoolMaxS];
    for (int s = 0; s < S; ++s) sw[s] = sw2[s] = sx[s] = 0.0;
    for (int t = 0; t < T; ++t) {
      const float v = xr[(long)t * C + c];
      for (int s = 0; s < S; ++s) {
        const float wv = pop ? 1.f : sWt[s][t];
        sw[s] += wv;
        sw2[s] += (double)(wv * wv);
        sx[s] += (double)(v * wv);
      }
    }
    float mean[kPoolMaxS], den[kPoolMaxS];
    for (int s = 0; s < S; ++s) {
      if (pop) {
        mean[s] = (float)(sx[s] / T);
        den[s] = (float)T;
      } else {
        const float v1 = (float)sw[s] + 1e-8f;
        mean[s] = (float)sx[s] / v1;
        den[s] = v1 - (float)sw2[s] / v1 + 1e-8f;
      }
    }
    double sd[kPoolMaxS];
    for (int s = 0; s < S; ++s) sd[s] = 0.0;
    for (int t = 0; t < T; ++t) {
      const float v = xr[(long)t * C + c];
      for (int s = 0; s < S; ++s) {
        const float d = v - mean[s];
        const float d2 = d * d;
        sd[s] += (double)(d2 * (pop ? 1.f : sWt[s][t]));
      }
    }
    for (int s = 0; s < S; ++s) {
      float* o = stats + ((long)n * S + s) * 2 * D;
      const float var = pop ? (float)(sd[s] / T) : (float)sd[s] / den[s];
      o[c * F + f] = mean[s];
      o[D + c * F + f] = sqrtf(var);
    }
  }
}

void launch_emb_pool(const float* x, const unsigned char* mask, int n, int F, int T, int C, int S,
                     int nseg, bool pop, float* stats, hipStream_t st) {
  if (n <= 0) return;
  ZASR_REQUIRE(S >= 1 && S <= kPoolMaxS && T >= 1 && (pop || T <= kPoolMaxT) && F >= 1 && C >= 1,
               "emb pool: 1-4 speakers; the masked form takes 1-1024 frames");
  ZASR_REQUIRE(pop || (mask != nullptr && nseg >= 1), "emb pool: the masked form takes masks");
  ZASR_REQUIRE((long)n * F <= INT32_MAX, "emb pool: too many samples");
  ZASR_LAUNCH(emb_pool_kernel, dim3((unsigned)(n * F)), dim3(256), 0, st, x, mask, F, T, C, S,
              nseg, pop ? 1 : 0, stats);
}

// out[n][c F + f][t] = x[n][f][t][c]: the reference's frame-feature layout at the API
__global__ __launch_bounds__(256) void emb_to_cft_kernel(const float* __restrict__ x, long total,
                                                         int F, int T, int C,
                                                         float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int t = (int)(i % T);
  long r = i / T;
  const int j = (int)(r % ((long)C * F));
  const long n = r / ((long)C * F);
  const int c = j / F, f = j - c * F;
  out[i] = x[((n * F + f) * T + t) * C + c];
}

void launch_emb_to_cft(const float* x, int n, int F, int T, int C, float* out, hipStream_t st) {
  const long total = (long)n * F * T * C;
  if (total <= 0) return;
  ZASR_REQUIRE(cdivl(total, 256) <= INT32_MAX, "emb transpose: too many elements");
  ZASR_LAUNCH(emb_to_cft_kernel, dim3((unsigned)cdivl(total, 256)), dim3(256), 0, st, x, total, F,
              T, C, out);
}

}  // namespace zasr
