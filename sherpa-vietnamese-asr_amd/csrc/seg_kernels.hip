// PyanNet segmentation kernels other than the projections.  conv_1, conv_2, the
// LSTM input projections and the two 128-wide linears run on the exact-f32 MFMA GEMM
// (gemm.hip); here are the chunk gather + input InstanceNorm + sinc convolution + |.| + max-pool
// front kernel, the InstanceNorm statistics and their application, the batched bidirectional
// LSTM recurrence, and the classifier head.  All float32 (statistics float64): the output is
// an argmax and two > 0.5 thresholds.  Replaces the onnxruntime session call at
// core/speaker_diarization_senko_campp_optimized.py:435.
#include "common.h"
#include "seg.h"

namespace zasr {

namespace {
constexpr float kLeaky = 0.01f;
constexpr double kEps = 1e-5;

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : kLeaky * v; }
__device__ __forceinline__ float seg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ void lds_barrier_seg() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// sum of one double per thread over a 256-thread block, fixed tree; every thread gets the sum
__device__ __forceinline__ double block_sum_256(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  return red[0];
}
}  // namespace

// ---- input InstanceNorm statistics: one block per chunk ----
__global__ __launch_bounds__(256) void seg_chunk_stats_kernel(const float* __restrict__ audio,
                                                              long total,
                                                              const long* __restrict__ starts,
                                                              int T, float2* __restrict__ stats) {
  __shared__ double red[256];
  const int k = blockIdx.x, t = threadIdx.x;
  const long s0 = starts[k];
  long avail = total - s0;  // samples of the chunk that exist; the rest are zeros
  if (avail < 0) avail = 0;
  if (avail > T) avail = T;
  double s = 0.0;
  for (long i = t; i < avail; i += 256) s += (double)audio[s0 + i];
  const double mean = block_sum_256(s, red) / (double)T;
  double q = 0.0;
  for (long i = t; i < T; i += 256) {
    const double d = (i < avail ? (double)audio[s0 + i] : 0.0) - mean;
    q += d * d;
  }
  const double var = block_sum_256(q, red) / (double)T;
  if (t == 0) stats[k] = make_float2((float)mean, (float)(1.0 / sqrt(var + kEps)));
}

// ---- front: gather + normalise + conv_0 (80 x 251, stride 10) + |.| + MaxPool1d(3, 3) ----
// A block makes 64 pooled frames x 80 channels of one chunk.  The 64 * 30 + 241 normalised
// samples those frames read sit in LDS; lane = pooled frame, wave w = channels [20 w, 20 w + 20)
// in two passes of 10 with the taps read through wave-uniform (scalar) loads of the tap-major
// filter bank.  Taps accumulate in ascending order with one fma each.  The un-pooled
// activation never leaves registers; the pooled tile goes out through LDS in whole rows.
constexpr int kFrontP = 64;                                    // pooled frames per block
constexpr int kFrontSamples = (kFrontP * 3 - 1) * kSegStride0 + kSegTaps;  // 2161
constexpr int kFrontCB = 10;                                   // channels per pass

__global__ __launch_bounds__(256) void seg_front_kernel(SegFrontArgs a) {
  __shared__ float xs[kFrontSamples + 3];
  __shared__ float so[kFrontP][kSegC0 + 1];
  const int k = blockIdx.y, p0 = blockIdx.x * kFrontP, tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long s0 = a.starts[k];
  const float2 ms = a.stats[k];
  const long base = (long)p0 * 3 * kSegStride0;
  for (int i = tid; i < kFrontSamples; i += 256) {
    const long s = base + i;  // sample of the chunk
    float v = 0.f;            // past the chunk: read only by frames past F1, never stored
    if (s < a.T) {
      const long g = s0 + s;
      const float x = g < a.total ? a.audio[g] : 0.f;
      v = __fmaf_rn(__fmul_rn(__fsub_rn(x, ms.x), ms.y), a.in_w, a.in_b);
    }
    xs[i] = v;
  }
  __syncthreads();
  const float* xl = xs + lane * 3 * kSegStride0;
  for (int pass = 0; pass < 2; ++pass) {
    const int c0 = wave * 20 + pass * kFrontCB;
    const float* w = a.w0t + c0;
    float acc[kFrontCB][3];
#pragma unroll
    for (int c = 0; c < kFrontCB; ++c) acc[c][0] = acc[c][1] = acc[c][2] = 0.f;
#pragma unroll 2
    for (int q = 0; q < kSegTaps; ++q) {
      const float x0 = xl[q], x1 = xl[q + kSegStride0], x2 = xl[q + 2 * kSegStride0];
#pragma unroll
      for (int c = 0; c < kFrontCB; ++c) {
        const float wv = w[q * kSegC0 + c];
        acc[c][0] = __fmaf_rn(wv, x0, acc[c][0]);
        acc[c][1] = __fmaf_rn(wv, x1, acc[c][1]);
        acc[c][2] = __fmaf_rn(wv, x2, acc[c][2]);
      }
    }
#pragma unroll
    for (int c = 0; c < kFrontCB; ++c)
      so[lane][c0 + c] = fmaxf(fmaxf(fabsf(acc[c][0]), fabsf(acc[c][1])), fabsf(acc[c][2]));
  }
  __syncthreads();
  const int rows = min(kFrontP, a.F1 - p0);
  float* dst = a.out + ((long)k * a.F1 + p0) * kSegC0;
  for (int i = tid; i < rows * kSegC0; i += 256) dst[i] = so[i / kSegC0][i % kSegC0];
}

// ---- MaxPool1d(3, 3) over frames ----
__global__ void seg_pool3_kernel(const float* __restrict__ x, long nout4, int L, int C4, int Fp,
                                 float* __restrict__ out) {
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float4* o4 = reinterpret_cast<float4*>(out);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nout4;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const long r = i / C4;
    const long n = r / Fp;
    const int p = (int)(r - n * Fp);
    const float4* s = x4 + (n * L + 3L * p) * C4 + c;
    const float4 u = s[0], v = s[C4], w = s[2 * C4];
    o4[i] = make_float4(fmaxf(fmaxf(u.x, v.x), w.x), fmaxf(fmaxf(u.y, v.y), w.y),
                        fmaxf(fmaxf(u.z, v.z), w.z), fmaxf(fmaxf(u.w, v.w), w.w));
  }
}

// ---- InstanceNorm statistics over frames: one block per chunk, thread = (frame slot, channel) ----
// G = 256 / C frame slots; slot g sums frames g, g + G, ... in float64, the G partial sums
// add in slot order.  Two passes (mean, then centred squares).
__global__ __launch_bounds__(256) void seg_frame_stats_kernel(const float* __restrict__ x, int F,
                                                              int C, float2* __restrict__ stats) {
  __shared__ double part[256];
  __shared__ double smean[128];
  const int n = blockIdx.x, t = threadIdx.x;
  const int G = 256 / C, g = t / C, c = t - g * C;
  const float* xn = x + (long)n * F * C;
  double s = 0.0;
  if (g < G)
    for (int f = g; f < F; f += G) s += (double)xn[(long)f * C + c];
  part[t] = s;
  __syncthreads();
  if (t < C) {
    double m = 0.0;
    for (int i = 0; i < G; ++i) m += part[i * C + t];
    smean[t] = m / (double)F;
  }
  __syncthreads();
  double q = 0.0;
  if (g < G) {
    const double m = smean[c];
    for (int f = g; f < F; f += G) {
      const double d = (double)xn[(long)f * C + c] - m;
      q += d * d;
    }
  }
  part[t] = q;
  __syncthreads();
  if (t < C) {
    double v = 0.0;
    for (int i = 0; i < G; ++i) v += part[i * C + t];
    stats[(long)n * C + t] = make_float2((float)smean[t], (float)(1.0 / sqrt(v / (double)F + kEps)));
  }
}

// ---- normalise + affine + leaky_relu, in place ----
__global__ void seg_norm_act_kernel(float* __restrict__ x, long total4, int F, int C4,
                                    const float2* __restrict__ stats, const float* __restrict__ w,
                                    const float* __restrict__ b) {
  float4* x4 = reinterpret_cast<float4*>(x);
  const long per = (long)F * C4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total4;
       i += (long)gridDim.x * blockDim.x) {
    const long n = i / per;
    const int c = (int)(i % C4) * 4;
    const float2* s = stats + n * (C4 * 4) + c;
    float4 v = x4[i];
    v.x = leaky(__fmaf_rn(__fmul_rn(__fsub_rn(v.x, s[0].x), s[0].y), w[c], b[c]));
    v.y = leaky(__fmaf_rn(__fmul_rn(__fsub_rn(v.y, s[1].x), s[1].y), w[c + 1], b[c + 1]));
    v.z = leaky(__fmaf_rn(__fmul_rn(__fsub_rn(v.z, s[2].x), s[2].y), w[c + 2], b[c + 2]));
    v.w = leaky(__fmaf_rn(__fmul_rn(__fsub_rn(v.w, s[3].x), s[3].y), w[c + 3], b[c + 3]));
    x4[i] = v;
  }
}

// ---- the recurrence: B sequences of one direction per workgroup ----
// 512 threads = 4 x 128 gate rows (torch order i, f, g, o; a wave holds rows of one gate), one
// W_hh row (128 floats) per thread in VGPRs as in vad_lstm_kernel.  The B hidden vectors sit in
// LDS; per step every thread makes its row's dot product with each of them (the same k order
// and the same instructions for every sequence, whatever B and its slot: two packed
// accumulators over ascending k, summed (x + y) + (z + w)), then the 128 B cells update on
// threads (slot = j / 128 + 4 i, unit = j % 128).  Two LDS-only barriers per step for B
// sequences; the next step's gx rows are loaded before the first of them and the h stores to
// HBM are never waited on.  Blocks [0, groups) walk frames upwards and write columns
// [0, 128), blocks [groups, 2 groups) walk downwards and write [128, 256).
template <int B>
__global__ __launch_bounds__(512) void seg_lstm_kernel(SegLstmArgs a, int groups) {
  constexpr int H = kSegH;
  constexpr int CI = (B + 3) / 4;  // cells per thread
  typedef float f2 __attribute__((ext_vector_type(2)));
  __shared__ float4 sh4[B][H / 4];
  __shared__ float sg[B][4 * H];
  const int j = threadIdx.x;
  const int dir = blockIdx.x >= groups ? 1 : 0;
  const int s0 = (blockIdx.x - dir * groups) * B;
  const int nb = min(B, a.n - s0);
  const int F = a.F;
  f2 wr[H / 2];
  {
    const float4* r = reinterpret_cast<const float4*>(a.whh + ((long)dir * 4 * H + j) * H);
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
      const float4 v = r[q];
      wr[2 * q] = f2{v.x, v.y};
      wr[2 * q + 1] = f2{v.z, v.w};
    }
  }
  const int gate = j >> 7, unit = j & (H - 1);
  float c[CI];
#pragma unroll
  for (int i = 0; i < CI; ++i) c[i] = 0.f;
  for (int i = j; i < B * H; i += 512) reinterpret_cast<float*>(sh4)[i] = 0.f;
  const float* gxd = a.gx + dir * 4 * H + j;
  float gnext[B];
#pragma unroll
  for (int b = 0; b < B; ++b) {
    const int tt = dir ? F - 1 : 0;
    gnext[b] = b < nb ? gxd[((long)(s0 + b) * F + tt) * (8 * H)] : 0.f;
  }
  lds_barrier_seg();
  for (int t = 0; t < F; ++t) {
    const int tt = dir ? F - 1 - t : t;
    float gcur[B];
#pragma unroll
    for (int b = 0; b < B; ++b) gcur[b] = gnext[b];
    if (t + 1 < F) {
      const int tn = dir ? tt - 1 : tt + 1;
#pragma unroll
      for (int b = 0; b < B; ++b)
        if (b < nb) gnext[b] = gxd[((long)(s0 + b) * F + tn) * (8 * H)];
    }
#pragma unroll
    for (int b = 0; b < B; ++b) {
      if (b < nb) {
        f2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
        for (int q = 0; q < H / 4; ++q) {
          const float4 hv = sh4[b][q];
          acc0 = __builtin_elementwise_fma(wr[2 * q], f2{hv.x, hv.y}, acc0);
          acc1 = __builtin_elementwise_fma(wr[2 * q + 1], f2{hv.z, hv.w}, acc1);
        }
        const float pre =
            __fadd_rn(gcur[b], __fadd_rn(__fadd_rn(acc0.x, acc0.y), __fadd_rn(acc1.x, acc1.y)));
        sg[b][j] = gate == 2 ? tanhf(pre) : seg_sigmoid(pre);
      }
    }
    lds_barrier_seg();
#pragma unroll
    for (int i = 0; i < CI; ++i) {
      const int b = gate + 4 * i;
      if (b < nb) {
        c[i] = __fmaf_rn(sg[b][H + unit], c[i], __fmul_rn(sg[b][unit], sg[b][2 * H + unit]));
        const float h = __fmul_rn(sg[b][3 * H + unit], tanhf(c[i]));
        reinterpret_cast<float*>(sh4[b])[unit] = h;
        a.out[((long)(s0 + b) * F + tt) * (2 * H) + dir * H + unit] = h;
      }
    }
    lds_barrier_seg();
  }
}

// ---- head: Linear(128, 7) + log_softmax + argmax, one frame per thread ----
__global__ __launch_bounds__(256) void seg_head_kernel(const float* __restrict__ x, long rows,
                                                       const float* __restrict__ w,
                                                       const float* __restrict__ b,
                                                       float* __restrict__ logits,
                                                       unsigned char* __restrict__ classes) {
  constexpr int H = kSegH, NC = kSegClasses;
  __shared__ float4 sw[NC][H / 4];
  __shared__ float sb[NC];
  for (int i = threadIdx.x; i < NC * H; i += 256) reinterpret_cast<float*>(sw)[i] = w[i];
  if (threadIdx.x < NC) sb[threadIdx.x] = b[threadIdx.x];
  __syncthreads();
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float4* xr = reinterpret_cast<const float4*>(x + r * H);
  float acc[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0.f;
  for (int q = 0; q < H / 4; ++q) {
    const float4 v = xr[q];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      const float4 u = sw[k][q];
      acc[k] = __fmaf_rn(v.w, u.w, __fmaf_rn(v.z, u.z, __fmaf_rn(v.y, u.y, __fmaf_rn(v.x, u.x, acc[k]))));
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    acc[k] = __fadd_rn(acc[k], sb[k]);
    m = fmaxf(m, acc[k]);
  }
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) se += expf(acc[k] - m);
  const float lse = logf(se);
  int best = 0;
  float bv = 0.f;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const float o = __fsub_rn(__fsub_rn(acc[k], m), lse);
    logits[r * NC + k] = o;
    if (k == 0 || o > bv) {  // strict: the lowest index wins a tie, as numpy's argmax
      bv = o;
      best = k;
    }
  }
  classes[r] = (unsigned char)best;
}

// ---- launchers ----
void launch_seg_chunk_stats(const float* audio, long total, const long* starts, int n, int T,
                            float2* stats, hipStream_t st) {
  if (n <= 0) return;
  ZASR_LAUNCH(seg_chunk_stats_kernel, dim3(n), dim3(256), 0, st, audio, total, starts, T, stats);
}

void launch_seg_front(const SegFrontArgs& a, int n, hipStream_t st) {
  if (n <= 0 || a.F1 <= 0) return;
  ZASR_REQUIRE(n <= 65535, "segmentation: more than 65535 chunks in one launch group");
  ZASR_LAUNCH(seg_front_kernel, dim3(cdiv(a.F1, kFrontP), n), dim3(256), 0, st, a);
}

namespace {
// blocks of a grid-stride launch over `items` float4s: one thread each up to 65536 blocks, or
// at most max_blocks when the caller caps it (the kernel-level tests: several passes per thread)
unsigned stride_grid(long items, int max_blocks) {
  return (unsigned)std::min<long>(cdivl(items, 256), max_blocks > 0 ? max_blocks : 1 << 16);
}
}  // namespace

void launch_seg_pool3(const float* x, int n, int L, int C, int Fp, float* out, hipStream_t st,
                      int max_blocks) {
  ZASR_REQUIRE(C % 4 == 0 && 3L * Fp <= L, "segmentation: bad pooling geometry");
  const long n4 = (long)n * Fp * (C / 4);
  if (n4 <= 0) return;
  ZASR_LAUNCH(seg_pool3_kernel, dim3(stride_grid(n4, max_blocks)), dim3(256), 0, st, x, n4, L, C / 4,
              Fp, out);
}

void launch_seg_frame_stats(const float* x, int n, int F, int C, float2* stats, hipStream_t st) {
  ZASR_REQUIRE(C > 0 && C <= 128 && F > 0, "segmentation: bad InstanceNorm geometry");
  if (n <= 0) return;
  ZASR_LAUNCH(seg_frame_stats_kernel, dim3(n), dim3(256), 0, st, x, F, C, stats);
}

void launch_seg_norm_act(float* x, int n, int F, int C, const float2* stats, const float* w,
                         const float* b, hipStream_t st, int max_blocks) {
  ZASR_REQUIRE(C % 4 == 0, "segmentation: channels must be a multiple of 4");
  const long n4 = (long)n * F * (C / 4);
  if (n4 <= 0) return;
  ZASR_LAUNCH(seg_norm_act_kernel, dim3(stride_grid(n4, max_blocks)), dim3(256), 0, st, x, n4, F,
              C / 4, stats, w, b);
}

void launch_seg_lstm(const SegLstmArgs& a, int group, hipStream_t st) {
  if (a.n <= 0 || a.F <= 0) return;
  const int groups = cdiv(a.n, group);
  const dim3 grid(2 * groups), block(512);
  switch (group) {
    case 1: ZASR_LAUNCH(seg_lstm_kernel<1>, grid, block, 0, st, a, groups); return;
    case 2: ZASR_LAUNCH(seg_lstm_kernel<2>, grid, block, 0, st, a, groups); return;
    case 4: ZASR_LAUNCH(seg_lstm_kernel<4>, grid, block, 0, st, a, groups); return;
    case 8: ZASR_LAUNCH(seg_lstm_kernel<8>, grid, block, 0, st, a, groups); return;
    case 16: ZASR_LAUNCH(seg_lstm_kernel<16>, grid, block, 0, st, a, groups); return;
    default: break;
  }
  throw std::runtime_error("zasr: segmentation recurrence group must be 1, 2, 4, 8 or 16");
}

void launch_seg_head(const float* x, long rows, const float* w, const float* b, float* logits,
                     unsigned char* classes, hipStream_t st) {
  if (rows <= 0) return;
  ZASR_LAUNCH(seg_head_kernel, dim3((unsigned)cdivl(rows, 256)), dim3(256), 0, st, x, rows, w, b,
              logits, classes);
}

}  // namespace zasr
