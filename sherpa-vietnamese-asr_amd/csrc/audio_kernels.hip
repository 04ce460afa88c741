// Kernels of the device audio front end (audio.h): convert + downmix + polyphase resample in
// one pass, and the level conditioning passes over the 16 kHz signal.  All of them are memory
// bound; none uses a floating-point atomic, so every result is bit-identical from run to run.
#include "audio.h"
#include "common.h"

namespace zasr {
namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float sample_f32(const float* p, long i) { return p[i]; }
__device__ __forceinline__ float sample_f32(const short* p, long i) {
  return (float)p[i] * 0x1p-15f;  // exact; soundfile's dtype='float32' read of PCM_16
}

// mean over the C channels of one frame held in e[0..C): f32 running sum in channel order,
// one f32 divide -- numpy's audio.mean(axis=1), core/asr_engine.py:500, bit for bit for
// C < 8.  At C = 8 numpy sums in an unrolled order of its own, so no running sum equals it;
// there the sum is taken in float64 (exact while the eight exponents lie within 27 of each
// other) and rounded once: the float64 mean to half an ulp, however the channels cancel.
template <int C>
__device__ __forceinline__ float mix(const float* e) {
  if constexpr (C == 8) {
    double s = (double)e[0];
#pragma unroll
    for (int c = 1; c < 8; ++c) s += (double)e[c];
    return (float)s / 8.f;
  } else {
    float s = e[0];
#pragma unroll
    for (int c = 1; c < C; ++c) s += e[c];
    return C == 1 ? s : s / (float)C;
  }
}

// frame f of the window (f relative to its first frame), any channel count
template <class S>
__device__ __forceinline__ float frame_scalar(const S* src, long f, int channels) {
  const long b = f * channels;
  if (channels == 8) {
    double s = (double)sample_f32(src, b);
    for (int c = 1; c < 8; ++c) s += (double)sample_f32(src, b + c);
    return (float)s / 8.f;
  }
  float s = sample_f32(src, b);
  for (int c = 1; c < channels; ++c) s += sample_f32(src, b + c);
  return channels == 1 ? s : s / (float)channels;
}

// The frames one 16-byte load holds: 16 / (C * sizeof(S)), for the frame sizes that divide 16.
template <class S, int C>
struct Vec {
  static constexpr int kElems = 16 / (int)sizeof(S);
  static constexpr int kFrames = kElems / C;
  // frames [v * kFrames, (v + 1) * kFrames) of a 16-byte aligned window -> o[0..kFrames)
  static __device__ __forceinline__ void load(const S* src, long v, float* o) {
    const uint4 raw = reinterpret_cast<const uint4*>(src)[v];
    float e[kElems];
    if constexpr (sizeof(S) == 4) {
      e[0] = __uint_as_float(raw.x);
      e[1] = __uint_as_float(raw.y);
      e[2] = __uint_as_float(raw.z);
      e[3] = __uint_as_float(raw.w);
    } else {
      const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        e[2 * k] = (float)(short)(u[k] & 0xffffu) * 0x1p-15f;
        e[2 * k + 1] = (float)(short)(u[k] >> 16) * 0x1p-15f;
      }
    }
#pragma unroll
    for (int f = 0; f < kFrames; ++f) o[f] = mix<C>(e + f * C);
  }
};

__device__ __forceinline__ long floor_div(long a, long b) {  // b > 0
  const long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// Stage the downmixed frames [base, base + count) of the signal into tile[0..count): frames
// outside the window [w0, w1) are zero (the window's ends are the signal's ends wherever a
// tile reaches past them).  CV > 0: 16-byte loads of whole vectors inside the window, scalar
// loads for the vectors that straddle its ends; CV == 0: scalar loads, any channel count.
template <class S, int CV>
__device__ __forceinline__ void stage_tile(const S* src, long w0, long w1, int channels,
                                           long base, int count, float* tile) {
  if constexpr (CV > 0) {
    constexpr int F = Vec<S, CV>::kFrames;
    const long v0 = floor_div(base - w0, F);
    const int nv = (int)(floor_div(base + count - 1 - w0, F) - v0) + 1;
    for (int v = threadIdx.x; v < nv; v += kThreads) {
      const long f0 = (v0 + v) * F;  // relative to w0
      float o[F];
      if (f0 >= 0 && f0 + F <= w1 - w0) {
        Vec<S, CV>::load(src, v0 + v, o);
      } else {
#pragma unroll
        for (int f = 0; f < F; ++f)
          o[f] = (f0 + f >= 0 && f0 + f < w1 - w0) ? frame_scalar(src, f0 + f, CV) : 0.f;
      }
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const long i = f0 + f + w0 - base;
        if (i >= 0 && i < count) tile[i] = o[f];
      }
    }
  } else {
    for (int i = threadIdx.x; i < count; i += kThreads) {
      const long f = base + i - w0;
      tile[i] = (f >= 0 && f < w1 - w0) ? frame_scalar(src, f, channels) : 0.f;
    }
  }
}

// One workgroup makes out_tile consecutive outputs per tile and walks the tiles grid-stride,
// so the phase table is staged once per workgroup.  LDS: [span] input tile, then (when the
// table fits) [P] lo and [P][taps | 1] weights, the odd row stride keeping neighbouring
// phases on different banks.  A table that does not fit (a rate coprime to 16000: P = 16000)
// is read through the caches from global memory.
template <class S, int CV>
__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleArgs a, int channels) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* tile = lds;
  int* lo_s = reinterpret_cast<int*>(lds + a.span);
  float* w_s = lds + a.span + a.P;
  const int T = a.taps, ts = a.table_in_lds ? (T | 1) : T;
  const int* lo = a.lo;
  const float* w = a.w;
  if (a.table_in_lds) {
    for (int p = threadIdx.x; p < a.P; p += kThreads) lo_s[p] = a.lo[p];
    for (int i = threadIdx.x; i < a.P * T; i += kThreads) w_s[(i / T) * ts + i % T] = a.w[i];
    lo = lo_s;
    w = w_s;
  }
  const S* src = static_cast<const S*>(a.src);
  const long n_tiles = cdivl(a.m_end - a.m_begin, a.out_tile);
  for (long tix = blockIdx.x; tix < n_tiles; tix += gridDim.x) {
    const long m0 = a.m_begin + tix * a.out_tile;
    const int cnt = (int)min((long)a.out_tile, a.m_end - m0);
    const long q0 = m0 / a.P;
    const int p0 = (int)(m0 - q0 * a.P);
    __syncthreads();  // the table is staged; the previous tile is consumed
    const int lo0 = lo[p0];
    const long base = q0 * a.Q + lo0;
    // the frames this tile's outputs read: [base, start(last output) + taps)
    const int dl = p0 + cnt - 1, dql = dl / a.P;
    const int need = dql * a.Q + lo[dl - dql * a.P] - lo0 + T;  // <= span by construction
    stage_tile<S, CV>(src, a.w0, a.w1, channels, base, min(need, a.span), tile);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += kThreads) {
      const int d = p0 + j, dq = d / a.P, p = d - dq * a.P;
      const float* x = tile + (dq * a.Q + lo[p] - lo0);
      const float* wp = w + (long)p * ts;
      float acc = 0.f;
      for (int t = 0; t < T; ++t) acc = fmaf(x[t], wp[t], acc);
      a.out[m0 + j] = acc;
    }
  }
}

template <class S, int CV>
__global__ __launch_bounds__(kThreads) void downmix_kernel(const S* src, int channels, long n,
                                                           float* out) {
  if constexpr (CV > 0) {
    constexpr int F = Vec<S, CV>::kFrames;
    const long nv = cdivl(n, F);
    for (long v = (long)blockIdx.x * kThreads + threadIdx.x; v < nv; v += (long)gridDim.x * kThreads) {
      const long f0 = v * F;
      if (f0 + F <= n) {
        float o[F];
        Vec<S, CV>::load(src, v, o);
#pragma unroll
        for (int f = 0; f < F; ++f) out[f0 + f] = o[f];
      } else {
        for (long f = f0; f < n; ++f) out[f] = frame_scalar(src, f, CV);
      }
    }
  } else {
    for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < n; f += (long)gridDim.x * kThreads)
      out[f] = frame_scalar(src, f, channels);
  }
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// block maximum of an unsigned per thread -> one integer atomicMax (order independent)
__device__ __forceinline__ void block_max_to(unsigned m, unsigned* dst) {
  __shared__ unsigned part[kThreads / kWave];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kThreads / kWave; ++k) m = max(m, part[k]);
    if (m != 0) atomicMax(dst, m);
  }
}

// n4 = whole float4 groups when x is 16-byte aligned (0 otherwise); the rest goes scalar
__global__ __launch_bounds__(kThreads) void peak_kernel(const float* x, long n, long n4,
                                                        unsigned* dst) {
  unsigned m = 0;
  const long stride = (long)gridDim.x * kThreads, i0 = (long)blockIdx.x * kThreads + threadIdx.x;
  for (long i = i0; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    m = max(max(m, abs_bits(v.x)), max(abs_bits(v.y), max(abs_bits(v.z), abs_bits(v.w))));
  }
  for (long i = 4 * n4 + i0; i < n; i += stride) m = max(m, abs_bits(x[i]));
  block_max_to(m, dst);
}

__global__ __launch_bounds__(kThreads) void scale_kernel(float* x, long n, long n4, float d,
                                                         float mul) {
  const long stride = (long)gridDim.x * kThreads, i0 = (long)blockIdx.x * kThreads + threadIdx.x;
  for (long i = i0; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = (v.x / d) * mul;
    v.y = (v.y / d) * mul;
    v.z = (v.z / d) * mul;
    v.w = (v.w / d) * mul;
    reinterpret_cast<float4*>(x)[i] = v;
  }
  for (long i = 4 * n4 + i0; i < n; i += stride) x[i] = (x[i] / d) * mul;
}

// largest k with key[k] <= v, -1 when none (key ascending)
__device__ __forceinline__ int last_le(const long* key, int n, long v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

// Block b sums the squares of one chunk of one segment in float64 (each square is exact): a
// fixed thread-strided order, then a fixed tree, so partial[b] never depends on scheduling.
__global__ __launch_bounds__(kThreads) void sumsq_partial_kernel(const float* x,
                                                                 const long* seg_begin,
                                                                 const long* seg_end,
                                                                 const long* blk_off, int n_seg,
                                                                 double* partial) {
  const long b = blockIdx.x;
  const int s = last_le(blk_off, n_seg, b);
  const long beg = seg_begin[s] + (b - blk_off[s]) * kAudioChunk;
  const long end = min(seg_end[s], beg + kAudioChunk);
  double acc = 0.0;
  for (long i = beg + threadIdx.x; i < end; i += kThreads) {
    const double v = (double)x[i];
    acc += v * v;
  }
  acc = wave_sum_d(acc);
  __shared__ double part[kThreads / kWave];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = ((part[0] + part[1]) + part[2]) + part[3];
}

// one wave per segment: its partials in chunk order (lane-strided, then the same tree)
__global__ __launch_bounds__(kWave) void sumsq_final_kernel(const double* partial,
                                                            const long* blk_off, int n_seg,
                                                            double* out) {
  const int s = blockIdx.x;
  double acc = 0.0;
  for (long b = blk_off[s] + threadIdx.x; b < blk_off[s + 1]; b += kWave) acc += partial[b];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) out[s] = acc;
}

struct GainPlan {
  const long* pb;
  const long* pe;
  const float* pg;
  const long* po;
  const float* vals;
  int n;
};

__device__ __forceinline__ float gain_at(const GainPlan& g, int& k, long i) {
  while (k + 1 < g.n && g.pb[k + 1] <= i) ++k;
  if (k < 0 || i >= g.pe[k]) return 1.f;
  const long o = g.po[k];
  return o < 0 ? g.pg[k] : g.vals[o + (i - g.pb[k])];
}

__global__ __launch_bounds__(kThreads) void apply_gain_kernel(float* x, long n, long n4,
                                                              GainPlan g, unsigned* dst) {
  unsigned m = 0;
  const long stride = (long)gridDim.x * kThreads, i0 = (long)blockIdx.x * kThreads + threadIdx.x;
  for (long i = i0; i < n4; i += stride) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    if (g.n > 0) {
      int k = last_le(g.pb, g.n, 4 * i);
      v.x *= gain_at(g, k, 4 * i);
      v.y *= gain_at(g, k, 4 * i + 1);
      v.z *= gain_at(g, k, 4 * i + 2);
      v.w *= gain_at(g, k, 4 * i + 3);
      reinterpret_cast<float4*>(x)[i] = v;
    }
    m = max(max(m, abs_bits(v.x)), max(abs_bits(v.y), max(abs_bits(v.z), abs_bits(v.w))));
  }
  for (long i = 4 * n4 + i0; i < n; i += stride) {
    float v = x[i];
    if (g.n > 0) {
      int k = last_le(g.pb, g.n, i);
      v *= gain_at(g, k, i);
      x[i] = v;
    }
    m = max(m, abs_bits(v));
  }
  block_max_to(m, dst);
}

int stream_grid(long work_items) {  // memory-bound grid: grid-stride past ~8 blocks per CU
  return (int)std::max(1L, std::min(cdivl(work_items, kThreads), 2048L));
}
long whole_vec4(const void* p, long n) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 ? n / 4 : 0; }

template <class S>
void resample_dispatch(const ResampleArgs& a, int channels, dim3 grid, size_t lds, hipStream_t st) {
  const int fb = channels * (int)sizeof(S);  // frame bytes: the vector forms need 16 % fb == 0
  if (!a.vec_ok || 16 % fb != 0) {
    ZASR_LAUNCH((resample_kernel<S, 0>), grid, dim3(kThreads), lds, st, a, channels);
    return;
  }
  switch (channels) {
    case 1: ZASR_LAUNCH((resample_kernel<S, 1>), grid, dim3(kThreads), lds, st, a, channels); break;
    case 2: ZASR_LAUNCH((resample_kernel<S, 2>), grid, dim3(kThreads), lds, st, a, channels); break;
    case 4: ZASR_LAUNCH((resample_kernel<S, 4>), grid, dim3(kThreads), lds, st, a, channels); break;
    default:
      if constexpr (sizeof(S) == 2)
        ZASR_LAUNCH((resample_kernel<S, 8>), grid, dim3(kThreads), lds, st, a, channels);
      break;
  }
}

template <class S>
void downmix_dispatch(const S* src, int channels, long n, float* out, bool vec_ok, hipStream_t st) {
  const int fb = channels * (int)sizeof(S);
  if (!vec_ok || 16 % fb != 0) {
    ZASR_LAUNCH((downmix_kernel<S, 0>), dim3(stream_grid(n)), dim3(kThreads), 0, st, src, channels, n, out);
    return;
  }
  const dim3 grid(stream_grid(cdivl(n, 16 / fb)));
  switch (channels) {
    case 1: ZASR_LAUNCH((downmix_kernel<S, 1>), grid, dim3(kThreads), 0, st, src, channels, n, out); break;
    case 2: ZASR_LAUNCH((downmix_kernel<S, 2>), grid, dim3(kThreads), 0, st, src, channels, n, out); break;
    case 4: ZASR_LAUNCH((downmix_kernel<S, 4>), grid, dim3(kThreads), 0, st, src, channels, n, out); break;
    default:
      if constexpr (sizeof(S) == 2)
        ZASR_LAUNCH((downmix_kernel<S, 8>), grid, dim3(kThreads), 0, st, src, channels, n, out);
      break;
  }
}

}  // namespace

size_t resample_lds_bytes(const ResampleArgs& a) {
  size_t words = (size_t)a.span;
  if (a.table_in_lds) words += (size_t)a.P + (size_t)a.P * (a.taps | 1);
  return words * 4;
}

void launch_resample(const ResampleArgs& a, int format, int channels, hipStream_t st) {
  if (a.m_end <= a.m_begin) return;
  const long n_tiles = cdivl(a.m_end - a.m_begin, a.out_tile);
  const dim3 grid((unsigned)std::min(n_tiles, 1024L));
  const size_t lds = resample_lds_bytes(a);
  ZASR_REQUIRE(lds <= 64 * 1024, "resample tile exceeds the LDS budget");
  if (format == kAudioF32) resample_dispatch<float>(a, channels, grid, lds, st);
  else resample_dispatch<short>(a, channels, grid, lds, st);
}

void launch_downmix(const void* src, int format, int channels, long n, float* out, bool vec_ok,
                    hipStream_t st) {
  if (n <= 0) return;
  if (format == kAudioF32) downmix_dispatch(static_cast<const float*>(src), channels, n, out, vec_ok, st);
  else downmix_dispatch(static_cast<const short*>(src), channels, n, out, vec_ok, st);
}

void launch_peak(const float* x, long n, unsigned* d_peak_bits, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = whole_vec4(x, n);
  ZASR_LAUNCH(peak_kernel, dim3(stream_grid(n / 4 + 1)), dim3(kThreads), 0, st, x, n, n4,
              d_peak_bits);
}

void launch_scale(float* x, long n, float divisor, float multiplier, hipStream_t st) {
  if (n <= 0) return;
  const long n4 = whole_vec4(x, n);
  ZASR_LAUNCH(scale_kernel, dim3(stream_grid(n / 4 + 1)), dim3(kThreads), 0, st, x, n, n4,
              divisor, multiplier);
}

void launch_segment_sumsq(const float* x, const long* seg_begin, const long* seg_end,
                          const long* blk_off, int n_seg, long n_blocks, double* partial,
                          double* out, hipStream_t st) {
  if (n_seg <= 0) return;
  if (n_blocks > 0)
    ZASR_LAUNCH(sumsq_partial_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, st, x,
                seg_begin, seg_end, blk_off, n_seg, partial);
  ZASR_LAUNCH(sumsq_final_kernel, dim3((unsigned)n_seg), dim3(kWave), 0, st, partial, blk_off,
              n_seg, out);
}

void launch_apply_gain(float* x, long n, const long* pb, const long* pe, const float* pg,
                       const long* po, int n_pieces, const float* vals, unsigned* d_peak_bits,
                       hipStream_t st) {
  if (n <= 0) return;
  const long n4 = whole_vec4(x, n);
  const GainPlan g{pb, pe, pg, po, vals, n_pieces};
  ZASR_LAUNCH(apply_gain_kernel, dim3(stream_grid(n / 4 + 1)), dim3(kThreads), 0, st, x, n, n4,
              g, d_peak_bits);
}

}  // namespace zasr
