// Conv-TasNet separation kernels other than the GEMMs.  The encoder and decoder
// filter banks and every 1x1 convolution run on the exact-f32 MFMA GEMM (gemm.hip) over the
// ragged [sum F][channels] activations of all regions of a launch; here are the operators that
// know where a region starts and ends: the framing of the signal, the global layer norm
// (statistics and application), the fused gLN + dilated depthwise convolution + PReLU middle of
// a TCN block, and the decoder's overlap-add.  All float32 with float64 statistics.  Replaces
// the onnxruntime session call at core/overlap_separator.py:291.
//
// Every kernel works on tiles of at most kSepTile frames that never straddle a region, and a
// region's norm statistics are the sum of its own tiles' float64 partial sums in tile order:
// what a region computes does not depend on what else is in the launch or where it sits in it.
#include "common.h"
#include "sep.h"

namespace zasr {

namespace {
constexpr double kGlnEps = 1e-8;

// sum of one double per thread over a 256-thread block, fixed tree; every thread gets the sum
__device__ __forceinline__ double sep_block_sum(double v, double* red) {
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

__device__ __forceinline__ float prelu(float v, float slope) { return v > 0.f ? v : slope * v; }
}  // namespace

// ---- framing: the encoder GEMM's A rows ----
__global__ __launch_bounds__(256) void sep_frames_kernel(const float* __restrict__ signal,
                                                         const SepRegion* __restrict__ regions,
                                                         const SepTile* __restrict__ tiles, int win,
                                                         int hop, float* __restrict__ frames) {
  const SepTile tl = tiles[blockIdx.x];
  const int rows = min(kSepTile, tl.F - tl.f0);
  const float* src = signal + regions[tl.region].sig_off;
  for (int i = threadIdx.x; i < rows * win; i += 256) {
    const int r = i / win, k = i - r * win;
    frames[((long)tl.row0 + r) * win + k] = src[(long)(tl.f0 + r) * hop + k];
  }
}

void launch_sep_frames(const float* signal, const SepRegion* regions, const SepTile* tiles,
                       int n_tiles, int win, int hop, float* frames, hipStream_t st) {
  if (n_tiles <= 0) return;
  ZASR_LAUNCH(sep_frames_kernel, dim3(n_tiles), dim3(256), 0, st, signal, regions, tiles, win, hop,
              frames);
}

// ---- gLN statistics ----
// A tile's rows are contiguous: thread t adds the float4s t, t + 256, ... in float64, then the
// fixed tree.
__global__ __launch_bounds__(256) void sep_tile_sums_kernel(const float* __restrict__ x, int C,
                                                            const SepTile* __restrict__ tiles,
                                                            double2* __restrict__ partial) {
  __shared__ double red[256];
  const SepTile tl = tiles[blockIdx.x];
  const int rows = min(kSepTile, tl.F - tl.f0);
  const float4* x4 = reinterpret_cast<const float4*>(x + (long)tl.row0 * C);
  const int n4 = rows * (C >> 2);
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < n4; i += 256) {
    const float4 v = x4[i];
    const double a = v.x, b = v.y, c = v.z, d = v.w;
    s += (a + b) + (c + d);
    q += (a * a + b * b) + (c * c + d * d);
  }
  s = sep_block_sum(s, red);
  q = sep_block_sum(q, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = make_double2(s, q);
}

void launch_sep_tile_sums(const float* x, int C, const SepTile* tiles, int n_tiles,
                          double2* partial, hipStream_t st) {
  if (n_tiles <= 0) return;
  ZASR_REQUIRE(C > 0 && C % 4 == 0, "separation: channels must be a multiple of 4");
  ZASR_LAUNCH(sep_tile_sums_kernel, dim3(n_tiles), dim3(256), 0, st, x, C, tiles, partial);
}

// one thread per region: its tiles' sums in tile order
__global__ void sep_region_stats_kernel(const double2* __restrict__ partial,
                                        const SepRegion* __restrict__ regions, int n_regions, int C,
                                        float2* __restrict__ stats) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_regions) return;
  const SepRegion rg = regions[r];
  const int nt = (rg.F + kSepTile - 1) / kSepTile;
  double s = 0.0, q = 0.0;
  for (int i = 0; i < nt; ++i) {
    const double2 p = partial[rg.tile0 + i];
    s += p.x;
    q += p.y;
  }
  const double n = (double)rg.F * (double)C;
  const double mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[r] = make_float2((float)mean, (float)(1.0 / sqrt(var + kGlnEps)));
}

void launch_sep_region_stats(const double2* partial, const SepRegion* regions, int n_regions, int C,
                             float2* stats, hipStream_t st) {
  if (n_regions <= 0) return;
  ZASR_LAUNCH(sep_region_stats_kernel, dim3(cdiv(n_regions, 64)), dim3(64), 0, st, partial, regions,
              n_regions, C, stats);
}

// ---- gLN application ----
__global__ __launch_bounds__(256) void sep_gln_apply_kernel(const float* __restrict__ src,
                                                            float* __restrict__ dst, int C,
                                                            const SepTile* __restrict__ tiles,
                                                            const float2* __restrict__ stats,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta) {
  const SepTile tl = tiles[blockIdx.x];
  const int rows = min(kSepTile, tl.F - tl.f0);
  const float2 ms = stats[tl.region];
  const int C4 = C >> 2;
  const float4* s4 = reinterpret_cast<const float4*>(src + (long)tl.row0 * C);
  float4* d4 = reinterpret_cast<float4*>(dst + (long)tl.row0 * C);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
  for (int i = threadIdx.x; i < rows * C4; i += 256) {
    const int c = i % C4;
    const float4 v = s4[i], g = g4[c], b = b4[c];
    d4[i] = make_float4(fmaf(v.x - ms.x, ms.y * g.x, b.x), fmaf(v.y - ms.x, ms.y * g.y, b.y),
                        fmaf(v.z - ms.x, ms.y * g.z, b.z), fmaf(v.w - ms.x, ms.y * g.w, b.w));
  }
}

void launch_sep_gln_apply(const float* src, float* dst, int C, const SepTile* tiles, int n_tiles,
                          const float2* stats, const float* gamma, const float* beta,
                          hipStream_t st) {
  if (n_tiles <= 0) return;
  ZASR_REQUIRE(C > 0 && C % 4 == 0, "separation: channels must be a multiple of 4");
  ZASR_LAUNCH(sep_gln_apply_kernel, dim3(n_tiles), dim3(256), 0, st, src, dst, C, tiles, stats,
              gamma, beta);
}

// ---- the middle of a TCN block: gLN -> depthwise conv (3 taps, dilation d) -> PReLU ----
// y[t][c] = prelu(w0[c] n(t - d) + w1[c] n(t) + w2[c] n(t + d) + bias[c]) with
// n(u) = (h[u][c] - mean) * rstd * gamma[c] + beta[c] for 0 <= u < F and 0 outside: the zero
// padding is in the normalised domain, so beta does not leak into the edges.  The normalised
// tensor is never stored: h is read, y is written once, and the block leaves the float64
// partial sums of its y tile for the second gLN, which saves that norm's statistics pass.
//
// Staging: plain global loads at t - d, t, t + d, no LDS halo.  A thread owns four adjacent
// channels and walks the tile's frames, so every load instruction of a wave reads 1 KB of one
// time-major row and a block reads whole 2 KB rows (at 512 channels), the shape in which
// gathered rows stream at HBM rate.  An LDS halo would hold 32 + 2 d rows: at d >= 32 the halo
// alone is as large as the tile and at d = 128 it is 576 KB against 160 KB of LDS, while the
// reuse it would serve does not exist inside a block once d >= 32 (the three taps of a frame
// then belong to three different tiles).  Each row of h is read by at most three blocks, close
// in launch order; the repeats are served by L2 / Infinity Cache (h of a 10 s region is 20 MB).
// For d < 32 the taps of neighbouring frames do share rows inside the block, and those repeats
// hit the CU's L1 / L2 the same way; one code path for all eight dilations.
__global__ __launch_bounds__(256) void sep_mid_kernel(SepMidArgs a,
                                                      const SepTile* __restrict__ tiles) {
  __shared__ double red[256];
  const SepTile tl = tiles[blockIdx.x];
  const int rows = min(kSepTile, tl.F - tl.f0);
  const float2 ms = a.stats[tl.region];
  const int C = a.C, C4 = C >> 2, d = a.dil;
  // thread = (channel quad, frame slot): CW quads across, 256 / CW frame slots
  const int CW = C4 < 256 ? C4 : 256, RW = 256 / CW;
  const int tx = threadIdx.x % CW, ty = threadIdx.x / CW;
  const float* hreg = a.h + ((long)tl.row0 - tl.f0) * C;  // frame 0 of the region
  float* yt = a.y + (long)tl.row0 * C;
  double s = 0.0, q = 0.0;
  for (int c4 = tx; c4 < C4; c4 += CW) {
    const float4 g = reinterpret_cast<const float4*>(a.gamma)[c4];
    const float4 be = reinterpret_cast<const float4*>(a.beta)[c4];
    const float4 w0 = reinterpret_cast<const float4*>(a.w)[c4];
    const float4 w1 = reinterpret_cast<const float4*>(a.w + C)[c4];
    const float4 w2 = reinterpret_cast<const float4*>(a.w + 2 * C)[c4];
    const float4 bi = reinterpret_cast<const float4*>(a.bias)[c4];
    const float4 sc = make_float4(ms.y * g.x, ms.y * g.y, ms.y * g.z, ms.y * g.w);
    auto norm = [&](int u) {
      if (u < 0 || u >= tl.F) return make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 v = reinterpret_cast<const float4*>(hreg + (long)u * C)[c4];
      return make_float4(fmaf(v.x - ms.x, sc.x, be.x), fmaf(v.y - ms.x, sc.y, be.y),
                         fmaf(v.z - ms.x, sc.z, be.z), fmaf(v.w - ms.x, sc.w, be.w));
    };
    for (int r = ty; r < rows; r += RW) {
      const int t = tl.f0 + r;
      const float4 l = norm(t - d), m = norm(t), h = norm(t + d);
      float4 o;
      o.x = prelu(fmaf(w2.x, h.x, fmaf(w1.x, m.x, fmaf(w0.x, l.x, bi.x))), a.slope);
      o.y = prelu(fmaf(w2.y, h.y, fmaf(w1.y, m.y, fmaf(w0.y, l.y, bi.y))), a.slope);
      o.z = prelu(fmaf(w2.z, h.z, fmaf(w1.z, m.z, fmaf(w0.z, l.z, bi.z))), a.slope);
      o.w = prelu(fmaf(w2.w, h.w, fmaf(w1.w, m.w, fmaf(w0.w, l.w, bi.w))), a.slope);
      reinterpret_cast<float4*>(yt + (long)r * C)[c4] = o;
      const double ox = o.x, oy = o.y, oz = o.z, ow = o.w;
      s += (ox + oy) + (oz + ow);
      q += (ox * ox + oy * oy) + (oz * oz + ow * ow);
    }
  }
  s = sep_block_sum(s, red);
  q = sep_block_sum(q, red);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = make_double2(s, q);
}

void launch_sep_mid(const SepMidArgs& a, const SepTile* tiles, int n_tiles, hipStream_t st) {
  if (n_tiles <= 0) return;
  const int C4 = a.C / 4;
  ZASR_REQUIRE(a.C % 4 == 0 && (C4 % 256 == 0 || (C4 <= 256 && 256 % C4 == 0)),
               "separation: hid_chan / 4 must divide 256 or be a multiple of it");
  ZASR_LAUNCH(sep_mid_kernel, dim3(n_tiles), dim3(256), 0, st, a, tiles);
}

// ---- PReLU in place on the first C columns of rows of stride ld ----
__global__ void sep_prelu_kernel(float* __restrict__ x, long n4, int C4, int ld, float slope) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / C4;
    const int c = (int)(i - r * C4);
    float4* p = reinterpret_cast<float4*>(x + r * ld) + c;
    const float4 v = *p;
    *p = make_float4(prelu(v.x, slope), prelu(v.y, slope), prelu(v.z, slope), prelu(v.w, slope));
  }
}

void launch_sep_prelu(float* x, long rows, int C, int ld, float slope, hipStream_t st,
                      int max_blocks) {
  ZASR_REQUIRE(C % 4 == 0 && ld % 4 == 0, "separation: PReLU columns and row stride must be multiples of 4");
  const long n4 = rows * (C / 4);
  if (n4 <= 0) return;
  const long blocks = std::min<long>(cdivl(n4, 256), max_blocks > 0 ? max_blocks : 65536);
  ZASR_LAUNCH(sep_prelu_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, n4, C / 4, ld, slope);
}

// ---- decoder overlap-add (win = 2 hop): a sample sums at most two frame rows ----
__global__ __launch_bounds__(256) void sep_overlap_add_kernel(const float* __restrict__ dec0,
                                                              const float* __restrict__ dec1,
                                                              const SepRegion* __restrict__ regions,
                                                              int win, int hop,
                                                              float* __restrict__ out) {
  const SepRegion rg = regions[blockIdx.y];
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= rg.T) return;
  const float* dec = blockIdx.z ? dec1 : dec0;
  const int f = t / hop, j = t - f * hop;
  float v = 0.f;  // stays exactly 0 from (F - 1) hop + win to T
  if (f >= 1 && f - 1 < rg.F) v = dec[((long)rg.row0 + f - 1) * win + hop + j];
  if (f < rg.F) v += dec[((long)rg.row0 + f) * win + j];
  out[rg.out_off + (long)blockIdx.z * rg.T + t] = v;
}

void launch_sep_overlap_add(const float* dec0, const float* dec1, const SepRegion* regions,
                            int n_regions, int max_T, int win, int hop, float* out,
                            hipStream_t st) {
  if (n_regions <= 0 || max_T <= 0) return;
  ZASR_REQUIRE(win == 2 * hop && hop > 0, "separation: the overlap-add needs kernel_size = 2 stride");
  ZASR_REQUIRE(n_regions <= 65535, "separation: more than 65535 regions in one overlap-add");
  ZASR_LAUNCH(sep_overlap_add_kernel, dim3(cdiv(max_T, 256), n_regions, 2), dim3(256), 0, st, dec0,
              dec1, regions, win, hop, out);
}

}  // namespace zasr
