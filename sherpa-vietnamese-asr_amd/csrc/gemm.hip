// f32-in / f32-accumulate MFMA GEMM (v_mfma_f32_32x32x2_f32: exact f32 fma chains, the
// "fp32" precision mode) for every dense projection on the Zipformer path.
//
// Structure: 64*WAVES threads per block, BM x BN block tile, BK = 16 K-slab staged through
// LDS (k-major images As[k][m], Bs[k][n] so that an MFMA operand read is 32 consecutive
// floats per lane half: conflict-free ds_read_b32), double-buffered with one barrier per
// K-slab, next slab's global loads (float4 per lane) in flight under the MFMAs.
// Each wave owns a (BM/WAVES_M) x (BN/WAVES_N) sub-tile of 32x32 MFMA tiles.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "gemm.h"
#include "gemm_dev.h"

namespace zasr {

namespace {

constexpr int BK = 16;

template <int BM, int BN, int WAVES_M, int WAVES_N, int ALOAD, bool BNC, int EPI, bool DEEP>
__global__ __launch_bounds__(64 * WAVES_M* WAVES_N) void gemm_f32_kernel(GemmParams p) {
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int LDA_S = BM + 4;
  constexpr int LDB_S = BN + 4;
  constexpr int WTM = BM / WAVES_M;
  constexpr int WTN = BN / WAVES_N;
  constexpr int FM = WTM / 32;
  constexpr int FN = WTN / 32;
  static_assert(FM >= 1 && FN >= 1, "wave tile must be a multiple of 32x32");
  constexpr int A_F4 = BM * BK / 4;
  constexpr int B_F4 = BN * BK / 4;
  constexpr int A_LD = (A_F4 + NT - 1) / NT;
  constexpr int B_LD = (B_F4 + NT - 1) / NT;

  __shared__ float As[2][BK * LDA_S];
  __shared__ float Bs[2][BK * LDB_S];

  const float* A = p.A;
  const float* B = p.B;
  float* C = p.C;
  const float* aux = p.aux;
  int M = p.M, K = p.K, lda = p.lda;
  if (p.slices) {
    const GemmSlice s = p.slices[blockIdx.z];
    A += s.a_off;
    B += s.b_off;
    C += s.c_off;
    if (aux) aux += s.aux_off;
    M = s.M;
    K = s.K;
    lda = s.lda;
  }
  const int m0 = blockIdx.y * BM;
  if (m0 >= M) return;
  const int n0 = blockIdx.x * BN;
  const int N = p.N;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid / WAVES_N;
  const int wn = wid - wm * WAVES_N;

  auto gload_to = [&](float4 (&ra)[A_LD], float4 (&rb)[B_LD], int kt) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      int idx = tid + NT * i;
      int row = idx >> 2, k4 = idx & 3;
      const float4 v = load_a4<ALOAD>(p, A, M, K, lda, m0 + (idx < A_F4 ? row : 0), kt * BK + 4 * k4);
      ra[i] = (idx < A_F4) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      int idx = tid + NT * i;
      float4 v;
      if constexpr (!BNC) {
        const int n = idx >> 2, k4 = idx & 3;
        const int gn = n0 + n, gk = kt * BK + 4 * k4;
        const bool ok = idx < B_F4 && gn < N && gk < K;
        const int nc = gn < N ? gn : N - 1, kc = gk < K ? gk : K - 4;
        v = *reinterpret_cast<const float4*>(B + (long)nc * p.sbn + kc);
        if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const int k = idx / (BN / 4), n4 = idx - k * (BN / 4);
        const int gk = kt * BK + k, gn = n0 + 4 * n4;
        const bool ok = idx < B_F4 && gk < K && gn < N;
        const int kc = gk < K ? gk : K - 1, nc = gn < N ? gn : N - 4;
        v = *reinterpret_cast<const float4*>(B + (long)kc * p.sbk + nc);
        if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      rb[i] = v;
    }
  };
  auto sstore_from = [&](const float4 (&ra)[A_LD], const float4 (&rb)[B_LD], int buf) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      int idx = tid + NT * i;
      if (idx < A_F4) {
        int row = idx >> 2, k4 = idx & 3;
        float* d = &As[buf][(4 * k4) * LDA_S + row];
        d[0] = ra[i].x;
        d[LDA_S] = ra[i].y;
        d[2 * LDA_S] = ra[i].z;
        d[3 * LDA_S] = ra[i].w;
      }
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      int idx = tid + NT * i;
      if (idx < B_F4) {
        if constexpr (!BNC) {
          int n = idx >> 2, k4 = idx & 3;
          float* d = &Bs[buf][(4 * k4) * LDB_S + n];
          d[0] = rb[i].x;
          d[LDB_S] = rb[i].y;
          d[2 * LDB_S] = rb[i].z;
          d[3 * LDB_S] = rb[i].w;
        } else {
          int k = idx / (BN / 4), n4 = idx - k * (BN / 4);
          *reinterpret_cast<float4*>(&Bs[buf][k * LDB_S + 4 * n4]) = rb[i];
        }
      }
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = (K + BK - 1) / BK;
  auto mma_slab = [&](int cur) {
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int kr = kk + (lane >> 5);
      float a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = As[cur][kr * LDA_S + wm * WTM + i * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = Bs[cur][kr * LDB_S + wn * WTN + j * 32 + (lane & 31)];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  if constexpr (DEEP) {
    // K a multiple of 2 BK (host-checked): two register sets, so each K slab's loads have two
    // slabs of MFMAs to land; LDS-only barriers (__syncthreads would drain the slab in flight
    // with vmcnt(0)); slab indices clamped so every load is unconditional
    float4 xa[2][A_LD], xb[2][B_LD];
    auto bar = []() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
    gload_to(xa[0], xb[0], 0);
    gload_to(xa[1], xb[1], 1);
    sstore_from(xa[0], xb[0], 0);
    bar();
    for (int kt = 0; kt < nkt; kt += 2) {
      gload_to(xa[0], xb[0], min(kt + 2, nkt - 1));
      mma_slab(0);
      sstore_from(xa[1], xb[1], 1);
      bar();
      gload_to(xa[1], xb[1], min(kt + 3, nkt - 1));
      mma_slab(1);
      sstore_from(xa[0], xb[0], 0);
      bar();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped tail loads
  } else {
    float4 ra[A_LD], rb[B_LD];
    gload_to(ra, rb, 0);
    sstore_from(ra, rb, 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nkt) gload_to(ra, rb, kt + 1);
      mma_slab(cur);
      if (kt + 1 < nkt) sstore_from(ra, rb, cur ^ 1);
      __syncthreads();
    }
  }

  // epilogue: lane holds column (lane & 31), rows (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = n0 + wn * WTN + j * 32 + (lane & 31);
      if (col >= N) continue;
      const float bcol = p.bias ? p.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= M) continue;
        float v = acc[i][j][r] + bcol;
        float* dst = C + (long)row * p.ldc + col;
        if constexpr (EPI == EPI_SWOOSHL) v = swooshl(v);
        if constexpr (EPI == EPI_SWOOSHR) v = swooshr(v);
        if constexpr (EPI == EPI_RELU) v = fmaxf(v, 0.f);
        if constexpr (EPI == EPI_GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
        if constexpr (EPI == EPI_LEAKY) v = v > 0.f ? v : 0.01f * v;
        if constexpr (EPI == EPI_PRELU) v = v > 0.f ? v : p.slope * v;
        if constexpr (EPI == EPI_MULAUX) v *= aux[(long)row * p.ldaux + col];
        if constexpr (EPI == EPI_RELUMUL) v = fmaxf(v, 0.f) * aux[(long)row * p.ldaux + col];
        if constexpr (EPI == EPI_RESADD) v += *dst;
        *dst = v;
      }
    }
  }
}

int g_gemm_f32_deep = -1;  // the two-slab prefetch (gemm_set_deep: the labs' A/B switch)

template <int BM, int BN, int WM, int WN, int ALOAD, bool BNC, int EPI>
void launch_t(const GemmParams& p, hipStream_t st) {
  dim3 grid(cdiv(p.N, BN), cdiv(p.max_M, BM), p.slices ? p.num_slices : 1);
  if (g_gemm_f32_deep < 0)
    g_gemm_f32_deep = 1;
  if (g_gemm_f32_deep && !p.slices && p.K % (2 * BK) == 0) {
    ZASR_LAUNCH((gemm_f32_kernel<BM, BN, WM, WN, ALOAD, BNC, EPI, true>), grid,
                       dim3(64 * WM * WN), 0, st, p);
    return;
  }
  ZASR_LAUNCH((gemm_f32_kernel<BM, BN, WM, WN, ALOAD, BNC, EPI, false>), grid,
                     dim3(64 * WM * WN), 0, st, p);
}

template <int ALOAD, bool BNC, int EPI>
void launch_tile(const GemmParams& p, hipStream_t st) {
  const auto [BN, big] = pick_tile(p);
  if (BN == 128) {
    if (big) launch_t<128, 128, 2, 2, ALOAD, BNC, EPI>(p, st);
    else launch_t<64, 128, 2, 2, ALOAD, BNC, EPI>(p, st);
  } else if (BN == 64) {
    if (big) launch_t<128, 64, 2, 2, ALOAD, BNC, EPI>(p, st);
    else launch_t<64, 64, 2, 2, ALOAD, BNC, EPI>(p, st);
  } else {
    if (big) launch_t<128, 32, 4, 1, ALOAD, BNC, EPI>(p, st);
    else launch_t<64, 32, 2, 1, ALOAD, BNC, EPI>(p, st);
  }
}


// ---------------------------------------------------------------------------------------
// bf16 MFMA variant (the "bf16" precision mode): v_mfma_f32_32x32x16_bf16, f32 accumulate.
// A is f32 (rounded to bf16, RNE, while staging) or bf16; B = weights pre-converted to bf16
// [N][K].  LDS images are row-major [row][BK + 8] bf16 (odd multiple of 16 B per row:
// conflict-free ds_read_b128 of the 8-element k-fragments), two stages, next stage's global
// loads in registers under the MFMAs.  The epilogue goes through LDS one 32x32 fragment per
// wave at a time so that bias / activation / residual run on float4 rows and every global
// access is a 16-byte vector.  Tiles are numbered so that the blocks sharing an A row-panel
// land on the same XCD (blocks are dealt round-robin over the 8 XCDs, each with its own L2):
// A is fetched from HBM once, not once per N tile.
// ---------------------------------------------------------------------------------------

template <int ALOAD, typename TA>
__device__ __forceinline__ bf16x8 load_a8(const GemmParams& p, const TA* A, int M, int K, int lda,
                                          int gm, int gk) {
  bf16x8 v;
  if constexpr (std::is_same<TA, __bf16>::value) {
    // unconditional, clamped (K % 8 == 0); the implicit-im2col loaders take the 8 channels
    // of one (time, freq) input position (k % 8 == 0 keeps them contiguous)
    const bool ok = gm < M && gk < K;
    const int m = gm < M ? gm : M - 1;
    const int k = gk < K ? gk : K - 8;
    if constexpr (ALOAD == ALOAD_DENSE) {
      v = *reinterpret_cast<const bf16x8*>(A + (long)m * lda + k);
    } else if constexpr (ALOAD == ALOAD_CONV2) {
      const int t = m / 39, f = m - t * 39;
      const int kk = k >> 3;
      const int kt = kk / 3, kf = kk - kt * 3;
      v = *reinterpret_cast<const bf16x8*>(A + ((long)(2 * t + kt) * 80 + 2 * f + kf) * 8);
    } else {  // ALOAD_CONV3
      const int t = m / 19, f = m - t * 19;
      const int kk = k >> 5, c = k & 31;
      const int kt = kk / 3, kf = kk - kt * 3;
      v = *reinterpret_cast<const bf16x8*>(A + ((long)(t + kt) * 39 + 2 * f + kf) * 32 + c);
    }
    if (!ok) {
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = (__bf16)0.f;
    }
  } else {
    const float4 x0 = load_a4<ALOAD>(p, A, M, K, lda, gm, gk);
    const float4 x1 = load_a4<ALOAD>(p, A, M, K, lda, gm, gk + 4);
    v[0] = (__bf16)x0.x; v[1] = (__bf16)x0.y; v[2] = (__bf16)x0.z; v[3] = (__bf16)x0.w;
    v[4] = (__bf16)x1.x; v[5] = (__bf16)x1.y; v[6] = (__bf16)x1.z; v[7] = (__bf16)x1.w;
  }
  return v;
}

template <int BM, int BN, int BK, int WAVES_M, int WAVES_N, int ALOAD, int EPI, typename TA,
          typename TC, bool DEEP>
// 8-wave tiles: hold 4 waves per SIMD (<= 128 VGPRs, two blocks per CU); at 130 VGPRs the
// f32-A variants drop to one block per CU (tools/gemm_bench: 53 -> 64 us)
__global__ __launch_bounds__(64 * WAVES_M* WAVES_N)
__attribute__((amdgpu_waves_per_eu(WAVES_M * WAVES_N >= 8 ? 4 : 1))) void gemm_bf16_kernel(GemmParams p,
                                                                          const __bf16* Bw,
                                                                          int tiles_n,
                                                                          int tiles_m) {
  constexpr int NT = 64 * WAVES_M * WAVES_N;
  constexpr int WTM = BM / WAVES_M;
  constexpr int WTN = BN / WAVES_N;
  constexpr int FM = WTM / 32;
  constexpr int FN = WTN / 32;
  static_assert(FM >= 1 && FN >= 1, "wave tile must be a multiple of 32x32");
  constexpr int LDH = BK + 8;
  constexpr int GPR = BK / 8;         // 8-element groups per row
  constexpr int A_G = BM * GPR;
  constexpr int B_G = BN * GPR;
  constexpr int A_LD = (A_G + NT - 1) / NT;
  constexpr int B_LD = (B_G + NT - 1) / NT;
  constexpr int STAGE = (BM + BN) * LDH;  // bf16 elements
  constexpr int LDE = kEpiLd;             // epilogue fragment row stride (floats)
  // bf16 C without side inputs: two adjacent 32x32 fragments go through LDS together so that
  // every row segment is one 128-byte line written by 8 lanes x 16 bytes (one fragment alone
  // gives 64-byte half lines of 8-byte stores)
  constexpr bool PAIR = std::is_same<TC, __bf16>::value && FN % 2 == 0 && EPI != EPI_MULAUX &&
                        EPI != EPI_MULAUX16 && EPI != EPI_RESADD && EPI != EPI_GLU && BM <= 128;
  constexpr int LDE2 = 72;                // paired epilogue row stride (floats)
  constexpr int OPER_BYTES = 2 * STAGE * 2;
  constexpr int EPI_BYTES = (NT / 64) * 32 * (PAIR ? LDE2 : LDE) * 4;
  constexpr int LDS_BYTES = OPER_BYTES > EPI_BYTES ? OPER_BYTES : EPI_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
  __bf16* const sbase = reinterpret_cast<__bf16*>(smem);

  const TA* A = reinterpret_cast<const TA*>(p.A);
  TC* C = reinterpret_cast<TC*>(p.C);
  const float* aux = p.aux;
  const __bf16* aux16 = EPI == EPI_MULAUX16 ? reinterpret_cast<const __bf16*>(p.aux) : nullptr;
  int M = p.M, K = p.K, lda = p.lda;
  long b_off = 0;
  // one linear grid over (slice, tile): the XCD grouping below then keeps the N tiles of
  // one (slice, row panel) on one XCD for every slice, not only when tiles % 8 == 0
  const int tiles = tiles_n * tiles_m;
  const int lin = xcd_tile(blockIdx.x, gridDim.x);
  const int zs = lin / tiles;
  if (p.slices) {
    const GemmSlice s = p.slices[zs];
    A += s.a_off;
    b_off = s.b_off;
    C += s.c_off;
    if (aux) aux += s.aux_off;
    if (aux16) aux16 += s.aux_off;
    M = s.M;
    K = s.K;
    lda = s.lda;
  }
  const __bf16* B = Bw + b_off;
  const int tile = lin - zs * tiles;
  const int m_tile = tile / tiles_n;
  const int m0 = m_tile * BM;
  if (m0 >= M) return;
  const int n0 = (tile - m_tile * tiles_n) * BN;
  const int N = p.N;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid / WAVES_N;
  const int wn = wid - wm * WAVES_N;

  bf16x8 ra[A_LD], rb[B_LD];
  // dense operands: the per-thread row pointers are k-invariant (rows past M / N are clamped
  // to a valid row: they only feed outputs that are never stored), so a full slab costs one
  // pointer add per load; only a K tail slab takes the clamped, zero-filling path
  const TA* arow[A_LD];
  const __bf16* brow[B_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const int idx = tid + NT * i;
    const int row = (idx < A_G ? idx : 0) / GPR, k8 = idx % GPR;
    const int gm = m0 + row < M ? m0 + row : M - 1;
    arow[i] = A + (long)gm * lda + 8 * k8;
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int idx = tid + NT * i;
    const int n = (idx < B_G ? idx : 0) / GPR, k8 = idx % GPR;
    const int gn = n0 + n < N ? n0 + n : N - 1;
    brow[i] = B + (long)gn * p.sbn + 8 * k8;
  }
  auto to_bf16x8 = [](float4 x0, float4 x1) {
    bf16x8 v;
    v[0] = (__bf16)x0.x; v[1] = (__bf16)x0.y; v[2] = (__bf16)x0.z; v[3] = (__bf16)x0.w;
    v[4] = (__bf16)x1.x; v[5] = (__bf16)x1.y; v[6] = (__bf16)x1.z; v[7] = (__bf16)x1.w;
    return v;
  };
  auto gload = [&](int kt) {
    const int k0 = kt * BK;
    if (ALOAD == ALOAD_DENSE && k0 + BK <= K) {
#pragma unroll
      for (int i = 0; i < A_LD; ++i) {
        if constexpr (std::is_same<TA, __bf16>::value) {
          ra[i] = *reinterpret_cast<const bf16x8*>(arow[i] + k0);
        } else {
          const float* a = reinterpret_cast<const float*>(arow[i]) + k0;
          ra[i] = to_bf16x8(*reinterpret_cast<const float4*>(a), *reinterpret_cast<const float4*>(a + 4));
        }
      }
#pragma unroll
      for (int i = 0; i < B_LD; ++i) rb[i] = *reinterpret_cast<const bf16x8*>(brow[i] + k0);
      return;
    }
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const int idx = tid + NT * i;
      const int row = idx / GPR, k8 = idx % GPR;
      ra[i] = load_a8<ALOAD, TA>(p, A, M, K, lda, m0 + (idx < A_G ? row : 0), kt * BK + 8 * k8);
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int idx = tid + NT * i;
      const int n = idx / GPR, k8 = idx % GPR;
      const int gn = n0 + n, gk = kt * BK + 8 * k8;
      const bool ok = idx < B_G && gn < N && gk < K;
      const int nc = gn < N ? gn : N - 1, kc = gk < K ? gk : K - 8;
      bf16x8 v = *reinterpret_cast<const bf16x8*>(B + (long)nc * p.sbn + kc);
      if (!ok) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (__bf16)0.f;
      }
      rb[i] = v;
    }
  };
  auto sstore = [&](int buf) {
    __bf16* As = sbase + buf * STAGE;
    __bf16* Bs = As + BM * LDH;
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const int idx = tid + NT * i;
      if (idx < A_G) *reinterpret_cast<bf16x8*>(&As[(idx / GPR) * LDH + 8 * (idx % GPR)]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int idx = tid + NT * i;
      if (idx < B_G) *reinterpret_cast<bf16x8*>(&Bs[(idx / GPR) * LDH + 8 * (idx % GPR)]) = rb[i];
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nkt = (K + BK - 1) / BK;
  auto mma_slab = [&](int cur) {
    const __bf16* As = sbase + cur * STAGE;
    const __bf16* Bs = As + BM * LDH;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(
            &As[(wm * WTM + i * 32 + (lane & 31)) * LDH + ks * 16 + 8 * (lane >> 5)]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(
            &Bs[(wn * WTN + j * 32 + (lane & 31)) * LDH + ks * 16 + 8 * (lane >> 5)]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };
  if constexpr (DEEP) {
    // dense A, K a multiple of 2 BK (host-checked): two register sets, so each K slab's loads
    // have two slabs of MFMAs to land; the barriers are LDS-only (__syncthreads would drain
    // the slab in flight with vmcnt(0)); every load is unconditional (slab index clamped), so
    // the in-order vmcnt waits stay exact
    bf16x8 xa[2][A_LD], xb[2][B_LD];
    auto gl = [&](bf16x8 (&ra_)[A_LD], bf16x8 (&rb_)[B_LD], int kt) {
      const int k0 = kt * BK;
#pragma unroll
      for (int i = 0; i < A_LD; ++i) {
        if constexpr (std::is_same<TA, __bf16>::value) {
          ra_[i] = *reinterpret_cast<const bf16x8*>(arow[i] + k0);
        } else {
          const float* a = reinterpret_cast<const float*>(arow[i]) + k0;
          ra_[i] = to_bf16x8(*reinterpret_cast<const float4*>(a), *reinterpret_cast<const float4*>(a + 4));
        }
      }
#pragma unroll
      for (int i = 0; i < B_LD; ++i) rb_[i] = *reinterpret_cast<const bf16x8*>(brow[i] + k0);
    };
    auto ss = [&](const bf16x8 (&ra_)[A_LD], const bf16x8 (&rb_)[B_LD], int buf) {
      __bf16* As = sbase + buf * STAGE;
      __bf16* Bs = As + BM * LDH;
#pragma unroll
      for (int i = 0; i < A_LD; ++i) {
        const int idx = tid + NT * i;
        if (idx < A_G) *reinterpret_cast<bf16x8*>(&As[(idx / GPR) * LDH + 8 * (idx % GPR)]) = ra_[i];
      }
#pragma unroll
      for (int i = 0; i < B_LD; ++i) {
        const int idx = tid + NT * i;
        if (idx < B_G) *reinterpret_cast<bf16x8*>(&Bs[(idx / GPR) * LDH + 8 * (idx % GPR)]) = rb_[i];
      }
    };
    auto bar = []() {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
    gl(xa[0], xb[0], 0);
    gl(xa[1], xb[1], 1);
    ss(xa[0], xb[0], 0);
    bar();
    for (int kt = 0; kt < nkt; kt += 2) {
      gl(xa[0], xb[0], min(kt + 2, nkt - 1));
      mma_slab(0);
      ss(xa[1], xb[1], 1);
      bar();
      gl(xa[1], xb[1], min(kt + 3, nkt - 1));
      mma_slab(1);
      ss(xa[0], xb[0], 0);
      bar();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped tail loads
  } else {
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nkt) gload(kt + 1);
    const __bf16* As = sbase + cur * STAGE;
    const __bf16* Bs = As + BM * LDH;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i)
        a[i] = *reinterpret_cast<const bf16x8*>(
            &As[(wm * WTM + i * 32 + (lane & 31)) * LDH + ks * 16 + 8 * (lane >> 5)]);
#pragma unroll
      for (int j = 0; j < FN; ++j)
        b[j] = *reinterpret_cast<const bf16x8*>(
            &Bs[(wn * WTN + j * 32 + (lane & 31)) * LDH + ks * 16 + 8 * (lane >> 5)]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nkt) sstore(cur ^ 1);
    __syncthreads();
  }
  }

  if constexpr (PAIR) {
    if (N % 8 == 0 && p.ldc % 8 == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0) {
      float* sP = reinterpret_cast<float*>(smem) + wid * (32 * LDE2);
      const int c8 = lane & 7;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int j = 0; j < FN; j += 2) {
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r)
              sP[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LDE2 + 32 * h + (lane & 31)] =
                  acc[i][j + h][r];
          __builtin_amdgcn_wave_barrier();
          const int col = n0 + wn * WTN + j * 32 + 8 * c8;
          float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
          if (p.bias && col < N) {
            b0 = *reinterpret_cast<const float4*>(p.bias + col);
            b1 = *reinterpret_cast<const float4*>(p.bias + col + 4);
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rl = (lane >> 3) + 8 * q;
            const int row = m0 + wm * WTM + i * 32 + rl;
            const float4 v0 = *reinterpret_cast<const float4*>(&sP[rl * LDE2 + 8 * c8]);
            const float4 v1 = *reinterpret_cast<const float4*>(&sP[rl * LDE2 + 8 * c8 + 4]);
            if (row < M && col < N) {
              bf16x8 hv;
              hv[0] = (__bf16)epi_act<EPI>(v0.x + b0.x);
              hv[1] = (__bf16)epi_act<EPI>(v0.y + b0.y);
              hv[2] = (__bf16)epi_act<EPI>(v0.z + b0.z);
              hv[3] = (__bf16)epi_act<EPI>(v0.w + b0.w);
              hv[4] = (__bf16)epi_act<EPI>(v1.x + b1.x);
              hv[5] = (__bf16)epi_act<EPI>(v1.y + b1.y);
              hv[6] = (__bf16)epi_act<EPI>(v1.z + b1.z);
              hv[7] = (__bf16)epi_act<EPI>(v1.w + b1.w);
              *reinterpret_cast<bf16x8*>(C + (long)row * p.ldc + col) = hv;
            }
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      return;
    }
  }
  tile_epilogue<EPI, TC, FM, FN>(C, p.ldc, M, N, p.bias,
                                 EPI == EPI_MULAUX16 ? (const void*)aux16 : (const void*)aux,
                                 p.ldaux, p.byp_orig, p.byp_scale,
                                 reinterpret_cast<float*>(smem) + wid * (32 * LDE), m0 + wm * WTM,
                                 n0 + wn * WTN, lane, acc);
}

// gemm_set_deep(0) turns the two-slab register prefetch off (the labs' A/B switch)
static int g_gemm_deep = -1;
void gemm_set_deep(int on) { g_gemm_deep = g_gemm_f32_deep = on; }

template <int BM, int BN, int BK, int WM, int WN, int ALOAD, int EPI, typename TA, typename TC>
void launch_h(const GemmParams& p, const __bf16* Bw, hipStream_t st) {
  const int tn = cdiv(p.N, BN), tm = cdiv(p.max_M, BM);
  dim3 grid(tn * tm * (p.slices ? p.num_slices : 1));
  if (g_gemm_deep < 0) g_gemm_deep = 1;
  if (g_gemm_deep && ALOAD == ALOAD_DENSE && !p.slices && p.K % (2 * BK) == 0 && p.lda % 8 == 0) {
    ZASR_LAUNCH((gemm_bf16_kernel<BM, BN, BK, WM, WN, ALOAD, EPI, TA, TC, true>), grid,
                       dim3(64 * WM * WN), 0, st, p, Bw, tn, tm);
    return;
  }
  ZASR_LAUNCH((gemm_bf16_kernel<BM, BN, BK, WM, WN, ALOAD, EPI, TA, TC, false>), grid,
                     dim3(64 * WM * WN), 0, st, p, Bw, tn, tm);
}

template <int BK, int ALOAD, int EPI, typename TA, typename TC>
void launch_tile_h(const GemmParams& p, const __bf16* Bw, hipStream_t st) {
  // the sliced NonlinAttention GEMM streams a K = L-deep A panel per N tile: a 32-wide tile
  // re-reads it N/32 times at one MFMA per wave per k-step -- take 64 despite the padding
  const auto [BN, big] = pick_tile(p, EPI == EPI_MULAUX || EPI == EPI_MULAUX16);
  // wide tiles: 128 x 256 on 8 waves (2 x 4, 64 x 64 each) for N >= 256 -- twice the MFMAs
  // per A slab and per barrier of the 128 x 128 kernel, each A row panel read by half as many
  // blocks; measured -5 % enc_gemm time at the bench's shapes (profiles/r01/v15_gemm_tiles.txt).
  // (256 x 128 on 8 waves, and 128 x 256 for N >= 512 only, measured slower; 256 x 256 7 %
  // slower.)  A two-slab register prefetch (two K slabs in flight in two register sets behind
  // the LDS slab) measured enc_gemm 16.7 -> 21.1 ms per step and was dropped (v17)
  if (BN == 128 && big && p.N >= 256) {
    launch_h<128, 256, BK, 2, 4, ALOAD, EPI, TA, TC>(p, Bw, st);
    return;
  }
  if (BN == 128) {
    if (big) launch_h<128, 128, BK, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
    else launch_h<64, 128, BK, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
  } else if (BN == 64) {
    if (big) launch_h<128, 64, BK, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
    else launch_h<64, 64, BK, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
  } else {
    if (big) launch_h<128, 32, BK, 4, 1, ALOAD, EPI, TA, TC>(p, Bw, st);
    else launch_h<64, 32, BK, 2, 1, ALOAD, EPI, TA, TC>(p, Bw, st);
  }
}

// ---------------------------------------------------------------------------------------
// Multi-stage LDS-DMA variant (K % 32 == 0, dense A, no z-slices).  The register-staged
// kernel above keeps one 32-deep K slab in flight, so every slab pays a full memory round
// trip behind 8 MFMAs per wave (tools/gemm_lab.hip: the MFMA-heavy FFN shapes run at
// ~15 % of peak).  Here each wave issues global_load_lds (16 B per lane, no VGPR destination)
// for its share of the slab NS - 1 slabs ahead; the loop waits with a counted vmcnt for the
// slab it is about to read, so NS - 2 slabs stay in flight across the raw s_barrier.
// LDS images are lane-linear per 1 KB wave instruction (the DMA destination is base +
// 16 * lane), bank-conflict-free for the fragment ds_read_b128 by an XOR swizzle applied to
// the per-lane GLOBAL address:
//   bf16 rows (64 B):  16-byte chunk c of row r stored at chunk c ^ ((r >> 2) & 3)
//   f32 rows (128 B):  chunk c of row r stored at chunk c ^ ((r >> 1) & 7)
// f32 A (the residual stream) is staged as f32 and rounded to bf16 at the fragment read.
// All LDS is one __shared__ array and the loop has no ordinary global loads (either would
// make hipcc drain the DMA queue with vmcnt(0)).
// ---------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __forceinline__ void glds16(const void* g, unsigned char* lds_base) {
  __builtin_amdgcn_global_load_lds(const_cast<void*>(g), (lds_ptr_t)(lds_base), 16, 0, 0);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// BN = 64 / 128 / 192 (the four waves split it in two halves); SL: z-slices (one linear grid over
// (slice, tile); every slice's K a multiple of 32) -- the NonlinAttention product A0 @ t1 per
// sequence, whose K = L-deep panels the register-staged kernel streams one slab at a time
template <int NS, int EPI, typename TA, typename TC, int BN = 128, bool SL = false>
__global__ __launch_bounds__(256) void gemm_glds_kernel(GemmParams p, const __bf16* Bw,
                                                        int tiles_n, int tiles_m = 0) {
  constexpr int BM = 128, BK = 32;
  constexpr int FN = BN / 64;  // 32-wide fragments per wave along N
  constexpr bool AF32 = std::is_same<TA, float>::value;
  constexpr int A_BYTES = BM * BK * (AF32 ? 4 : 2);
  constexpr int B_BYTES = BN * BK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int GA = A_BYTES / 1024 / 4;  // DMA instructions per wave per slab
  constexpr int GB = B_BYTES / 1024 / 4;
  constexpr int G = GA + GB;
  constexpr int LDE = kEpiLd;
  constexpr int EPI_BYTES = 4 * 32 * LDE * 4;
  constexpr int LDS_BYTES = NS * STAGE > EPI_BYTES ? NS * STAGE : EPI_BYTES;
  static_assert(NS >= 2 && NS <= 4, "stages");
  __shared__ __attribute__((aligned(1024))) unsigned char smem[LDS_BYTES];

  const TA* A = reinterpret_cast<const TA*>(p.A);
  TC* C = reinterpret_cast<TC*>(p.C);
  const __bf16* aux16 = EPI == EPI_MULAUX16 ? reinterpret_cast<const __bf16*>(p.aux) : nullptr;
  int M = p.M, K = p.K, lda = p.lda;
  int tile = xcd_tile(blockIdx.x, gridDim.x);
  const __bf16* B = Bw;
  if constexpr (SL) {
    const int zs = tile / (tiles_n * tiles_m);
    tile -= zs * tiles_n * tiles_m;
    const GemmSlice sl = p.slices[zs];
    A += sl.a_off;
    B += sl.b_off;
    C += sl.c_off;
    if (aux16) aux16 += sl.aux_off;
    M = sl.M;
    K = sl.K;
    lda = sl.lda;
  }
  const int m_tile = tile / tiles_n;
  const int m0 = m_tile * BM;
  if (SL && m0 >= M) return;
  const int n0 = (tile - m_tile * tiles_n) * BN;
  const int N = p.N;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int nkt = K / BK;

  // per-lane global source pointers of this wave's DMA instructions (slab 0)
  const TA* asrc[GA];
  const __bf16* bsrc[GB];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int ins = wid * GA + g;
    if constexpr (AF32) {
      const int row = ins * 8 + (lane >> 3);
      const int lc = (lane & 7) ^ ((row >> 1) & 7);
      const int gr = m0 + row < M ? m0 + row : M - 1;
      asrc[g] = A + (long)gr * lda + 4 * lc;
    } else {
      const int row = ins * 16 + (lane >> 2);
      const int lc = (lane & 3) ^ ((row >> 2) & 3);
      const int gr = m0 + row < M ? m0 + row : M - 1;
      asrc[g] = A + (long)gr * lda + 8 * lc;
    }
  }
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    const int ins = wid * GB + g;
    const int row = ins * 16 + (lane >> 2);
    const int lc = (lane & 3) ^ ((row >> 2) & 3);
    const int gn = n0 + row < N ? n0 + row : N - 1;
    bsrc[g] = B + (long)gn * p.sbn + 8 * lc;
  }
  auto issue = [&](int kt) {
    unsigned char* st = smem + (kt % NS) * STAGE;
    const int k0 = kt * BK;
#pragma unroll
    for (int g = 0; g < GA; ++g) glds16(asrc[g] + k0, st + (wid * GA + g) * 1024);
#pragma unroll
    for (int g = 0; g < GB; ++g) glds16(bsrc[g] + k0, st + A_BYTES + (wid * GB + g) * 1024);
  };

  f32x16 acc[2][FN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nkt) issue(s);
  const int r32 = lane & 31, h = lane >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    const int ahead = nkt - 1 - kt < NS - 2 ? nkt - 1 - kt : NS - 2;
    if (ahead >= 2) wait_vmcnt<2 * G>();
    else if (ahead == 1) wait_vmcnt<G>();
    else wait_vmcnt<0>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + NS - 1 < nkt) issue(kt + NS - 1);  // the buffer every wave finished reading
    const unsigned char* st = smem + (kt % NS) * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ch = 2 * ks + h;  // 16-byte bf16 chunk of the fragment's k range
      bf16x8 a[2], b[FN];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + r32;
        if constexpr (AF32) {
          const int sw = (row >> 1) & 7;
          const float4 x0 = *reinterpret_cast<const float4*>(st + row * 128 + (((2 * ch) ^ sw) << 4));
          const float4 x1 = *reinterpret_cast<const float4*>(st + row * 128 + (((2 * ch + 1) ^ sw) << 4));
          a[i][0] = (__bf16)x0.x; a[i][1] = (__bf16)x0.y; a[i][2] = (__bf16)x0.z; a[i][3] = (__bf16)x0.w;
          a[i][4] = (__bf16)x1.x; a[i][5] = (__bf16)x1.y; a[i][6] = (__bf16)x1.z; a[i][7] = (__bf16)x1.w;
        } else {
          a[i] = *reinterpret_cast<const bf16x8*>(st + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4));
        }
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int row = wn * (BN / 2) + j * 32 + r32;
        b[j] = *reinterpret_cast<const bf16x8*>(st + A_BYTES + row * 64 + ((ch ^ ((row >> 2) & 3)) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();  // every DMA retired (vmcnt(0) above) and every stage read: reuse smem

  tile_epilogue<EPI, TC, 2, FN>(C, p.ldc, M, N, p.bias, aux16, p.ldaux, p.byp_orig, p.byp_scale,
                                reinterpret_cast<float*>(smem) + wid * (32 * kEpiLd),
                                m0 + wm * 64, n0 + wn * (BN / 2), lane, acc);
}

template <int NS, int EPI, typename TA, typename TC>
void launch_glds(const GemmParams& p, const __bf16* Bw, hipStream_t st) {
  const int tn = cdiv(p.N, 128), tm = cdiv(p.M, 128);
  ZASR_LAUNCH((gemm_glds_kernel<NS, EPI, TA, TC>), dim3(tn * tm), dim3(256), 0, st, p, Bw,
                     tn);
}


// the multi-stage kernel for the long-K / wide-N projections (dense, K % 32 == 0)
template <int EPI, typename TA, typename TC>
bool try_glds(const GemmParams& p, const __bf16* Bw, hipStream_t st) {
  // measured (tools/rp_bench.hip): ahead of the register-staged kernel only on the long-K
  // bf16-A output projections (K >= 1024: +11 %); behind it on the short-K / f32-A shapes
  if (p.slices != nullptr || p.K % 32 != 0 || p.K < 128 || p.M < 128) return false;
  if (std::is_same<TA, float>::value || p.K < 1024) return false;
  if (p.lda % (std::is_same<TA, float>::value ? 4 : 8) != 0 || p.sbn % 8 != 0) return false;
  if (std::is_same<TA, float>::value)
    launch_glds<3, EPI, TA, TC>(p, Bw, st);
  else
    launch_glds<4, EPI, TA, TC>(p, Bw, st);
  return true;
}

// Measured tile per projection shape of the Zipformer stacks (tools/gemm_tune.hip over the
// bench's shape table, profiles/r03/gemm_tune/): every variant accumulates each output over
// the same 32-deep K slabs in the same MFMA order, so the choice changes speed only (the lab
// checks the outputs are bit-identical).  Used for large row counts (the batched encoder);
// other shapes keep the generic heuristics below.  enc_gemm 7.87 -> 7.40 ms in the lab.
enum TunedTile { TT_NONE, TT_GLDS3, TT_GLDS3_192, TT_64x64, TT_64x128, TT_128x64, TT_128x128, TT_256x128 };
struct TunedEntry {
  short K, N;
  signed char a16, c16, epi;
  signed char tile;
};
constexpr TunedEntry kTuned[] = {
    // residual projections: bf16 A -> f32 C += (EPI_RESADD)
    {384, 384, 1, 0, EPI_RESADD, TT_GLDS3},   {288, 384, 1, 0, EPI_RESADD, TT_GLDS3},
    {256, 256, 1, 0, EPI_RESADD, TT_128x64},  {192, 256, 1, 0, EPI_RESADD, TT_64x128},
    {48, 384, 1, 0, EPI_RESADD, TT_64x64},    {48, 256, 1, 0, EPI_RESADD, TT_64x64},
    {48, 192, 1, 0, EPI_RESADD, TT_64x64},    {96, 512, 1, 0, EPI_RESADD, TT_64x64},
    {144, 192, 1, 0, EPI_RESADD, TT_64x64},
    // in-projections from the f32 residual stream -> bf16
    {384, 864, 0, 1, EPI_NONE, TT_128x128},   {192, 384, 0, 1, EPI_NONE, TT_128x128},
    {192, 272, 0, 1, EPI_NONE, TT_128x128},   {384, 272, 0, 1, EPI_NONE, TT_128x128},
    {256, 272, 0, 1, EPI_NONE, TT_256x128},   {256, 576, 0, 1, EPI_NONE, TT_256x128},
    {512, 544, 0, 1, EPI_NONE, TT_256x128},   {512, 96, 0, 1, EPI_NONE, TT_64x128},
    {384, 48, 0, 1, EPI_NONE, TT_128x64},     {256, 48, 0, 1, EPI_NONE, TT_64x64},
    {192, 48, 0, 1, EPI_NONE, TT_64x64},
    // Conv2dSubsampling output linear (K = 128 channels x 19 freq): one 192-wide column tile,
    // so the 2432-deep A panel is streamed once (399 -> 333 us, profiles/r03/gemm_tune/bn192/)
    {2432, 192, 1, 0, EPI_NONE, TT_GLDS3_192},
};

template <int EPI, typename TA, typename TC>
int tuned_tile(const GemmParams& p) {
  static const bool off = getenv("ZASR_GEMM_TUNED") != nullptr && atoi(getenv("ZASR_GEMM_TUNED")) == 0;
  if (off || p.slices != nullptr || p.M < 16384 || p.lda != p.K || p.sbn % 8 != 0) return TT_NONE;
  const int a16 = std::is_same<TA, __bf16>::value, c16 = std::is_same<TC, __bf16>::value;
  for (const TunedEntry& e : kTuned)
    if (e.K == p.K && e.N == p.N && e.a16 == a16 && e.c16 == c16 && e.epi == EPI) return e.tile;
  return TT_NONE;
}

// BK = 32: at these K (72..1920) the 2-stage 64-deep variant measured 20-60 % slower (LDS
// occupancy), tools/gemm_bench.hip
template <int ALOAD, int EPI, typename TA, typename TC>
void launch_bk_h(const GemmParams& p, const __bf16* Bw, hipStream_t st) {
  if constexpr (ALOAD == ALOAD_DENSE && EPI != EPI_MULAUX && EPI != EPI_MULAUX16) {
    switch (tuned_tile<EPI, TA, TC>(p)) {
      case TT_GLDS3:
        if (p.K % 32 == 0 && p.K >= 128 && p.lda % 8 == 0) return launch_glds<3, EPI, TA, TC>(p, Bw, st);
        break;
      case TT_GLDS3_192:
        if (p.K % 32 == 0 && p.K >= 128 && p.lda % 8 == 0 && p.N % 192 == 0) {
          const int tn = p.N / 192, tm = cdiv(p.M, 128);
          ZASR_LAUNCH((gemm_glds_kernel<3, EPI, TA, TC, 192, false>), dim3(tn * tm), dim3(256),
                             0, st, p, Bw, tn);
          return;
        }
        break;
      case TT_64x64: return launch_h<64, 64, 32, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
      case TT_64x128: return launch_h<64, 128, 32, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
      case TT_128x64: return launch_h<128, 64, 32, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
      case TT_128x128: return launch_h<128, 128, 32, 2, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
      case TT_256x128: return launch_h<256, 128, 32, 4, 2, ALOAD, EPI, TA, TC>(p, Bw, st);
      default: break;
    }
    if (try_glds<EPI, TA, TC>(p, Bw, st)) return;
  }
  launch_tile_h<32, ALOAD, EPI, TA, TC>(p, Bw, st);
}

}  // namespace

void gemm_f32(const GemmParams& p, int epi, int aload, bool b_ncontig, hipStream_t st) {
  ZASR_REQUIRE(p.N > 0, "gemm: N must be positive");
  if (p.max_M <= 0) return;
  ZASR_REQUIRE(p.slices != nullptr || (p.lda % 4 == 0 && p.K % 4 == 0),
               "gemm: lda and K must be multiples of 4");
  if (aload == ALOAD_DENSE && !b_ncontig) {
    switch (epi) {
      case EPI_NONE: return launch_tile<ALOAD_DENSE, false, EPI_NONE>(p, st);
      case EPI_SWOOSHL: return launch_tile<ALOAD_DENSE, false, EPI_SWOOSHL>(p, st);
      case EPI_SWOOSHR: return launch_tile<ALOAD_DENSE, false, EPI_SWOOSHR>(p, st);
      case EPI_RESADD: return launch_tile<ALOAD_DENSE, false, EPI_RESADD>(p, st);
      case EPI_RELU: return launch_tile<ALOAD_DENSE, false, EPI_RELU>(p, st);
      case EPI_GELU: return launch_tile<ALOAD_DENSE, false, EPI_GELU>(p, st);
      case EPI_LEAKY: return launch_tile<ALOAD_DENSE, false, EPI_LEAKY>(p, st);
      case EPI_PRELU: return launch_tile<ALOAD_DENSE, false, EPI_PRELU>(p, st);
      case EPI_RELUMUL: return launch_tile<ALOAD_DENSE, false, EPI_RELUMUL>(p, st);
      case EPI_MULAUX: return launch_tile<ALOAD_DENSE, false, EPI_MULAUX>(p, st);
      default: break;
    }
  } else if (aload == ALOAD_DENSE && b_ncontig) {
    switch (epi) {
      case EPI_NONE: return launch_tile<ALOAD_DENSE, true, EPI_NONE>(p, st);
      case EPI_MULAUX: return launch_tile<ALOAD_DENSE, true, EPI_MULAUX>(p, st);
      default: break;
    }
  } else if (aload == ALOAD_CONV2 && !b_ncontig && epi == EPI_SWOOSHR) {
    return launch_tile<ALOAD_CONV2, false, EPI_SWOOSHR>(p, st);
  } else if (aload == ALOAD_CONV3 && !b_ncontig && epi == EPI_SWOOSHR) {
    return launch_tile<ALOAD_CONV3, false, EPI_SWOOSHR>(p, st);
  } else if (aload == ALOAD_BNRELU && !b_ncontig && !p.slices) {
    ZASR_REQUIRE(p.a_scale && p.a_shift, "gemm_f32: ALOAD_BNRELU needs a_scale / a_shift");
    if (epi == EPI_NONE) return launch_tile<ALOAD_BNRELU, false, EPI_NONE>(p, st);
    if (epi == EPI_RELU) return launch_tile<ALOAD_BNRELU, false, EPI_RELU>(p, st);
  } else if (aload == ALOAD_IM2COL1D && !b_ncontig && !p.slices) {
    ZASR_REQUIRE(p.i2c.C > 0 && p.i2c.C % 4 == 0 && p.i2c.Tout > 0 && p.K % p.i2c.C == 0 &&
                     (long)p.M % p.i2c.Tout == 0,
                 "gemm_f32: bad ALOAD_IM2COL1D geometry");
    if (epi == EPI_NONE) return launch_tile<ALOAD_IM2COL1D, false, EPI_NONE>(p, st);
    if (epi == EPI_RELU) return launch_tile<ALOAD_IM2COL1D, false, EPI_RELU>(p, st);
    if (epi == EPI_MULAUX) return launch_tile<ALOAD_IM2COL1D, false, EPI_MULAUX>(p, st);
  }
  throw std::runtime_error("gemm_f32: unsupported (aload, epi, layout) combination");
}

}  // namespace zasr

namespace zasr {
void gemm_bf16(const GemmParams& p, const void* Bw, int epi, int aload, hipStream_t st,
               bool a_bf16, bool c_bf16) {
  ZASR_REQUIRE(p.N > 0, "gemm: N must be positive");
  if (p.max_M <= 0) return;
  ZASR_REQUIRE(p.N % 4 == 0 && p.ldc % 4 == 0 && ((epi != EPI_MULAUX && epi != EPI_MULAUX16) || p.ldaux % 4 == 0),
               "gemm_bf16: N and the C / aux row strides must be multiples of 4");
  ZASR_REQUIRE(p.slices != nullptr || p.K % 8 == 0, "gemm_bf16: K must be a multiple of 8");
  const __bf16* B = reinterpret_cast<const __bf16*>(Bw);
  if (aload == ALOAD_DENSE && !a_bf16 && !c_bf16) {
    switch (epi) {
      case EPI_NONE: return launch_bk_h<ALOAD_DENSE, EPI_NONE, float, float>(p, B, st);
      case EPI_SWOOSHL: return launch_bk_h<ALOAD_DENSE, EPI_SWOOSHL, float, float>(p, B, st);
      case EPI_SWOOSHR: return launch_bk_h<ALOAD_DENSE, EPI_SWOOSHR, float, float>(p, B, st);
      case EPI_RESADD: return launch_bk_h<ALOAD_DENSE, EPI_RESADD, float, float>(p, B, st);
      default: break;
    }
  } else if (aload == ALOAD_DENSE && !a_bf16 && c_bf16) {
    switch (epi) {
      case EPI_NONE: return launch_bk_h<ALOAD_DENSE, EPI_NONE, float, __bf16>(p, B, st);
      case EPI_SWOOSHL: return launch_bk_h<ALOAD_DENSE, EPI_SWOOSHL, float, __bf16>(p, B, st);
      case EPI_GLU: return launch_bk_h<ALOAD_DENSE, EPI_GLU, float, __bf16>(p, B, st);
      default: break;
    }
  } else if (aload == ALOAD_DENSE && a_bf16 && !c_bf16) {
    switch (epi) {
      case EPI_NONE: return launch_bk_h<ALOAD_DENSE, EPI_NONE, __bf16, float>(p, B, st);
      case EPI_RESADD: return launch_bk_h<ALOAD_DENSE, EPI_RESADD, __bf16, float>(p, B, st);
      default: break;
    }
  } else if (aload == ALOAD_DENSE && a_bf16 && c_bf16) {
    switch (epi) {
      case EPI_NONE: return launch_bk_h<ALOAD_DENSE, EPI_NONE, __bf16, __bf16>(p, B, st);
      case EPI_MULAUX: return launch_bk_h<ALOAD_DENSE, EPI_MULAUX, __bf16, __bf16>(p, B, st);
      case EPI_MULAUX16: return launch_bk_h<ALOAD_DENSE, EPI_MULAUX16, __bf16, __bf16>(p, B, st);
      default: break;
    }
  } else if (aload == ALOAD_CONV2 && epi == EPI_SWOOSHR && !a_bf16 && !c_bf16) {
    return launch_bk_h<ALOAD_CONV2, EPI_SWOOSHR, float, float>(p, B, st);
  } else if (aload == ALOAD_CONV3 && epi == EPI_SWOOSHR && !a_bf16 && !c_bf16) {
    return launch_bk_h<ALOAD_CONV3, EPI_SWOOSHR, float, float>(p, B, st);
  } else if (aload == ALOAD_CONV3 && epi == EPI_SWOOSHR && !a_bf16 && c_bf16) {
    return launch_bk_h<ALOAD_CONV3, EPI_SWOOSHR, float, __bf16>(p, B, st);
  } else if (aload == ALOAD_CONV2 && epi == EPI_SWOOSHR && a_bf16 && c_bf16) {
    return launch_bk_h<ALOAD_CONV2, EPI_SWOOSHR, __bf16, __bf16>(p, B, st);
  } else if (aload == ALOAD_CONV3 && epi == EPI_SWOOSHR && a_bf16 && c_bf16) {
    return launch_bk_h<ALOAD_CONV3, EPI_SWOOSHR, __bf16, __bf16>(p, B, st);
  }
  throw std::runtime_error("gemm_bf16: unsupported (aload, epi, operand types) combination");
}
}  // namespace zasr

namespace zasr {
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst,
                                   long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (__bf16)src[i];
}
__global__ void rows_to_bf16_kernel(const float* __restrict__ src, const float* __restrict__ rs,
                                    __bf16* __restrict__ dst, long n, int K) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (__bf16)(src[i] * rs[i / K]);
}
void convert_rows_to_bf16(const float* src, const float* row_scale, void* dst, long N, int K,
                          hipStream_t st) {
  const long n = N * K;
  if (n <= 0) return;
  ZASR_LAUNCH(rows_to_bf16_kernel, dim3(cdivl(n, 256)), dim3(256), 0, st, src, row_scale,
                     reinterpret_cast<__bf16*>(dst), n, K);
}
void convert_to_bf16(const float* src, void* dst, long n, hipStream_t st) {
  if (n <= 0) return;
  ZASR_LAUNCH(f32_to_bf16_kernel, dim3(cdivl(n, 256)), dim3(256), 0, st, src,
                     reinterpret_cast<__bf16*>(dst), n);
}
}  // namespace zasr
