// Helpers shared by the GEMM translation units (gemm.hip, gemm_x3.hip, gemm_rp.hip): operand
// loaders, the split formats, the fragment epilogue, and the launchers' tile pick.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm.h"

namespace zasr {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// the f16x3 format's piece scale: x = hi + lo * 2^-11 (split_h8 below)
constexpr float kF16Lo = 2048.f;
constexpr float kF16LoInv = 1.f / 2048.f;

// A operand, 4 consecutive k of row gm.  Loads are unconditional (clamped into the valid
// range, zero selected afterwards): a guarded load compiles to a branch with a vmcnt(0) wait,
// which serialises the tile's memory round trips.  Requires M >= 1 and K % 4 == 0.
template <int ALOAD>
__device__ __forceinline__ float4 load_a4(const GemmParams& p, const float* A, int M, int K,
                                          int lda, int gm, int gk) {
  const bool ok = gm < M && gk < K;
  const int m = gm < M ? gm : M - 1;
  const int k = gk < K ? gk : K - 4;
  float4 v;
  if constexpr (ALOAD == ALOAD_DENSE) {
    v = *reinterpret_cast<const float4*>(A + (long)m * lda + k);
  } else if constexpr (ALOAD == ALOAD_CONV2) {
    // out (t, f) of conv.4; k = (kt*3 + kf)*8 + c over conv1 output [T1][80][8]
    const int t = m / 39, f = m - t * 39;
    const int kk = k >> 3, c = k & 7;
    const int kt = kk / 3, kf = kk - kt * 3;
    v = *reinterpret_cast<const float4*>(A + ((long)(2 * t + kt) * 80 + 2 * f + kf) * 8 + c);
  } else if constexpr (ALOAD == ALOAD_CONV3) {
    // out (t, f) of conv.7; k = (kt*3 + kf)*32 + c over conv2 output [L2][39][32]
    const int t = m / 19, f = m - t * 19;
    const int kk = k >> 5, c = k & 31;
    const int kt = kk / 3, kf = kk - kt * 3;
    v = *reinterpret_cast<const float4*>(A + ((long)(t + kt) * 39 + 2 * f + kf) * 32 + c);
  } else if constexpr (ALOAD == ALOAD_BNRELU) {
    v = *reinterpret_cast<const float4*>(A + (long)m * lda + k);
    const float4 s = *reinterpret_cast<const float4*>(p.a_scale + k);
    const float4 b = *reinterpret_cast<const float4*>(p.a_shift + k);
    v = make_float4(fmaxf(fmaf(v.x, s.x, b.x), 0.f), fmaxf(fmaf(v.y, s.y, b.y), 0.f),
                    fmaxf(fmaf(v.z, s.z, b.z), 0.f), fmaxf(fmaf(v.w, s.w, b.w), 0.f));
  } else {  // ALOAD_IM2COL1D
    const GemmIm2col1d& g = p.i2c;
    const int n = m / g.Tout, t = m - n * g.Tout;
    const int q = k / g.C, c = k - q * g.C;
    const int ts = t * g.stride + q * g.dil - g.pad;
    const bool in = ts >= 0 && ts < g.Tin;
    v = *reinterpret_cast<const float4*>(A + ((long)n * g.Tin + (in ? ts : 0)) * lda + c);
    return (ok && in) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

// logical tile of this block (see header comment): XCD x owns tiles [x*per + min(x, rem) ...)
__device__ __forceinline__ int xcd_tile(int b, int nb) {
  const int per = nb >> 3, rem = nb & 7;
  const int xcd = b & 7, slot = b >> 3;
  return xcd < rem ? xcd * (per + 1) + slot : rem * (per + 1) + (xcd - rem) * per + slot;
}

// Tile pick of the generic launchers: BN = the largest of {128, 64, 32} whose padded width is
// within 15 % of the tightest (no32: 64 instead of 32 above N = 64); big = 128-row tiles, from
// 512 blocks of them up.
struct TilePick {
  int BN;
  bool big;
};
inline TilePick pick_tile(const GemmParams& p, bool no32 = false) {
  const int pad128 = cdiv(p.N, 128) * 128, pad64 = cdiv(p.N, 64) * 64, pad32 = cdiv(p.N, 32) * 32;
  int BN = (pad128 * 100 <= pad32 * 115) ? 128 : (pad64 * 100 <= pad32 * 115 ? 64 : 32);
  if (no32 && BN == 32 && p.N > 64) BN = 64;
  const long blocks128 = (long)cdiv(p.max_M, 128) * cdiv(p.N, BN) * (p.slices ? p.num_slices : 1);
  return {BN, blocks128 >= 512};
}

// ---- fragment epilogue of the bf16 / split MFMA kernels ----
// native exp2 / log forms (common.h: ~1e-7 absolute from the libm forms, below the f32 rounding
// of the values they feed; the libm pair made the SwooshL shapes 2-3x slower)
template <int EPI>
__device__ __forceinline__ float epi_act(float v) {
  if constexpr (EPI == EPI_SWOOSHL) return swooshl_fast(v);
  if constexpr (EPI == EPI_SWOOSHR) return swooshr_fast(v);
  return v;
}

constexpr int kEpiLd = 40;  // row stride of a wave's epilogue LDS slice (floats)

// The wave's FM x FN accumulator fragments of 32 x 32, one at a time: acc[i][j] (H3, the f16x3
// format's two accumulators: acc + lo[i % FL][j % FLN] * 2^-11; lane: column lane & 31, rows
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) -> the wave's LDS slice sE (32 x kEpiLd floats) ->
// float4 rows (8 lanes per 32-column row) with bias, activation and the EPI's side input, so
// every global access is a 16-byte vector.  M, N, C, aux and the strides are the z-slice's;
// row0 / col0: the wave's first output row / column.  Side inputs (the old C, the bypass
// operands, an f32 aux) are loaded unconditionally from clamped addresses, all in flight
// before the guarded stores: a guarded load compiles to a branch with its own vmcnt(0).
// EPI_RESADD with byp_orig: the layer's bypass_mid folded in after the residual add.
// (The accumulators come in as arrays, each fragment copied whole before its LDS stores: with
// a functor in their place the 8-wave 256 x 128 bf16 tiles spilled 4 VGPRs at their 128-VGPR
// cap and the 64 x 128 residual tile lost a wave per SIMD, profiles/gemm_epilogue/.)
template <int EPI, typename TC, bool H3, int FM, int FN, int FL, int FLN>
__device__ __forceinline__ void tile_epilogue(TC* C, int ldc, int M, int N, const float* bias,
                                              const void* aux, int ldaux, const float* byp_orig,
                                              const float* byp_scale, float* sE, int row0,
                                              int col0, int lane, const f32x16 (&acc)[FM][FN],
                                              const f32x16 (&lo)[FL][FLN]) {
  constexpr int LDE = kEpiLd;
  constexpr bool F32C = std::is_same<TC, float>::value;
  const int c4 = lane & 7;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x16 fr = acc[i][j], fl = lo[i % FL][j % FLN];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        sE[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * LDE + (lane & 31)] =
            H3 ? fr[r] + fl[r] * kF16LoInv : fr[r];
      __builtin_amdgcn_wave_barrier();
      const int col = col0 + j * 32 + 4 * c4;
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bias && col < N) bv = *reinterpret_cast<const float4*>(bias + col);
      float4 pre_o[4], pre_b[4], pre_k = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr ((EPI == EPI_RESADD && F32C) || EPI == EPI_MULAUX) {
        const int cc = col < N ? col : N - 4;
        if (EPI == EPI_RESADD && byp_orig != nullptr)
          pre_k = *reinterpret_cast<const float4*>(byp_scale + cc);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = row0 + i * 32 + (lane >> 3) + 8 * q;
          const int rc = row < M ? row : M - 1;
          if constexpr (EPI == EPI_RESADD) {
            const long off = (long)rc * ldc + cc;
            pre_o[q] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(C) + off);
            if (byp_orig != nullptr) pre_b[q] = *reinterpret_cast<const float4*>(byp_orig + off);
          } else {
            pre_o[q] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(aux) +
                                                        (long)rc * ldaux + cc);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rl = (lane >> 3) + 8 * q;
        const int row = row0 + i * 32 + rl;
        float4 v = *reinterpret_cast<const float4*>(&sE[rl * LDE + 4 * c4]);
        if (row < M && col < N) {
          v.x = epi_act<EPI>(v.x + bv.x);
          v.y = epi_act<EPI>(v.y + bv.y);
          v.z = epi_act<EPI>(v.z + bv.z);
          v.w = epi_act<EPI>(v.w + bv.w);
          if constexpr (EPI == EPI_MULAUX) {
            v.x *= pre_o[q].x; v.y *= pre_o[q].y; v.z *= pre_o[q].z; v.w *= pre_o[q].w;
          }
          if constexpr (EPI == EPI_MULAUX16) {
            const bf16x4 x = *reinterpret_cast<const bf16x4*>(
                reinterpret_cast<const __bf16*>(aux) + (long)row * ldaux + col);
            v.x *= (float)x[0]; v.y *= (float)x[1]; v.z *= (float)x[2]; v.w *= (float)x[3];
          }
          if constexpr (EPI == EPI_GLU) {  // columns (2c, 2c + 1) -> channel c
            const float g0 = v.x * sigmoid_fast(v.y), g1 = v.z * sigmoid_fast(v.w);
            TC* dst = C + (long)row * ldc + col / 2;
            if constexpr (F32C) {
              *reinterpret_cast<float2*>(dst) = make_float2(g0, g1);
            } else {
              bf16x2 h;
              h[0] = (__bf16)g0; h[1] = (__bf16)g1;
              *reinterpret_cast<bf16x2*>(dst) = h;
            }
            continue;
          }
          TC* dst = C + (long)row * ldc + col;
          if constexpr (F32C) {
            if constexpr (EPI == EPI_RESADD) {
              v.x += pre_o[q].x; v.y += pre_o[q].y; v.z += pre_o[q].z; v.w += pre_o[q].w;
              if (byp_orig != nullptr) bypass_mix(v, pre_b[q], pre_k);
            }
            *reinterpret_cast<float4*>(dst) = v;
          } else {
            bf16x4 h;
            h[0] = (__bf16)v.x; h[1] = (__bf16)v.y; h[2] = (__bf16)v.z; h[3] = (__bf16)v.w;
            *reinterpret_cast<bf16x4*>(dst) = h;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// one accumulator per fragment (H3 false: `lo` is never read, acc stands in for it)
template <int EPI, typename TC, int FM, int FN>
__device__ __forceinline__ void tile_epilogue(TC* C, int ldc, int M, int N, const float* bias,
                                              const void* aux, int ldaux, const float* byp_orig,
                                              const float* byp_scale, float* sE, int row0,
                                              int col0, int lane, const f32x16 (&acc)[FM][FN]) {
  tile_epilogue<EPI, TC, false>(C, ldc, M, N, bias, aux, ldaux, byp_orig, byp_scale, sE, row0, col0,
                                lane, acc, acc);
}

// ---- split-bf16 helpers (the bf16x3 / bf16x6 modes) ----
template <int NP>
__device__ __forceinline__ void split_f8(const float (&v)[8], bf16x8 (&pc)[NP]) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float r = v[q];
#pragma unroll
    for (int t = 0; t < NP; ++t) {
      const __bf16 h = (__bf16)r;
      pc[t][q] = h;
      if (t + 1 < NP) r -= (float)h;
    }
  }
}

// ---- fp16 hi + scaled-lo pieces (the "f16x3" mode) ----
// x = hi + lo * 2^-11 with hi = fp16(x), lo = fp16((x - hi) * 2^11): 11 + 11 significant bits
// (~2^-22 relative; the residual is exact in f32 and its scaled value stays in the fp16 normal
// range wherever hi does).  A product is hi*hi + (hi*lo + lo*hi) * 2^-11: three fp16 MFMAs at
// the bf16 rate, two accumulators.  Operands must stay below 65504 in magnitude.

__device__ __forceinline__ void split_h8(const float (&v)[8], bf16x8 (&pc)[2]) {
  f16x8 h, l;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    h[q] = (_Float16)v[q];
    l[q] = (_Float16)((v[q] - (float)h[q]) * kF16Lo);
  }
  pc[0] = __builtin_bit_cast(bf16x8, h);
  pc[1] = __builtin_bit_cast(bf16x8, l);
}

// FMT 0: NP bf16 pieces (split_f8); FMT 1: the two fp16 pieces (split_h8, NP = 2)
template <int FMT, int NP>
__device__ __forceinline__ void split_fx(const float (&v)[8], bf16x8 (&pc)[NP]) {
  if constexpr (FMT == 1) {
    static_assert(NP == 2, "fp16 format: two pieces");
    split_h8(v, pc);
  } else {
    split_f8<NP>(v, pc);
  }
}

// hi += x0 y0; lo += x1 y0 + x0 y1 (fp16 MFMAs; pieces carried in bf16x8 containers)
__device__ __forceinline__ void mfma_h3(const bf16x8 (&x)[2], const bf16x8 (&y)[2], f32x16& hi,
                                        f32x16& lo) {
  const f16x8 x0 = __builtin_bit_cast(f16x8, x[0]), x1 = __builtin_bit_cast(f16x8, x[1]);
  const f16x8 y0 = __builtin_bit_cast(f16x8, y[0]), y1 = __builtin_bit_cast(f16x8, y[1]);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1, y0, lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0, y1, lo, 0, 0, 0);
  hi = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0, y0, hi, 0, 0, 0);
}

// acc += sum over u + v < NP of x[u] * y[v], smallest terms first (written out: every index
// a constant, so the piece arrays stay in registers)
template <int NP>
__device__ __forceinline__ f32x16 mfma_split(const bf16x8 (&x)[NP], const bf16x8 (&y)[NP], f32x16 acc) {
#define ZASR_MF(u, v) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[u], y[v], acc, 0, 0, 0)
  if constexpr (NP == 3) {
    ZASR_MF(2, 0); ZASR_MF(1, 1); ZASR_MF(0, 2);
  }
  if constexpr (NP >= 2) {
    ZASR_MF(NP - 1 == 1 ? 1 : 1, 0); ZASR_MF(0, 1);
  }
  ZASR_MF(0, 0);
#undef ZASR_MF
  return acc;
}

}  // namespace zasr
