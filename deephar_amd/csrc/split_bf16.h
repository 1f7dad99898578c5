// The split-bf16 arithmetic of the LDS-DMA GEMM family (gemm1x1s.hip says what it computes and why): an fp32 operand as P bf16
// parts, the products kept per mode and their order.  Used by the kernel body (gemm1x1s_body.h), the wide tiling
// (gemm1x1s_launch.h) and the kernels built on the body (gemm1x1s_ext_launch.h, convt2x2s.hip).
#pragma once
#include "conv_common.h"
#include "lds_dma.h"

namespace dh {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// (x0, x1) -> packed bf16 pair (v_cvt_pk_bf16_f32, RNE) and the exact residuals
__device__ __forceinline__ unsigned split_pair(float& x0, float& x1) {
  const f32x2 v = {x0, x1};
  const bf16x2 h = __builtin_convertvector(v, bf16x2);
  const unsigned p = __builtin_bit_cast(unsigned, h);
  x0 -= __uint_as_float(p << 16);
  x1 -= __uint_as_float(p & 0xffff0000u);
  return p;
}
__device__ __forceinline__ unsigned pack_pair(float x0, float x1) {
  const f32x2 v = {x0, x1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// P = number of bf16 parts kept per operand (3: "bf16x3", 2: "bf16x2", 1: plain "bf16"); the products kept are those
// with (a part) + (b part) <= P + 1 (1-based): 6, 3, 1 of them
template <int P> struct Frag { bf16x8 p[P]; };
constexpr int nprod(int P) { return P * (P + 1) / 2; }
// VALU instructions of one split8 (8 of them the ReLU; 8 more, one fused multiply-add per element, with a BN prologue)
constexpr int split_valu(int P, bool PRE = false) { return (P == 3 ? 52 : (P == 2 ? 32 : 12)) + (PRE ? 8 : 0); }

// per-channel scale | shift of the 8 k-values of one split8 (BatchNormalization prologue)
struct Affine8 { float4 sc[2], sh[2]; };

// 8 consecutive k of one row (two float4) -> P bf16x8 operands: P - 1 residual passes, the last part is one
// v_cvt_pk_bf16_f32 per pair.  PRE: x * scale[k] + shift[k] first -- ONE fused multiply-add per element, in front of the
// ReLU, exactly the prologue of the fp32 kernels (gemm1x1_body.h: relu_frags): the operand that is split has the same bits.
template <bool RELU, int P = 3, bool PRE = false>
__device__ __forceinline__ Frag<P> split8(float4 lo4, float4 hi4, const Affine8* af = nullptr) {
  float x[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
  if constexpr (PRE) {
    const float s[8] = {af->sc[0].x, af->sc[0].y, af->sc[0].z, af->sc[0].w, af->sc[1].x, af->sc[1].y, af->sc[1].z, af->sc[1].w};
    const float t[8] = {af->sh[0].x, af->sh[0].y, af->sh[0].z, af->sh[0].w, af->sh[1].x, af->sh[1].y, af->sh[1].z, af->sh[1].w};
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = fmaf(x[i], s[i], t[i]);
  }
  if constexpr (RELU) {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = relu1(x[i]);
  }
  unsigned a[4], b[4], c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = P > 1 ? split_pair(x[2 * i], x[2 * i + 1]) : pack_pair(x[2 * i], x[2 * i + 1]);
  if constexpr (P > 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = P > 2 ? split_pair(x[2 * i], x[2 * i + 1]) : pack_pair(x[2 * i], x[2 * i + 1]);
  }
  if constexpr (P > 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = pack_pair(x[2 * i], x[2 * i + 1]);
  }
  Frag<P> f;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  f.p[0] = __builtin_bit_cast(bf16x8, (u32x4){a[0], a[1], a[2], a[3]});
  if constexpr (P > 1) f.p[1] = __builtin_bit_cast(bf16x8, (u32x4){b[0], b[1], b[2], b[3]});
  if constexpr (P > 2) f.p[2] = __builtin_bit_cast(bf16x8, (u32x4){c[0], c[1], c[2], c[3]});
  return f;
}

__device__ __forceinline__ bf16x8 as_bf(float4 v) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  return __builtin_bit_cast(bf16x8, (f32x4){v.x, v.y, v.z, v.w});
}

// Six partial products, smallest first: (a part, b part) = (2,0) (0,2) (1,1) (1,0) (0,1) (0,0).  They are issued
// product-major over all TM x TN tiles of the wave: consecutive MFMAs then write DIFFERENT accumulators.  Issued
// tile-major (six dependent MFMAs on one accumulator back to back) every MFMA waits out its predecessor's result
// latency, which is longer than the 32-cycle issue interval of v_mfma_f32_32x32x16_bf16 (measured: matrix pipe 42 % busy,
// 56 % of the wave cycles in issue stalls).  The order per accumulator -- and with it every result bit -- is unchanged.
// With P parts the list is its tail: P = 2 keeps (1,0) (0,1) (0,0), P = 1 keeps (0,0) -- still smallest first.
// products [T0, T1) of the P-part sequence, T1 <= nprod(P)
template <int TM, int TN, int T0, int T1, int P = 3>
__device__ __forceinline__ void mfma_products(const Frag<P> (&a)[TM], const bf16x8 (&b)[TN][P], f32x16 (&acc)[TM][TN]) {
  constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
  static_assert(T1 <= nprod(P), "product list");
#pragma unroll
  for (int t = T0 + 6 - nprod(P); t < T1 + 6 - nprod(P); ++t)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i].p[PA[t]], b[j][PB[t]], acc[i][j], 0, 0, 0);
}

}  // namespace dh
