// The split-bf16 convolution kernels of the LDS-DMA GEMM family and their launch side, for P parts per operand.  One
// translation unit per mode instantiates launch_split_parts<P> (the instantiations of a mode compile for about as long as the
// rest of the library): gemm1x1s.hip (P = 3, with the rule and the dispatch), gemm1x1s_p2.hip, gemm1x1s_p1.hip.
#pragma once
#include "gemm_family.h"
#include "split_bf16.h"

namespace dh {
namespace {

#ifndef DH_WIDE_CHROWS
#define DH_WIDE_CHROWS 6
#endif
constexpr int WIDE_CHROWS = DH_WIDE_CHROWS;   // epilogue rows per chunk of the wide tiling (see conv_epilogue)

// NS = number of LDS stages: 2 (next K-step in flight) or 3 (two K-steps in flight: the split kernel's K-step is short
// enough that one DMA round trip no longer fits under it).
// P = bf16 parts per operand: the ninth template argument (a profiler spells the three-part kernels <..., 3>)
// The body is shared, as text, with gemm1x1s_ext_launch.h and convt2x2s.hip (gemm1x1s_body.h says why).
template <int WM, int WN, int TM, int TN, bool UP2, bool RELU, bool KXK = false, int NS = 2, int P = 3>
__global__ __launch_bounds__(WM* WN * 64, WM * WN >= 8 ? 2 : 2) void gemm1x1s_kernel(const ConvArgs p, const int epi_vec) {
  constexpr bool PRE = false, D2S = false, K16 = false;
  constexpr int cb = 0;
#include "gemm1x1s_body.h"
}

// ---------------------------------------------------------------------------------------------------------------
// Wide per-wave tile: 32 rows x 192 columns per wave, WM waves stacked over M (work-group tile 32 WM x 192), 16-k
// K-steps, two LDS stages (52 KB at WM = 4: two work-groups per CU, so one tile's epilogue runs beside another's K loop).
// What bounds the 32 x 96 tiling above is not the matrix pipe but everything the wave issues between its MFMAs
// (tools/micro/split_loop_model*.hip: that instruction mix reaches 58-62 % pipe occupancy with memory taken away, the
// mix of this tiling 80-84 %): the activation split costs 52 VALU per 32 rows x 8 k however many columns use it, and an
// LDS-DMA piece costs its wave ~60 issue cycles.  Twice the columns per wave halve the VALU per MFMA, 128 x 192 instead
// of 128 x 96 per work-group takes the DMA pieces per MFMA from 0.25 to 0.18.
// The 96 accumulator registers leave room for ONE set of B operands per half tile (3 column tiles x 3 parts): the K-step
// is processed as two halves (column tiles 0-2, then 3-5), each half's B operands are read from LDS while the other
// half is multiplied, the next K-step's activation rows are read at the start of the second half and split under its
// MFMAs.  One barrier per K-step, at the start of its second half: every wave has read the whole stage by then (it is
// refilled with K-step kt+2), and K-step kt+1 -- issued one K-step earlier -- has landed.
// Per accumulator the products arrive in the same order as in every other tiling: results are bit-identical.
template <int WM, bool UP2, bool RELU, bool KXK>
__global__ __launch_bounds__(WM * 64, 2) void gemm1x1s_wide_kernel(const ConvArgs p, const int epi_vec) {
  constexpr int NT = WM * 64;
  constexpr int BKW = 16;
  constexpr int BM = WM * 32, BN = 192;
  constexpr int APASS = BM * 4 / NT;                      // = 2: 16-byte units of the A stage per thread
  constexpr int BROWS = 6 * BN;                          // 16-byte units of the B stage: 2 k-groups x 3 parts x BN
  constexpr int BPASS = (BROWS + NT - 1) / NT;
  constexpr int A_BYTES = BM * BKW * 4;
  constexpr int STAGE_BYTES = A_BYTES + BROWS * 16;
  static_assert(STAGE_BYTES + 2 * BN * 16 + 5 * 512 < 65536, "ds_read immediate offsets");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int M = p.N * p.OH * p.OW;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x), 0, (int)(((unsigned)(p.N * p.H * p.W - 1) * p.ldx + (unsigned)p.Cin) * 4u), 0x00020000);
  const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)((unsigned)p.Kp * p.Np * 6u),
                                                      0x00020000);
  // A stage: 64-byte rows of four 16-byte slots, slot XOR ((row >> 2) & 3): the 16 lanes ds_read_b128 serves per cycle
  // (rows {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} of a wave's block) then fall on 16 different bank groups
  unsigned a_off[APASS];
  int a_slot[APASS];
  int a_pix[KXK ? APASS : 1], a_ih0[KXK ? APASS : 1], a_iw0[KXK ? APASS : 1];
#pragma unroll
  for (int ps = 0; ps < APASS; ++ps) {
    const int r = (tid >> 2) + ps * (NT / 4);
    int m = m0 + r;
    m = m < M ? m : M - 1;
    a_slot[ps] = ((tid & 3) ^ ((r >> 2) & 3)) * 4;
    if constexpr (KXK) {
      const int n = m / (p.OH * p.OW);
      const int rem = m - n * (p.OH * p.OW);
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      a_pix[ps] = n * p.H * p.W;
      a_ih0[ps] = oh * p.SH - p.PT;
      a_iw0[ps] = ow * p.SW - p.PL;
      a_off[ps] = 0;
    } else {
      a_off[ps] = ((unsigned)m * p.ldx + a_slot[ps]) * 4u;
    }
  }
  const int chunks_per_tap = KXK ? p.Cin / BKW : 1;
  unsigned b_off[BPASS];
#pragma unroll
  for (int q = 0; q < BPASS; ++q) {
    const int idx = tid + q * NT;
    const int r = idx / BN;
    const int j = idx - r * BN;
    b_off[q] = r < 6 && n0 + j < p.Np ? ((unsigned)r * p.Np + n0 + j) * 16u : OOB;
  }
  const int b_step = 6 * p.Np * 16;                       // bytes per 16-k K-step in the packed weight
  // the last B pass is partial: the waves beyond it send their piece (out-of-range offset: zeros, no fetch) to a dump
  // slot behind the stages, so that every wave issues the same branch-free sequence
  constexpr int DUMP_BYTES = 2 * STAGE_BYTES;

  auto issue = [&](int kt, int stage) {
    float* sA = smem + stage * (STAGE_BYTES / 4);
    float* sB = sA + A_BYTES / 4;
    int kh = 0, kw = 0, c0 = 0;
    if constexpr (KXK) {
      const int tap = kt / chunks_per_tap;
      c0 = (kt - tap * chunks_per_tap) * BKW;
      kh = tap / p.KW;
      kw = tap - kh * p.KW;
    }
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
      if constexpr (KXK) {
        const int ih = a_ih0[ps] + kh, iw = a_iw0[ps] + kw;
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W && kt * BKW < p.K;
        const unsigned off = ok ? ((unsigned)(a_pix[ps] + ih * p.W + iw) * p.ldx + c0 + a_slot[ps]) * 4u : OOB;
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, off, 0);
      } else {
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, a_off[ps], kt * BKW * 4);
      }
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      if ((q + 1) * NT <= BROWS) {
        dma16(rs_w, sB + (q * NT + wave_u * 64) * 4, b_off[q], kt * b_step);
      } else {
        const bool mine = q * NT + wave_u * 64 < BROWS;   // wave-uniform
        dma16(rs_w, mine ? sB + (q * NT + wave_u * 64) * 4 : smem + DUMP_BYTES / 4 + wave_u * 256, b_off[q], kt * b_step);
      }
    }
  };

  f32x16 acc[2][1][3];                                    // [half][1][column tile of the half]
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[h][0][j][r] = 0.f;

  const int nk = p.Kp / BKW;                              // even, >= 2 (Kp is a multiple of 32)
  issue(0, 0);
  issue(1, 1);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(APASS + BPASS) : "memory");
  __syncthreads();

  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)smem;
  const unsigned sw = (unsigned)((li >> 2) & 3);
  const unsigned a_rd0 = lds0 + (unsigned)((wave * 32 + li) * 64) + (((2u * lh) ^ sw) << 4);
  const unsigned a_rd1 = lds0 + (unsigned)((wave * 32 + li) * 64) + (((2u * lh + 1u) ^ sw) << 4);
  const unsigned b_rd = lds0 + (unsigned)A_BYTES + (unsigned)((lh * 3 * BN + li) * 16);

  Frag<3> fa0[1], fa1[1];
  bf16x8 bq0[3][3], bq1[3][3];                            // B operands of column tiles 0-2 / 3-5
  float4 ra[2];
  // stage and half are compile-time: every ds_read is one base register plus an immediate
#define DH_RD_B1(DST, ST, HALF, J)                                                                      \
  DST[J][0] = as_bf(lds_rd<(ST) * STAGE_BYTES + ((HALF) * 3 + (J)) * 512>(b_rd));                       \
  DST[J][1] = as_bf(lds_rd<(ST) * STAGE_BYTES + BN * 16 + ((HALF) * 3 + (J)) * 512>(b_rd));             \
  DST[J][2] = as_bf(lds_rd<(ST) * STAGE_BYTES + 2 * BN * 16 + ((HALF) * 3 + (J)) * 512>(b_rd));
#define DH_RD_B(DST, ST, HALF) DH_RD_B1(DST, ST, HALF, 0) DH_RD_B1(DST, ST, HALF, 1) DH_RD_B1(DST, ST, HALF, 2)
#define DH_RD_A(ST)                                        \
  ra[0] = lds_rd<(ST) * STAGE_BYTES>(a_rd0);               \
  ra[1] = lds_rd<(ST) * STAGE_BYTES>(a_rd1);

  constexpr int VPM = (52 + 11) / 12;
  // one K-step: multiply (CUR, stage ST).  MODE 0: open K-step kt+1 (stage 1 - ST), split its rows into NXT and refill
  // stage ST with K-step kt+2; MODE 1: the same without the refill (last but one); MODE 2: last K-step.
  // The refill's DMA pieces cost the wave ~60 issue cycles each: they go out one behind each of the next MFMAs instead
  // of in one burst behind the barrier (tools/micro/split_loop_model2.hip: 80 -> 84 % pipe occupancy).
#define DH_KSTEP(CUR, NXT, ST, MODE)                                                                             \
  {                                                                                                              \
    DH_RD_B(bq1, ST, 1)                                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    mfma_products<1, 3, 0, 6>(CUR, bq0, acc[0]);                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    lgkm_wait();                                                                                                 \
    if constexpr ((MODE) != 2) {                                                                                 \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                           \
      __syncthreads();                                                                                           \
      DH_RD_B(bq0, 1 - (ST), 0)                                                                                  \
      DH_RD_A(1 - (ST))                                                                                          \
      __builtin_amdgcn_sched_barrier(0);                                                                         \
      if constexpr ((MODE) == 0) issue(kt + 2, ST);                                                              \
      mfma_products<1, 3, 0, 2>(CUR, bq1, acc[1]);                                                               \
      if constexpr ((MODE) == 0) {                                                                               \
        _Pragma("unroll") for (int u = 0; u < 5; ++u) {                                                          \
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                     \
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                     \
        }                                                                                                        \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                       \
        __builtin_amdgcn_sched_group_barrier(0x020, APASS + BPASS - 5, 0);                                       \
      }                                                                                                          \
      lgkm_wait();                                                                                               \
      NXT[0] = split8<RELU>(ra[0], ra[1]);                                                                       \
      mfma_products<1, 3, 2, 6>(CUR, bq1, acc[1]);                                                               \
      _Pragma("unroll") for (int q = 0; q < 3; ++q) asm volatile("" : "+v"(NXT[0].p[q]));                        \
      _Pragma("unroll") for (int u = 0; u < 12; ++u) {                                                           \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                       \
        __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);                                                     \
      }                                                                                                          \
    } else {                                                                                                     \
      pre0.template issue<WM, 1>(p, m0, n0, M, epi_vec);                                                         \
      mfma_products<1, 3, 0, 6>(CUR, bq1, acc[1]);                                                               \
    }                                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
  }

  EpiPrefetch<1, 3> pre0;
  // K-step 0: rows and the first half's B operands
  DH_RD_B(bq0, 0, 0)
  DH_RD_A(0)
  lgkm_wait();
  fa0[0] = split8<RELU>(ra[0], ra[1]);

  int kt = 0;
  for (; kt < nk - 2; kt += 2) {
    DH_KSTEP(fa0, fa1, 0, 0)
    ++kt;
    DH_KSTEP(fa1, fa0, 1, 0)
    --kt;
  }
  DH_KSTEP(fa0, fa1, 0, 1)
  ++kt;
  DH_KSTEP(fa1, fa0, 1, 2)
#undef DH_KSTEP
#undef DH_RD_A
#undef DH_RD_B
#undef DH_RD_B1

  // columns 0-95 (residual rows requested during the last K-step), then 96-191 through the same slab.  Holding the
  // second slice's residual rows in registers across the first slice's row loop spills (measured: 80 dwords); its
  // round trip is covered by the other work-group of the CU instead.
  conv_epilogue<WM, 1, 1, 3, UP2, true, EpiNoHook, true, WIDE_CHROWS>(p, acc[0], smem, m0, n0, M, epi_vec, pre0);
  conv_epilogue<WM, 1, 1, 3, UP2, false, EpiNoHook, true, WIDE_CHROWS>(p, acc[1], smem, m0, n0 + 96, M, epi_vec, pre0);
}

template <int WM, bool UP2, bool RELU, bool KXK>
int launch_wide_variant(const ConvArgs& a, int epi, unsigned tiles, hipStream_t s) {
  constexpr int kStage = 2 * (WM * 32 * 16 * 4 + 6 * 192 * 16) + WM * 1024, kEpi = WM * 32 * (3 * 32 + 4) * 4;
  constexpr size_t lds = kStage > kEpi ? kStage : kEpi;
  auto kern = gemm1x1s_wide_kernel<WM, UP2, RELU, KXK>;
  if (lds > 64 * 1024) {
    static LdsLimit lim;
    lim.raise((const void*)kern, (int)lds);
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * 64), lds, s, a, epi);
  return check_launch();
}

template <int WM>
int launch_wide(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  if (a.up2)
    return a.pre_relu ? launch_wide_variant<WM, true, true, false>(a, r.epi, r.tiles, s)
                      : launch_wide_variant<WM, true, false, false>(a, r.epi, r.tiles, s);
  if (!conv_is_1x1(a))
    return a.pre_relu ? launch_wide_variant<WM, false, true, true>(a, r.epi, r.tiles, s)
                      : launch_wide_variant<WM, false, false, true>(a, r.epi, r.tiles, s);
  return a.pre_relu ? launch_wide_variant<WM, false, true, false>(a, r.epi, r.tiles, s)
                    : launch_wide_variant<WM, false, false, false>(a, r.epi, r.tiles, s);
}

template <int P, int WM, int WN, int TM, int TN, bool UP2, bool RELU, bool KXK = false, int NS = 2>
int launch_variant(const ConvArgs& a, int epi, unsigned tiles, hipStream_t s) {
  constexpr size_t lds = gemm_split_lds(P, WM, WN, TM, TN, NS, false, 0).launch;
  static_assert(lds <= 160 * 1024, "LDS budget");
  auto kern = gemm1x1s_kernel<WM, WN, TM, TN, UP2, RELU, KXK, NS, P>;
  if (lds > 64 * 1024) {
    static LdsLimit lim;
    lim.raise((const void*)kern, (int)lds);
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), lds, s, a, epi);
  return check_launch();
}

template <int P, int WM, int WN, int TM, int TN, int NS = 2>
int launch_cfg(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  if constexpr (tile_has_up2(GemmTile{WM, WN, TM, TN})) {
    if (a.up2)
      return a.pre_relu ? launch_variant<P, WM, WN, TM, TN, true, true, false, NS>(a, r.epi, r.tiles, s)
                        : launch_variant<P, WM, WN, TM, TN, true, false, false, NS>(a, r.epi, r.tiles, s);
  }
  if (!conv_is_1x1(a))
    return a.pre_relu ? launch_variant<P, WM, WN, TM, TN, false, true, true, NS>(a, r.epi, r.tiles, s)
                      : launch_variant<P, WM, WN, TM, TN, false, false, true, NS>(a, r.epi, r.tiles, s);
  return a.pre_relu ? launch_variant<P, WM, WN, TM, TN, false, true, false, NS>(a, r.epi, r.tiles, s)
                    : launch_variant<P, WM, WN, TM, TN, false, false, false, NS>(a, r.epi, r.tiles, s);
}

// every tiling one mode (P parts) has (tile_has_parts: the wide tiling exists for three parts only)
template <int P>
int launch_split_parts(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  return dispatch_tile<kNumSplitCfgs>(r.tile_cfg, [&](auto c) -> int {
    constexpr GemmTile t = kGemmTiles[decltype(c)::value];
    if constexpr (!tile_has_parts(t, P, false)) {
      return DH_EUNSUPPORTED;
    } else if constexpr (t.wide) {
      return launch_wide<t.wm>(a, r, s);
    } else {
      return launch_cfg<P, t.wm, t.wn, t.tm, t.tn, t.ns>(a, r, s);
    }
  });
}

}  // namespace
}  // namespace dh
