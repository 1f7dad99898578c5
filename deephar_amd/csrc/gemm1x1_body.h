// The fp32 LDS-DMA GEMM kernel body as a device function (gemm1x1.hip says what it computes and how it stages): shared by
// gemm1x1_kernel / conv_dw_group_kernel (gemm1x1.hip) and convt2x2_kernel (convt2x2.hip), each instantiating its own variants.
#pragma once
#include "conv_common.h"
#include "gemm_family.h"
#include "lds_dma.h"

namespace dh {

// PRE: scale / shift of the four k values this lane's A fragment of sub-step S covers (k = kt*32 + (2S + lh)*4 + e)
template <bool PRE, int S>
__device__ __forceinline__ void fetch_affine(unsigned t_sc, unsigned t_sh, float4& sc, float4& sh) {
  if constexpr (PRE) {
    sc = lds_rd<S * 32>(t_sc);
    sh = lds_rd<S * 32>(t_sh);
  }
}

template <int TM, int TN, int BN, int BOFF, int S>
__device__ __forceinline__ void fetch_frags(const unsigned (&a_addr)[TM][4], unsigned b_addr, float4 (&fa)[TM],
                                            float4 (&fb)[TN]) {
  fa[0] = lds_rd<0>(a_addr[0][S]);
  if constexpr (TM > 1) fa[1] = lds_rd<0>(a_addr[1][S]);
  constexpr int BO = BOFF + S * 2 * BN * 16;
  fb[0] = lds_rd<BO>(b_addr);
  if constexpr (TN > 1) fb[1] = lds_rd<BO + 512>(b_addr);
  if constexpr (TN > 2) fb[2] = lds_rd<BO + 1024>(b_addr);
}

// f(std::integral_constant<int, I>{}) for I in [I0, N): an unrolled loop whose index is a constant expression (asm offsets)
template <int I0, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I0 < N) {
    f(std::integral_constant<int, I0>{});
    static_for<I0 + 1, N>(f);
  }
}

// at most N of the asm ds_reads are still in flight (they return in order): the older ones have landed
template <int N>
__device__ __forceinline__ void lgkm_wait_n() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// KXK: the same kernel as an implicit GEMM over a K x K (strided, zero-padded) convolution whose Cin is a multiple
// of 32: K-step kt covers 32 channels of ONE filter tap, so each staged row is still one contiguous 128-byte run -- of
// the tap's input pixel, or of a page of zeros when the tap falls into the padding (ReLU-on-load keeps zeros zero).
// The kernel body as a device function: `block` of `nblocks` is the work-group's index among the GEMM work-groups (the
// kernel's blockIdx.x / gridDim.x, or its share of a grouped launch: gemm1x1.hip, conv_dw_group_kernel), `smem` the work-group's
// dynamic LDS; threads 0 .. WM * WN * 64 - 1 run it.
// D2S: the main loop of the pointwise form in front of the depth-to-space epilogue of the transposed 2x2 / stride-2
// convolution (conv_common.h: d2s_epilogue; `cb` = columns per output-pixel block).
template <int WM, int WN, int TM, int TN, bool UP2, bool RELU, bool KXK = false, bool PRE = false, bool D2S = false>
__device__ __forceinline__ void gemm1x1_body(const ConvArgs& p, const int epi_vec, const int block, const int nblocks,
                                             float* const smem, const int cb = 0) {
  static_assert(!(PRE && (KXK || UP2)), "the BN prologue is built for the plain pointwise form");
  static_assert(!(D2S && (KXK || UP2)), "the depth-to-space epilogue follows the plain pointwise main loop");
  constexpr int NT = WM * WN * 64;
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  constexpr int APASS = BM * 8 / NT;
  constexpr int BPASS = 8 * BN / NT;
  constexpr int STAGE = BM * BK + BK * BN;  // floats per stage
  static_assert(BM * 8 % NT == 0 && (8 * BN) % NT == 0, "tile/thread mismatch");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int M = p.N * p.OH * p.OW;
  const int tiles_n = (p.Cout + BN - 1) / BN;
  const int tile = xcd_tile(block, nblocks);
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  // ---- per-thread DMA sources: byte offsets into two buffer descriptors (activations, packed weight), fixed over K;
  // the K-step offset is SCALAR (soffset of buffer_load ... lds), so a K-step costs no 64-bit address VALU -- on gfx950
  // every VALU instruction beside an fp32 MFMA is paid in full (profiles/r02_sepconv_fusion_study.md section 3)
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.x), 0, (int)(((unsigned)(p.N * p.H * p.W - 1) * p.ldx + (unsigned)p.Cin) * 4u), 0x00020000);
  const auto rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)((unsigned)p.Kp * p.Np * 4u),
                                                      0x00020000);
  unsigned a_off[APASS];                            // pointwise: (pixel * ldx + slot) * 4
  int a_slot[APASS];
  int a_pix[KXK ? APASS : 1], a_ih0[KXK ? APASS : 1], a_iw0[KXK ? APASS : 1];   // KXK: frame base pixel, top-left tap
#pragma unroll
  for (int ps = 0; ps < APASS; ++ps) {
    const int r = (tid >> 3) + ps * (NT / 8);       // row inside the tile; lane-linear LDS slot' = tid&7
    int m = m0 + r;
    m = m < M ? m : M - 1;
    a_slot[ps] = ((tid & 7) ^ (r & 7)) * 4;          // swizzle on the source side
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
  const int chunks_per_tap = KXK ? p.Cin / BK : 1;
  unsigned b_off[BPASS];
#pragma unroll
  for (int q = 0; q < BPASS; ++q) {
    const int idx = tid + q * NT;
    const int kq = idx / BN, j = idx - kq * BN;
    const int col = n0 + j < p.Np ? n0 + j : 0;
    b_off[q] = ((unsigned)kq * p.Np + col) * 16u;
  }
  const int b_step = 8 * p.Np * 16;                 // bytes per K-step in the packed weight

  auto issue = [&](int kt, int stage) {
    float* sA = smem + stage * STAGE;
    float* sB = sA + BM * BK;
    int kh = 0, kw = 0, c0 = 0;
    if constexpr (KXK) {
      const int tap = kt / chunks_per_tap;
      c0 = (kt - tap * chunks_per_tap) * BK;
      kh = tap / p.KW;
      kw = tap - kh * p.KW;
    }
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
      if constexpr (KXK) {                          // padding taps: out-of-range offset -> the DMA writes zeros
        const int ih = a_ih0[ps] + kh, iw = a_iw0[ps] + kw;
        const bool ok = (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W && kt * BK < p.K;
        const unsigned off = ok ? ((unsigned)(a_pix[ps] + ih * p.W + iw) * p.ldx + c0 + a_slot[ps]) * 4u : OOB;
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, off, 0);
      } else {                                      // k >= K: the next pixel's (finite) data or zeros, times zero weights
        dma16(rs_x, sA + (ps * NT + wave_u * 64) * 4, a_off[ps], kt * BK * 4);
      }
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) dma16(rs_w, sB + (q * NT + wave_u * 64) * 4, b_off[q], kt * b_step);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.Kp / BK;
  issue(0, 0);
  if constexpr (PRE) {              // scale | shift tables behind the stages, zero beyond K (k >= K meets zero weights)
    float* tab = smem + 2 * STAGE;
    for (int i = tid; i < p.Kp; i += NT) {
      tab[i] = i < p.K ? p.pre_scale[i] : 0.f;
      tab[p.Kp + i] = i < p.K ? p.pre_shift[i] : 0.f;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- fragment read addresses (LDS byte offsets), stage 0; tile row blocks start at multiples of 32 so
  // (row & 7) == (lane & 7) and the XOR swizzle only depends on the lane
  const unsigned lds0 = (unsigned)(uintptr_t)(lptr_t)smem;
  unsigned a_base[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a_base[i][q] = lds0 + (unsigned)(((wm * TM + i) * 32 + li) * BK * 4 + (((q * 2 + lh) ^ (li & 7)) << 4));
  const unsigned b_base = lds0 + (unsigned)((lh * BN + wn * TN * 32 + li) * 16);
  constexpr int BOFF = BM * BK * 4;   // B tile follows the A tile inside a stage

  auto mfma_block = [&](const float4 (&a)[TM], const float4 (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
      }
  };
  auto relu_frags = [&](float4 (&a)[TM], const float4& sc, const float4& sh) {
    if constexpr (PRE) {            // same fused multiply-add as the general kernel's prologue (conv_igemm.hip): same bits
#pragma unroll
      for (int i = 0; i < TM; ++i)
        a[i] = make_float4(fmaf(a[i].x, sc.x, sh.x), fmaf(a[i].y, sc.y, sh.y), fmaf(a[i].z, sc.z, sh.z), fmaf(a[i].w, sc.w, sh.w));
    }
    if constexpr (RELU) {
#pragma unroll
      for (int i = 0; i < TM; ++i) a[i] = relu4(a[i]);
    }
  };
  const unsigned t_sc0 = lds0 + (unsigned)(2 * STAGE * 4 + lh * 16);

  // NB: an asm ds_read result must be awaited inside the basic block that issued it -- register copies the
  // allocator inserts at block boundaries (loop back-edge, if/else joins) would otherwise copy registers the
  // data has not reached yet.  Hence every fetch and its wait live in the straight-line body of one K-step.
  // (Fetching tile kt+1's first fragments before the loop back-edge was tried: correct with a tail wait, but
  // the loop-carried fragment registers cost more than the hidden LDS latency buys: 111 vs 118 TFLOP/s.)
  EpiPrefetch<TM, TN> pre;
  // Direct tiles of the one-row-block tilings (gemm_family.h: tile_epi_sliced) leave the loop one K-step early: the last
  // step runs column tile by column tile below, each tile finished under the next one's MFMAs.
  constexpr bool kSliced = tile_epi_sliced(GemmTile{WM, WN, TM, TN}, PRE, KXK) && !UP2 && !D2S;
  const bool sliced = kSliced && EpiPrefetch<TM, TN>::template direct_tile<WM, WN>(p, m0, n0, M, epi_vec);
  const int nloop = sliced ? nk - 1 : nk;
  for (int kt = 0; kt < nloop; ++kt) {
    const int cur = kt & 1;
    if constexpr (!D2S) {             // (D2S reads its residual at the output resolution, in its own epilogue)
      if (kt == nk - 1) pre.template issue<WM, WN, !kSliced>(p, m0, n0, M, epi_vec);   // lands during the last MFMA block
    }
    const unsigned so = (unsigned)(cur * STAGE * 4);
    unsigned a_addr[TM][4];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) a_addr[i][q] = a_base[i][q] + so;
    const unsigned b_addr = b_base + so;

    // sub-step s+1's fragments are in flight (asm ds_read) while sub-step s's MFMAs run; the first read of the
    // K-step has no MFMAs to hide behind, so the DMA issue of the next tile (address VALU + 6 loads) goes there
    float4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    float4 sc0, sh0, sc1, sh1;                        // PRE only
    const unsigned t_sc = t_sc0 + (unsigned)(kt * BK * 4), t_sh = t_sc + (unsigned)(p.Kp * 4);
    fetch_frags<TM, TN, BN, BOFF, 0>(a_addr, b_addr, fa0, fb0);
    fetch_affine<PRE, 0>(t_sc, t_sh, sc0, sh0);
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) issue(kt + 1, cur ^ 1);          // DMA of the next tile flies during this MFMA block
    lgkm_wait();
    fetch_frags<TM, TN, BN, BOFF, 1>(a_addr, b_addr, fa1, fb1);
    fetch_affine<PRE, 1>(t_sc, t_sh, sc1, sh1);
    __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs they overlap with
    relu_frags(fa0, sc0, sh0);
    mfma_block(fa0, fb0);
    lgkm_wait();
    fetch_frags<TM, TN, BN, BOFF, 2>(a_addr, b_addr, fa0, fb0);
    fetch_affine<PRE, 2>(t_sc, t_sh, sc0, sh0);
    __builtin_amdgcn_sched_barrier(0);
    relu_frags(fa1, sc1, sh1);
    mfma_block(fa1, fb1);
    lgkm_wait();
    fetch_frags<TM, TN, BN, BOFF, 3>(a_addr, b_addr, fa1, fb1);
    fetch_affine<PRE, 3>(t_sc, t_sh, sc1, sh1);
    __builtin_amdgcn_sched_barrier(0);
    relu_frags(fa0, sc0, sh0);
    mfma_block(fa0, fb0);
    lgkm_wait();
    relu_frags(fa1, sc1, sh1);
    mfma_block(fa1, fb1);

    // tile kt+1 has landed (this wave's DMA) and every wave is done reading tile kt
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  if constexpr (kSliced) {
    if (sliced) {
      // ---- the last K-step, column-major: the wave's TN accumulator tiles are independent, so issuing their MFMAs tile by
      // tile changes no bit (each element still accumulates k ascending) and tile j's BN / residual VALU and its 16
      // stores drain under tile j + 1's 16 MFMAs; only the last tile's finish is exposed.  All four sub-steps' A
      // fragments are read (and BN'd / ReLU'd) once; tile j + 1's B fragments land in the registers tile j's leave.
      // Every fragment read is awaited before the next branch (the NB above): request() and finish() branch on the
      // launch's flags.
      const int kt = nk - 1;
      const unsigned so = (unsigned)((kt & 1) * STAGE * 4);
      const unsigned b_addr = b_base + so;
      const unsigned t_sc = t_sc0 + (unsigned)(kt * BK * 4), t_sh = t_sc + (unsigned)(p.Kp * 4);
      const EpiDirect<WM, WN, TN> epi(p, m0, n0, M);
      EpiSlice sl[2];                                  // at most two slices' residuals in flight: slice j + 1's are
      epi.request(p, 0, sl[0]);                        // requested before slice j's MFMAs, slice 0's here
      float4 fa[4][1], fb[4], sc[4], sh[4];
      auto read_a = [&](auto sc_) {
        constexpr int S = decltype(sc_)::value;
        fa[S][0] = lds_rd<0>(a_base[0][S] + so);
        fetch_affine<PRE, S>(t_sc, t_sh, sc[S], sh[S]);
      };
      auto read_b0 = [&](auto sc_) {
        constexpr int S = decltype(sc_)::value;
        fb[S] = lds_rd<BOFF + S * 2 * BN * 16>(b_addr);
      };
      if constexpr (PRE) {
        // the scale / shift fragments need registers too: one sub-step's reads (three) run ahead of the sub-step being
        // BN'd -- LDS reads return in order, so a counted wait releases the older ones
        read_a(std::integral_constant<int, 0>{});
        static_for<0, 3>([&](auto sc_) {
          constexpr int S = decltype(sc_)::value;
          read_a(std::integral_constant<int, S + 1>{});
          lgkm_wait_n<3>();
          relu_frags(fa[S], sc[S], sh[S]);
        });
        static_for<0, 4>(read_b0);
        lgkm_wait_n<4>();
        relu_frags(fa[3], sc[3], sh[3]);
        lgkm_wait();
      } else {
        static_for<0, 4>(read_a);
        static_for<0, 4>(read_b0);
        lgkm_wait();
        static_for<0, 4>([&](auto sc_) { relu_frags(fa[decltype(sc_)::value], sc[0], sh[0]); });
      }
      static_for<0, TN>([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if constexpr (J + 1 < TN) epi.request(p, J + 1, sl[(J + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, 4>([&](auto sc_) {
          constexpr int S = decltype(sc_)::value;
          acc[0][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[S][0].x, fb[S].x, acc[0][J], 0, 0, 0);
          acc[0][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[S][0].y, fb[S].y, acc[0][J], 0, 0, 0);
          acc[0][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[S][0].z, fb[S].z, acc[0][J], 0, 0, 0);
          acc[0][J] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[S][0].w, fb[S].w, acc[0][J], 0, 0, 0);
          if constexpr (J + 1 < TN) {
            __builtin_amdgcn_sched_barrier(0);         // the read follows the MFMAs whose operand registers it takes over
            fb[S] = lds_rd<BOFF + S * 2 * BN * 16 + (J + 1) * 512>(b_addr);
            __builtin_amdgcn_sched_barrier(0);
          }
        });
        if constexpr (J + 1 < TN) lgkm_wait();
        epi.finish(p, J, acc[0][J], sl[J & 1]);
      });
      return;
    }
  }
  constexpr int kDirect = kSliced ? kDirectNone : kDirectSlices;   // (the direct tiles of a sliced kernel have left above)
  if constexpr (D2S) d2s_epilogue<WM, WN, TM, TN>(p, acc, smem, m0, n0, M, epi_vec, cb);
  else conv_epilogue<WM, WN, TM, TN, UP2, true, EpiNoHook, true, 0, kDirect>(p, acc, smem, m0, n0, M, epi_vec, pre);
}

}  // namespace dh
