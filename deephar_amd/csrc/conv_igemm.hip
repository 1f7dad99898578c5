// Implicit-GEMM convolution for gfx950 on the fp32 matrix cores.
//
// Replaces what Keras Conv2D / the pointwise half of SeparableConv2D lower to in the reference
// (deephar/layers.py:66-80, 202-325), with the surrounding BatchNormalization / ReLU / add layers folded
// into the prologue and epilogue.  fp32 in, fp32 accumulate (v_mfma_f32_32x32x2_f32 is a k-ordered fmaf
// chain, so numerics are plain IEEE fp32) -- the 1e-3 px parity bar rules out bf16/fp8.
//
// Tiling (wave = 64 lanes, 32x32 MFMA tiles):
//   workgroup = WM x WN waves, each wave owns TM x TN tiles of 32x32 -> BM = 32*WM*TM, BN = 32*WN*TN
//   K is walked in steps of BK = 32.  A (activations) is gathered global -> registers -> LDS with row
//   stride 36 floats so that the ds_read_b128 fragment reads are bank-conflict free; B (weights) is
//   host-packed as [K/4][N][4] so both its global->LDS copy and its fragment reads are 16-byte wide.
//   One LDS stage + register prefetch of the next K-step (loads are issued before the MFMA block and
//   written to LDS after it), two workgroups per CU so one block's MFMAs cover the other's barriers.
//   A b128 fragment read hands each lane 4 consecutive k; MFMA t consumes element t of both operands, so
//   the lane halves (k, k+4) pair up -- a permutation of the K order, which the sum does not care about.
//   blockIdx is remapped so that the N-tiles sharing one A tile run back to back on the same XCD (L2).
#include "conv_common.h"

namespace dh {

namespace {

constexpr int LDA = BK + 4;  // floats; 144 B rows keep ds_read_b128 conflict-free (odd multiple of 16 B)

template <int WM, int WN, int TM, int TN, bool VEC4, bool UP2>
__global__ __launch_bounds__(WM* WN * 64, 2) void conv_igemm_kernel(const ConvArgs p, const int epi_vec) {
  constexpr int NT = WM * WN * 64;
  constexpr int BM = WM * TM * 32;
  constexpr int BN = WN * TN * 32;
  constexpr int APASS = BM * 8 / NT;       // float4 A loads per thread per K-step
  constexpr int AROWS = NT / 8;            // rows covered per pass
  constexpr int BPASS = 8 * BN / NT;       // float4 B loads per thread per K-step
  static_assert(BM * 8 % NT == 0 && (8 * BN) % NT == 0, "tile/thread mismatch");

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;             // [BM][LDA]
  float* sB = smem + BM * LDA;  // [8][BN][4]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int M = p.N * p.OH * p.OW;
  const int tiles_n = (p.Cout + BN - 1) / BN;

  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;

  // ---- per-thread A-row bookkeeping (fixed over the K loop)
  const int a_col = (tid & 7) * 4;
  int a_pix[APASS], a_ih0[APASS], a_iw0[APASS];
#pragma unroll
  for (int ps = 0; ps < APASS; ++ps) {
    const int m = m0 + (tid >> 3) + ps * AROWS;
    if (m < M) {
      const int n = m / (p.OH * p.OW);
      const int rem = m - n * (p.OH * p.OW);
      const int oh = rem / p.OW, ow = rem - oh * p.OW;
      a_pix[ps] = n * p.H * p.W;
      a_ih0[ps] = oh * p.SH - p.PT;
      a_iw0[ps] = ow * p.SW - p.PL;
    } else {
      a_pix[ps] = 0;
      a_ih0[ps] = -(1 << 28);
      a_iw0[ps] = 0;
    }
  }

  const float4* __restrict__ w4 = reinterpret_cast<const float4*>(p.w);
  const int nk = p.Kp / BK;
  const bool has_pre = p.pre_scale != nullptr;

  // B columns handled by this thread are fixed over the K loop
  int b_off[BPASS];
  unsigned bmask = 0;
#pragma unroll
  for (int q = 0; q < BPASS; ++q) {
    const int idx = tid + q * NT;
    const int kq = idx / BN, j = idx - kq * BN;
    const bool ok = n0 + j < p.Np;
    b_off[q] = kq * p.Np + (ok ? n0 + j : 0);
    bmask |= (ok ? 1u : 0u) << q;
  }

  // Raw register staging: loads are issued unconditionally (clamped addresses) so that nothing waits on
  // them until store_tile(), i.e. until after the MFMA block of the current K-step.
  float4 ra[APASS], rb[BPASS];
  float4 psc = make_float4(1.f, 1.f, 1.f, 1.f), psh = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned amask = 0;   // VEC4: bit ps ; scalar path: bit (ps*4 + e)
  int lut_c[4] = {0, 0, 0, 0};   // scalar path with uint8 input: LUT row (channel * 256) of the staged elements

  // running decode of this thread's k index (k = kt*32 + a_col) into (kh, kw, c); VEC4 only
  int t_c = a_col % p.Cin, t_kw, t_kh;
  {
    const int tap = a_col / p.Cin;
    t_kh = tap / p.KW;
    t_kw = tap - t_kh * p.KW;
  }

  auto load_tile = [&](int kt) {
    amask = 0;
    if constexpr (VEC4) {
      const bool kvalid = kt * BK + a_col < p.K;
      if (has_pre) {
        psc = *reinterpret_cast<const float4*>(p.pre_scale + t_c);
        psh = *reinterpret_cast<const float4*>(p.pre_shift + t_c);
      }
#pragma unroll
      for (int ps = 0; ps < APASS; ++ps) {
        const int ih = a_ih0[ps] + t_kh, iw = a_iw0[ps] + t_kw;
        const bool ok = kvalid && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
        const size_t off = ok ? (size_t)(a_pix[ps] + ih * p.W + iw) * p.ldx + t_c : 0;
        ra[ps] = *reinterpret_cast<const float4*>(p.x + off);
        amask |= (ok ? 1u : 0u) << ps;
      }
      // advance to the next K-step
      t_c += BK;
      while (t_c >= p.Cin) {
        t_c -= p.Cin;
        if (++t_kw == p.KW) { t_kw = 0; ++t_kh; }
      }
    } else {
      const int k0 = kt * BK + a_col;
      float sc[4], sh[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + e;
        const int tap = k / p.Cin;
        const int cc = k - tap * p.Cin;
        const int kh = tap / p.KW, kw = tap - kh * p.KW;
        const bool kv = k < p.K;
        sc[e] = has_pre ? p.pre_scale[cc] : 1.f;
        sh[e] = has_pre ? p.pre_shift[cc] : 0.f;
        lut_c[e] = (kv ? cc : 0) * 256;
#pragma unroll
        for (int ps = 0; ps < APASS; ++ps) {
          const int ih = a_ih0[ps] + kh, iw = a_iw0[ps] + kw;
          const bool ok = kv && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
          const size_t off = ok ? (size_t)(a_pix[ps] + ih * p.W + iw) * p.ldx + cc : 0;
          // uint8 frames: stage the raw byte (exact in fp32); the LUT is applied in store_tile()
          (&ra[ps].x)[e] = p.x_u8 ? (float)reinterpret_cast<const unsigned char*>(p.x)[off] : p.x[off];
          amask |= (ok ? 1u : 0u) << (ps * 4 + e);
        }
      }
      psc = make_float4(sc[0], sc[1], sc[2], sc[3]);
      psh = make_float4(sh[0], sh[1], sh[2], sh[3]);
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) rb[q] = w4[(size_t)kt * 8 * p.Np + b_off[q]];
  };

  auto store_tile = [&]() {
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
      float4 v = ra[ps];
      if constexpr (!VEC4) {
        if (p.x_u8) {
          v.x = p.in_lut[lut_c[0] + (int)v.x]; v.y = p.in_lut[lut_c[1] + (int)v.y];
          v.z = p.in_lut[lut_c[2] + (int)v.z]; v.w = p.in_lut[lut_c[3] + (int)v.w];
        }
      }
      if (has_pre) {
        v.x = v.x * psc.x + psh.x; v.y = v.y * psc.y + psh.y;
        v.z = v.z * psc.z + psh.z; v.w = v.w * psc.w + psh.w;
      }
      if (p.pre_relu) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
      }
      if constexpr (VEC4) {
        if (!((amask >> ps) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const unsigned mk = amask >> (ps * 4);
        if (!(mk & 1u)) v.x = 0.f;
        if (!(mk & 2u)) v.y = 0.f;
        if (!(mk & 4u)) v.z = 0.f;
        if (!(mk & 8u)) v.w = 0.f;
      }
      *reinterpret_cast<float4*>(&sA[((tid >> 3) + ps * AROWS) * LDA + a_col]) = v;
    }
#pragma unroll
    for (int q = 0; q < BPASS; ++q) {
      float4 v = rb[q];
      if (!((bmask >> q) & 1u)) v = make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&sB[(tid + q * NT) * 4]) = v;
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  load_tile(0);
  store_tile();
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const bool more = (kt + 1) < nk;
    if (more) load_tile(kt + 1);

#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i)
        fa[i] = *reinterpret_cast<const float4*>(&sA[((wm * TM + i) * 32 + li) * LDA + s * 8 + lh * 4]);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[j] = *reinterpret_cast<const float4*>(&sB[((s * 2 + lh) * BN + (wn * TN + j) * 32 + li) * 4]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
    if (more) {
      store_tile();
      __syncthreads();
    }
  }

  EpiPrefetch<TM, TN> pre;   // (register-staged kernel: no spare VGPRs to hold a residual tile across the K loop)
  conv_epilogue<WM, WN, TM, TN, UP2, false>(p, acc, smem, m0, n0, M, epi_vec, pre);
}

// every tiling of kGemmTiles[0..8] in three forms: float4 gather + fused up-sampling (where the tiling has it), float4, scalar
template <int WM, int WN, int TM, int TN>
int launch_cfg(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  constexpr int BM = WM * TM * 32, BN = WN * TN * 32, NT = WM * WN * 64;
  constexpr int kStage = BM * LDA + BK * BN, kEpi = gemm_epi_floats(WM, WN, TN);
  const size_t lds = (size_t)(kStage > kEpi ? kStage : kEpi) * sizeof(float);
  if constexpr (tile_has_up2(GemmTile{WM, WN, TM, TN})) {
    if (a.up2) {
      hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, TM, TN, true, true>), dim3(r.tiles), dim3(NT), lds, s, a, r.epi);
      return check_launch();
    }
  }
  if (r.vec4) {
    hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, TM, TN, true, false>), dim3(r.tiles), dim3(NT), lds, s, a, r.epi);
  } else {
    hipLaunchKernelGGL((conv_igemm_kernel<WM, WN, TM, TN, false, false>), dim3(r.tiles), dim3(NT), lds, s, a, r.epi);
  }
  return check_launch();
}

}  // namespace

int launch_conv_igemm(const ConvArgs& a, int cfg, hipStream_t s) {
  const ConvRoute r = conv_route(a, cfg);
  if (r.rc != DH_OK) return r.rc;
  ConvArgs b = a;                        // the split kernels of the extended scope's codes are those of 1 / 3 / 4
  if (a.w_split >= 5) b.w_split = conv_split_wide_base(a.w_split);
  switch (r.kernel) {
    case DH_CONV_GENERAL:
      return dispatch_tile<kNumF32Cfgs>(r.tile_cfg, [&](auto c) {
        constexpr GemmTile t = kGemmTiles[decltype(c)::value];
        return launch_cfg<t.wm, t.wn, t.tm, t.tn>(a, r, s);
      });
    case DH_CONV_DMA: return launch_gemm1x1(a, r, s);
    case DH_CONV_SPLIT: return launch_gemm1x1_split(b, r, s);
    case DH_CONV_SPLIT_EXT: return launch_gemm1x1_split_ext(b, r, s);
    case DH_CONV_HALO: return launch_conv_halo(a, r, s);
    case DH_CONV_SKINNY: return launch_conv_splitk(a, r, s);
    case DH_CONV_FIRST_LAYER: return launch_conv_stem(a, r, s);
  }
  return DH_EINVAL;
}

}  // namespace dh
