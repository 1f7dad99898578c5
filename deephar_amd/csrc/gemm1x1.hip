// Pointwise (1x1, stride 1, no padding) convolution = GEMM [M = N*H*W, K = Cin] x [K, Cout] for gfx950.
// 80 % of ReceptionNet's MACs: the pointwise half of every SeparableConv2D plus the
// 1x1 projections (reference deephar/layers.py:74-80, 258-301; models/reception.py:43-59,145-164).
//
// Same MFMA core and fragment mapping as conv_igemm.hip (v_mfma_f32_32x32x2_f32, exact fp32), but the
// staging is LDS-DMA: buffer_load_dwordx4 ... lds writes both operand tiles straight into LDS, double buffered,
// so a K-step costs no staging VGPRs, no ds_write and ONE barrier; the DMA of tile k+1 is in flight
// during the whole MFMA block of tile k.
//   A (activations, rows = pixels): LDS image [BM][32] floats, 128-byte rows, 16-byte slots XOR-swizzled
//      with (row & 7).  The DMA destination is lane-linear (wave base + lane*16), so the swizzle lives on the
//      per-lane SOURCE address and on the fragment read (both-sides-or-neither).
//   B (weights): host-packed [K/4][N][4] -> the LDS image is the global image, copied linearly.
//   ReLU-on-load (act_conv_bn) is applied to the A fragments after the ds_read; so is a BatchNormalization prologue
//   (PRE: x * scale[k] + shift[k] before the ReLU -- the pre-activation 1x1 convs of SPNet's residual units,
//   common.py:25-67, whose input has other readers and therefore cannot take the BN in its producer's epilogue): the
//   per-channel scale / shift sit in LDS behind the two operand stages and are read with the fragments.
//   Rows >= M and k >= K are clamped to valid addresses: padded weight rows are zero, tail rows never stored.
#include "dw_lds.h"
#include "gemm1x1_body.h"

namespace dh {
namespace {

template <int WM, int WN, int TM, int TN, bool UP2, bool RELU, bool KXK = false, bool PRE = false>
__global__ __launch_bounds__(WM* WN * 64, 2) void gemm1x1_kernel(const ConvArgs p, const int epi_vec) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  gemm1x1_body<WM, WN, TM, TN, UP2, RELU, KXK, PRE>(p, epi_vec, (int)blockIdx.x, (int)gridDim.x, smem);
}

// [r06] Grouped launch for the LATENCY regime: the 1x1 shortcut convolution of a residual unit and the depthwise convolution
// of its main path (deephar/models/common.py:25-67: `shortcut = conv2d(relu(BN(x)))` beside `sepconv2d(relu(BN(x)))`) read
// the same tensor and do not depend on each other, but as two nodes of a one-stream graph they run one after the other, and
// a node costs ~5 us plus its work however small (profiles/r06_speed2d_timeline.md); putting one of them on another stream
// costs more than it saves (profiles/r06_helper_stream_experiment.txt).  Here ONE launch runs both: work-groups
// [0, nb_conv) are the GEMM's, the rest the depthwise kernel's (dw_lds.h), each running exactly the code of its stand-alone
// kernel -- same bits.  Work-groups are 256 threads; the waves a body does not need end at once (s_barrier counts only the
// waves still alive).
template <int WM, bool PRE, bool RELU, int KS, int DNT, int MAXT, int MAXN, bool AFF, bool DRELU>
__global__ __launch_bounds__(256) void conv_dw_group_kernel(const ConvArgs pc, const int epi_vec, const int nb_conv,
                                                            const DwArgs pd, const int tw, const int rows,
                                                            const int twh_magic) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if ((int)blockIdx.x < nb_conv) {
    if (threadIdx.x < WM * 64)
      gemm1x1_body<WM, 1, 1, 1, false, RELU, false, PRE>(pc, epi_vec, (int)blockIdx.x, nb_conv, smem);
  } else {
    if (threadIdx.x < DNT)
      dwl::dwconv_lds_body<KS, DNT, MAXT, MAXN, AFF, DRELU>(pd, tw, rows, twh_magic, (int)blockIdx.x - nb_conv,
                                                            reinterpret_cast<float4*>(smem));
  }
}

template <int WM, int WN, int TM, int TN, bool UP2, bool RELU, bool KXK = false, bool PRE = false>
int launch_variant(const ConvArgs& a, int epi, unsigned tiles, hipStream_t s) {
  constexpr size_t kMax = gemm_f32_lds(WM, WN, TM, TN, PRE, 0).limit;
  static_assert(kMax <= 160 * 1024, "LDS budget");
  auto kern = gemm1x1_kernel<WM, WN, TM, TN, UP2, RELU, KXK, PRE>;
  if (kMax > 64 * 1024) {
    static LdsLimit lim;
    lim.raise((const void*)kern, (int)kMax);
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), gemm_f32_lds(WM, WN, TM, TN, PRE, a.Kp).launch, s, a, epi);
  return check_launch();
}

// every tiling in its forms: fused up-sampling (where the tiling has it), K x K, BN prologue, plain -- each with and without ReLU
template <int WM, int WN, int TM, int TN>
int launch_cfg(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  if constexpr (tile_has_up2(GemmTile{WM, WN, TM, TN})) {
    if (a.up2)
      return a.pre_relu ? launch_variant<WM, WN, TM, TN, true, true>(a, r.epi, r.tiles, s)
                        : launch_variant<WM, WN, TM, TN, true, false>(a, r.epi, r.tiles, s);
  }
  if (!conv_is_1x1(a))
    return a.pre_relu ? launch_variant<WM, WN, TM, TN, false, true, true>(a, r.epi, r.tiles, s)
                      : launch_variant<WM, WN, TM, TN, false, false, true>(a, r.epi, r.tiles, s);
  if (a.pre_scale != nullptr)       // BatchNormalization (+ ReLU) prologue on the A fragments
    return a.pre_relu ? launch_variant<WM, WN, TM, TN, false, true, false, true>(a, r.epi, r.tiles, s)
                      : launch_variant<WM, WN, TM, TN, false, false, false, true>(a, r.epi, r.tiles, s);
  return a.pre_relu ? launch_variant<WM, WN, TM, TN, false, true>(a, r.epi, r.tiles, s)
                    : launch_variant<WM, WN, TM, TN, false, false>(a, r.epi, r.tiles, s);
}

template <int WM, int KS, int DNT, int MAXT, int MAXN>
int launch_group(const ConvArgs& a, int epi, const DwArgs& d, const dwl::DwLdsGeom& g, hipStream_t s) {
  unsigned tiles;
  if (gemm_tile_count(a, WM * 32, 32, &tiles) != DH_OK || (long long)tiles + g.blocks > 0x7fffffffLL) return DH_EINVAL;
  const size_t lds = std::max(gemm_f32_lds(WM, 1, 1, 1, true, a.Kp).launch, g.lds);
  auto kern = conv_dw_group_kernel<WM, true, true, KS, DNT, MAXT, MAXN, true, true>;
  static LdsLimit lim;
  lim.raise((const void*)kern, 160 * 1024);
  if (lds > 160 * 1024) return DH_EUNSUPPORTED;
  hipLaunchKernelGGL(kern, dim3(tiles + g.blocks), dim3(256), lds, s, a, epi, (int)tiles, d, g.tw, g.rows,
                     65536 / (g.tw + KS - 1) + 1);
  return check_launch();
}

}  // namespace

// The 1x1 shortcut convolution `a` (BatchNormalization + ReLU prologue, fp32 tap-major weights, LDS-DMA GEMM family) and the
// 5x5 depthwise convolution `d` (BatchNormalization + ReLU prologue, LDS-tiled kernel) in one launch; DH_EUNSUPPORTED for
// anything else -- the caller then launches the two on their own, with the same result bits.
int launch_conv_dw_group(const ConvArgs& a, const DwArgs& d, hipStream_t s) {
  if (conv_check_packing(a) != DH_OK || d.N <= 0 || d.C <= 0) return DH_EINVAL;
  if (!(conv_is_1x1(a) && a.H == a.OH && a.W == a.OW) || a.up2 || a.y_pool != nullptr || a.x_u8 || a.w_split || a.pre_scale == nullptr || !a.pre_relu ||
      a.Kp > kMaxPreKp || !gemm1x1_eligible(a) || conv_is_skinny(a) || conv_stem_eligible(a))
    return DH_EUNSUPPORTED;
  if (a.res2_down && (a.res2 == nullptr || (a.OH & 1) || (a.OW & 1))) return DH_EINVAL;
  dwl::DwLdsGeom g;
  if (d.KW != 5 || d.pre_scale == nullptr || !d.pre_relu || !dwl::dw_lds_geometry(d, g)) return DH_EUNSUPPORTED;
  if (d.up_in && ((d.H & 1) || (d.W & 1))) return DH_EINVAL;
  const int epi = epi_with_direct(a, conv_epi_vec(a));
  const long long M = (long long)a.N * a.OH * a.OW;
  if (M > 0x7fffffffLL) return DH_EINVAL;
  // (all tilings of the family give the same bits: the group picks its own -- 128-row tiles once they fill the chip)
  const bool wide = ((M + 127) / 128) * ((a.Cout + 31) / 32) >= 256;
  if (g.nt == 256) return wide ? launch_group<4, 5, 256, 5, 10>(a, epi, d, g, s) : launch_group<2, 5, 256, 5, 10>(a, epi, d, g, s);
  return wide ? launch_group<4, 5, 64, 6, 12>(a, epi, d, g, s) : launch_group<2, 5, 64, 6, 12>(a, epi, d, g, s);
}

int launch_gemm1x1(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  return dispatch_tile<kNumF32Cfgs>(r.tile_cfg, [&](auto c) {
    constexpr GemmTile t = kGemmTiles[decltype(c)::value];
    return launch_cfg<t.wm, t.wn, t.tm, t.tn>(a, r, s);
  });
}

}  // namespace dh
