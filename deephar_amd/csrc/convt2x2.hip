// Conv2DTranspose((2, 2), strides=(2, 2), padding='same', use_bias=False) for gfx950 -- the up-scaling unit of SPNet's
// learned-resampling flavour (reference deephar/models/common.py:103-106, deephar/layers.py:83-89).
//
// Kernel = strides, so every output pixel (2i + a, 2j + b) sees exactly ONE tap: y[n, 2i+a, 2j+b, :] = W[a, b] @ x[n, i, j, :].
// That is one GEMM [M = N*H*W, K = Cin] x [Cin, 4 * Cout] whose column block (a, b) of row (n, i, j) is stored at pixel
// (2i + a, 2j + b): the LDS-DMA main loop of gemm1x1.hip (fp32 MFMA, K ascending in every tiling -- the bits of an output
// depend on neither tiling nor batch size) in front of a depth-to-space epilogue (conv_common.h: d2s_epilogue).
// Prologue: BatchNormalization (scale / shift) + ReLU on the input, as in the pointwise form.  Epilogue: an optional residual
// read at the OUTPUT resolution (the pyramid's add([xp, lp[i]]) right behind the unit, spnet.py:303) and an optional ReLU.
// The kernel body of gemm1x1.hip (gemm1x1_body.h) is compiled here for this layer's instantiations only.
#include "gemm1x1_body.h"

namespace dh {
namespace {

template <int WM, int WN, int TM, int TN, bool RELU, bool PRE>
__global__ __launch_bounds__(WM* WN * 64, 2) void convt2x2_kernel(const ConvArgs p, const int epi_vec, const int cb) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  gemm1x1_body<WM, WN, TM, TN, false, RELU, false, PRE, true>(p, epi_vec, (int)blockIdx.x, (int)gridDim.x, smem, cb);
}

template <int WM, int WN, int TM, int TN, bool RELU, bool PRE>
int launch_convt_variant(const ConvArgs& a, int vec, int cb, unsigned tiles, hipStream_t s) {
  constexpr size_t kMax = gemm_f32_lds(WM, WN, TM, TN, PRE, 0).limit;
  static_assert(kMax <= 160 * 1024, "LDS budget");
  auto kern = convt2x2_kernel<WM, WN, TM, TN, RELU, PRE>;
  if (kMax > 64 * 1024) {
    static LdsLimit lim;
    lim.raise((const void*)kern, (int)kMax);
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), gemm_f32_lds(WM, WN, TM, TN, PRE, a.Kp).launch, s, a, vec, cb);
  return check_launch();
}

template <int WM, int WN, int TM, int TN>
int launch_convt_cfg(const ConvArgs& a, int vec, int cb, hipStream_t s) {
  unsigned t;
  if (gemm_tile_count(a, WM * TM * 32, WN * TN * 32, &t) != DH_OK) return DH_EINVAL;
  if (a.pre_scale != nullptr)
    return a.pre_relu ? launch_convt_variant<WM, WN, TM, TN, true, true>(a, vec, cb, t, s)
                      : launch_convt_variant<WM, WN, TM, TN, false, true>(a, vec, cb, t, s);
  return a.pre_relu ? launch_convt_variant<WM, WN, TM, TN, true, false>(a, vec, cb, t, s)
                    : launch_convt_variant<WM, WN, TM, TN, false, false>(a, vec, cb, t, s);
}

}  // namespace

int convt2x2_num_cfgs() { return 4; }

// `a` describes the GEMM: N, H = OH, W = OW the INPUT frames, Cin = K, Cout = 4 * cb columns, y / ldy the output at
// [N, 2H, 2W, cb], res1 / ldr1 the residual at the output resolution; w packed as the [Cin, 4 * cb] pointwise kernel.
int launch_convt2x2(const ConvArgs& a, int cb, int cfg, hipStream_t s) {
  if (a.N <= 0 || a.H <= 0 || a.W <= 0 || a.Cin <= 0 || cb <= 0 || a.Cout != 4 * cb) return DH_EINVAL;
  if (a.Kp % BK != 0 || a.Np % 32 != 0 || a.Kp < a.Cin || a.Np < a.Cout || a.ldx < a.Cin || a.ldy < cb ||
      (a.res1 != nullptr && a.ldr1 < cb))
    return DH_EINVAL;
  const long long M = (long long)a.N * a.H * a.W;
  if (M > 0x7fffffffLL / 4) return DH_EINVAL;                          // 4 M output pixels are indexed in 32 bits per frame row
  // the LDS-DMA loads move 16 bytes per lane through 32-bit buffer offsets
  if (a.Cin % 4 != 0 || a.ldx % 4 != 0 || !al16(a.x) || !al16(a.w) || M * a.ldx * 4 > kMaxBufferBytes) return DH_EUNSUPPORTED;
  if (a.pre_scale != nullptr && a.Kp > kMaxPreKp) return DH_EUNSUPPORTED;
  const int vec = (cb % 4 == 0) && (a.ldy % 4 == 0) && al16(a.y) && (a.res1 == nullptr || (a.ldr1 % 4 == 0 && al16(a.res1)));
  if (cfg < 0) {
    // the widest tile that still gives every CU a work-group (256 CUs); all tilings sum K in the same order: same bits
    auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn); };
    cfg = tiles(128, 96) >= 256 ? 0 : tiles(128, 32) >= 256 ? 1 : tiles(64, 32) >= 128 ? 2 : 3;
  }
  switch (cfg) {
    case 0: return launch_convt_cfg<4, 1, 1, 3>(a, vec, cb, s);
    case 1: return launch_convt_cfg<4, 1, 1, 1>(a, vec, cb, s);
    case 2: return launch_convt_cfg<2, 1, 1, 1>(a, vec, cb, s);
    case 3: return launch_convt_cfg<1, 1, 1, 1>(a, vec, cb, s);
  }
  return DH_EINVAL;
}

}  // namespace dh
