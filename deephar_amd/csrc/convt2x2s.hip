// Conv2DTranspose((2, 2), strides=(2, 2), padding='same', use_bias=False) on the split-bf16 precision ladder -- the up-scaling
// unit of SPNet's learned-resampling flavour (reference deephar/models/common.py:103-106, deephar/layers.py:83-89) under
// Model.gemm_precision = 'bf16x3' / 'bf16x2' / 'bf16'.
//
// The same GEMM as convt2x2.hip, [M = N*H*W, K = Cin] x [Cin, 4 * Cout] with a depth-to-space store, on the bf16 matrix cores:
// the software-pipelined main loop of gemm1x1s.hip (activations split on the fly into P bf16 parts, weights split on the host,
// the products with (a part) + (b part) <= P + 1, smallest first per 16 k, K ascending in every tiling: the bits of an output
// depend on the mode and the layer's geometry only) in front of the depth-to-space epilogue the fp32 kernel uses
// (conv_common.h: d2s_epilogue).  What the convolution kernels of the family do not have and this layer always needs
// (BN -> ReLU -> Conv2DTranspose) is the BatchNormalization prologue: scale | shift tables in LDS behind the operand stages,
// one fused multiply-add per element in front of the ReLU and the split (gemm1x1s.hip: split8, PRE) -- the operand that is
// split has the bits of the fp32 kernel's operand.
// Pointwise only, per-wave tiles of 32 rows (the pipelined loop), two LDS stages: the layer has few rows (M = frames x 16 /
// 64 / 256 in SPNet) and 1152 ... 1920 columns, so the tilings go down to 32 x 32 to keep 256 CUs busy.
// The kernel body of the family (gemm1x1s_body.h) is compiled here for this layer's instantiations only.
#include "gemm_family.h"
#include "split_bf16.h"

namespace dh {
namespace {

template <int P, int WM, int WN, int TN, bool RELU, bool PRE>
__global__ __launch_bounds__(WM* WN * 64, 2) void convt2x2s_kernel(const ConvArgs p, const int epi_vec, const int cb) {
  constexpr int TM = 1, NS = 2;
  constexpr bool UP2 = false, KXK = false, D2S = true, K16 = false;
#include "gemm1x1s_body.h"
}

template <int P, int WM, int WN, int TN, bool RELU, bool PRE>
int launch_convts_variant(const ConvArgs& a, int vec, int cb, unsigned tiles, hipStream_t s) {
  constexpr size_t kMax = gemm_split_lds(P, WM, WN, 1, TN, 2, PRE, 0).limit;
  static_assert(kMax <= 160 * 1024, "LDS budget");
  auto kern = convt2x2s_kernel<P, WM, WN, TN, RELU, PRE>;
  if (kMax > 64 * 1024) {
    static LdsLimit lim;
    lim.raise((const void*)kern, (int)kMax);
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), gemm_split_lds(P, WM, WN, 1, TN, 2, PRE, a.Kp).launch, s, a, vec, cb);
  return check_launch();
}

template <int P, int WM, int WN, int TN>
int launch_convts_cfg(const ConvArgs& a, int vec, int cb, hipStream_t s) {
  unsigned t;
  if (gemm_tile_count(a, WM * 32, WN * TN * 32, &t) != DH_OK) return DH_EINVAL;
  if (a.pre_scale != nullptr)
    return a.pre_relu ? launch_convts_variant<P, WM, WN, TN, true, true>(a, vec, cb, t, s)
                      : launch_convts_variant<P, WM, WN, TN, false, true>(a, vec, cb, t, s);
  return a.pre_relu ? launch_convts_variant<P, WM, WN, TN, true, false>(a, vec, cb, t, s)
                    : launch_convts_variant<P, WM, WN, TN, false, false>(a, vec, cb, t, s);
}

constexpr int kNumCfgs = 5;

template <int P>
int launch_convts_parts(const ConvArgs& a, int cfg, int vec, int cb, hipStream_t s) {
  switch (cfg) {
    case 0: return launch_convts_cfg<P, 4, 1, 3>(a, vec, cb, s);     // 128 x 96
    case 1: return launch_convts_cfg<P, 2, 1, 3>(a, vec, cb, s);     // 64 x 96
    case 2: return launch_convts_cfg<P, 4, 1, 1>(a, vec, cb, s);     // 128 x 32
    case 3: return launch_convts_cfg<P, 2, 1, 1>(a, vec, cb, s);     // 64 x 32
    case 4: return launch_convts_cfg<P, 1, 1, 1>(a, vec, cb, s);     // 32 x 32
  }
  return DH_EINVAL;
}

// DH_OK: a layer launch_convt2x2_split runs (a.w aside); DH_EINVAL: arguments that describe no layer; DH_EUNSUPPORTED: a layer
// the kernel is not built for.  Geometry and alignment only: no pointer is dereferenced, the weight pointer is not looked at.
int convts_check(const ConvArgs& a, int cb) {
  if (a.N <= 0 || a.H <= 0 || a.W <= 0 || a.Cin <= 0 || cb <= 0 || a.Cout != 4 * cb) return DH_EINVAL;
  if (a.Kp % BK != 0 || a.Np % 32 != 0 || a.Kp < a.Cin || a.Np < a.Cout || a.ldx < a.Cin || a.ldy < cb ||
      (a.res1 != nullptr && a.ldr1 < cb))
    return DH_EINVAL;
  const long long M = (long long)a.N * a.H * a.W;
  if (M > 0x7fffffffLL / 4) return DH_EINVAL;                          // 4 M output pixels are indexed in 32 bits per frame row
  // the LDS-DMA loads move 16 bytes per lane through 32-bit buffer offsets (activations, packed split weight)
  if (a.Cin % 4 != 0 || a.ldx % 4 != 0 || !al16(a.x)) return DH_EUNSUPPORTED;
  if (M * a.ldx * 4 > kMaxBufferBytes || (long long)a.Kp * a.Np * 6 > kMaxBufferBytes) return DH_EUNSUPPORTED;
  return a.pre_scale == nullptr || a.Kp <= kMaxPreKp ? DH_OK : DH_EUNSUPPORTED;
}

}  // namespace

int convt2x2_split_num_cfgs() { return kNumCfgs; }

// What launch_convt2x2_split accepts, for every `parts` (a binding asks before it packs).  `a` describes the GEMM as for
// launch_convt2x2.
bool convt2x2_split_eligible(const ConvArgs& a, int cb) { return convts_check(a, cb) == DH_OK; }

// `a`, `cb` as for launch_convt2x2 (convt2x2.hip); a.w is the [Kp/8][parts][Np][8] bf16 packing of the [Cin, 4 * cb] matrix.
int launch_convt2x2_split(const ConvArgs& a, int cb, int parts, int cfg, hipStream_t s) {
  if (parts < 1 || parts > 3) return DH_EINVAL;
  if (const int rc = convts_check(a, cb); rc != DH_OK) return rc;
  if (!al16(a.w)) return DH_EUNSUPPORTED;
  const long long M = (long long)a.N * a.H * a.W;
  const int vec = (cb % 4 == 0) && (a.ldy % 4 == 0) && al16(a.y) && (a.res1 == nullptr || (a.ldr1 % 4 == 0 && al16(a.res1)));
  if (cfg < 0) {
    // the widest tile that still gives every CU a work-group (256 CUs); all tilings sum K in the same order: same bits
    auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn); };
    cfg = tiles(128, 96) >= 256 ? 0 : tiles(64, 96) >= 256 ? 1 : tiles(128, 32) >= 256 ? 2 : tiles(64, 32) >= 128 ? 3 : 4;
  }
  switch (parts) {
    case 3: return launch_convts_parts<3>(a, cfg, vec, cb, s);
    case 2: return launch_convts_parts<2>(a, cfg, vec, cb, s);
    case 1: return launch_convts_parts<1>(a, cfg, vec, cb, s);
  }
  return DH_EINVAL;
}

}  // namespace dh
