// The extended scope of the split-bf16 GEMM family (dh_conv_args.w_split = 5 / 6 / 7, Model.gemm_scope = 'extended'): the two
// layer classes of SPNet that the standard rule (gemm1x1_split_eligible) leaves on the fp32 kernels, on the main loop of
// gemm1x1s.hip / gemm1x1s_body.h with the same arithmetic contract -- operands split by repeated round-to-nearest-even AFTER the
// prologue and the ReLU, the products with (a part) + (b part) <= P + 1, smallest first per 16 k, fp32 accumulation, K ascending
// tap-major in every tiling, the fp32 epilogue: the bits of an output depend on the mode and the layer's geometry only.
//   (a) pointwise convolution with a BatchNormalization prologue (the residual units' shortcut convolutions, reference
//       deephar/models/common.py:25-67): the pipelined loop with PRE -- scale | shift tables in LDS behind the NS operand stages,
//       zero beyond K, one fused multiply-add per element in front of the ReLU and the split (split8): the operand that is split
//       has the bits of the fp32 kernel's operand.  The per-wave tiles of 32 rows (TM == 1) only.
//   (b) dense K x K convolution with Cin % 16 == 0 but Cin % 32 != 0 (the entry flow's 48- and 144-channel 3 x 3, reference
//       deephar/models/spnet.py:317-340): the tap-major loop with (kh, kw, c0) resolved per 16-channel half of the 32-k K-step
//       (K16 of the body), every tiling of the body kernel.
// A layer the standard rule takes runs the standard kernels under these codes too (launch_gemm1x1_split): the same bits.
// The packings are those of w_split = 1 / 3 / 4 byte for byte ([Kp/8][P parts][Np][8] bf16, K tap-major, Kp rounded to 32).
// One translation unit per mode, as gemm1x1s_p2.hip / _p1.hip: this file is the three-part mode, the rule and the dispatch; the
// kernel and its launch side are gemm1x1s_ext_launch.h.
#include "gemm1x1s_ext_launch.h"

namespace dh {

bool gemm1x1_eligible(const ConvArgs& a);
int launch_gemm1x1_split(const ConvArgs& a, int cfg, int epi, hipStream_t s);
int launch_gemm1x1_split_ext_p2(const ConvArgs& a, int cfg, int epi, hipStream_t s);
int launch_gemm1x1_split_ext_p1(const ConvArgs& a, int cfg, int epi, hipStream_t s);

// w_split of the extended scope -> the standard code with the same packing and arithmetic (5 / 6 / 7 -> 1 / 3 / 4), else 0
int conv_split_wide_base(int w_split) { return w_split == 5 ? 1 : (w_split == 6 ? 3 : (w_split == 7 ? 4 : 0)); }

namespace {
// which of the two added layer classes a convolution belongs to: 1 = (a), 2 = (b), 0 = neither.  Geometry and alignment
// only; `a.w` is not looked at.
int ext_class(const ConvArgs& a0) {
  ConvArgs a = a0;
  a.w = reinterpret_cast<const float*>(uintptr_t(16));
  a.w_split = 0;                       // (conv_is_skinny / conv_stem_eligible answer for the fp32 packing)
  if (a.N <= 0 || a.H <= 0 || a.W <= 0 || a.OH <= 0 || a.OW <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.KH < 1 || a.KW < 1) return 0;
  if (a.K != a.KH * a.KW * a.Cin || a.Kp % BK != 0 || a.Kp < a.K || a.Np % 32 != 0 || a.Np < a.Cout || a.ldx < a.Cin) return 0;
  if (a.x_u8 || a.up2 || a.x_resample || conv_is_skinny(a) || conv_stem_eligible(a)) return 0;
  if (a.ldx % 4 != 0 || !al16(a.x)) return 0;
  // 32-bit byte offsets into the buffer descriptors
  if ((long long)a.N * a.H * a.W * a.ldx * 4 > kMaxBufferBytes || (long long)a.Kp * a.Np * 6 > kMaxBufferBytes) return 0;
  if (a.pre_scale != nullptr || a.pre_shift != nullptr)      // a prologue needs both tables, and LDS room for them
    return conv_is_pointwise(a) && a.pre_scale != nullptr && a.pre_shift != nullptr && a.Kp <= kMaxPreKp ? 1 : 0;
  return !conv_is_1x1(a) && a.Cin % 16 == 0 && a.SH >= 1 && a.SW >= 1 && a.PT >= 0 && a.PL >= 0 ? 2 : 0;
}
}  // namespace

// What dh_conv2d_f32 accepts with w_split = 5 / 6 / 7: one rule for the three modes, everything the standard rule accepts and
// the two classes above (the weight pointer is not looked at: a binding asks before it packs).
bool gemm1x1_split_wide_eligible(const ConvArgs& a) { return gemm1x1_split_eligible(a) || ext_class(a) != 0; }

int launch_gemm1x1_split_wide(const ConvArgs& a0, int cfg, int epi, hipStream_t s) {
  const int base = conv_split_wide_base(a0.w_split);
  if (base == 0) return DH_EINVAL;
  if (!al16(a0.w)) return DH_EUNSUPPORTED;
  ConvArgs a = a0;
  a.w_split = base;
  if (gemm1x1_split_eligible(a)) {     // a layer of the standard scope: the standard kernels, the same bits
    if (!gemm1x1_eligible(a)) return DH_EUNSUPPORTED;
    if (a.up2 && cfg == 0) cfg = 2;
    return launch_gemm1x1_split(a, cfg, epi, s);
  }
  if (ext_class(a) == 0) return DH_EUNSUPPORTED;       // never run on another kernel
  switch (conv_split_parts(base)) {
    case 3: return launch_ext_parts<3>(a, cfg, epi, s);
    case 2: return launch_gemm1x1_split_ext_p2(a, cfg, epi, s);
    case 1: return launch_gemm1x1_split_ext_p1(a, cfg, epi, s);
  }
  return DH_EINVAL;
}
}  // namespace dh
