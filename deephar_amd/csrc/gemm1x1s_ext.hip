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
// A layer the standard rule takes runs the standard kernels under these codes too (conv_route): the same bits.
// The packings are those of w_split = 1 / 3 / 4 byte for byte ([Kp/8][P parts][Np][8] bf16, K tap-major, Kp rounded to 32).
// One translation unit per mode, as gemm1x1s_p2.hip / _p1.hip: this file is the three-part mode and the dispatch (the rule: conv_rules.h, conv_split_ext_class); the
// kernel and its launch side are gemm1x1s_ext_launch.h.
#include "gemm1x1s_ext_launch.h"

namespace dh {

int launch_gemm1x1_split_ext_p2(const ConvArgs& a, const ConvRoute& r, hipStream_t s);
int launch_gemm1x1_split_ext_p1(const ConvArgs& a, const ConvRoute& r, hipStream_t s);

int launch_gemm1x1_split_ext(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  switch (r.parts) {
    case 3: return launch_ext_parts<3>(a, r, s);
    case 2: return launch_gemm1x1_split_ext_p2(a, r, s);
    case 1: return launch_gemm1x1_split_ext_p1(a, r, s);
  }
  return DH_EINVAL;
}

}  // namespace dh
