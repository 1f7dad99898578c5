// Split-bf16 ("bf16x3") variant of the LDS-DMA GEMM of gemm1x1.hip: the same pointwise / K x K implicit GEMM, the same
// fp32 inputs, outputs, epilogue and K order, but every fp32 operand is split EXACTLY into three bf16 parts
//   x = x1 + x2 + x3,   x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)      (round to nearest even)
// and a product is evaluated on the bf16 matrix cores as the six largest of the nine partial products
//   a b ~ a3 b1 + a1 b3 + a2 b2 + a2 b1 + a1 b2 + a1 b1          (dropped: a2 b3 + a3 b2 + a3 b3 <= 2^-23 |a b|)
// accumulated in fp32 inside v_mfma_f32_32x32x16_bf16.  Six bf16 MFMAs cover 16 k-values in 6 x 32 = 192 cycles per
// SIMD; the fp32 MFMA (v_mfma_f32_32x32x2_f32, vector rate) needs 8 x 64 = 512 -- and, unlike the fp32 MFMA, the bf16
// MFMA lets about four VALU instructions per MFMA issue underneath it (LDS reads and DMA pieces do not hide): the K loops
// below are arranged around that budget (profiles/r02_sepconv_fusion_study.md section 3, profiles/r02_split_loop_model.txt).
// The nominal 2.5 PFLOP/s is only sustained on constant operands; on real data the bf16 cores run at ~1.9 PFLOP/s
// (profiles/r02_mfma_data_power.txt).
// The per-product error (2^-23 relative, typically 2^-25) is below what the fp32 accumulation itself contributes
// (sqrt(K) roundings of the running sum), so results stay within the same 1e-3 px of the fp64 oracle
// (profiles/parity_r02_bf16x3.json); they are NOT bit-identical to the fp32-MFMA path, which remains the default.
// Weights are split once on the host (dh_conv2d_pack_weights_split_host / engine/packing.py):
//   [K/8][3 parts][Np][8 bf16]  -- one 16-byte unit per (k-group, part, column) = one lane's B operand.
// The same kernel with P = 2 or 1 parts per operand is the reduced-precision ladder below bf16x3 (dh_conv_args.w_split = 3 / 4,
// Model.gemm_precision = 'bf16x2' / 'bf16'): the products with (a part) + (b part) <= P + 1 -- a2 b1, a1 b2, a1 b1 (about 2^-16
// per product) or a1 b1 alone (plain bf16 operands, about 2^-8) -- i.e. 3 or 1 MFMA per 16 k instead of 6, one or no
// residual pass in the activation split, a B stage of 4 P BN units, weights packed [K/8][P parts][Np][8].  Same K order,
// same epilogue, bit-identical across tilings within a mode; the wide tiling below exists for P = 3 only.
// This file is the three-part mode and the dispatch (the rule: conv_rules.h, gemm1x1_split_eligible); the kernels and their launch side are gemm1x1s_launch.h, the
// two- and one-part modes gemm1x1s_p2.hip / gemm1x1s_p1.hip (one translation unit per mode: compile time).
// Reference layers replaced: as gemm1x1.hip (deephar/layers.py:74-80, 258-301; models/reception.py:43-98).
#include "gemm1x1s_launch.h"

namespace dh {

int launch_gemm1x1_split_p2(const ConvArgs& a, const ConvRoute& r, hipStream_t s);
int launch_gemm1x1_split_p1(const ConvArgs& a, const ConvRoute& r, hipStream_t s);

int launch_gemm1x1_split(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  switch (r.parts) {
    case 3: return launch_split_parts<3>(a, r, s);
    case 2: return launch_gemm1x1_split_p2(a, r, s);
    case 1: return launch_gemm1x1_split_p1(a, r, s);
  }
  return DH_EINVAL;
}

}  // namespace dh
