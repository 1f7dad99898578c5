// What the host side decides about a convolution from its arguments alone: the argument checks and the rules that say
// which kernel family a layer belongs to.  No HIP header, no stream: conv_route.h builds the launch decision from these,
// the C-ABI exports (capi.hip) answer with them, and a plain C++ compiler can sweep them.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "deephar_hip.h"

namespace dh {

using ConvArgs = dh_conv_args;

constexpr int BK = 32;             // k values per K-step of the MFMA convolution kernels (the wide split tiling walks 16)
constexpr int kMaxPreKp = 4096;    // BN prologue of the LDS-DMA GEMMs: scale + shift tables of at most 2 x 16 KB in LDS
constexpr int kSkinnyMaxCin = 4096;   // skinny-conv kernel: prologue table in LDS, 2 x Cin floats
constexpr int kStemOW = 128;       // first-layer kernel: output columns of a row
constexpr long long kInt31 = 0x7fffffffLL;

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
// bytes a buffer descriptor may span: every 32-bit byte offset into it stays below the out-of-range offsets the kernels use
constexpr long long kMaxBufferBytes = 0xf0000000LL;
// a 1x1 / stride-1 / unpadded filter ...
inline bool conv_is_1x1(const ConvArgs& a) { return a.KH == 1 && a.KW == 1 && a.SH == 1 && a.SW == 1 && a.PT == 0 && a.PL == 0; }
// ... over a map it leaves the size of, with 16-byte channel runs: the pointwise form of the LDS-DMA GEMM family
inline bool conv_is_pointwise(const ConvArgs& a) { return conv_is_1x1(a) && a.H == a.OH && a.W == a.OW && a.Cin % 4 == 0; }

// The checks every entry point that launches an MFMA or skinny convolution makes on the geometry: positive extents and a
// packing that covers K x Cout ...
inline int conv_check_packing(const ConvArgs& a) {
  if (a.N <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.OH <= 0 || a.OW <= 0) return DH_EINVAL;
  if (a.Kp % BK != 0 || a.Np % 32 != 0 || a.Kp < a.K || a.Np < a.Cout || a.K != a.KH * a.KW * a.Cin) return DH_EINVAL;
  return DH_OK;
}
// ... and pixel counts inside 31 bits
inline int conv_check_geometry(const ConvArgs& a) {
  if (conv_check_packing(a) != DH_OK) return DH_EINVAL;
  if ((long long)a.N * a.H * a.W > kInt31 || (long long)a.N * a.OH * a.OW * (a.up2 ? 4 : 1) > kInt31) return DH_EINVAL;
  return DH_OK;
}
// The NULL / pairing checks of dh_conv2d_f32 in front of them.
inline int conv_check_pointers(const ConvArgs* a) {
  if (a == nullptr || a->x == nullptr || a->w == nullptr || a->y == nullptr) return DH_EINVAL;
  if ((a->pre_scale == nullptr) != (a->pre_shift == nullptr)) return DH_EINVAL;
  if ((a->post_scale == nullptr) != (a->post_shift == nullptr)) return DH_EINVAL;
  if (a->SH <= 0 || a->SW <= 0 || a->KH <= 0 || a->KW <= 0) return DH_EINVAL;
  return DH_OK;
}

// Work-groups of a bm x bn tiling of the GEMM [M = N * OH * OW] x [Cout]: the grid's x dimension, so DH_EINVAL outside (0, 2^31)
inline int gemm_tile_count(const ConvArgs& a, int bm, int bn, unsigned* tiles) {
  const long long M = (long long)a.N * a.OH * a.OW;
  const long long t = ((M + bm - 1) / bm) * ((a.Cout + bn - 1) / bn);
  if (t <= 0 || t > kInt31) return DH_EINVAL;
  *tiles = (unsigned)t;
  return DH_OK;
}

// 1 = the 16-byte epilogue; 0 as soon as ONE of y, res1, res2 or the BN tables is misaligned
inline int conv_epi_vec(const ConvArgs& a) {
  return (a.Cout % 4 == 0) && (a.ldy % 4 == 0) && al16(a.y) && (a.res1 == nullptr || (a.ldr1 % 4 == 0 && al16(a.res1))) &&
         (a.res2 == nullptr || (a.ldr2 % 4 == 0 && al16(a.res2))) &&
         (a.post_scale == nullptr || (al16(a.post_scale) && al16(a.post_shift)));
}
// Launch-side half of the direct epilogue: `epi` (1 = 16-byte epilogue possible) gains bit 1 when interior tiles may
// store straight from the accumulators -- no up-sampling, no pooled second output, a second residual only at half
// resolution, and every byte offset of y / res1 / res2 inside 31 bits (buffer offsets are 32-bit).
inline int epi_with_direct(const ConvArgs& a, int epi, bool half_res_residual = true) {
  const long long M = (long long)a.N * a.OH * a.OW;
  const int ohw = a.OH * a.OW;
  // a second residual only in its half-resolution form, on maps where a wave's 32 pixels sit in one frame, start at an
  // even image row and split into shifts: 2^a x 2^b >= 32 pixels, at least 8 wide
  const bool r2ok = a.res2 == nullptr || (half_res_residual && a.res2_down && (a.OW & (a.OW - 1)) == 0 && (ohw & (ohw - 1)) == 0 && a.OW >= 8 &&
                                          ohw >= 32 && (M / 4) * a.ldr2 * 4 < kInt31);
  const bool direct = epi && !a.up2 && a.y_pool == nullptr && r2ok && M * a.ldy * 4 < kInt31 &&
                      (a.res1 == nullptr || M * a.ldr1 * 4 < kInt31);
  return epi | (direct ? 2 : 0);
}
// the float4 A gather of the general kernel
inline bool conv_vec4(const ConvArgs& a) {
  return !a.x_u8 && (a.Cin % 4 == 0) && (a.ldx % 4 == 0) && al16(a.x) && (a.pre_scale == nullptr || (al16(a.pre_scale) && al16(a.pre_shift)));
}

// ---- skinny-conv kernel (conv_splitk.hip) ------------------------------------------------------------------------------
// Shape rule -- deterministic, independent of timing, of the batch size and of buffer alignment (the bits of a layer
// must not depend on any of them): at most 256 output positions per frame / clip, at most 256 output channels, a
// reduction of at least 64 (shorter ones are one or two K-steps of the general kernel anyway).  [r05: was K >= 768 and
// Cin % 4 == 0 -- the action heads' 1x1 / 3x3 convolutions with K = 70 .. 720 ran 15-33 us on one wave per tile.]
inline bool conv_is_skinny(const ConvArgs& a) {
  if (a.x_u8 || a.w_split) return false;
  // kernel extent: `locate` decodes tap -> (kh, kw) as (tap * magic_kw) >> 16, exact while tap * KW < 2^16 -- KH * KW < 256
  // keeps tap < 256 and KW < 256 (KW < 256 alone admitted KW = 255, KH >= 2, where tap >= 258 decodes wrong)
  // DEEPHAR_SKINNY_MIN_K: A/B aid for the rule's K threshold (read once; planner.split_k_rule reads the same variable)
  static const int min_k = [] { const char* e = getenv("DEEPHAR_SKINNY_MIN_K"); return e != nullptr ? atoi(e) : 64; }();
  return a.OH * a.OW <= 256 && a.K >= min_k && a.Cout <= 256 && a.Cin >= 2 && a.Cin <= kSkinnyMaxCin && a.KH >= 1 && a.KW >= 1 &&
         (long long)a.KH * a.KW < 256 && (long long)a.K * a.Cin < (1ll << 31);
}

// ---- first-layer kernel (conv_stem.hip) --------------------------------------------------------------------------------
// The layers it takes (a rule on the layer's geometry; the route asks it for every launch):
// 3 dense input channels, stride 2, 3x3 or 7x7, 128 output columns, an even number of output rows, 32 or 64 output
// channels, fp32 tap-major weights, BN / ReLU epilogue only.
inline bool conv_stem_eligible(const ConvArgs& a) {
  const bool geom = a.Cin == 3 && a.ldx == 3 && a.SH == 2 && a.SW == 2 && a.KH == a.KW && (a.KH == 3 || a.KH == 7) &&
                    a.OW == kStemOW && (a.OH & 1) == 0 && (a.Cout == 32 || a.Cout == 64) && a.PT >= 0 && a.PL >= 0 &&
                    a.PL <= a.KW && a.K == a.KH * a.KW * 3;
  const bool plain = a.pre_scale == nullptr && !a.pre_relu && a.res1 == nullptr && a.res2 == nullptr && !a.up2 &&
                     a.y_pool == nullptr && a.w_split == 0 && (!a.x_u8 || a.in_lut != nullptr);
  const bool fits = (long long)a.N * a.OH * a.OW * a.ldy * 4 < kInt31 && (reinterpret_cast<uintptr_t>(a.y) & 3) == 0;
  return geom && plain && fits;
}
// pairs of output rows per work-group
inline int conv_stem_pairs_per_wg(const ConvArgs& a) {
  const int pairs = a.OH / 2;
  return pairs % 4 == 0 ? 4 : (pairs % 2 == 0 ? 2 : 1);
}

// ---- LDS-DMA GEMM family (gemm1x1.hip, gemm1x1s*.hip) ---------------------------------------------------------------------
inline bool gemm1x1_eligible(const ConvArgs& a) {
  const bool aligned = a.ldx % 4 == 0 && al16(a.x) && al16(a.w);
  const bool pointwise = conv_is_pointwise(a);
  // K x K: a K-step must not straddle filter taps, the up-sampling epilogue is only built for the pointwise form
  const bool kxk = a.Cin % BK == 0 && !a.up2 && a.KH >= 1 && a.KW >= 1 && a.SH >= 1 && a.SW >= 1 && a.PT >= 0 &&
                   a.PL >= 0;
  // a BatchNormalization prologue: the plain pointwise form only (no zero padding to apply it around, no fused
  // up-sampling), fp32 weights, tables that fit LDS
  const bool pre_ok = a.pre_scale == nullptr || (pointwise && !a.up2 && a.w_split == 0 && a.Kp <= kMaxPreKp);
  const bool fits32 = (long long)a.N * a.H * a.W * a.ldx * 4 <= kMaxBufferBytes;   // 32-bit buffer offsets
  return aligned && pre_ok && fits32 && (pointwise || kxk);
}

// bf16 parts per operand of a split packing (dh_conv_args.w_split 1 / 3 / 4 -> 3 / 2 / 1), 0 for the fp32 packings
inline int conv_split_parts(int w_split) { return w_split == 1 ? 3 : (w_split == 3 ? 2 : (w_split == 4 ? 1 : 0)); }
// w_split of the extended scope -> the standard code with the same packing and arithmetic (5 / 6 / 7 -> 1 / 3 / 4), else 0
inline int conv_split_wide_base(int w_split) { return w_split == 5 ? 1 : (w_split == 6 ? 3 : (w_split == 7 ? 4 : 0)); }

// What dh_conv2d_f32 accepts with a split packing, w_split = 1 / 3 / 4: one rule for every mode (the weight pointer itself
// is not looked at: a binding asks before it packs).
inline bool gemm1x1_split_eligible(const ConvArgs& a0) {
  ConvArgs a = a0;
  a.w = reinterpret_cast<const float*>(uintptr_t(16));
  a.w_split = 0;                       // (conv_is_skinny answers for the fp32 packing)
  if (a.x_u8 || a.pre_scale != nullptr || conv_is_skinny(a) || !gemm1x1_eligible(a)) return false;   // (no BN prologue on the split path)
  // 32-bit byte offsets into the buffer descriptors
  return (long long)a.N * a.H * a.W * a.ldx * 4 <= kMaxBufferBytes && (long long)a.Kp * a.Np * 6 <= kMaxBufferBytes;
}

// The extended scope (w_split = 5 / 6 / 7, gemm1x1s_ext.hip): which of the two added layer classes a convolution belongs to,
// 1 = (a) pointwise with a BN prologue, 2 = (b) dense K x K with Cin % 16 == 0, 0 = neither.  Geometry and alignment only;
// `a.w` is not looked at.
inline int conv_split_ext_class(const ConvArgs& a0) {
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
// What dh_conv2d_f32 accepts with w_split = 5 / 6 / 7: one rule for the three modes, everything the standard rule accepts and
// the two classes above (the weight pointer is not looked at: a binding asks before it packs).
inline bool gemm1x1_split_wide_eligible(const ConvArgs& a) { return gemm1x1_split_eligible(a) || conv_split_ext_class(a) != 0; }

// ---- halo-resident K x K kernel (conv_halo.hip) ------------------------------------------------------------------------
constexpr int HCH = 16;                   // channels per resident chunk
constexpr int HPIX = 80;                  // LDS bytes per halo pixel (64 + 16 pad)
constexpr int HMAXA = 12;                 // halo DMA instructions per wave (<= 48 KB per chunk)
constexpr int HMAXB = 8;                  // weight-stage DMA passes (KW * BN <= 512)

struct HaloTile {
  int ct_log2;      // output columns per tile = 1 << ct_log2 (OW, or 128 for wider rows)
  int hr, hc;       // halo rows / columns
  int a_bytes;      // one halo buffer, rounded up to whole 1 KB DMA instructions
  int nbuf_a;       // 1 or 2 halo buffers
  int b_bytes;      // one weight stage, rounded up to whole 4 KB DMA passes
  int bpass;
  int hc_magic;     // (1 << 20) / hc + 1: px / hc for px < 1024 as one multiply and a shift (an integer divide is ~40 VALU)
};

// the tile of the tiling with tn x 32 output channels; false when it does not exist for this layer
inline bool conv_halo_tile(const ConvArgs& a, int tn, HaloTile* g) {
  const int bn = tn * 32;
  int ct;
  if (a.OW >= 128) {
    if (a.OW % 128) return false;
    ct = 128;
  } else {
    ct = a.OW;
    if (ct < 8 || (ct & (ct - 1)) || (a.OH * a.OW) % 128) return false;
  }
  int lg = 0;
  while ((1 << lg) < ct) ++lg;
  const int rt = 128 / ct;
  g->ct_log2 = lg;
  g->hr = (rt - 1) * a.SH + a.KH;
  g->hc = (ct - 1) * a.SW + a.KW;
  g->a_bytes = (g->hr * g->hc * HPIX + 1023) & ~1023;
  g->b_bytes = (4 * a.KW * bn * 16 + 4095) & ~4095;
  g->bpass = g->b_bytes >> 12;
  g->hc_magic = (1 << 20) / g->hc + 1;
  if ((g->a_bytes >> 10) > 4 * HMAXA || g->bpass > HMAXB) return false;
  // two work-groups per CU need <= 80 KB each; a second halo buffer (prefetch of the next chunk) when it fits
  const int epi = 4 * 32 * (bn + 4) * 4;
  const int one = g->a_bytes + 2 * g->b_bytes, two = 2 * g->a_bytes + 2 * g->b_bytes;
  g->nbuf_a = (two <= 80 * 1024 && a.Cin > HCH) ? 2 : 1;
  const int total = g->nbuf_a == 2 ? two : one;
  return (total > epi ? total : epi) <= 80 * 1024;
}

// What the kernel can run: dense K x K with K > 1 somewhere, stride 1 (stride 2 keeps the tap-major kernels: its halo is
// 4x the output tile), Cin a multiple of 16, float input, 16-byte aligned views, no BN prologue / fused up-sampling,
// whole-row output tiles of 128 pixels, LDS budget.
inline bool conv_halo_supported(const ConvArgs& a0) {
  ConvArgs a = a0;
  a.w_split = 0;
  if (a.x_u8 || a.up2 || a.pre_scale != nullptr || conv_is_skinny(a)) return false;
  if (a.KH * a.KW <= 1 || a.KH > 7 || !(a.KW == 1 || a.KW == 3 || a.KW == 5)) return false;
  if (a.SH != 1 || a.SW != 1 || a.PT < 0 || a.PL < 0) return false;
  if (a.Cin % HCH || a.Cin < 32 || a.ldx % 4 || !al16(a.x)) return false;
  if ((long long)a.N * a.H * a.W * a.ldx * 4 > kMaxBufferBytes) return false;
  if (a.OH * a.OW < 1024) return false;      // small maps keep the tap-major kernels (a per-frame rule: never on N)
  HaloTile g;
  return conv_halo_tile(a, 1, &g);
}
// The layers a binding gives to this kernel (dh_conv2d_halo_eligible; a rule on the per-frame geometry only): what it can
// run AND what the LDS-DMA tap-major kernel cannot -- Cin not a multiple of 32 (SPNet's 48- and 144-channel 3x3 convs,
// which otherwise fall to the register-gather kernel: 1.17-1.21x faster here).  With Cin % 32 == 0 the two kernels are
// within +-5 % of each other (tools/bench_halo.py, profiles/r03_bench_halo.json), so those layers keep the tap-major
// family and its tiling freedom.
inline bool conv_halo_eligible(const ConvArgs& a) { return a.Cin % 32 != 0 && conv_halo_supported(a); }
constexpr int kNumHaloCfgs = 3;           // tile_cfg 0, 1, 2 -> TN = 1, 2, 3 (output-channel tile 32, 64, 96)

}  // namespace dh
