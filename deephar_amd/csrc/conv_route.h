// dh_conv2d_f32's launch decision as one pure function: which kernel family runs a request, in which tiling and epilogue
// form, or the code that refuses it.  No HIP header, no stream, no pointer dereferenced.  launch_conv_igemm launches what
// the route says and dh_conv2d_route exports it, so a test asks the library what it will do instead of restating it.
#pragma once
#include "gemm_family.h"

namespace dh {

using ConvRoute = dh_conv_route;

inline ConvRoute conv_refuse(int rc) {
  ConvRoute r = {};
  r.rc = rc;
  r.tile_cfg = -1;
  return r;
}

// Default tiling when the caller does not autotune (measured on MI355X, tools/bench_ops.py): four waves
// side by side along M with narrow per-wave tiles (more resident waves per SIMD) beat the 2x2-wave layouts;
// memory/epilogue-bound shapes (tiny K or tiny M) want the narrowest tile.
inline int conv_igemm_pick_cfg(int M, int Cout) {
  const int np = (Cout + 31) / 32 * 32;
  auto blocks = [&](int bm, int bn) { return (long long)((M + bm - 1) / bm) * ((np + bn - 1) / bn); };
  int bn = 32;
  if (np % 96 == 0) bn = 96;
  else if (np % 64 == 0) bn = 64;
  if (bn == 96) return blocks(128, 96) >= 512 ? 2 : (blocks(128, 32) >= 512 ? 4 : 7);
  if (bn == 64) return blocks(128, 64) >= 512 ? 3 : (blocks(128, 32) >= 512 ? 4 : 7);
  if (blocks(128, 32) >= 512) return 4;
  if (blocks(64, 32) >= 256) return 7;
  return 8;
}

// A tiling of kGemmTiles on one of the four MFMA GEMM kernels; `parts`: bf16 parts per operand (split kernels), else 0.
inline ConvRoute conv_route_tiled(const ConvArgs& a, int kernel, int cfg, int parts, int epi) {
  if (a.up2 && cfg == 0) cfg = 2;        // 128 x 192 + the fused up-sampling epilogue exceeds the register budget
  const GemmTile& t = kGemmTiles[cfg];
  const bool ext = kernel == DH_CONV_SPLIT_EXT;
  ConvRoute r = {DH_OK, kernel, cfg, parts, t.bm(), t.bn(), t.tm, 1, epi, a.y_pool == nullptr ? 0 : (a.OW == 32 ? 1 : 2), 0};
  if (parts != 0 && !tile_has_parts(t, parts, ext)) return conv_refuse(DH_EUNSUPPORTED);
  if (gemm_tile_count(a, r.bm, r.bn, &r.tiles) != DH_OK) return conv_refuse(DH_EINVAL);
  if (a.y_pool != nullptr && !tile_pools_for(t, a.OW)) return conv_refuse(DH_EUNSUPPORTED);
  if (kernel == DH_CONV_GENERAL) {
    r.vec4 = conv_vec4(a);
    if (a.up2 && !r.vec4) return conv_refuse(DH_EUNSUPPORTED);
  }
  if (a.up2 && !tile_has_up2(t)) return conv_refuse(DH_EUNSUPPORTED);     // (the heuristic never asks for it)
  if (ext) {
    const bool pre = a.pre_scale != nullptr;
    if ((pre && !tile_has_ext_prologue(t)) || !tile_ext_fits(t, parts, pre)) return conv_refuse(DH_EUNSUPPORTED);
  }
  return r;
}

// cfg: 0, 1, 2 -> TN = 1, 2, 3; < 0: the widest that fits and divides the work well
inline ConvRoute conv_route_halo(const ConvArgs& a, int cfg, int epi) {
  if (!conv_halo_supported(a) || !al16(a.w)) return conv_refuse(DH_EUNSUPPORTED);
  if (cfg >= kNumHaloCfgs) return conv_refuse(DH_EINVAL);
  int tn = cfg + 1;
  HaloTile g;
  if (cfg < 0) {
    const int np = (a.Cout + 31) / 32;
    tn = np % 3 == 0 ? 3 : (np % 2 == 0 ? 2 : (np >= 3 ? 3 : np));
    while (tn > 1 && !conv_halo_tile(a, tn, &g)) --tn;
  }
  if (!conv_halo_tile(a, tn, &g)) return conv_refuse(DH_EUNSUPPORTED);
  const long long M = (long long)a.N * a.OH * a.OW;
  const long long tiles = (M / 128) * ((a.Cout + tn * 32 - 1) / (tn * 32));
  if (tiles <= 0 || tiles > kInt31) return conv_refuse(DH_EINVAL);
  return {DH_OK, DH_CONV_HALO, tn - 1, 0, 128, tn * 32, 1, 1, epi, a.y_pool == nullptr ? 0 : (a.OW == 32 ? 1 : 2), (unsigned)tiles};
}

// tile_cfg is ignored (but must name a tiling): one wave-count per K, tiles of 16 pixels x 16 channels
inline ConvRoute conv_route_skinny(const ConvArgs& a, int cfg) {
  if (a.res2_down) return conv_refuse(DH_EUNSUPPORTED);          // (the split-K kernel has its own, simpler epilogue)
  if (cfg >= kNumConvCfgs) return conv_refuse(DH_EINVAL);
  const long long M = (long long)a.N * a.OH * a.OW;
  const long long tiles = ((M + 15) / 16) * ((a.Cout + 15) / 16);
  if (tiles <= 0 || tiles > kInt31 || (long long)a.H * a.W * a.ldx * (a.x_resample >= 2 ? 4 : 1) > kInt31 || a.Kp % 16 != 0)
    return conv_refuse(DH_EINVAL);
  if (a.x_resample < 0 || a.x_resample > 3 || (a.x_resample == 1 && ((a.H | a.W) & 1))) return conv_refuse(DH_EINVAL);
  // (the vector form is a property of the layer wherever the engine lays tensors out 16-byte aligned; both forms load
  //  the same values and run the same arithmetic: same bits)
  const int vec = a.Cin % 4 == 0 && a.ldx % 4 == 0 && al16(a.x);
  return {DH_OK, DH_CONV_SKINNY, -1, 0, 16, 16, 0, vec, 0, 0, (unsigned)tiles};
}

inline ConvRoute conv_route_stem(const ConvArgs& a, int cfg) {
  if (cfg >= kNumConvCfgs) return conv_refuse(DH_EINVAL);
  const long long blocks = (long long)a.N * (a.OH / 2 / conv_stem_pairs_per_wg(a));
  if (blocks <= 0 || blocks > kInt31) return conv_refuse(DH_EINVAL);
  return {DH_OK, DH_CONV_FIRST_LAYER, -1, 0, 0, 0, 0, 0, 0, 0, (unsigned)blocks};
}

// PRE: conv_check_pointers(&a) == DH_OK and the res2_down check of dh_conv2d_f32.  When several refusals apply, the first
// in this order answers.
inline ConvRoute conv_route(const ConvArgs& a, int cfg) {
  if (conv_check_geometry(a) != DH_OK) return conv_refuse(DH_EINVAL);
  if (a.x_u8 && a.in_lut == nullptr) return conv_refuse(DH_EINVAL);
  if (a.w_split < 0 || a.w_split > 7) return conv_refuse(DH_EINVAL);
  const bool skinny = conv_is_skinny(a);
  if (a.y_pool != nullptr) {             // pooled second output: one image row per wave (pairs of waves pool), or [r06] two /
                                         // four whole image rows per wave (OW = 16 / 8: the wave pools alone)
    const bool ok = (a.OW == 32 || ((a.OW == 16 || a.OW == 8) && (a.OH * a.OW) % 32 == 0)) && a.OH % 2 == 0 && !a.up2 && !a.x_u8 &&
                    a.ldyp % 4 == 0 && a.Cout % 4 == 0 && al16(a.y_pool) && a.ldy % 4 == 0 && a.w_split != 2 && al16(a.y) && !skinny;
    if (!ok) return conv_refuse(DH_EUNSUPPORTED);
  }
  if (a.x_resample && !skinny) return conv_refuse(DH_EUNSUPPORTED);   // (resampling on load: the skinny-conv kernel only)
  // tiny output, long reduction: the in-work-group split-K kernel, whatever tiling was asked for (shape rule: the
  // result bits of a layer must not depend on a timing-based choice)
  if (skinny) return conv_route_skinny(a, cfg);
  // first layer (3 input channels, stride 2): its own kernel, by a rule on the layer's geometry like the split-K layers --
  // it pairs the k values of an MFMA differently from the tap-major kernels, so its last bits differ from theirs and a
  // layer must never move between the two on a timing-based choice
  if (conv_stem_eligible(a)) return conv_route_stem(a, cfg);
  const int epi = conv_epi_vec(a);
  if (a.y_pool != nullptr && !epi) return conv_refuse(DH_EUNSUPPORTED);
  // chunk-major fp32 packing: the halo-resident kernel only (its direct epilogue carries no second residual)
  if (a.w_split == 2) return conv_route_halo(a, cfg, epi_with_direct(a, epi, false));
  const bool dma = !a.w_split && gemm1x1_eligible(a);
  if (cfg < 0 && a.y_pool != nullptr) {
    cfg = conv_igemm_pick_cfg(a.N * a.OH * a.OW, a.Cout);
    if (cfg == 8 && a.OW == 32) cfg = 7;  // 32 x 32 has no wave pair
    if (cfg == 0 || cfg == 1) cfg = 2;    // 64-row waves do not pool
    if (dma) cfg += kNumF32Cfgs;
  }
  if (cfg < 0) cfg = conv_igemm_pick_cfg(a.N * a.OH * a.OW, a.Cout) + (dma && !a.x_u8 ? kNumF32Cfgs : 0);
  if (!a.w_split && cfg >= kNumConvCfgs) return conv_refuse(DH_EINVAL);
  if (a.x_u8 && cfg >= kNumF32Cfgs) return conv_refuse(DH_EUNSUPPORTED);
  if (a.w_split) {                       // split-bf16 weights: only the LDS-DMA GEMM family reads that packing
    ConvArgs b = a;
    if (a.w_split >= 5) {                // the extended scope (5 / 6 / 7): its own rule, refused layers run on no other kernel
      if (cfg >= kNumSplitCfgs) return conv_refuse(DH_EINVAL);
      if (!al16(a.w)) return conv_refuse(DH_EUNSUPPORTED);
      b.w_split = conv_split_wide_base(a.w_split);
      if (!gemm1x1_split_eligible(b)) {  // not a layer of the standard scope (those run the standard kernels: the same bits)
        if (conv_split_ext_class(b) == 0) return conv_refuse(DH_EUNSUPPORTED);
        return conv_route_tiled(b, DH_CONV_SPLIT_EXT, cfg, conv_split_parts(b.w_split), epi);
      }
    }
    // w_split 1 / 3 / 4: three / two / one part
    if (b.x_u8 || !gemm1x1_eligible(b)) return conv_refuse(DH_EUNSUPPORTED);
    if (cfg >= kNumSplitCfgs) return conv_refuse(DH_EINVAL);
    if (!gemm1x1_split_eligible(b)) return conv_refuse(DH_EUNSUPPORTED);
    return conv_route_tiled(b, DH_CONV_SPLIT, cfg, conv_split_parts(b.w_split), epi);
  }
  if (cfg >= kNumF32Cfgs) {              // interior tiles: epilogue straight from the accumulators
    if (!dma) return conv_refuse(DH_EUNSUPPORTED);
    return conv_route_tiled(a, DH_CONV_DMA, cfg - kNumF32Cfgs, 0, epi_with_direct(a, epi));
  }
  return conv_route_tiled(a, DH_CONV_GENERAL, cfg, 0, epi);
}

}  // namespace dh
