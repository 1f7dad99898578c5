// Launch-side arithmetic of the MFMA GEMM families, stated once: the tilings dh_conv2d_f32's tile_cfg names and what each of
// them has a kernel for, and the dynamic LDS of the fp32 form (gemm1x1.hip, convt2x2.hip) and of the split-bf16 form
// (gemm1x1s_launch.h, gemm1x1s_ext_launch.h, convt2x2s.hip) of the LDS-DMA GEMM.  No HIP header: conv_route.h reads the
// table at run time, the launch templates read it in their `if constexpr` guards.
#pragma once
#include <algorithm>
#include <utility>

#include "conv_rules.h"

namespace dh {

// `launch`: dynamic LDS bytes of a launch; `limit`: what hipFuncAttributeMaxDynamicSharedMemorySize is raised to once per
// kernel and device, so it cannot depend on the layer (LdsLimit).
struct GemmLds { size_t launch, limit; };

constexpr int gemm_epi_floats(int WM, int WN, int TN) { return WM * WN * 32 * (TN * 32 + 4); }   // one 32-row slab per wave
constexpr GemmLds gemm_lds(int stage, int epi, bool PRE, int Kp, bool limit_adds_tables) {
  const size_t lds = (size_t)(stage > epi ? stage : epi) * sizeof(float);
  // PRE: the scale | shift tables sit behind the operand stages (the epilogue slab, when larger, only starts after the K loop)
  const size_t launch = PRE ? std::max(lds, (size_t)(stage + 2 * Kp) * sizeof(float)) : lds;
  const size_t limit = !PRE ? lds
                       : limit_adds_tables ? lds + 2 * kMaxPreKp * sizeof(float)
                                           : std::max(lds, (size_t)(stage + 2 * kMaxPreKp) * sizeof(float));
  return {launch, limit};
}
// The two forms differ in the limit of a kernel with a BN prologue, and are kept as they are: the fp32 launchers raise it to
// (stages or slab) + the largest tables, the split ones to max(stages or slab, stages + the largest tables).
constexpr GemmLds gemm_f32_lds(int WM, int WN, int TM, int TN, bool PRE, int Kp) {     // two stages of A [BM][BK] | B [BK][BN]
  return gemm_lds(2 * (WM * TM * 32 * BK + BK * WN * TN * 32), gemm_epi_floats(WM, WN, TN), PRE, Kp, true);
}
constexpr GemmLds gemm_split_lds(int P, int WM, int WN, int TM, int TN, int NS, bool PRE, int Kp) {   // B: 4 k-groups x P parts x BN units
  return gemm_lds(NS * (WM * TM * 32 * BK + 4 * P * WN * TN * 32 * 4), gemm_epi_floats(WM, WN, TN), PRE, Kp, false);
}
constexpr size_t kMaxLds = 160 * 1024;

// ---- the tilings: work-group = wm x wn waves, a wave owns tm x tn MFMA tiles of 32 x 32; ns LDS stages (split kernels) -----
struct GemmTile {
  int wm, wn, tm, tn, ns;
  bool wide;        // gemm1x1s_wide_kernel: wm waves of 32 x 192 (two halves of three column tiles), 16-k K-steps
  constexpr int bm() const { return wm * tm * 32; }
  constexpr int bn() const { return wn * tn * 32; }
};
// Rows 0..8 are the tilings of the two fp32 kernels (tile_cfg 0..8: general implicit GEMM, 9..17: LDS-DMA GEMM) and of the
// split-bf16 kernels; 9..15 exist in the split-bf16 kernels only.  Every tiling of a kernel and mode gives the same bits.
constexpr GemmTile kGemmTiles[] = {
    {2, 2, 2, 3, 2},  //  0: 128 x 192
    {2, 2, 2, 2, 2},  //  1: 128 x 128
    {4, 1, 1, 3, 2},  //  2: 128 x  96
    {4, 1, 1, 2, 2},  //  3: 128 x  64
    {4, 1, 1, 1, 2},  //  4: 128 x  32
    {2, 1, 1, 3, 2},  //  5:  64 x  96
    {2, 1, 1, 2, 2},  //  6:  64 x  64
    {2, 1, 1, 1, 2},  //  7:  64 x  32
    {1, 1, 1, 1, 2},  //  8:  32 x  32
    // one work-group per CU, three LDS stages: two K-steps of DMA in flight, bigger tiles = less L2 -> LDS traffic per MAC
    {8, 1, 1, 3, 3},  //  9: 256 x  96, 8 waves
    {4, 1, 1, 3, 3},  // 10: 128 x  96, 4 waves
    {8, 1, 1, 2, 3},  // 11: 256 x  64
    {4, 2, 1, 3, 2},  // 12: 128 x 192, 8 waves, two stages
    {4, 2, 2, 3, 2},  // 13: 256 x 192, 8 waves of 64 x 96
    {4, 1, 1, 6, 2, true},  // 14: 128 x 192, 4 waves of 32 x 192, 16-k K-steps
    {2, 1, 1, 6, 2, true},  // 15:  64 x 192
};
constexpr int kNumF32Cfgs = 9;
constexpr int kNumSplitCfgs = sizeof(kGemmTiles) / sizeof(kGemmTiles[0]);
constexpr int kNumConvCfgs = 2 * kNumF32Cfgs;     // dh_conv2d_num_tile_cfgs()

// What a tiling has a kernel for.
// The epilogue can also write the 2x2 max-pooled output (dh_conv_args.y_pool) in waves pairs: every wave owns ONE 32-row
// block = one image row at OW == 32, and the waves come in (even, odd) pairs over M.
constexpr bool tile_pools_in_pairs(int WM, int TM, bool UP2 = false) { return TM == 1 && WM % 2 == 0 && !UP2; }
// [r06] OW == 16 / OW == 8: a wave's 32-row block is two / four WHOLE image rows (OH * OW a multiple of 32, so a block
// never straddles frames and starts at an even row) -- the wave pools its own slab, no partner needed: any TM == 1 tiling.
constexpr bool tile_pools_in_wave(int TM, bool UP2 = false) { return TM == 1 && !UP2; }
constexpr bool tile_pools_for(const GemmTile& t, int OW) { return OW == 32 ? tile_pools_in_pairs(t.wm, t.tm) : tile_pools_in_wave(t.tm); }
// The fp32 LDS-DMA GEMM finishes its direct tiles column tile by column tile under the last K-step's MFMAs (gemm1x1_body.h):
// a wave with ONE row block holds TN independent accumulator tiles and has the registers for two residual slices.  The
// compile-time switch: a kernel taken out here keeps the whole-tile direct epilogue -- every tiling gives the same bits.
// Taken out: the forms whose K loop carries the most state at the narrow tilings (BN prologue below three column tiles, the
// K x K form of the one-wave tiling), where the peeled step would cost a wave per SIMD of occupancy
// (profiles/epilogue_slices.md).
constexpr bool tile_epi_sliced(const GemmTile& t, bool PRE = false, bool KXK = false) {
  return t.tm == 1 && !(PRE && t.tn < 3) && !(KXK && t.wm == 1 && t.tn == 1);
}
// the fused up-sampling epilogue: six 32 x 32 accumulators per wave would spill beside it (the wide tiling holds them in halves)
constexpr bool tile_has_up2(const GemmTile& t) { return t.wide || t.tm * t.tn < 6; }
// the wide tiling: with fewer than three parts its fixed half-tile choreography has nothing left to hide the operand traffic
// under, and it is not built for the extended scope
constexpr bool tile_has_parts(const GemmTile& t, int P, bool ext) { return !t.wide || (P == 3 && !ext); }
// extended scope: the BN prologue exists on the pipelined loop (per-wave tiles of 32 rows) only ...
constexpr bool tile_has_ext_prologue(const GemmTile& t) { return t.tm == 1; }
// ... and three stages of the 256-row tiles leave no room for the largest tables
constexpr bool tile_ext_fits(const GemmTile& t, int P, bool PRE) {
  return gemm_split_lds(P, t.wm, t.wn, t.tm, t.tn, t.ns, PRE, 0).limit <= kMaxLds;
}

// f(std::integral_constant<int, cfg>{}) for cfg in [0, N): kGemmTiles[cfg] is a constant expression inside f.  DH_EINVAL
// for a cfg that is no tiling.
template <int... I, typename F>
int dispatch_tile_seq(int cfg, std::integer_sequence<int, I...>, F&& f) {
  int rc = DH_EINVAL;
  (void)((cfg == I && (rc = f(std::integral_constant<int, I>{}), true)) || ...);
  return rc;
}
template <int N, typename F>
int dispatch_tile(int cfg, F&& f) {
  return dispatch_tile_seq(cfg, std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

}  // namespace dh
