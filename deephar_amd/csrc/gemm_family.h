// Launch-side arithmetic of the LDS-DMA GEMM family, stated once: the K-step, the dynamic LDS of the fp32 form (gemm1x1.hip,
// convt2x2.hip) and of the split-bf16 form (gemm1x1s_launch.h, gemm1x1s_ext_launch.h, convt2x2s.hip), and the tilings of
// the split-bf16 convolution kernels.
#pragma once
#include <algorithm>

#include "conv_common.h"

namespace dh {

constexpr int BK = 32;   // k values per K-step (the wide split tiling walks 16)

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

// ---- the tilings of the split-bf16 convolution kernels: dh_conv2d_f32's tile_cfg -> per-wave tile and LDS stages ----------
template <int WM_, int WN_, int TM_, int TN_, int NS_ = 2>
struct SplitTile {
  static constexpr bool kWide = false;
  static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_, NS = NS_;
};
template <int WM_>
struct SplitWideTile {                   // gemm1x1s_wide_kernel: WM waves of 32 x 192, 16-k K-steps
  static constexpr bool kWide = true;
  static constexpr int WM = WM_;
};
constexpr int kNumSplitCfgs = 16;

// f(tile type{}) for the tiling `cfg`, DH_EINVAL for a cfg that is none.  Every tiling of a mode gives the same bits.
template <typename F>
int dispatch_split_tile(int cfg, F&& f) {
  switch (cfg) {
    case 0: return f(SplitTile<2, 2, 2, 3>{});
    case 1: return f(SplitTile<2, 2, 2, 2>{});
    case 2: return f(SplitTile<4, 1, 1, 3>{});
    case 3: return f(SplitTile<4, 1, 1, 2>{});
    case 4: return f(SplitTile<4, 1, 1, 1>{});
    case 5: return f(SplitTile<2, 1, 1, 3>{});
    case 6: return f(SplitTile<2, 1, 1, 2>{});
    case 7: return f(SplitTile<2, 1, 1, 1>{});
    case 8: return f(SplitTile<1, 1, 1, 1>{});
    // one work-group per CU, three LDS stages: two K-steps of DMA in flight, bigger tiles = less L2 -> LDS traffic per MAC
    case 9: return f(SplitTile<8, 1, 1, 3, 3>{});       // 256 x 96, 8 waves
    case 10: return f(SplitTile<4, 1, 1, 3, 3>{});      // 128 x 96, 4 waves
    case 11: return f(SplitTile<8, 1, 1, 2, 3>{});      // 256 x 64
    case 12: return f(SplitTile<4, 2, 1, 3, 2>{});      // 128 x 192, 8 waves, two stages
    case 13: return f(SplitTile<4, 2, 2, 3, 2>{});      // 256 x 192, 8 waves of 64 x 96
    case 14: return f(SplitWideTile<4>{});              // 128 x 192, 4 waves of 32 x 192, 16-k K-steps
    case 15: return f(SplitWideTile<2>{});              // 64 x 192
  }
  return DH_EINVAL;
}

}  // namespace dh
