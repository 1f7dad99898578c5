// The kernel of the extended split-bf16 scope (gemm1x1s_ext.hip) and its launch side, for P parts per operand.  One translation
// unit per mode instantiates launch_ext_parts<P>: gemm1x1s_ext.hip (P = 3, with the rule and the dispatch), gemm1x1s_ext_p2.hip,
// gemm1x1s_ext_p1.hip.
#pragma once
#include "gemm_family.h"
#include "split_bf16.h"

namespace dh {
namespace {

template <int P, int WM, int WN, int TM, int TN, bool RELU, bool KXK, bool PRE, int NS>
__global__ __launch_bounds__(WM* WN * 64, 2) void gemm1x1s_ext_kernel(const ConvArgs p, const int epi_vec) {
  constexpr bool UP2 = false, D2S = false, K16 = KXK;
  constexpr int cb = 0;
#include "gemm1x1s_body.h"
}

template <int P, int WM, int WN, int TM, int TN, bool RELU, bool KXK, bool PRE, int NS>
int launch_ext_variant(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  if constexpr (!tile_ext_fits(GemmTile{WM, WN, TM, TN, NS}, P, PRE)) {
    return DH_EUNSUPPORTED;
  } else {
    constexpr size_t kMax = gemm_split_lds(P, WM, WN, TM, TN, NS, PRE, 0).limit;
    auto kern = gemm1x1s_ext_kernel<P, WM, WN, TM, TN, RELU, KXK, PRE, NS>;
    if (kMax > 64 * 1024) {
      static LdsLimit lim;
      lim.raise((const void*)kern, (int)kMax);
    }
    hipLaunchKernelGGL(kern, dim3(r.tiles), dim3(WM * WN * 64), gemm_split_lds(P, WM, WN, TM, TN, NS, PRE, a.Kp).launch, s, a, r.epi);
    return check_launch();
  }
}

template <int P, int WM, int WN, int TM, int TN, int NS = 2>
int launch_ext_cfg(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  if constexpr (tile_has_ext_prologue(GemmTile{WM, WN, TM, TN, NS})) {
    if (a.pre_scale != nullptr)        // (a): the BN prologue
      return a.pre_relu ? launch_ext_variant<P, WM, WN, TM, TN, true, false, true, NS>(a, r, s)
                        : launch_ext_variant<P, WM, WN, TM, TN, false, false, true, NS>(a, r, s);
  }
  return a.pre_relu ? launch_ext_variant<P, WM, WN, TM, TN, true, true, false, NS>(a, r, s)
                    : launch_ext_variant<P, WM, WN, TM, TN, false, true, false, NS>(a, r, s);
}

// every tiling of one mode; the wide tiling (14, 15) is not built for these layers
template <int P>
int launch_ext_parts(const ConvArgs& a, const ConvRoute& r, hipStream_t s) {
  return dispatch_tile<kNumSplitCfgs>(r.tile_cfg, [&](auto c) -> int {
    constexpr GemmTile t = kGemmTiles[decltype(c)::value];
    if constexpr (!tile_has_parts(t, P, true)) {
      return DH_EUNSUPPORTED;
    } else {
      return launch_ext_cfg<P, t.wm, t.wn, t.tm, t.tn, t.ns>(a, r, s);
    }
  });
}

}  // namespace
}  // namespace dh
