// Host-only sweep of dh::conv_route (deephar_amd/csrc/conv_route.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc \
//       tools/route_sweep.cpp -o /tmp/route_sweep && /tmp/route_sweep
//
// The grid crosses layer geometries, every w_split, every tile_cfg and operand alignments, and adds extents on both sides of
// the 2^31 limits the rules guard (N*OH*OW, M*ldy*4, K*Cin, N*H*W*ldx*4).  It checks what must hold of every route: an
// accepted one names a family, a tiling that exists and a grid inside (0, 2^31); a refused one is all zero.  Not a pytest
// test: nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "conv_route.h"

using namespace dh;

static long long n_routes = 0, n_ok = 0, per_kernel[8];

static void check(const ConvArgs& a, int cfg) {
  const ConvRoute r = conv_route(a, cfg);
  ++n_routes;
  bool good;
  if (r.rc != DH_OK) {
    good = (r.rc == DH_EINVAL || r.rc == DH_EUNSUPPORTED) && r.kernel == 0 && r.tile_cfg == -1 && r.tiles == 0 && r.bm == 0 && r.epi == 0;
  } else {
    ++n_ok;
    good = r.kernel >= DH_CONV_GENERAL && r.kernel <= DH_CONV_FIRST_LAYER && r.tiles > 0 && r.tiles <= 0x7fffffffu;
    if (good) ++per_kernel[r.kernel];
    const bool tiled = r.kernel <= DH_CONV_SPLIT_EXT;
    if (tiled) good = good && r.tile_cfg >= 0 && r.tile_cfg < (r.kernel <= DH_CONV_DMA ? kNumF32Cfgs : kNumSplitCfgs) &&
                      r.bm == kGemmTiles[r.tile_cfg].bm() && r.bn == kGemmTiles[r.tile_cfg].bn() && !(a.up2 && r.tile_cfg == 0);
    if (r.kernel == DH_CONV_HALO) good = good && r.tile_cfg >= 0 && r.tile_cfg < kNumHaloCfgs && r.bn == 32 * (r.tile_cfg + 1);
    good = good && (r.pool != 0) == (a.y_pool != nullptr) && (r.pool == 0 || (r.epi & 1)) && !((r.epi & 2) && !(r.epi & 1));
    good = good && ((r.parts != 0) == (r.kernel == DH_CONV_SPLIT || r.kernel == DH_CONV_SPLIT_EXT));
  }
  if (!good) {
    std::printf("bad route: rc %d kernel %d cfg %d tiles %u (N %d H %d W %d Cin %d Cout %d K %d w_split %d tile_cfg %d)\n", r.rc, r.kernel,
                r.tile_cfg, r.tiles, a.N, a.H, a.W, a.Cin, a.Cout, a.KH, a.w_split, cfg);
    std::exit(1);
  }
}

static const float* ptr(uintptr_t p) { return reinterpret_cast<const float*>(p); }

// one layer; `mis`: bit k misaligns operand k (x, y, res1, res2, tables, y_pool, w)
static void layer(int N, int H, int W, int Cin, int Cout, int k, int stride, int ldx, int ldy, int flags, int mis) {
  ConvArgs a;
  std::memset(&a, 0, sizeof(a));
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ldx = ldx; a.ldy = ldy;
  a.KH = a.KW = k; a.SH = a.SW = stride;
  a.OH = (H + stride - 1) / stride; a.OW = (W + stride - 1) / stride;
  a.PT = a.PL = (k - 1) / 2;
  const long long K = (long long)k * k * Cin;
  a.K = (int)K; a.Kp = (int)((K + 31) / 32 * 32); a.Np = (Cout + 31) / 32 * 32;
  a.x = ptr(0x1000000 + ((mis & 1) ? 4 : 0));
  a.y = const_cast<float*>(ptr(0x2000000 + ((mis & 2) ? 4 : 0)));
  a.w = ptr(0x3000000 + ((mis & 64) ? 4 : 0));
  if (flags & 1) { a.res1 = ptr(0x4000000 + ((mis & 4) ? 4 : 0)); a.ldr1 = ldy; }
  if (flags & 2) { a.res2 = ptr(0x5000000 + ((mis & 8) ? 4 : 0)); a.ldr2 = ldy; a.res2_down = (flags & 4) && !(a.OH & 1) && !(a.OW & 1); }
  if (flags & 8) { a.post_scale = ptr(0x6000000 + ((mis & 16) ? 4 : 0)); a.post_shift = ptr(0x6100000); }
  if (flags & 16) { a.pre_scale = ptr(0x6200000 + ((mis & 16) ? 4 : 0)); a.pre_shift = ptr(0x6300000); }
  if (flags & 32) { a.y_pool = const_cast<float*>(ptr(0x7000000 + ((mis & 32) ? 4 : 0))); a.ldyp = Cout; }
  if (flags & 64) a.up2 = 1;
  if (flags & 128) { a.x_u8 = 1; a.in_lut = (flags & 256) ? nullptr : ptr(0x8000000); }
  a.pre_relu = (flags >> 9) & 1;
  a.x_resample = (flags >> 10) & 3;
  for (int ws = -1; ws <= 8; ++ws) {
    a.w_split = ws;
    for (int cfg = -2; cfg <= 19; ++cfg) check(a, cfg);
  }
}

int main() {
  static const int shapes[][7] = {   // N, H, W, Cin, Cout, k, stride
      {2, 19, 23, 96, 200, 1, 1}, {2, 19, 23, 100, 200, 1, 1}, {2, 35, 33, 64, 72, 3, 1}, {2, 35, 33, 64, 72, 3, 2}, {2, 13, 11, 64, 72, 3, 1},
      {2, 8, 8, 32, 96, 1, 1}, {2, 16, 16, 32, 96, 1, 1}, {1, 32, 32, 32, 40, 1, 1}, {4, 8, 8, 32, 40, 1, 1}, {1, 32, 32, 48, 72, 3, 1},
      {1, 64, 64, 144, 70, 3, 1}, {1, 128, 128, 48, 96, 5, 1}, {2, 8, 8, 64, 24, 3, 1}, {2, 8, 16, 70, 40, 1, 1}, {1, 16, 256, 3, 32, 3, 2},
      {1, 256, 256, 3, 64, 7, 2}, {1, 1, 1, 1, 1, 1, 1}, {3, 7, 5, 2, 300, 3, 1}, {1, 64, 64, 576, 576, 1, 1}, {2, 32, 32, 4128, 48, 1, 1},
      {1, 4, 4, 4096, 256, 3, 1}, {1, 2, 2, 32768, 16, 1, 1}, {1, 1, 1, 65536, 8, 1, 1},
      // 2^31: N*OH*OW on both sides, M*ldy*4, N*H*W*ldx*4 against 0xf0000000, K*Cin
      {32768, 256, 256, 32, 32, 1, 1}, {32767, 256, 256, 32, 32, 1, 1}, {16384, 256, 256, 32, 32, 1, 1}, {8192, 256, 256, 4, 8, 1, 1},
      {8191, 256, 256, 8, 4, 1, 1}, {2048, 256, 256, 32, 32, 3, 2}, {4096, 128, 128, 16, 64, 1, 1}, {65536, 128, 256, 3, 32, 3, 2},
      {1, 46341, 46341, 4, 4, 1, 1}, {1, 46340, 46340, 4, 4, 1, 1}, {2000000000, 1, 1, 64, 16, 1, 1}, {1, 16, 16, 46341, 8, 1, 1},
  };
  const int flag_sets[] = {0, 1, 3, 7, 8, 9, 16, 17, 16 | 512, 32 | 8 | 1, 32, 64, 64 | 3, 128, 128 | 256, 512, 1024, 2048, 3072, 1024 | 16 | 512};
  const int mis_sets[] = {0, 1, 2, 4, 8, 16, 32, 64, 127};
  for (const auto& s : shapes)
    for (int flags : flag_sets)
      for (int mis : mis_sets)
        for (int pad = 0; pad <= 1; ++pad)
          layer(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[3] + (pad ? 4 + (mis & 1) : 0), s[4] + (pad ? 4 + ((mis >> 1) & 1) : 0), flags, mis);
  std::printf("%lld routes, %lld accepted: general %lld, dma %lld, split %lld, split-ext %lld, halo %lld, skinny %lld, first layer %lld\n", n_routes, n_ok,
              per_kernel[1], per_kernel[2], per_kernel[3], per_kernel[4], per_kernel[5], per_kernel[6], per_kernel[7]);
  return per_kernel[1] && per_kernel[2] && per_kernel[3] && per_kernel[4] && per_kernel[5] && per_kernel[6] && per_kernel[7] ? 0 : 2;
}
