// The index arithmetic of the output pack launch (dh_pack_outputs_f32, out_pack.hip) as pure functions: which float of an
// arena view [npix, C] at pixel pitch ld a float of the caller's dense [npix, C] tensor comes from, when a segment may move
// 16 bytes at a time, and how many copy units a segment has.  No HIP header, no stream.  The kernel, the host loop
// dh_pack_outputs_host and the host tests all use these.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "deephar_hip.h"

#if defined(__HIPCC__)
#define DH_OUT_HD __host__ __device__
#else
#define DH_OUT_HD
#endif

namespace dh {

constexpr int kPackMaxSegs = 64;                  // segments per launch: they travel in the kernel arguments
constexpr int kPackGroupUnits = 1024;             // copy units (16-byte runs or floats) per work-group: 256 lanes x 4
constexpr int64_t kPackMaxFloats = (int64_t)1 << 40;

// a segment the pack may touch (dst == NULL is "not wanted": dropped before this is asked)
DH_OUT_HD inline bool out_seg_ok(const dh_out_seg& s) {
  return s.src != nullptr && s.npix >= 1 && s.C >= 1 && s.ld >= s.C && s.npix <= kPackMaxFloats / s.ld;
}
// the 16-byte predicate: every pixel row of both sides starts on a 16-byte boundary and holds whole float4s
DH_OUT_HD inline bool out_vec4(int C, int ld, uintptr_t src, uintptr_t dst) {
  return ((C | ld) & 3) == 0 && ((src | dst) & 15) == 0;
}
// copy units of a segment: float4s on the 16-byte path, floats otherwise
DH_OUT_HD inline int64_t out_units(const dh_out_seg& s, bool vec4) { return s.npix * (vec4 ? s.C / 4 : s.C); }
// unit u of a segment with w units per pixel (w = C / 4 or C) -> its unit index on the source side, pitch lw (ld / 4 or ld)
DH_OUT_HD inline int64_t out_src_unit(int64_t u, int w, int lw) {
  const int64_t p = u / w;
  return p * lw + (u - p * w);
}

// The host form of the launch: the same index function, one float at a time.  NULL destinations are skipped.
inline int pack_outputs_host(const dh_out_seg* segs, int nseg) {
  if (nseg < 0 || (nseg > 0 && segs == nullptr)) return DH_EINVAL;
  for (int s = 0; s < nseg; ++s)
    if (segs[s].dst != nullptr && !out_seg_ok(segs[s])) return DH_EINVAL;
  for (int s = 0; s < nseg; ++s) {
    const dh_out_seg& g = segs[s];
    if (g.dst == nullptr) continue;
    const int64_t n = out_units(g, false);
    for (int64_t u = 0; u < n; ++u) g.dst[u] = g.src[out_src_unit(u, g.C, g.ld)];
  }
  return DH_OK;
}

}  // namespace dh
