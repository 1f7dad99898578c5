// The clip boundary's index arithmetic as pure functions: which float of the rank-major gather buffer [G, m, Tl, P, Cp] a
// float of a dense cut tensor [m, T = G * Tl, P, c] comes from, when a segment may move 16 bytes at a time, and the parser
// of the 'DHCL' container (deephar_amd/engine/serialize.py).  No HIP header, no stream, no pointer dereferenced except the
// blob's own bytes.  The unpack kernel (clip.hip), the host loop dh_unpack_cut_host and tools/clip_sweep.cpp all use
// these, so a test asks the library instead of restating it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <initializer_list>
#include "deephar_hip.h"

#if defined(__HIPCC__)
#define DH_CUT_HD __host__ __device__
#else
#define DH_CUT_HD
#endif

namespace dh {

struct CutGeom { int G, m, Tl; int64_t P; int Cp; };

// A chunk (g, n) holds Tl * P pixel rows that are consecutive on BOTH sides; r = t * P + p counts them.
DH_CUT_HD inline int64_t cut_chunk_rows(const CutGeom& q) { return (int64_t)q.Tl * q.P; }
// source: float index of channel ch of row r of chunk (g, n) in gathered [G, m, Tl, P, Cp]
DH_CUT_HD inline int64_t cut_src_index(const CutGeom& q, int g, int n, int64_t r, int ch) {
  return (((int64_t)g * q.m + n) * cut_chunk_rows(q) + r) * q.Cp + ch;
}
// destination: pixel row of the same float in a dense [m, T, P, .] tensor: frame g * Tl + t of clip n
DH_CUT_HD inline int64_t cut_dst_row(const CutGeom& q, int g, int n, int64_t r) {
  return ((int64_t)n * q.G + g) * cut_chunk_rows(q) + r;
}

// a segment the unpack may touch: channels inside the packed axis, a pitch that holds them
DH_CUT_HD inline bool cut_seg_ok(int Cp, int coff, int c, int ld) {
  return c >= 1 && coff >= 0 && coff <= Cp - c && ld >= c;
}
// the 16-byte predicate of one segment: every row of both sides starts on a 16-byte boundary and holds whole float4s
DH_CUT_HD inline bool cut_vec4(int Cp, int coff, int c, int ld, uintptr_t src, uintptr_t dst) {
  return ((Cp | coff | c | ld) & 3) == 0 && ((src | dst) & 15) == 0;
}

constexpr int64_t kCutMaxFloats = (int64_t)1 << 40;      // bound on G * m * Tl * P * Cp: no product below can overflow

// DH_OK when the geometry is usable; every factor is bounded before it is multiplied
inline int cut_geom_check(int G, int m, int Tl, int64_t P, int Cp) {
  if (G < 1 || m < 1 || Tl < 1 || P < 1 || Cp < 1 || P > kCutMaxFloats) return DH_EINVAL;
  int64_t room = kCutMaxFloats;
  for (int64_t f : {(int64_t)G, (int64_t)m, (int64_t)Tl, P, (int64_t)Cp}) {
    room /= f;
    if (room == 0) return DH_EINVAL;
  }
  return DH_OK;
}

// ---- 'DHCL' container ------------------------------------------------------------------------------------------------
constexpr uint32_t kClipVersion = 1, kClipMaxTable = 4096;
constexpr size_t kClipHeader = 4 + 4 * 5 + 8 + 4 * 2 + 8 * 4;      // bytes in front of the cut table

struct ClipBlob {
  dh_clip_info info;
  const unsigned char* cut;        // num_cut x (u32 channel offset, u32 channels)
  const unsigned char* outputs;    // num_outputs x (u32 kind, u32 index)
};

inline uint32_t clip_u32(const unsigned char* p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t clip_u64(const unsigned char* p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline uint64_t clip_align(uint64_t v) { return (v + 255) & ~(uint64_t)255; }

// Parses and bounds-checks only: nothing is allocated, no byte outside [blob, blob + bytes) is read.
inline int clip_parse(const void* blob, size_t bytes, ClipBlob* out) {
  if (blob == nullptr || out == nullptr || bytes < kClipHeader) return DH_EINVAL;
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  if (memcmp(b, "DHCL", 4) != 0 || clip_u32(b + 4) != kClipVersion) return DH_EINVAL;
  const uint32_t world = clip_u32(b + 8), T = clip_u32(b + 12), Tl = clip_u32(b + 16), Cp = clip_u32(b + 20);
  const uint64_t P = clip_u64(b + 24);
  const uint32_t ncut = clip_u32(b + 32), nout = clip_u32(b + 36);
  const uint64_t foff = clip_u64(b + 40), fbytes = clip_u64(b + 48), hoff = clip_u64(b + 56), hbytes = clip_u64(b + 64);
  const uint32_t lim = 1u << 24;
  if (world < 1 || world > lim || T < 1 || T > lim || Tl < 1 || Tl > T || T % world != 0 || T / world != Tl) return DH_EINVAL;
  if (Cp < 1 || Cp > lim || P < 1 || P > (uint64_t)kCutMaxFloats) return DH_EINVAL;
  if (ncut < 1 || ncut > kClipMaxTable || nout < 1 || nout > kClipMaxTable) return DH_EINVAL;
  const uint64_t tables = kClipHeader + 8ull * ncut + 8ull * nout;
  if (tables > bytes) return DH_EINVAL;
  // the two plan blobs: 256-byte aligned, back to back, and the container ends where the head plan ends
  if (foff != clip_align(tables) || fbytes < 44 || fbytes > bytes || foff > bytes - fbytes) return DH_EINVAL;
  if (hoff != clip_align(foff + fbytes) || hbytes > bytes || hoff > bytes || hoff + hbytes != bytes) return DH_EINVAL;
  if (hbytes != 0 && hbytes < 44) return DH_EINVAL;
  if (memcmp(b + foff, "DHPL", 4) != 0 || (hbytes != 0 && memcmp(b + hoff, "DHPL", 4) != 0)) return DH_EINVAL;
  const unsigned char* cut = b + kClipHeader;
  const unsigned char* outs = cut + 8ull * ncut;
  for (uint32_t i = 0; i < ncut; ++i) {
    const uint32_t off = clip_u32(cut + 8 * i), c = clip_u32(cut + 8 * i + 4);
    if (c < 1 || c > Cp || off > Cp - c) return DH_EINVAL;
  }
  uint32_t nhead = 0;
  for (uint32_t k = 0; k < nout; ++k) nhead += clip_u32(outs + 8 * k) == 1;
  if ((nhead != 0) != (hbytes != 0)) return DH_EINVAL;         // a head plan exactly when an output comes from it
  for (uint32_t k = 0; k < nout; ++k) {
    const uint32_t kind = clip_u32(outs + 8 * k), idx = clip_u32(outs + 8 * k + 4);
    if (kind > 1 || idx >= (kind == 0 ? ncut : nhead)) return DH_EINVAL;
  }
  dh_clip_info& o = out->info;
  o.version = (int32_t)kClipVersion; o.world = (int32_t)world; o.T = (int32_t)T; o.Tl = (int32_t)Tl;
  o.packed_channels = (int32_t)Cp; o.num_cut = (int32_t)ncut; o.num_outputs = (int32_t)nout; o.num_head_outputs = (int32_t)nhead;
  o.P = (int64_t)P; o.frames_offset = foff; o.frames_bytes = fbytes; o.head_offset = hoff; o.head_bytes = hbytes;
  out->cut = cut;
  out->outputs = outs;
  return DH_OK;
}

// The host form of the unpack launch: the same two index functions, one float at a time.
inline int unpack_cut_host(const float* gathered, int G, int m, int Tl, int64_t P, int Cp, const dh_cut_seg* segs, int nseg) {
  if (gathered == nullptr || nseg < 0 || (nseg > 0 && segs == nullptr) || cut_geom_check(G, m, Tl, P, Cp) != DH_OK) return DH_EINVAL;
  for (int s = 0; s < nseg; ++s)
    if (segs[s].dst == nullptr || !cut_seg_ok(Cp, segs[s].coff, segs[s].c, segs[s].ld)) return DH_EINVAL;
  const CutGeom q = {G, m, Tl, P, Cp};
  const int64_t rows = cut_chunk_rows(q);
  for (int s = 0; s < nseg; ++s)
    for (int g = 0; g < G; ++g)
      for (int n = 0; n < m; ++n)
        for (int64_t r = 0; r < rows; ++r) {
          float* d = segs[s].dst + cut_dst_row(q, g, n, r) * segs[s].ld;
          for (int j = 0; j < segs[s].c; ++j) d[j] = gathered[cut_src_index(q, g, n, r, segs[s].coff + j)];
        }
  return DH_OK;
}

}  // namespace dh
