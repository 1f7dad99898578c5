// The arithmetic of the crop-and-resize front end (dh_crop_resize_u8, crop.hip) as pure functions: the fixed-point resampling
// coefficients of one axis (PIL's 8-bit bilinear resize restated: Image.crop(box).resize(size, BILINEAR), which is what the
// reference's loaders run per frame -- deephar/data/mpii.py:114-115, pennaction.py:157-158), the tap bound, the clipping of a
// crop window against its image, and the layout of a CROP PROGRAM: one contiguous table a builder writes and a launch reads.
// No HIP header, no stream.  The kernels, the host twin dh_crop_resize_host, tools/crop_sweep.cpp and the host tests use these.
//
// The doubles below run on the host (crop_program_build) AND on the device (dh_crop_program_build_dev: one lane per output
// index calls crop_axis_output), and both must give the same bits.  Every operation is one IEEE double operation -- in / out,
// 1 / fs, the centre, the triangle weights summed in ascending j, w / ww, 0.5 + v * 2^22 -- so the only hazard is CONTRACTION
// of a product and the addition it feeds into one fused multiply-add:
//   clang (hipcc, host and device passes): `#pragma clang fp contract(off)` in every function that holds such a pair.  On
//     gfx950 the only v_fma_f64 left are those of the division expansions, which are the correctly rounded quotient (the
//     build has no fast-math flag, and must not get one: an approximate fp64 division would change coefficients).
//   other host compilers: the two products that feed an addition go through a volatile.  Not on the device, where a volatile
//     local costs scratch memory.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "deephar_hip.h"

#if defined(__HIPCC__)
#define DH_CROP_HD __host__ __device__
#else
#define DH_CROP_HD
#endif

namespace dh {

constexpr int kCropPrecisionBits = 22;            // coefficients are fixed point with 22 fractional bits: 32 - 8 - 2
constexpr int kCropMaxScale = 16;                 // per-axis down-scaling the launch is built for (any up-scaling is)
constexpr int kCropMaxTaps = 2 * kCropMaxScale + 1;
constexpr int kCropThreads = 256;
constexpr int kCropLdsBytes = 64 * 1024;          // the horizontally resampled rows of one band, uint8
constexpr int kCropMaxBand = 16;                  // output rows a work-group resamples from one fill of its LDS
constexpr int kCropGroupRows = 8;                 // the grid has ceil(OH / 8) work-groups per job; each walks its job's bands
constexpr uint32_t kCropMagic = 0x50524344u;      // "DCRP"
constexpr int kCropMaxExtent = 1 << 20;           // image / window / output extents: offsets stay far inside 32 bits per row

#if defined(__HIP_DEVICE_COMPILE__)
#define DH_CROP_NOFUSE
#else
#define DH_CROP_NOFUSE volatile
#endif
#if defined(__clang__)
#define DH_CROP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define DH_CROP_NO_CONTRACT
#endif

// ---- one axis --------------------------------------------------------------------------------------------------------------
// taps an output of this axis can have: PIL's ksize = (int)ceil(support) * 2 + 1 with support = max(in / out, 1)
DH_CROP_HD inline int crop_axis_taps(int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  int c = (int)support;
  if ((double)c < support) ++c;
  return 2 * c + 1;
}
// scale <= 16 without a division: in <= 16 * out
DH_CROP_HD inline bool crop_axis_supported(int in, int out) { return (int64_t)in <= (int64_t)kCropMaxScale * out; }

// what every output of an axis shares: scale = in / out, support = max(scale, 1), ss = 1 / support
struct CropAxis {
  double scale, support, ss;
};
DH_CROP_HD inline CropAxis crop_axis_setup(int in, int out) {
  CropAxis a;
  a.scale = (double)in / (double)out;
  a.support = a.scale < 1.0 ? 1.0 : a.scale;
  a.ss = 1.0 / a.support;
  return a;
}
// the triangle weight of input x for an output centred at c: the same double every time it is asked
DH_CROP_HD inline double crop_axis_weight(int x, double c, double ss) {
  DH_CROP_NO_CONTRACT
  DH_CROP_NOFUSE double p = ((double)x - c + 0.5) * ss;
  double a = p;
  if (a < 0.0) a = -a;
  return a < 1.0 ? 1.0 - a : 0.0;
}
// ONE output index i of an axis: first[i], count[i], k[i * taps + j] -- output i reads input first[i] + j with weight
// k / 2^22 for j < count[i]; the slots behind count[i] are 0.  `taps` >= crop_axis_taps(in, out).  Host and device: the
// device builder runs one lane per i.  No scratch array, any tap count.
DH_CROP_HD inline void crop_axis_output(const CropAxis& ax, int in, int taps, int i, int32_t* first, int32_t* count, int32_t* k) {
  DH_CROP_NO_CONTRACT
  DH_CROP_NOFUSE double center = ((double)i + 0.5) * ax.scale;
  const double c = center;
  int xmin = (int)(c - ax.support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(c + ax.support + 0.5);
  if (xmax > in) xmax = in;
  int n = xmax - xmin;
  if (n > taps) n = taps;                         // never with taps >= crop_axis_taps
  double ww = 0.0;
  for (int j = 0; j < n; ++j) ww += crop_axis_weight(j + xmin, c, ax.ss);
  first[i] = xmin;
  count[i] = n;
  int32_t* row = k + (size_t)i * taps;
  for (int j = 0; j < n; ++j) {
    const double w = crop_axis_weight(j + xmin, c, ax.ss);
    const double v = ww != 0.0 ? w / ww : w;
    row[j] = (int32_t)(0.5 + v * (double)(1 << kCropPrecisionBits));     // (v * 2^22 is exact: fused or not, the same double)
  }
  for (int j = n; j < taps; ++j) row[j] = 0;
}
// the whole axis on the host: the loop over crop_axis_output
inline void crop_axis_coeffs(int in, int out, int taps, int32_t* first, int32_t* count, int32_t* k) {
  const CropAxis ax = crop_axis_setup(in, out);
  for (int i = 0; i < out; ++i) crop_axis_output(ax, in, taps, i, first, count, k);
}

// ---- the arithmetic both passes share --------------------------------------------------------------------------------------
// acc already holds the rounding constant 2^21.  Bilinear weights are never negative, so acc >= 2^21 and clip_0_255 only has an
// upper side; the shift and the minimum are UNSIGNED on purpose: for the signed shift-and-clamp of two neighbouring
// accumulators hipcc (ROCm 7.2, gfx950) selects v_ashr_pk_u8_i32 and ORs the next byte into its result, and on the device bits
// 16 - 23 of that result were not zero -- byte 2 of every dword of a 16-byte run came out wrong (tests/test_gpu_crop.py caught it).
DH_CROP_HD inline int crop_round(int32_t acc) {
  const uint32_t v = (uint32_t)acc >> kCropPrecisionBits;
  return (int)(v > 255u ? 255u : v);
}
constexpr int32_t kCropHalf = 1 << (kCropPrecisionBits - 1);
// crop clipping: window coordinate c of a window starting at `origin` -> is that pixel inside an image axis of n pixels
DH_CROP_HD inline bool crop_inside(int origin, int c, int n) {
  const int v = origin + c;
  return v >= 0 && v < n;
}
// The horizontal pass for one output pixel: the three channels of sum_j k[j] * S[row][x0 + first + j], zero outside the image.
// `row` is the source row (NULL: the row lies outside the image), W its pixels.
DH_CROP_HD inline void crop_hpixel(const uint8_t* row, int W, int x0, int first, int n, const int32_t* k, int out[3]) {
  int32_t a0 = kCropHalf, a1 = kCropHalf, a2 = kCropHalf;
  if (row != nullptr) {
    for (int j = 0; j < n; ++j) {
      if (!crop_inside(x0, first + j, W)) continue;
      const uint8_t* p = row + (size_t)(x0 + first + j) * 3;
      const int32_t kv = k[j];
      a0 += kv * p[0];
      a1 += kv * p[1];
      a2 += kv * p[2];
    }
  }
  out[0] = crop_round(a0);
  out[1] = crop_round(a1);
  out[2] = crop_round(a2);
}
// bytes between the rows of a band in LDS: a 16-byte multiple, so the vertical pass reads 16 bytes per lane
DH_CROP_HD inline int crop_lds_pitch(int OW) { return (3 * OW + 15) & ~15; }
// the 16-byte store predicate: every output row of every item starts on a 16-byte boundary and holds whole 16-byte runs
DH_CROP_HD inline bool crop_vec16(int OW, uintptr_t y, int64_t item_pitch) {
  return (3 * OW) % 16 == 0 && (y & 15) == 0 && (item_pitch & 15) == 0;
}

// ---- the crop program --------------------------------------------------------------------------------------------------------
//   CropHeader | dh_crop_src[nsrc] | CropJobRec[njobs] | per job: the x table, then the y table
//   axis table: int32 first[out] | int32 count[out] | int32 k[out * taps]
// Every offset is in bytes from the start of the program and a multiple of 8; the program itself is 8-byte aligned.
struct CropHeader {
  uint32_t magic;
  int32_t nsrc, njobs, OH, OW;
  uint32_t src_off, job_off, bytes;
};
struct CropJobRec {
  int32_t src, x0, y0, x1, y1, hflip;
  int32_t xtaps, ytaps;              // row length of the k tables
  int32_t band;                      // output rows per fill of LDS, chosen so that the rows they read fit kCropLdsBytes
  uint32_t xtab, ytab;
  int32_t reserved;
};
static_assert(sizeof(CropHeader) == 32 && sizeof(CropJobRec) == 48 && sizeof(dh_crop_src) == 24 && sizeof(dh_crop_job) == 24,
              "crop program layout");

DH_CROP_HD inline bool crop_job_ok(const dh_crop_job& j, int nsrc) {
  return j.src >= 0 && j.src < nsrc && j.x1 > j.x0 && j.y1 > j.y0 && j.x0 > -kCropMaxExtent && j.y0 > -kCropMaxExtent &&
         j.x1 < kCropMaxExtent && j.y1 < kCropMaxExtent && (int64_t)j.x1 - j.x0 <= kCropMaxExtent &&
         (int64_t)j.y1 - j.y0 <= kCropMaxExtent;
}
DH_CROP_HD inline bool crop_src_ok(const dh_crop_src& s) {
  return s.ptr != nullptr && s.H >= 1 && s.W >= 1 && s.H <= kCropMaxExtent && s.W <= kCropMaxExtent && s.pitch >= (int64_t)3 * s.W;
}
DH_CROP_HD inline size_t crop_axis_table_bytes(int out, int taps) { return ((size_t)out * (2 + (size_t)taps) * 4 + 7) & ~(size_t)7; }
// an odd `out` leaves 4 bytes between the table's last int32 and its 8-byte end: both builders write 0 there, so a program is
// the same bytes whoever built it and whatever its buffer held
DH_CROP_HD inline bool crop_axis_table_pad(int out, int taps) { return (((size_t)out * (2 + (size_t)taps)) & 1) != 0; }
// What a caller allocates before the boxes are known: header + source table + job records + per job both axis tables at
// kCropMaxTaps.  >= crop_program_bytes of every table crop_program_bytes accepts.  0: a bad argument.
DH_CROP_HD inline size_t crop_program_max_bytes(int njobs, int nsrc, int OH, int OW) {
  if (njobs < 1 || nsrc < 1 || OH < 1 || OW < 1 || OH > kCropMaxExtent || OW > kCropMaxExtent) return 0;
  return sizeof(CropHeader) + (size_t)nsrc * sizeof(dh_crop_src) +
         (size_t)njobs * (sizeof(CropJobRec) + crop_axis_table_bytes(OW, kCropMaxTaps) + crop_axis_table_bytes(OH, kCropMaxTaps));
}

// rows of the intermediate a band [r0, r1) of output rows reads
DH_CROP_HD inline int crop_band_rows(const int32_t* yfirst, const int32_t* ycount, int r0, int r1) {
  return yfirst[r1 - 1] + ycount[r1 - 1] - yfirst[r0];
}
// the largest band (a power of two <= kCropMaxBand) all of whose fills fit LDS; 0: not even single rows do
DH_CROP_HD inline int crop_pick_band(const int32_t* yfirst, const int32_t* ycount, int OH, int OW) {
  const int pitch = crop_lds_pitch(OW);
  for (int band = kCropMaxBand; band >= 1; band >>= 1) {
    bool fits = true;
    for (int r0 = 0; r0 < OH && fits; r0 += band) {
      const int r1 = r0 + band < OH ? r0 + band : OH;
      fits = (int64_t)crop_band_rows(yfirst, ycount, r0, r1) * pitch <= kCropLdsBytes;
    }
    if (fits) return band;
  }
  return 0;
}

// DH_OK and *bytes; DH_EINVAL for a bad table, DH_EUNSUPPORTED for a window beyond the scale cap
inline int crop_program_bytes(const dh_crop_job* jobs, int njobs, int nsrc, int OH, int OW, size_t* bytes) {
  if (jobs == nullptr || bytes == nullptr || njobs < 1 || nsrc < 1 || OH < 1 || OW < 1 || OH > kCropMaxExtent || OW > kCropMaxExtent)
    return DH_EINVAL;
  size_t n = sizeof(CropHeader) + (size_t)nsrc * sizeof(dh_crop_src) + (size_t)njobs * sizeof(CropJobRec);
  for (int j = 0; j < njobs; ++j) {
    if (!crop_job_ok(jobs[j], nsrc)) return DH_EINVAL;
    const int cw = jobs[j].x1 - jobs[j].x0, ch = jobs[j].y1 - jobs[j].y0;
    if (!crop_axis_supported(cw, OW) || !crop_axis_supported(ch, OH)) return DH_EUNSUPPORTED;
    n += crop_axis_table_bytes(OW, crop_axis_taps(cw, OW)) + crop_axis_table_bytes(OH, crop_axis_taps(ch, OH));
  }
  if (n > 0x7fffffffu) return DH_EUNSUPPORTED;
  *bytes = n;
  return DH_OK;
}

// Writes the program into `out` (`bytes` as crop_program_bytes answered, 8-byte aligned).  Nothing is written on a refusal.
inline int crop_program_build(const dh_crop_src* srcs, int nsrc, const dh_crop_job* jobs, int njobs, int OH, int OW, void* out,
                              size_t bytes) {
  if (srcs == nullptr || out == nullptr || ((uintptr_t)out & 7) != 0) return DH_EINVAL;
  size_t need = 0;
  const int rc = crop_program_bytes(jobs, njobs, nsrc, OH, OW, &need);
  if (rc != DH_OK) return rc;
  if (bytes < need) return DH_EINVAL;
  for (int s = 0; s < nsrc; ++s)
    if (!crop_src_ok(srcs[s])) return DH_EINVAL;
  uint8_t* base = static_cast<uint8_t*>(out);
  CropHeader h = {kCropMagic, nsrc, njobs, OH, OW, (uint32_t)sizeof(CropHeader),
                  (uint32_t)(sizeof(CropHeader) + (size_t)nsrc * sizeof(dh_crop_src)), (uint32_t)need};
  for (int j = 0; j < njobs; ++j) {                // the last refusal, before anything is written: one output row reads at most
    const int ch = jobs[j].y1 - jobs[j].y0;        // `taps` rows of the intermediate, and those must fit LDS (very wide outputs)
    if ((int64_t)crop_axis_taps(ch, OH) * crop_lds_pitch(OW) > kCropLdsBytes) return DH_EUNSUPPORTED;
  }
  memcpy(base, &h, sizeof(h));
  memcpy(base + h.src_off, srcs, (size_t)nsrc * sizeof(dh_crop_src));
  size_t off = h.job_off + (size_t)njobs * sizeof(CropJobRec);
  for (int j = 0; j < njobs; ++j) {
    const dh_crop_job& g = jobs[j];
    const int cw = g.x1 - g.x0, ch = g.y1 - g.y0;
    CropJobRec r = {g.src, g.x0, g.y0, g.x1, g.y1, g.hflip ? 1 : 0, crop_axis_taps(cw, OW), crop_axis_taps(ch, OH), 0, 0, 0, 0};
    r.xtab = (uint32_t)off;
    int32_t* xt = reinterpret_cast<int32_t*>(base + off);
    crop_axis_coeffs(cw, OW, r.xtaps, xt, xt + OW, xt + 2 * (size_t)OW);
    if (crop_axis_table_pad(OW, r.xtaps)) xt[(size_t)OW * (2 + (size_t)r.xtaps)] = 0;
    off += crop_axis_table_bytes(OW, r.xtaps);
    r.ytab = (uint32_t)off;
    int32_t* yt = reinterpret_cast<int32_t*>(base + off);
    crop_axis_coeffs(ch, OH, r.ytaps, yt, yt + OH, yt + 2 * (size_t)OH);
    if (crop_axis_table_pad(OH, r.ytaps)) yt[(size_t)OH * (2 + (size_t)r.ytaps)] = 0;
    off += crop_axis_table_bytes(OH, r.ytaps);
    r.band = crop_pick_band(yt, yt + OH, OH, OW);  // >= 1: a single row reads at most ytaps rows, checked above
    memcpy(base + h.job_off + (size_t)j * sizeof(CropJobRec), &r, sizeof(r));
  }
  return DH_OK;
}

// The views of a job a reader needs, bounds-checked against the program (host side: the twin and the tests)
struct CropJobView {
  CropJobRec rec;
  dh_crop_src src;
  const int32_t *xfirst, *xcount, *xk, *yfirst, *ycount, *yk;
};

// A program a reader may walk: header, table extents, every index a pass will form.  Host only (it dereferences the program).
inline int crop_program_check(const void* program, size_t bytes, int njobs, int OH, int OW) {
  if (program == nullptr || ((uintptr_t)program & 7) != 0 || bytes < sizeof(CropHeader) || njobs < 1 || OH < 1 || OW < 1)
    return DH_EINVAL;
  const uint8_t* base = static_cast<const uint8_t*>(program);
  CropHeader h;
  memcpy(&h, base, sizeof(h));
  if (h.magic != kCropMagic || h.bytes > bytes || h.OH != OH || h.OW != OW || h.nsrc < 1 || h.njobs < njobs) return DH_EINVAL;
  if (h.src_off != sizeof(CropHeader) || h.job_off != h.src_off + (uint64_t)h.nsrc * sizeof(dh_crop_src) ||
      h.job_off + (uint64_t)h.njobs * sizeof(CropJobRec) > h.bytes)
    return DH_EINVAL;
  for (int s = 0; s < h.nsrc; ++s) {
    dh_crop_src sr;
    memcpy(&sr, base + h.src_off + (size_t)s * sizeof(sr), sizeof(sr));
    if (!crop_src_ok(sr)) return DH_EINVAL;
  }
  for (int j = 0; j < njobs; ++j) {
    CropJobRec r;
    memcpy(&r, base + h.job_off + (size_t)j * sizeof(r), sizeof(r));
    const dh_crop_job g = {r.src, r.x0, r.y0, r.x1, r.y1, r.hflip};
    if (!crop_job_ok(g, h.nsrc)) return DH_EINVAL;
    const int cw = r.x1 - r.x0, ch = r.y1 - r.y0;
    if (!crop_axis_supported(cw, OW) || !crop_axis_supported(ch, OH)) return DH_EUNSUPPORTED;
    if (r.xtaps < 1 || r.xtaps > kCropMaxTaps || r.ytaps < 1 || r.ytaps > kCropMaxTaps || r.band < 1 || r.band > kCropMaxBand)
      return DH_EINVAL;
    if ((r.xtab & 7) || (r.ytab & 7) || (uint64_t)r.xtab + crop_axis_table_bytes(OW, r.xtaps) > h.bytes ||
        (uint64_t)r.ytab + crop_axis_table_bytes(OH, r.ytaps) > h.bytes || r.xtab < h.job_off || r.ytab < h.job_off)
      return DH_EINVAL;
    const int32_t* xt = reinterpret_cast<const int32_t*>(base + r.xtab);
    const int32_t* yt = reinterpret_cast<const int32_t*>(base + r.ytab);
    for (int i = 0; i < OW; ++i)
      if (xt[i] < 0 || xt[OW + i] < 0 || xt[OW + i] > r.xtaps || xt[i] + xt[OW + i] > cw) return DH_EINVAL;
    for (int i = 0; i < OH; ++i)
      if (yt[i] < 0 || yt[OH + i] < 0 || yt[OH + i] > r.ytaps || yt[i] + yt[OH + i] > ch) return DH_EINVAL;
  }
  return DH_OK;
}

inline CropJobView crop_job_view(const void* program, int j, int OH, int OW) {
  const uint8_t* base = static_cast<const uint8_t*>(program);
  CropHeader h;
  memcpy(&h, base, sizeof(h));
  CropJobView v;
  memcpy(&v.rec, base + h.job_off + (size_t)j * sizeof(CropJobRec), sizeof(CropJobRec));
  memcpy(&v.src, base + h.src_off + (size_t)v.rec.src * sizeof(dh_crop_src), sizeof(dh_crop_src));
  v.xfirst = reinterpret_cast<const int32_t*>(base + v.rec.xtab);
  v.xcount = v.xfirst + OW;
  v.xk = v.xcount + OW;
  v.yfirst = reinterpret_cast<const int32_t*>(base + v.rec.ytab);
  v.ycount = v.yfirst + OH;
  v.yk = v.ycount + OH;
  return v;
}

// The host form of the launch: the same tables, the same two rounded passes, one output byte at a time (the horizontal pass
// is recomputed per vertical tap: nothing is allocated).  Nothing is written on a refusal.
inline int crop_resize_host(const void* program, size_t bytes, int njobs, int OH, int OW, uint8_t* y, int64_t item_pitch) {
  if (y == nullptr || OH < 1 || OW < 1 || item_pitch < (int64_t)OH * OW * 3) return DH_EINVAL;
  const int rc = crop_program_check(program, bytes, njobs, OH, OW);
  if (rc != DH_OK) return rc;
  for (int j = 0; j < njobs; ++j) {
    const CropJobView v = crop_job_view(program, j, OH, OW);
    uint8_t* dst = y + (size_t)j * item_pitch;
    for (int oy = 0; oy < OH; ++oy)
      for (int ox = 0; ox < OW; ++ox) {
        int32_t acc[3] = {kCropHalf, kCropHalf, kCropHalf};
        for (int t = 0; t < v.ycount[oy]; ++t) {
          const int cy = v.yfirst[oy] + t;
          const uint8_t* row = crop_inside(v.rec.y0, cy, v.src.H) ? v.src.ptr + (size_t)(v.rec.y0 + cy) * v.src.pitch : nullptr;
          int hp[3];
          crop_hpixel(row, v.src.W, v.rec.x0, v.xfirst[ox], v.xcount[ox], v.xk + (size_t)ox * v.rec.xtaps, hp);
          const int32_t kv = v.yk[(size_t)oy * v.rec.ytaps + t];
          for (int c = 0; c < 3; ++c) acc[c] += kv * hp[c];
        }
        const int dx = v.rec.hflip ? OW - 1 - ox : ox;
        for (int c = 0; c < 3; ++c) dst[((size_t)oy * OW + dx) * 3 + c] = (uint8_t)crop_round(acc[c]);
      }
  }
  return DH_OK;
}

}  // namespace dh
