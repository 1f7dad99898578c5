// The arithmetic of the box-refinement loop (dh_refine_boxes_f64, refine.hip) as pure functions: the integer window of a float
// box -- crop_box(*bbox_to_objposwin(b)) of deephar_amd/frontend.py, what the loaders crop (deephar/data/mpii.py:102-115) --
// and one pose -> box step of the MPII evaluation's refinement (exp/common/mpii_tools.py:13-52 in the reference) in closed
// form: the crop-normalised joints go back to image pixels through the job's own window instead of through an inverted affine
// map.  No HIP header, no stream.  The kernels, the host twins, tools/refine_sweep.cpp and the host tests use these.
//
// Like crop_index.h, the doubles run on the host AND on the device and both must give the same bits: every operation below is
// one IEEE double operation, and contraction of a product with the addition it feeds is switched off (DH_CROP_NO_CONTRACT for
// clang on both passes, a volatile product for other host compilers).  Two more things could differ between the two sides and
// are therefore pinned here:
//   NaN   : x86 and gfx950 do not produce the same NaN bits from the same invalid operation, so every NaN leaves as ONE quiet
//           NaN (refine_canon).  A NaN joint coordinate makes the whole box that NaN.
//   +-0   : the float min / max of the joints may be either zero when both signs occur, depending on the order of the
//           reduction; the zero is multiplied by the window's extent and ADDED to the window's origin, a sum that is the same
//           double for both signs, so the order of the reduction cannot move a bit of the result.
#pragma once
#include <stdint.h>
#include <string.h>
#include "crop_index.h"

namespace dh {

constexpr int kRefineWave = 64;                   // lanes over the joints of one sample
constexpr int kRefineWaves = 4;                   // samples (wavefronts) per work-group

DH_CROP_HD inline double refine_nan() {
  const uint64_t bits = 0x7ff8000000000000ull;
  double v;
  memcpy(&v, &bits, 8);
  return v;
}
DH_CROP_HD inline double refine_canon(double v) { return v != v ? refine_nan() : v; }
DH_CROP_HD inline float refine_inf() {
  const uint32_t bits = 0x7f800000u;
  float v;
  memcpy(&v, &bits, 4);
  return v;
}

DH_CROP_HD inline dh_crop_job refine_empty_job(int32_t src) {
  const dh_crop_job g = {src, 0, 0, 0, 0, 0};
  return g;
}
DH_CROP_HD inline bool refine_job_empty(const dh_crop_job& g) { return !(g.x1 > g.x0 && g.y1 > g.y0); }
// a corner truncates toward zero into int32: finite and of magnitude below 2^31
DH_CROP_HD inline bool refine_corner_ok(double c) { return c < 2147483648.0 && c > -2147483648.0; }

// The window of a float box: centre and size as bbox_to_objposwin takes them, the corners as crop_box truncates them.  A
// corner that is not finite or does not fit makes the job the empty job, which the program builders refuse with DH_EINVAL.
DH_CROP_HD inline dh_crop_job refine_window(const double b[4], int32_t src) {
  const double cx = (b[0] + b[2]) / 2, cy = (b[1] + b[3]) / 2;
  const double w = b[2] - b[0], h = b[3] - b[1];
  const double c0 = cx - w / 2, c1 = cy - h / 2, c2 = cx + w / 2, c3 = cy + h / 2;
  if (!(refine_corner_ok(c0) && refine_corner_ok(c1) && refine_corner_ok(c2) && refine_corner_ok(c3))) return refine_empty_job(src);
  const dh_crop_job g = {src, (int32_t)c0, (int32_t)c1, (int32_t)c2, (int32_t)c3, 0};
  return g;
}

// the extent of a pose: min / max of both coordinates (float comparisons are exact) and whether any coordinate was NaN
struct RefineExtent {
  float ulo, uhi, vlo, vhi;
  int nan;
};
DH_CROP_HD inline RefineExtent refine_extent_none() {
  const RefineExtent e = {refine_inf(), -refine_inf(), refine_inf(), -refine_inf(), 0};
  return e;
}
DH_CROP_HD inline float refine_min(float a, float b) { return b < a ? b : a; }
DH_CROP_HD inline float refine_max(float a, float b) { return b > a ? b : a; }
DH_CROP_HD inline void refine_extent_add(RefineExtent& e, float u, float v) {
  if (u != u || v != v) {
    e.nan = 1;
    return;
  }
  e.ulo = refine_min(e.ulo, u);
  e.uhi = refine_max(e.uhi, u);
  e.vlo = refine_min(e.vlo, v);
  e.vhi = refine_max(e.vhi, v);
}
// joints j0, j0 + step, ... of one pose: channels 0 and 1 of every joint, joint_stride floats apart
DH_CROP_HD inline RefineExtent refine_extent(const float* pose, int64_t joint_stride, int J, int j0, int step) {
  RefineExtent e = refine_extent_none();
  for (int j = j0; j < J; j += step) refine_extent_add(e, pose[(int64_t)j * joint_stride], pose[(int64_t)j * joint_stride + 1]);
  return e;
}

// One refinement step of one sample.  `bout` may be `bin`, `jout` may point at `jin`.
DH_CROP_HD inline void refine_step(const dh_crop_job& jin, const double bin[4], const RefineExtent& e, double winsize_scale,
                                   double momentum, double bout[4], dh_crop_job* jout) {
  DH_CROP_NO_CONTRACT
  const dh_crop_job g = jin;
  const double b0 = bin[0], b1 = bin[1], b2 = bin[2], b3 = bin[3];
  if (g.hflip != 0 || refine_job_empty(g)) {     // the loop crops unflipped, and an empty window has no pose: the box passes
    bout[0] = b0; bout[1] = b1; bout[2] = b2; bout[3] = b3;
    *jout = refine_empty_job(g.src);
    return;
  }
  if (e.nan) {
    bout[0] = bout[1] = bout[2] = bout[3] = refine_nan();
    *jout = refine_empty_job(g.src);
    return;
  }
  const double x0 = (double)g.x0, y0 = (double)g.y0;
  const double cw = (double)g.x1 - x0, ch = (double)g.y1 - y0;
  DH_CROP_NOFUSE double plx = (double)e.ulo * cw;
  DH_CROP_NOFUSE double phx = (double)e.uhi * cw;
  DH_CROP_NOFUSE double ply = (double)e.vlo * ch;
  DH_CROP_NOFUSE double phy = (double)e.vhi * ch;
  const double lx = x0 + plx, hx = x0 + phx, ly = y0 + ply, hy = y0 + phy;
  const double px = (lx + hx) / 2, py = (ly + hy) / 2;
  const double dx = hx - lx, dy = hy - ly;
  const double side = winsize_scale * (dx < dy ? dy : dx);
  const double tx = (b0 + b2) / 2, ty = (b1 + b3) / 2;
  const double keep = 1 - momentum;
  DH_CROP_NOFUSE double mtx = momentum * tx;
  DH_CROP_NOFUSE double mpx = keep * px;
  DH_CROP_NOFUSE double mty = momentum * ty;
  DH_CROP_NOFUSE double mpy = keep * py;
  const double ox = mtx + mpx, oy = mty + mpy;
  const double half = side / 2;
  double nb[4] = {refine_canon(ox - half), refine_canon(oy - half), refine_canon(ox + half), refine_canon(oy + half)};
  *jout = refine_window(nb, g.src);
  bout[0] = nb[0]; bout[1] = nb[1]; bout[2] = nb[2]; bout[3] = nb[3];
}

// ---- argument checks both launches and both host twins share -----------------------------------------------------------------
inline int refine_jobs_args(const double* boxes, const int32_t* src, int n, const dh_crop_job* jobs) {
  return (boxes == nullptr || src == nullptr || jobs == nullptr || n < 1) ? DH_EINVAL : DH_OK;
}
// strides are in floats: a joint spans its channels 0 and 1, a sample its J joints
inline int refine_boxes_args(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                             const double* boxes_in, int n, const double* boxes_out, const dh_crop_job* jobs_out) {
  if (poses == nullptr || jobs_in == nullptr || boxes_in == nullptr || boxes_out == nullptr || jobs_out == nullptr || n < 1 || J < 1)
    return DH_EINVAL;
  if (joint_stride < 2 || joint_stride > ((int64_t)1 << 40) || sample_stride > ((int64_t)1 << 40) ||
      sample_stride < (int64_t)(J - 1) * joint_stride + 2)
    return DH_EINVAL;
  return DH_OK;
}

// ---- the host twins ------------------------------------------------------------------------------------------------------------
inline int jobs_from_boxes_host(const double* boxes, const int32_t* src, int n, dh_crop_job* jobs) {
  const int rc = refine_jobs_args(boxes, src, n, jobs);
  if (rc != DH_OK) return rc;
  for (int i = 0; i < n; ++i) jobs[i] = refine_window(boxes + (size_t)4 * i, src[i]);
  return DH_OK;
}
inline int refine_boxes_host(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                             const double* boxes_in, int n, double winsize_scale, double momentum, double* boxes_out,
                             dh_crop_job* jobs_out) {
  const int rc = refine_boxes_args(poses, sample_stride, joint_stride, J, jobs_in, boxes_in, n, boxes_out, jobs_out);
  if (rc != DH_OK) return rc;
  for (int i = 0; i < n; ++i) {
    const RefineExtent e = refine_extent(poses + (int64_t)i * sample_stride, joint_stride, J, 0, 1);
    refine_step(jobs_in[i], boxes_in + (size_t)4 * i, e, winsize_scale, momentum, boxes_out + (size_t)4 * i, jobs_out + i);
  }
  return DH_OK;
}

// dh_refine_frames_shape: what dh_refine_frames_host asks of a plan before anything is enqueued.  A clip plan (more than one
// frame per item), a float input, a batch too small, an output out of range or with fewer than the two channels the step reads.
inline int refine_frames_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW,
                               int num_outputs, int outidx, int64_t out_items, int out_channels, int num_iter, int* J) {
  if (num_inputs != 1 || input_is_u8 != 1 || batch < 1 || n < 1 || n > batch || OH < 1 || OW < 1 || OH > kCropMaxExtent ||
      OW > kCropMaxExtent || num_iter < 1)
    return DH_EINVAL;
  if (input_items != (int64_t)OH * OW * 3) return DH_EINVAL;             // one image per item: no clip plans
  if (outidx < 0 || outidx >= num_outputs || out_channels < 2 || out_items < out_channels || out_items % out_channels != 0 ||
      out_items / out_channels > 0x7fffffff)
    return DH_EINVAL;
  if (J != nullptr) *J = (int)(out_items / out_channels);
  return DH_OK;
}

}  // namespace dh
