// The arithmetic of the per-frame person-box pass (dh_pose_boxes_f64, posebox.hip) as pure functions: one box in image pixels
// around the confident joints of an ITEM -- F poses (F = 1 for an image model, F = T for a clip model) of J joints and D channels
// predicted in one unflipped integer crop window.  It restates get_bbox_from_poses(poses, afmat, scale) of
// deephar_amd/evaltools/bbox.py (exp/common/generic.py:7-27 in the reference) in closed form: get_valid_bbox_array per frame in
// float32 (the pose array is float32 and numpy keeps it so), the union over the frames, and the corners back to image pixels
// through the item's own window in double instead of through np.linalg.inv of the affine map.  No HIP header, no stream.  The
// kernel, the host twin, tools/posebox_sweep.cpp and the host tests use these.
//
// Like refine_index.h, the arithmetic runs on the host AND on the device and both must give the same bits: every operation
// below is one IEEE float or double operation, and contraction is switched off (DH_CROP_NO_CONTRACT for clang on both passes, a
// volatile product for other host compilers).  What could still differ between the two sides is pinned here:
//   NaN   : x86 and gfx950 do not produce the same NaN bits from the same invalid operation, and a conversion of a double that
//           int32 does not hold is undefined.  Neither is ever stored or reached: every such case leaves through the item's
//           STATUS word, and a non-zero status writes both boxes as four zeros.
//   +-0   : the float min / max of the kept joints may be either zero when zeros of both signs occur, depending on the order of
//           the reduction.  Follow the zero through the sums.  If only the min (or only the max) is such a zero, the other
//           end is not zero, and xmin + xmax and xmax - xmin are the same floats for both signs.  If both ends are zeros, the
//           centre (xmin + xmax) / 2 and the side relsize * (xmax - xmin) are zeros whose signs do depend on the order, and so
//           may a corner cx -+ s / 2 be when the larger side is a zero too -- and with it the union's min / max over the
//           frames.  But a float corner u leaves only as x0 + (double)u * (x1 - x0): the zero is multiplied by the window's
//           positive extent, which keeps it a zero, and ADDED to the window's origin, an int32 converted to double and so
//           never -0; that sum is the same double for both signs (x0 itself, or +0 when x0 == 0 under round-to-nearest).  So
//           neither the order of the lanes nor the order of the frames can move a bit of either box.
// Status precedence is order-free as well: 1 if ANY frame keeps no joint, else 2 if ANY kept joint has a NaN coordinate, else 4
// for the window, else 3 for the corners.
#pragma once
#include <stdint.h>
#include <string.h>
#include "crop_index.h"

namespace dh {

constexpr int kPoseBoxWave = 64;                  // lanes over the joints of one frame
constexpr int kPoseBoxWaves = 4;                  // items (wavefronts) per work-group
constexpr float kPoseBoxConfThr = 0.25f;          // generic.py:11: a joint is kept when its confidence is > 0.25
constexpr int64_t kPoseBoxMaxStride = (int64_t)1 << 40;
constexpr int64_t kPoseBoxMaxSpan = (int64_t)1 << 58;   // (n - 1) * item_stride floats, (n - 1) * job_stride jobs

enum PoseBoxStatus : int32_t {
  kPoseBoxOk = 0,
  kPoseBoxNoJoint = 1,                            // a frame keeps no joint: get_valid_bbox raises 'all points are invalid!'
  kPoseBoxNan = 2,                                // a kept joint has a NaN coordinate
  kPoseBoxRange = 3,                              // a corner is not finite or of magnitude >= 2^31
  kPoseBoxWindow = 4,                             // the window is empty or flipped
};

DH_CROP_HD inline float posebox_inf() {
  const uint32_t bits = 0x7f800000u;
  float v;
  memcpy(&v, &bits, 4);
  return v;
}
DH_CROP_HD inline float posebox_min(float a, float b) { return b < a ? b : a; }
DH_CROP_HD inline float posebox_max(float a, float b) { return b > a ? b : a; }
DH_CROP_HD inline bool posebox_finite(float c) { return c < posebox_inf() && c > -posebox_inf(); }   // (false for a NaN)
// a pixel corner truncates toward zero into int32: finite and of magnitude below 2^31
DH_CROP_HD inline bool posebox_corner_ok(double c) { return c < 2147483648.0 && c > -2147483648.0; }

// the extent of the KEPT joints of one frame (or of one lane's share of them): min / max of both coordinates (float
// comparisons are exact), whether any joint was kept, whether a kept joint had a NaN coordinate
struct PoseSpan {
  float ulo, uhi, vlo, vhi;
  int kept, nan;
};
DH_CROP_HD inline PoseSpan posebox_span_none() {
  const PoseSpan e = {posebox_inf(), -posebox_inf(), posebox_inf(), -posebox_inf(), 0, 0};
  return e;
}
DH_CROP_HD inline void posebox_span_add(PoseSpan& e, float u, float v, float conf) {
  if (!(conf > kPoseBoxConfThr)) return;           // a float32 comparison; a NaN confidence keeps nothing
  e.kept = 1;
  if (u != u || v != v) {
    e.nan = 1;
    return;
  }
  e.ulo = posebox_min(e.ulo, u);
  e.uhi = posebox_max(e.uhi, u);
  e.vlo = posebox_min(e.vlo, v);
  e.vhi = posebox_max(e.vhi, v);
}
// joints j0, j0 + step, ... of one frame: channels 0, 1 and conf_channel of every joint, joint_stride floats apart
DH_CROP_HD inline PoseSpan posebox_span(const float* pose, int64_t joint_stride, int J, int conf_channel, int j0, int step) {
  PoseSpan e = posebox_span_none();
  for (int j = j0; j < J; j += step) {
    const float* p = pose + (int64_t)j * joint_stride;
    posebox_span_add(e, p[0], p[1], p[conf_channel]);
  }
  return e;
}

// the running union over the frames of an item: the float32 corners of get_valid_bbox_array's boxes, min / max per column
struct PoseUnion {
  float u0, v0, u1, v1;
  int nojoint, nan, wild;                          // a frame kept nothing / had a NaN joint / gave a corner that is not finite
};
DH_CROP_HD inline PoseUnion posebox_union_none() {
  const PoseUnion a = {posebox_inf(), posebox_inf(), -posebox_inf(), -posebox_inf(), 0, 0, 0};
  return a;
}
// get_valid_bbox(square=True) of one frame in float32, folded into the union.  `relsize` is the caller's double rounded once.
DH_CROP_HD inline void posebox_union_add(PoseUnion& a, const PoseSpan& e, float relsize) {
  DH_CROP_NO_CONTRACT
  if (!e.kept) {
    a.nojoint = 1;
    return;
  }
  if (e.nan) {
    a.nan = 1;
    return;
  }
  const float cx = (e.ulo + e.uhi) / 2.0f, cy = (e.vlo + e.vhi) / 2.0f;
  const float dx = e.uhi - e.ulo, dy = e.vhi - e.vlo;
  DH_CROP_NOFUSE float w = relsize * dx;
  DH_CROP_NOFUSE float h = relsize * dy;
  const float wv = w, hv = h;
  const float s = hv > wv ? hv : wv;               // Python's max(w, h)
  const float half = s / 2.0f;
  const float c0 = cx - half, c1 = cy - half, c2 = cx + half, c3 = cy + half;
  if (!(posebox_finite(c0) && posebox_finite(c1) && posebox_finite(c2) && posebox_finite(c3))) {
    a.wild = 1;                                    // (an infinite coordinate: the pixel corner would not be finite either)
    return;
  }
  a.u0 = posebox_min(a.u0, c0);
  a.v0 = posebox_min(a.v0, c1);
  a.u1 = posebox_max(a.u1, c2);
  a.v1 = posebox_max(a.v1, c3);
}

// The union's corners to image pixels through the item's window, the two corners ordered, each truncated toward zero.
// Returns the status; a non-zero status leaves both boxes zero.
DH_CROP_HD inline int32_t posebox_finish(const dh_crop_job& g, const PoseUnion& a, int32_t box[4], double boxf[4]) {
  DH_CROP_NO_CONTRACT
  box[0] = box[1] = box[2] = box[3] = 0;
  boxf[0] = boxf[1] = boxf[2] = boxf[3] = 0.0;
  if (a.nojoint) return kPoseBoxNoJoint;
  if (a.nan) return kPoseBoxNan;
  if (g.hflip != 0 || !(g.x1 > g.x0 && g.y1 > g.y0)) return kPoseBoxWindow;
  if (a.wild) return kPoseBoxRange;
  const double x0 = (double)g.x0, y0 = (double)g.y0;
  const double cw = (double)g.x1 - x0, ch = (double)g.y1 - y0;
  DH_CROP_NOFUSE double pax = (double)a.u0 * cw;
  DH_CROP_NOFUSE double pay = (double)a.v0 * ch;
  DH_CROP_NOFUSE double pbx = (double)a.u1 * cw;
  DH_CROP_NOFUSE double pby = (double)a.v1 * ch;
  const double ax = x0 + pax, ay = y0 + pay, bx = x0 + pbx, by = y0 + pby;
  const double lx = bx < ax ? bx : ax, ly = by < ay ? by : ay;
  const double hx = bx > ax ? bx : ax, hy = by > ay ? by : ay;
  if (!(posebox_corner_ok(lx) && posebox_corner_ok(ly) && posebox_corner_ok(hx) && posebox_corner_ok(hy))) return kPoseBoxRange;
  boxf[0] = lx; boxf[1] = ly; boxf[2] = hx; boxf[3] = hy;
  box[0] = (int32_t)lx; box[1] = (int32_t)ly; box[2] = (int32_t)hx; box[3] = (int32_t)hy;
  return kPoseBoxOk;
}

// ---- argument checks the launch and the host twin share ---------------------------------------------------------------------
// strides are in floats: a joint spans its channels 0, 1 and conf_channel, a frame its J joints, an item its F frames; a job
// stride is in jobs.  Every stride lies in [its extent, 2^40] and the span of all n items in [0, 2^58] elements, so neither a
// product here nor i * item_stride / i * job_stride in the kernel and the twin, nor its byte offset, can leave int64.
inline int pose_boxes_args(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                           int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, const int32_t* boxes_out,
                           const double* boxes_f64_out, const int32_t* status_out) {
  if (poses == nullptr || jobs == nullptr || boxes_out == nullptr || boxes_f64_out == nullptr || status_out == nullptr || n < 1 ||
      F < 1 || J < 1 || conf_channel < 0)
    return DH_EINVAL;
  const int64_t ext = conf_channel < 2 ? 2 : (int64_t)conf_channel + 1;       // floats one joint spans
  if (joint_stride < ext || joint_stride > kPoseBoxMaxStride || frame_stride < ext || frame_stride > kPoseBoxMaxStride ||
      item_stride < ext || item_stride > kPoseBoxMaxStride || job_stride < 1 || job_stride > kPoseBoxMaxStride)
    return DH_EINVAL;
  if ((int64_t)(J - 1) > (frame_stride - ext) / joint_stride) return DH_EINVAL;          // frame_stride < (J - 1) joint_stride + ext
  const int64_t frame_ext = (int64_t)(J - 1) * joint_stride + ext;                        // <= frame_stride
  if (item_stride < frame_ext) return DH_EINVAL;                                          // (before the division: F = 1 too)
  if ((int64_t)(F - 1) > (item_stride - frame_ext) / frame_stride) return DH_EINVAL;      // item_stride < (F - 1) frame_stride + ...
  if ((int64_t)(n - 1) > kPoseBoxMaxSpan / item_stride || (int64_t)(n - 1) > kPoseBoxMaxSpan / job_stride) return DH_EINVAL;
  return DH_OK;
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------
inline void pose_boxes_item(const float* item, int64_t frame_stride, int64_t joint_stride, int F, int J, int conf_channel,
                            const dh_crop_job& g, float relsize, int32_t box[4], double boxf[4], int32_t* status) {
  PoseUnion a = posebox_union_none();
  for (int f = 0; f < F; ++f)
    posebox_union_add(a, posebox_span(item + (int64_t)f * frame_stride, joint_stride, J, conf_channel, 0, 1), relsize);
  *status = posebox_finish(g, a, box, boxf);
}
inline int pose_boxes_host(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                           int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, double relsize, int32_t* boxes_out,
                           double* boxes_f64_out, int32_t* status_out) {
  const int rc = pose_boxes_args(poses, item_stride, frame_stride, joint_stride, F, J, conf_channel, jobs, job_stride, n, boxes_out,
                                 boxes_f64_out, status_out);
  if (rc != DH_OK) return rc;
  const float rs = (float)relsize;
  for (int64_t i = 0; i < n; ++i)
    pose_boxes_item(poses + i * item_stride, frame_stride, joint_stride, F, J, conf_channel, jobs[i * job_stride], rs,
                    boxes_out + 4 * i, boxes_f64_out + 4 * i, status_out + i);
  return DH_OK;
}

// dh_frame_boxes_shape: what dh_frame_boxes_host asks of a plan before anything is enqueued.  A clip plan (more than one frame
// per item), a float input, a batch too small, an output out of range or with fewer than the two channels the pass reads.
inline int frame_boxes_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW, int num_outputs,
                             int outidx, int64_t out_items, int out_channels, int* J) {
  if (num_inputs != 1 || input_is_u8 != 1 || batch < 1 || n < 1 || n > batch || OH < 1 || OW < 1 || OH > kCropMaxExtent ||
      OW > kCropMaxExtent)
    return DH_EINVAL;
  if (input_items != (int64_t)OH * OW * 3) return DH_EINVAL;             // one image per item: no clip plans
  if (outidx < 0 || outidx >= num_outputs || out_channels < 2 || out_items < out_channels || out_items % out_channels != 0 ||
      out_items / out_channels > 0x7fffffff)
    return DH_EINVAL;
  if (J != nullptr) *J = (int)(out_items / out_channels);
  return DH_OK;
}

}  // namespace dh
