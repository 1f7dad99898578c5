// dh_pose_boxes_f64: the pose -> box step of the per-frame person-box pass (evaltools.bbox.get_bbox_from_poses) for every item
// of a chunk, in ONE small launch that reads the poses where the forward left them (a strided view of the plan's arena) and
// the item's window from the resident crop job table -- so only 16 + 32 + 4 bytes per item ever have to leave the device.
//   grid ceil(n / 4), 256 threads: one wavefront per item, lanes over the joints (a loop when J > 64), an outer loop over the
//   item's F frames.  Lane l reads channels 0, 1 and conf_channel of joints l, l + 64, ...: neighbouring lanes read neighbouring
//   joints.  Per frame the four float min / max values go across the wave through __shfl_xor butterflies and the "kept any" /
//   "NaN" flags through __any: no LDS, no scratch, no atomics.  Min and max are exact, so the order of the reduction cannot
//   move a bit (posebox_index.h on the one case where it picks another zero).  After the butterfly every lane holds the frame's
//   span, and every lane folds it into its copy of the running union (posebox_union_add, float32, contraction off): uniform
//   work, no broadcast.  After the last frame lane 0 runs posebox_finish -- the host twin's doubles -- and stores the int32
//   box, the float64 box and the status: 52 bytes of plain vector stores.
//   A wave touches no other item's rows.
// gfx950 cross-compile (hipcc -O3, --save-temps): pose_boxes_kernel 28 VGPRs, 0 AGPRs, 40 SGPRs, no scratch, no LDS,
// occupancy 8 waves per SIMD.
#include "dh_kernels.h"
#include "posebox_index.h"

namespace {

using namespace dh;

constexpr int kPoseBoxThreads = kPoseBoxWave * kPoseBoxWaves;

__global__ __launch_bounds__(kPoseBoxThreads) void pose_boxes_kernel(const float* __restrict__ poses, int64_t item_stride,
                                                                     int64_t frame_stride, int64_t joint_stride, int F, int J,
                                                                     int conf_channel, const dh_crop_job* __restrict__ jobs,
                                                                     int64_t job_stride, int n, float relsize,
                                                                     int32_t* __restrict__ boxes_out, double* __restrict__ boxes_f64_out,
                                                                     int32_t* __restrict__ status_out) {
  const int lane = threadIdx.x & (kPoseBoxWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kPoseBoxWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                                   // (uniform in the wave)
  const float* item = poses + i * item_stride;
  PoseUnion a = posebox_union_none();
  for (int f = 0; f < F; ++f) {
    PoseSpan e = posebox_span(item + (int64_t)f * frame_stride, joint_stride, J, conf_channel, lane, kPoseBoxWave);
#pragma unroll
    for (int d = kPoseBoxWave / 2; d > 0; d >>= 1) {
      e.ulo = posebox_min(e.ulo, __shfl_xor(e.ulo, d));
      e.uhi = posebox_max(e.uhi, __shfl_xor(e.uhi, d));
      e.vlo = posebox_min(e.vlo, __shfl_xor(e.vlo, d));
      e.vhi = posebox_max(e.vhi, __shfl_xor(e.vhi, d));
    }
    e.kept = __any(e.kept) ? 1 : 0;
    e.nan = __any(e.nan) ? 1 : 0;
    posebox_union_add(a, e, relsize);
  }
  if (lane != 0) return;
  const dh_crop_job g = jobs[i * job_stride];
  int32_t box[4];
  double boxf[4];
  const int32_t status = posebox_finish(g, a, box, boxf);
  boxes_out[4 * i] = box[0];
  boxes_out[4 * i + 1] = box[1];
  boxes_out[4 * i + 2] = box[2];
  boxes_out[4 * i + 3] = box[3];
  boxes_f64_out[4 * i] = boxf[0];
  boxes_f64_out[4 * i + 1] = boxf[1];
  boxes_f64_out[4 * i + 2] = boxf[2];
  boxes_f64_out[4 * i + 3] = boxf[3];
  status_out[i] = status;
}

}  // namespace

extern "C" {

int dh_pose_boxes_host(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                       int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, double relsize, int32_t* boxes_out,
                       double* boxes_f64_out, int32_t* status_out) {
  return dh::pose_boxes_host(poses, item_stride, frame_stride, joint_stride, F, J, conf_channel, jobs, job_stride, n, relsize,
                             boxes_out, boxes_f64_out, status_out);
}

int dh_pose_boxes_f64(const float* poses, int64_t item_stride, int64_t frame_stride, int64_t joint_stride, int F, int J,
                      int conf_channel, const dh_crop_job* jobs, int64_t job_stride, int n, double relsize, int32_t* boxes_out,
                      double* boxes_f64_out, int32_t* status_out, void* stream) {
  const int rc = dh::pose_boxes_args(poses, item_stride, frame_stride, joint_stride, F, J, conf_channel, jobs, job_stride, n,
                                     boxes_out, boxes_f64_out, status_out);
  if (rc != DH_OK) return rc;
  if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)jobs & 3) != 0 || ((uintptr_t)boxes_out & 3) != 0 ||
      ((uintptr_t)boxes_f64_out & 7) != 0 || ((uintptr_t)status_out & 3) != 0)
    return DH_EINVAL;
  const unsigned groups = (unsigned)(((int64_t)n + kPoseBoxWaves - 1) / kPoseBoxWaves);
  hipLaunchKernelGGL(pose_boxes_kernel, dim3(groups), dim3(kPoseBoxThreads), 0, reinterpret_cast<hipStream_t>(stream), poses,
                     item_stride, frame_stride, joint_stride, F, J, conf_channel, jobs, job_stride, n, (float)relsize, boxes_out,
                     boxes_f64_out, status_out);
  return dh::check_launch();
}

int dh_frame_boxes_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW, int num_outputs,
                         int outidx, int64_t out_items, int out_channels, int* J) {
  return dh::frame_boxes_shape(num_inputs, input_is_u8, input_items, batch, n, OH, OW, num_outputs, outidx, out_items, out_channels,
                               J);
}

}  // extern "C"
