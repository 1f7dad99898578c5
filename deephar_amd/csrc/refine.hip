// dh_refine_boxes_f64: one pose -> box step of the box-refinement loop for every sample of a chunk, in ONE small launch that
// reads the poses where the forward left them (a strided view of the plan's arena) and writes the next iteration's float
// boxes and crop jobs into device memory -- so the job table dh_crop_program_build_dev reads never visits the host.
//   grid ceil(n / 4), 256 threads: one wavefront per sample, lanes over the joints (a loop when J > 64).  Lane l reads channels 0
//   and 1 of joints l, l + 64, ...: neighbouring lanes read neighbouring joints.  The four float min / max values go across the
//   wave through __shfl_xor butterflies and the NaN flag through __any: no LDS, no scratch, no atomics.  Min and max are exact,
//   so the order of the reduction cannot move a bit (refine_index.h on the one case where it picks another zero).  Lane 0 then
//   runs refine_step -- the host twin's doubles, contraction off -- and stores 32 + 24 bytes.
//   A wave reads its sample's box and job before it writes them, and touches no other sample's: in and out may alias.
// dh_jobs_from_boxes_f64: iteration 0's jobs from the uploaded float boxes, one lane per sample.
#include "dh_kernels.h"
#include "refine_index.h"

namespace {

using namespace dh;

constexpr int kRefineThreads = kRefineWave * kRefineWaves;

__global__ __launch_bounds__(kRefineThreads) void refine_boxes_kernel(const float* __restrict__ poses, int64_t sample_stride,
                                                                      int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                                                                      const double* boxes_in, int n, double winsize_scale,
                                                                      double momentum, double* boxes_out, dh_crop_job* jobs_out) {
  const int lane = threadIdx.x & (kRefineWave - 1);
  const int64_t i = (int64_t)blockIdx.x * kRefineWaves + (threadIdx.x >> 6);
  if (i >= n) return;                                                   // (uniform in the wave)
  RefineExtent e = refine_extent(poses + i * sample_stride, joint_stride, J, lane, kRefineWave);
#pragma unroll
  for (int d = kRefineWave / 2; d > 0; d >>= 1) {
    e.ulo = refine_min(e.ulo, __shfl_xor(e.ulo, d));
    e.uhi = refine_max(e.uhi, __shfl_xor(e.uhi, d));
    e.vlo = refine_min(e.vlo, __shfl_xor(e.vlo, d));
    e.vhi = refine_max(e.vhi, __shfl_xor(e.vhi, d));
  }
  e.nan = __any(e.nan) ? 1 : 0;
  if (lane != 0) return;
  const dh_crop_job g = jobs_in[i];
  const double b[4] = {boxes_in[4 * i], boxes_in[4 * i + 1], boxes_in[4 * i + 2], boxes_in[4 * i + 3]};
  double nb[4];
  dh_crop_job ng;
  refine_step(g, b, e, winsize_scale, momentum, nb, &ng);
  boxes_out[4 * i] = nb[0];
  boxes_out[4 * i + 1] = nb[1];
  boxes_out[4 * i + 2] = nb[2];
  boxes_out[4 * i + 3] = nb[3];
  jobs_out[i] = ng;
}

__global__ __launch_bounds__(kRefineThreads) void jobs_from_boxes_kernel(const double* __restrict__ boxes, const int32_t* __restrict__ src,
                                                                         int n, dh_crop_job* __restrict__ jobs) {
  const int64_t i = (int64_t)blockIdx.x * kRefineThreads + threadIdx.x;
  if (i >= n) return;
  const double b[4] = {boxes[4 * i], boxes[4 * i + 1], boxes[4 * i + 2], boxes[4 * i + 3]};
  jobs[i] = refine_window(b, src[i]);
}

}  // namespace

extern "C" {

int dh_jobs_from_boxes_host(const double* boxes, const int32_t* src, int n, dh_crop_job* jobs) {
  return dh::jobs_from_boxes_host(boxes, src, n, jobs);
}

int dh_jobs_from_boxes_f64(const double* boxes, const int32_t* src, int n, dh_crop_job* jobs, void* stream) {
  const int rc = dh::refine_jobs_args(boxes, src, n, jobs);
  if (rc != DH_OK) return rc;
  if (((uintptr_t)boxes & 7) != 0 || ((uintptr_t)src & 3) != 0 || ((uintptr_t)jobs & 3) != 0) return DH_EINVAL;
  const unsigned groups = (unsigned)(((int64_t)n + kRefineThreads - 1) / kRefineThreads);
  hipLaunchKernelGGL(jobs_from_boxes_kernel, dim3(groups), dim3(kRefineThreads), 0, reinterpret_cast<hipStream_t>(stream), boxes, src,
                     n, jobs);
  return dh::check_launch();
}

int dh_refine_boxes_host(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                         const double* boxes_in, int n, double winsize_scale, double momentum, double* boxes_out,
                         dh_crop_job* jobs_out) {
  return dh::refine_boxes_host(poses, sample_stride, joint_stride, J, jobs_in, boxes_in, n, winsize_scale, momentum, boxes_out,
                               jobs_out);
}

int dh_refine_boxes_f64(const float* poses, int64_t sample_stride, int64_t joint_stride, int J, const dh_crop_job* jobs_in,
                        const double* boxes_in, int n, double winsize_scale, double momentum, double* boxes_out,
                        dh_crop_job* jobs_out, void* stream) {
  const int rc = dh::refine_boxes_args(poses, sample_stride, joint_stride, J, jobs_in, boxes_in, n, boxes_out, jobs_out);
  if (rc != DH_OK) return rc;
  if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)jobs_in & 3) != 0 || ((uintptr_t)jobs_out & 3) != 0 ||
      ((uintptr_t)boxes_in & 7) != 0 || ((uintptr_t)boxes_out & 7) != 0)
    return DH_EINVAL;
  const unsigned groups = (unsigned)(((int64_t)n + kRefineWaves - 1) / kRefineWaves);
  hipLaunchKernelGGL(refine_boxes_kernel, dim3(groups), dim3(kRefineThreads), 0, reinterpret_cast<hipStream_t>(stream), poses,
                     sample_stride, joint_stride, J, jobs_in, boxes_in, n, winsize_scale, momentum, boxes_out, jobs_out);
  return dh::check_launch();
}

int dh_refine_frames_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int n, int OH, int OW,
                           int num_outputs, int outidx, int64_t out_items, int out_channels, int num_iter, int* J) {
  return dh::refine_frames_shape(num_inputs, input_is_u8, input_items, batch, n, OH, OW, num_outputs, outidx, out_items,
                                 out_channels, num_iter, J);
}

}  // extern "C"
