// dh_vote_products_f64: the vote of the multi-clip action evaluation (evaltools.action._multiclip: a_pred[b, i, :] *= pred[b][0],
// then np.argmax) for every item of a chunk, in ONE small launch that reads the action outputs where the forward left them
// (strided views of the plan's arena) -- so no model output has to leave the device; the products, the labels and, if wanted,
// the per-clip scores leave once, at the end of a run.
//   grid nb, 64 threads: one wavefront owns one output b for the whole launch; lanes over the classes (c = lane, lane + 64, ...);
//   a SERIAL loop over the n items, because item k + 1 of a sequence multiplies what item k left.  acc is read and written with
//   plain loads and stores: lane l only ever touches classes l, l + 64, ... of its own output's rows, so it reads back only
//   addresses it wrote itself, in program order.  seq[k] is uniform in the wave.  The arg-max goes across the wave through
//   __shfl_xor butterflies on (value, index) pairs under the TOTAL order of vote_index.h (NaN first, larger value, lower index),
//   so the order of the reduction cannot move the label; after the butterfly every lane holds it and lane 0 stores it.
//   No LDS, no atomics, no scratch.  The sources travel by value in the kernel arguments (at most kVoteMaxSrcs per launch, as
//   dh_out_seg does in dh_pack_outputs_f32; more go out as further launches over disjoint b): nothing is uploaded per call, the
//   launch is capturable.
// gfx950 cross-compile (hipcc -O3, --save-temps): vote_products_kernel 26 VGPRs, 0 AGPRs, 60 SGPRs, no scratch, no LDS,
// occupancy 8 waves per SIMD; one v_mul_f64 and no fused multiply-add in the loop.
#include "dh_kernels.h"
#include "vote_index.h"

namespace {

using namespace dh;

struct VoteArgs {
  dh_vote_src src[kVoteMaxSrcs];
};
static_assert(sizeof(VoteArgs) <= 1024, "the sources must fit the kernel argument segment");

__global__ __launch_bounds__(kVoteWave) void vote_products_kernel(const VoteArgs a, int C, const int32_t* __restrict__ seq, int n,
                                                                  int nseq, double* acc, int32_t* __restrict__ label_out,
                                                                  float* __restrict__ scores_out) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const dh_vote_src g = a.src[b];
  double* accb = acc + b * nseq * C;
  int32_t* label = label_out + b * n;
  for (int64_t k = 0; k < n; ++k) {
    const int32_t s = seq[k];
    if (s < 0 || s >= nseq) {                                           // (uniform in the wave)
      if (lane == 0) label[k] = -1;
      continue;
    }
    float* srow = scores_out != nullptr ? scores_out + (b * n + k) * C : nullptr;
    VoteBest e = vote_item(g.p + k * g.item_stride, accb + (int64_t)s * C, srow, C, lane, kVoteWave);
#pragma unroll
    for (int d = kVoteWave / 2; d > 0; d >>= 1) {
      VoteBest o;
      o.v = __shfl_xor(e.v, d);
      o.i = __shfl_xor(e.i, d);
      e = vote_first(e, o);
    }
    if (lane == 0) label[k] = e.i;
  }
}

}  // namespace

extern "C" {

int dh_vote_products_host(const dh_vote_src* srcs, int nb, int C, const int32_t* seq, int n, int nseq, double* acc,
                          int32_t* label_out, float* scores_out) {
  return dh::vote_products_host(srcs, nb, C, seq, n, nseq, acc, label_out, scores_out);
}

int dh_vote_products_f64(const dh_vote_src* srcs, int nb, int C, const int32_t* seq, int n, int nseq, double* acc,
                         int32_t* label_out, float* scores_out, void* stream) {
  const int rc = dh::vote_args(srcs, nb, C, seq, n, nseq, acc, label_out, scores_out);
  if (rc != DH_OK) return rc;
  VoteArgs a = {};
  for (int64_t b0 = 0; b0 < nb; b0 += kVoteMaxSrcs) {                   // disjoint b per launch: no order between them matters
    const int m = nb - b0 < kVoteMaxSrcs ? (int)(nb - b0) : kVoteMaxSrcs;
    for (int b = 0; b < m; ++b) a.src[b] = srcs[b0 + b];
    hipLaunchKernelGGL(vote_products_kernel, dim3((unsigned)m), dim3(kVoteWave), 0, reinterpret_cast<hipStream_t>(stream), a, C,
                       seq, n, nseq, acc + b0 * nseq * C, label_out + b0 * n,
                       scores_out != nullptr ? scores_out + b0 * n * C : nullptr);
    const int lrc = dh::check_launch();
    if (lrc != DH_OK) return lrc;
  }
  return DH_OK;
}

}  // extern "C"
