// dh_pack_outputs_f32: every wanted output of a plan from its arena view to the caller's dense tensor in ONE launch (the
// counterpart of dh_unpack_cut_f32 at the other end of a C forward).  The segments travel by value in the kernel arguments
// (at most kPackMaxSegs per launch; more go out as further launches): nothing is uploaded per call, the launch is
// capturable.  The index arithmetic lives in out_index.h, GPU-free, shared with the host loop dh_pack_outputs_host.
#include "dh_kernels.h"
#include "out_index.h"

namespace {

using dh::kPackGroupUnits;
using dh::kPackMaxSegs;

struct PackArgs {
  dh_out_seg seg[kPackMaxSegs];
  uint32_t first[kPackMaxSegs + 1];      // work-groups [first[s], first[s + 1]) belong to segment s
  uint64_t vec;                          // bit s: segment s moves 16 bytes per lane
  int32_t nseg;
};
static_assert(sizeof(PackArgs) <= 4096, "the segments must fit the kernel argument segment");

// Work-groups are dealt to segments by the prefix table over copy units, so a 15-float action score gets one work-group
// and a heat-map slab as many as its float4s need.  One work-group moves kPackGroupUnits consecutive units of one segment:
// consecutive lanes on consecutive destination addresses (one contiguous run on the source side too when ld == C).
__global__ __launch_bounds__(256) void pack_outputs_kernel(const PackArgs a) {
  const uint32_t b = blockIdx.x;
  int lo = 0, hi = a.nseg;               // the segment of this work-group: the last s with first[s] <= b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid; else hi = mid;
  }
  const dh_out_seg g = a.seg[lo];
  const int64_t u0 = (int64_t)(b - a.first[lo]) * kPackGroupUnits + threadIdx.x;
  if ((a.vec >> lo) & 1) {
    const int w = g.C >> 2, lw = g.ld >> 2;
    const int64_t n = g.npix * w;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(g.src);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(g.dst);
#pragma unroll
    for (int k = 0; k < kPackGroupUnits / 256; ++k) {
      const int64_t u = u0 + k * 256;
      if (u < n) d4[u] = s4[dh::out_src_unit(u, w, lw)];
    }
  } else {
    const int64_t n = g.npix * g.C;
#pragma unroll
    for (int k = 0; k < kPackGroupUnits / 256; ++k) {
      const int64_t u = u0 + k * 256;
      if (u < n) g.dst[u] = g.src[dh::out_src_unit(u, g.C, g.ld)];
    }
  }
}

}  // namespace

extern "C" {

int dh_pack_outputs_vec4(int C, int ld, const void* src, const void* dst) {
  return dh::out_vec4(C, ld, reinterpret_cast<uintptr_t>(src), reinterpret_cast<uintptr_t>(dst)) ? 1 : 0;
}

int dh_pack_outputs_host(const dh_out_seg* segs, int nseg) { return dh::pack_outputs_host(segs, nseg); }

int dh_pack_outputs_f32(const dh_out_seg* segs, int nseg, void* stream) {
  if (nseg < 0 || (nseg > 0 && segs == nullptr)) return DH_EINVAL;
  for (int s = 0; s < nseg; ++s)
    if (segs[s].dst != nullptr && !dh::out_seg_ok(segs[s])) return DH_EINVAL;      // nothing is launched for a bad table
  PackArgs a = {};
  int s = 0;
  while (s < nseg) {
    a.nseg = 0;
    a.vec = 0;
    a.first[0] = 0;
    uint64_t groups = 0;
    for (; s < nseg && a.nseg < kPackMaxSegs; ++s) {
      const dh_out_seg& g = segs[s];
      if (g.dst == nullptr) continue;                                               // an output the caller does not want
      const bool v = dh::out_vec4(g.C, g.ld, reinterpret_cast<uintptr_t>(g.src), reinterpret_cast<uintptr_t>(g.dst));
      const uint64_t ng = (uint64_t)((dh::out_units(g, v) + kPackGroupUnits - 1) / kPackGroupUnits);
      if (ng > 0x7fffffffull) return DH_EINVAL;
      if (groups + ng > 0x7fffffffull) break;                                       // this one opens the next launch
      groups += ng;
      a.seg[a.nseg] = g;
      if (v) a.vec |= 1ull << a.nseg;
      a.first[++a.nseg] = (uint32_t)groups;
    }
    if (a.nseg == 0) continue;
    hipLaunchKernelGGL(pack_outputs_kernel, dim3((unsigned)groups), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
    const int rc = dh::check_launch();
    if (rc != DH_OK) return rc;
  }
  return DH_OK;
}

}  // extern "C"
