// LDS-DMA primitives of the GEMM family (gemm1x1.hip, the split-bf16 kernels of gemm1x1s_body.h, conv_halo.hip): operand
// tiles go global -> LDS by buffer_load ... lds, fragments come back through asm ds_read_b128.  relu1 also serves dw_lds.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dh {

typedef __attribute__((address_space(3))) void* lptr_t;
constexpr unsigned OOB = 0xfffffff0u;   // a buffer offset beyond every descriptor used here: the load returns zeros

// buffer_load_dwordx4 ... offen lds: 16 bytes per lane from (descriptor base + voff + soff) to LDS (wave-uniform `dst`
// + lane * 16).  A 32-bit per-lane offset fixed over K plus a SCALAR K-step offset: no per-step 64-bit address VALU
// (5.7 VALU per MFMA were measured in the first version of the split-bf16 kernel; about 4 hide under a bf16 MFMA).
// The builtin only exists for the gfx950 pass: hipcc's host pass silently drops a kernel TEMPLATE whose
// body names it (no host stub is emitted), hence the guard.
template <typename RSRC>
__device__ __forceinline__ void dma16(RSRC rs, void* dst, unsigned voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lptr_t)dst, 16, voff, soff, 0, 0);
#endif
}

// Fragment reads go through inline asm on purpose: with an LDS-DMA in flight hipcc cannot prove that the DMA's
// LDS destination (the other stage) does not alias an ordinary ds_read and puts `s_waitcnt vmcnt(0)` in front
// of the first fragment read of every K-step, which serialises the DMA with the MFMA block it is meant to
// overlap.  An asm ds_read is invisible to that pass; its completion is awaited by hand (lgkm_wait) and the
// consumers are fenced behind the wait with sched_barrier (hipcc would otherwise hoist the MFMAs).
template <int OFF>
__device__ __forceinline__ float4 lds_rd(unsigned addr) {
  float4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
__device__ __forceinline__ void lgkm_wait() {
  __builtin_amdgcn_sched_barrier(0);   // MFMAs issued before the wait stay before it: they are what hides the read
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// ReLU as ONE integer instruction per element: non-negative floats order like non-negative ints and everything with
// the sign bit set is a negative int, so max_i32(bits, 0) is relu(v) (-0 -> +0).  fmaxf costs two v_max_f32 (a
// canonicalising one first), and on gfx950 nothing issues beside an fp32 MFMA (profiles/r02_sepconv_fusion_study.md):
// every VALU instruction of the K loop is paid in full -- 32 instead of 16 per K-step was 4-8 % of the ReLU-on-load
// GEMMs.  (An asm v_max_f32 is not an option: hipcc pads no VALU->MFMA hazard wait states after inline asm.)
__device__ __forceinline__ float relu1(float v) {
  const int b = __float_as_int(v);
  return __int_as_float(b > 0 ? b : 0);
}
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)); }

}  // namespace dh
