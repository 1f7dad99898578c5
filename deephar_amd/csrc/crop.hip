// dh_crop_resize_u8: every crop of a chunk -- window out of a full frame, PIL's 8-bit bilinear resize, optional mirror -- in
// ONE launch, written straight into the network's uint8 input.  Integer arithmetic only: the coefficients arrive in the crop
// program (crop_index.h), computed in double on the host.
//   grid (njobs, ceil(OH / kCropGroupRows)): work-group (j, g) walks the bands g, g + gridDim.y, ... of job j; a band is
//   `band` output rows (chosen by the builder from the job's vertical scale so that the rows it reads fit LDS).
//   pass 1: the source rows the band's vertical taps need, one lane per (row, output column), lanes along the row; clipped to
//           the image; resampled horizontally and rounded to uint8 into LDS (mirrored here when hflip is set).
//   pass 2: the vertical pass from LDS, 16 output bytes per lane (LDS rows are 16-byte multiples apart), stored as one 16-byte
//           vector store, or one byte per lane when the row length or the destination does not allow it.
// The intermediate never reaches memory.  No atomics.  The index arithmetic is shared with the host twin dh_crop_resize_host.
#include "dh_kernels.h"
#include "crop_index.h"

namespace {

using namespace dh;

__global__ __launch_bounds__(kCropThreads) void crop_resize_kernel(const uint8_t* __restrict__ prog, int njobs, int OH, int OW,
                                                                    uint8_t* __restrict__ y, int64_t item_pitch, int vec16) {
  __shared__ __attribute__((aligned(16))) uint8_t rows[kCropLdsBytes];
  const CropHeader h = *reinterpret_cast<const CropHeader*>(prog);
  const int j = blockIdx.x;
  if (h.magic != kCropMagic || h.OH != OH || h.OW != OW || j >= h.njobs || j >= njobs) return;      // not this launch's program
  const CropJobRec jr = reinterpret_cast<const CropJobRec*>(prog + h.job_off)[j];
  if (jr.band < 1 || jr.src < 0 || jr.src >= h.nsrc) return;
  const dh_crop_src sr = reinterpret_cast<const dh_crop_src*>(prog + h.src_off)[jr.src];
  const int32_t* __restrict__ xfirst = reinterpret_cast<const int32_t*>(prog + jr.xtab);
  const int32_t* __restrict__ xcount = xfirst + OW;
  const int32_t* __restrict__ xk = xcount + OW;
  const int32_t* __restrict__ yfirst = reinterpret_cast<const int32_t*>(prog + jr.ytab);
  const int32_t* __restrict__ ycount = yfirst + OH;
  const int32_t* __restrict__ yk = ycount + OH;
  const int pitch = crop_lds_pitch(OW);
  const int nbands = (OH + jr.band - 1) / jr.band;
  uint8_t* __restrict__ dst = y + (size_t)j * item_pitch;
  const int tid = threadIdx.x;

  for (int b = blockIdx.y; b < nbands; b += gridDim.y) {
    const int r0 = b * jr.band, r1 = min(OH, r0 + jr.band);
    const int ylo = yfirst[r0];
    const int nrows = crop_band_rows(yfirst, ycount, r0, r1);
    if (nrows < 1 || (int64_t)nrows * pitch > kCropLdsBytes) continue;                               // (uniform in the work-group)
    // ---- pass 1: source rows [y0 + ylo, y0 + ylo + nrows) -> LDS, resampled along x
    for (int i = tid; i < nrows * OW; i += kCropThreads) {
      const int r = i / OW, ox = i - r * OW;
      const uint8_t* row = crop_inside(jr.y0, ylo + r, sr.H) ? sr.ptr + (size_t)(jr.y0 + ylo + r) * sr.pitch : nullptr;
      int px[3];
      crop_hpixel(row, sr.W, jr.x0, xfirst[ox], min(xcount[ox], jr.xtaps), xk + (size_t)ox * jr.xtaps, px);
      uint8_t* o = rows + r * pitch + (jr.hflip ? OW - 1 - ox : ox) * 3;
      o[0] = (uint8_t)px[0];
      o[1] = (uint8_t)px[1];
      o[2] = (uint8_t)px[2];
    }
    __syncthreads();
    // ---- pass 2: output rows [r0, r1) from LDS, resampled along y
    if (vec16) {
      const int upr = (3 * OW) >> 4;                                                                 // 16-byte units per output row
      for (int u = tid; u < (r1 - r0) * upr; u += kCropThreads) {
        const int rr = r0 + u / upr, cb = (u % upr) << 4;
        const int base = yfirst[rr] - ylo, n = min(ycount[rr], jr.ytaps);
        int32_t acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = kCropHalf;
        for (int t = 0; t < n && base + t < nrows; ++t) {
          const int32_t kv = yk[(size_t)rr * jr.ytaps + t];
          const uint4 v = *reinterpret_cast<const uint4*>(rows + (base + t) * pitch + cb);
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[e] += kv * (int32_t)((w[e >> 2] >> ((e & 3) * 8)) & 0xffu);
        }
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e >> 2] |= (uint32_t)crop_round(acc[e]) << ((e & 3) * 8);
        *reinterpret_cast<uint4*>(dst + (size_t)rr * OW * 3 + cb) = make_uint4(o[0], o[1], o[2], o[3]);
      }
    } else {
      const int rowb = 3 * OW;
      for (int u = tid; u < (r1 - r0) * rowb; u += kCropThreads) {
        const int rr = r0 + u / rowb, cb = u % rowb;
        const int base = yfirst[rr] - ylo, n = min(ycount[rr], jr.ytaps);
        int32_t acc = kCropHalf;
        for (int t = 0; t < n && base + t < nrows; ++t) acc += yk[(size_t)rr * jr.ytaps + t] * (int32_t)rows[(base + t) * pitch + cb];
        dst[(size_t)rr * rowb + cb] = (uint8_t)crop_round(acc);
      }
    }
    __syncthreads();                                                                                 // the next band refills LDS
  }
}

}  // namespace

extern "C" {

int dh_crop_axis_taps(int in, int out) { return in >= 1 && out >= 1 ? dh::crop_axis_taps(in, out) : DH_EINVAL; }

int dh_crop_axis_coeffs_host(int in, int out, int taps, int32_t* first, int32_t* count, int32_t* k) {
  if (in < 1 || out < 1 || first == nullptr || count == nullptr || k == nullptr || in > dh::kCropMaxExtent ||
      out > dh::kCropMaxExtent)
    return DH_EINVAL;
  if (taps < dh::crop_axis_taps(in, out)) return DH_EINVAL;           // (no scale cap here: that belongs to the launch)
  dh::crop_axis_coeffs(in, out, taps, first, count, k);
  return DH_OK;
}

int dh_crop_program_bytes(const dh_crop_job* jobs, int njobs, int nsrc, int OH, int OW, size_t* bytes) {
  return dh::crop_program_bytes(jobs, njobs, nsrc, OH, OW, bytes);
}

int dh_crop_program_build_host(const dh_crop_src* srcs, int nsrc, const dh_crop_job* jobs, int njobs, int OH, int OW,
                               void* program_host, size_t bytes) {
  return dh::crop_program_build(srcs, nsrc, jobs, njobs, OH, OW, program_host, bytes);
}

int dh_crop_resize_host(const void* program_host, size_t bytes, int njobs, int OH, int OW, uint8_t* y, int64_t item_pitch) {
  return dh::crop_resize_host(program_host, bytes, njobs, OH, OW, y, item_pitch);
}

int dh_crop_resize_u8(const void* program_dev, int njobs, int OH, int OW, uint8_t* y, int64_t item_pitch, void* stream) {
  if (program_dev == nullptr || y == nullptr || njobs < 1 || OH < 1 || OW < 1 || OH > dh::kCropMaxExtent || OW > dh::kCropMaxExtent ||
      ((uintptr_t)program_dev & 7) != 0 || item_pitch < (int64_t)OH * OW * 3)
    return DH_EINVAL;
  if ((int64_t)dh::crop_lds_pitch(OW) * 2 > dh::kCropLdsBytes) return DH_EUNSUPPORTED;            // not even up-scaling's two rows
  const int groups = (OH + dh::kCropGroupRows - 1) / dh::kCropGroupRows;
  const dim3 grid((unsigned)njobs, (unsigned)(groups < 65535 ? groups : 65535));
  hipLaunchKernelGGL(crop_resize_kernel, grid, dim3(dh::kCropThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(program_dev), njobs, OH, OW, y, item_pitch,
                     dh::crop_vec16(OW, reinterpret_cast<uintptr_t>(y), item_pitch) ? 1 : 0);
  return dh::check_launch();
}

}  // extern "C"
