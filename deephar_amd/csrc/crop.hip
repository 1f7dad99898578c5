// dh_crop_resize_u8: every crop of a chunk -- window out of a full frame, PIL's 8-bit bilinear resize, optional mirror -- in
// ONE launch, written straight into the network's uint8 input.  Integer arithmetic only: the coefficients arrive in the crop
// program (crop_index.h), computed in double by a builder -- on the host, or on the device (below).
//   grid (njobs, ceil(OH / kCropGroupRows)): work-group (j, g) walks the bands g, g + gridDim.y, ... of job j; a band is
//   `band` output rows (chosen by the builder from the job's vertical scale so that the rows it reads fit LDS).
//   pass 1: the source rows the band's vertical taps need, one lane per (row, output column), lanes along the row; clipped to
//           the image; resampled horizontally and rounded to uint8 into LDS (mirrored here when hflip is set).
//   pass 2: the vertical pass from LDS, 16 output bytes per lane (LDS rows are 16-byte multiples apart), stored as one 16-byte
//           vector store, or one byte per lane when the row length or the destination does not allow it.
// The intermediate never reaches memory.  No atomics.  The index arithmetic is shared with the host twin dh_crop_resize_host.
//
// dh_crop_program_build_dev: the crop program itself built on the device from a job table in device memory -- byte for byte
// what crop_program_build (crop_index.h) writes on the host -- as two small launches:
//   layout: ONE work-group.  Lane t validates jobs t, t + 256, ..., takes their tap counts and table bytes; an exclusive scan
//           over the work-group with a running carry from chunk to chunk of 256 jobs gives every job its two table offsets;
//           then the header, the source table and every job record are written.  A job that fails a check gets a record
//           with band = 0 (crop_resize_kernel skips it), no table bytes, and its code in status[j].
//   tables: grid (njobs, 2): work-group (j, 0) fills the x table of job j, (j, 1) the y table, one lane per output index
//           (crop_axis_output: the host's doubles, contraction off); (j, 1) then picks the job's band from its finished table.
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

// ---- the program builder --------------------------------------------------------------------------------------------------
// DH_OK, or why job g cannot run: the host builder's checks in its order, per job (a bad source fails only the jobs naming it)
__device__ inline int crop_job_status(const dh_crop_job& g, const dh_crop_src* srcs, int nsrc, int OH, int OW) {
  if (!crop_job_ok(g, nsrc)) return DH_EINVAL;
  if (!crop_axis_supported(g.x1 - g.x0, OW) || !crop_axis_supported(g.y1 - g.y0, OH)) return DH_EUNSUPPORTED;
  if (!crop_src_ok(srcs[g.src])) return DH_EINVAL;
  return DH_OK;
}

__global__ __launch_bounds__(kCropThreads) void crop_layout_kernel(const dh_crop_src* __restrict__ srcs, int nsrc,
                                                                    const dh_crop_job* __restrict__ jobs, int njobs, int OH, int OW,
                                                                    uint8_t* __restrict__ prog, int32_t* __restrict__ status) {
  __shared__ uint32_t scan[kCropThreads];
  const int tid = threadIdx.x;
  const uint32_t src_off = (uint32_t)sizeof(CropHeader);
  const uint32_t job_off = src_off + (uint32_t)nsrc * (uint32_t)sizeof(dh_crop_src);
  uint32_t carry = job_off + (uint32_t)njobs * (uint32_t)sizeof(CropJobRec);     // where the next chunk's first table starts
  CropJobRec* recs = reinterpret_cast<CropJobRec*>(prog + job_off);
  for (int base = 0; base < njobs; base += kCropThreads) {                       // (uniform: every lane runs every chunk)
    const int j = base + tid;
    CropJobRec r = {};
    uint32_t xbytes = 0, ybytes = 0;
    int rc = DH_OK;
    if (j < njobs) {
      const dh_crop_job g = jobs[j];
      rc = crop_job_status(g, srcs, nsrc, OH, OW);
      r.src = g.src; r.x0 = g.x0; r.y0 = g.y0; r.x1 = g.x1; r.y1 = g.y1; r.hflip = g.hflip ? 1 : 0;
      if (rc == DH_OK) {
        r.xtaps = crop_axis_taps(g.x1 - g.x0, OW);
        r.ytaps = crop_axis_taps(g.y1 - g.y0, OH);
        xbytes = (uint32_t)crop_axis_table_bytes(OW, r.xtaps);
        ybytes = (uint32_t)crop_axis_table_bytes(OH, r.ytaps);
      }
    }
    // inclusive scan of the chunk's table bytes (the host refused a program above 2^31 - 1 bytes: no sum wraps)
    scan[tid] = xbytes + ybytes;
    __syncthreads();
    for (int d = 1; d < kCropThreads; d <<= 1) {
      const uint32_t below = tid >= d ? scan[tid - d] : 0u;
      __syncthreads();
      scan[tid] += below;
      __syncthreads();
    }
    if (j < njobs) {
      if (rc == DH_OK) {
        r.xtab = carry + scan[tid] - (xbytes + ybytes);
        r.ytab = r.xtab + xbytes;
      }
      recs[j] = r;                                 // band = 0 until the y table's work-group has picked it (never, for a refused job)
      if (status != nullptr) status[j] = rc;
    }
    carry += scan[kCropThreads - 1];
    __syncthreads();                               // the next chunk overwrites scan[]
  }
  if (tid == 0) {
    const CropHeader h = {kCropMagic, nsrc, njobs, OH, OW, src_off, job_off, carry};
    *reinterpret_cast<CropHeader*>(prog) = h;
  }
  // the source table, 8 bytes per lane (both tables are 8-byte aligned, a descriptor is 24 bytes)
  const uint64_t* s8 = reinterpret_cast<const uint64_t*>(srcs);
  uint64_t* d8 = reinterpret_cast<uint64_t*>(prog + src_off);
  for (int i = tid; i < nsrc * 3; i += kCropThreads) d8[i] = s8[i];
}

__global__ __launch_bounds__(kCropThreads) void crop_tables_kernel(uint8_t* __restrict__ prog, int njobs, int OH, int OW) {
  __shared__ int too_big[5];                       // per band candidate 16, 8, 4, 2, 1: some fill of LDS does not fit
  const int tid = threadIdx.x, j = blockIdx.x, yaxis = blockIdx.y;
  const CropHeader h = *reinterpret_cast<const CropHeader*>(prog);
  if (h.magic != kCropMagic || j >= njobs || j >= h.njobs) return;                                   // (uniform)
  CropJobRec* rec = reinterpret_cast<CropJobRec*>(prog + h.job_off) + j;
  const CropJobRec r = *rec;
  if (r.xtaps < 1 || r.ytaps < 1) return;                                                            // a refused job: no tables
  const int in = yaxis ? r.y1 - r.y0 : r.x1 - r.x0, out = yaxis ? OH : OW, taps = yaxis ? r.ytaps : r.xtaps;
  int32_t* tab = reinterpret_cast<int32_t*>(prog + (yaxis ? r.ytab : r.xtab));
  const CropAxis ax = crop_axis_setup(in, out);
  for (int i = tid; i < out; i += kCropThreads) crop_axis_output(ax, in, taps, i, tab, tab + out, tab + 2 * (size_t)out);
  if (tid == 0 && crop_axis_table_pad(out, taps)) tab[(size_t)out * (2 + (size_t)taps)] = 0;
  if (!yaxis) return;
  // The band, from the finished y table.  first / count are walked from GLOBAL memory (an LDS copy would need up to
  // 2 * kCropMaxExtent ints): the barrier below carries the work-group-scope fence that makes this work-group's table stores
  // visible to its own lanes; nobody else reads them before the launch ends.
  if (tid < 5) too_big[tid] = 0;
  __threadfence_block();
  __syncthreads();
  const int32_t* yfirst = tab;
  const int32_t* ycount = tab + OH;
  const int pitch = crop_lds_pitch(OW);
  for (int b = 0; b < 5; ++b) {                    // crop_pick_band's test, the fills of a candidate dealt to the lanes
    const int band = kCropMaxBand >> b;
    for (int64_t r0 = (int64_t)tid * band; r0 < OH; r0 += (int64_t)kCropThreads * band) {
      const int r1 = r0 + band < OH ? (int)r0 + band : OH;
      if ((int64_t)crop_band_rows(yfirst, ycount, (int)r0, r1) * pitch > kCropLdsBytes) too_big[b] = 1;   // (same value from every lane)
    }
  }
  __syncthreads();
  if (tid == 0) {
    int band = 0;
    for (int b = 4; b >= 0; --b)
      if (!too_big[b]) band = kCropMaxBand >> b;
    rec->band = band;
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

int dh_crop_program_max_bytes(int njobs, int nsrc, int OH, int OW, size_t* bytes) {
  const size_t n = dh::crop_program_max_bytes(njobs, nsrc, OH, OW);
  if (bytes == nullptr || n == 0) return DH_EINVAL;
  if (n > 0x7fffffffu) return DH_EUNSUPPORTED;                       // offsets inside a program are 32 bits, like the size query says
  *bytes = n;
  return DH_OK;
}

int dh_crop_program_build_dev(const dh_crop_src* srcs_dev, int nsrc, const dh_crop_job* jobs_dev, int njobs, int OH, int OW,
                              void* program_dev, size_t capacity, int32_t* status_dev, void* stream) {
  size_t need = 0;
  const int rc = dh_crop_program_max_bytes(njobs, nsrc, OH, OW, &need);
  if (rc != DH_OK) return rc;
  if (srcs_dev == nullptr || jobs_dev == nullptr || program_dev == nullptr || ((uintptr_t)program_dev & 7) != 0 ||
      ((uintptr_t)srcs_dev & 7) != 0 || ((uintptr_t)jobs_dev & 3) != 0 || ((uintptr_t)status_dev & 3) != 0 || capacity < need)
    return DH_EINVAL;
  // the host builder's last refusal, for the worst job the table may hold: one output row reads at most kCropMaxTaps rows
  if ((int64_t)dh::kCropMaxTaps * dh::crop_lds_pitch(OW) > dh::kCropLdsBytes) return DH_EUNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint8_t* prog = static_cast<uint8_t*>(program_dev);
  hipLaunchKernelGGL(crop_layout_kernel, dim3(1), dim3(dh::kCropThreads), 0, s, srcs_dev, nsrc, jobs_dev, njobs, OH, OW, prog, status_dev);
  int lrc = dh::check_launch();
  if (lrc != DH_OK) return lrc;
  hipLaunchKernelGGL(crop_tables_kernel, dim3((unsigned)njobs, 2u), dim3(dh::kCropThreads), 0, s, prog, njobs, OH, OW);
  return dh::check_launch();
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
