// Frame-sharded clip models behind the C ABI: dh_clip_inspect / dh_clip_create / dh_clip_forward / dh_clip_forward_host /
// dh_clip_destroy and the unpack launch dh_unpack_cut_f32 (include/deephar_hip.h).  The container is written by
// deephar_amd/engine/serialize.py (dump_clip_plan, format documented there); its parser and the index arithmetic of the
// clip boundary live in cut_index.h, GPU-free.  This file owns the two plans, the gather buffer and the segment table, and
// enqueues frame plan -> the host's all-gather (a callback: nothing here links a collective library) -> ONE unpack launch
// -> head plan on the caller's stream: what deephar_amd/parallel.py's ShardedClipModel does in its serial form, with every
// strided copy between the stages folded into that one launch.
#include <cstring>
#include <vector>
#include "cut_index.h"
#include "dh_kernels.h"

namespace {

using dh::CutGeom;

constexpr int kCutLdsFloats = 8192;      // 32 KiB tile: R pixel rows x Cp packed channels
constexpr int kCutMaxRows = 64;

// One work-group moves R consecutive pixel rows of one chunk (g, n): the R * Cp source floats are one contiguous run, read
// with consecutive lanes on consecutive addresses into LDS; every segment then writes its R x c floats from LDS with
// consecutive lanes on consecutive destination addresses (one contiguous run when ld == c) -- a 500-channel feature
// segment and a dozen one-channel confidences both stay coalesced on the global side, the transposition happens in LDS.
__global__ __launch_bounds__(256) void unpack_cut_kernel(const float* __restrict__ src, CutGeom q,
                                                         const dh_cut_seg* __restrict__ segs, int nseg, int R,
                                                         int tiles_per_chunk, int src_vec) {
  __shared__ __attribute__((aligned(16))) float tile[kCutLdsFloats];
  const int chunk = (int)(blockIdx.x / (unsigned)tiles_per_chunk);
  const int64_t r0 = (int64_t)(blockIdx.x - (unsigned)chunk * (unsigned)tiles_per_chunk) * R;
  const int g = chunk / q.m, n = chunk - g * q.m;
  const int64_t left = dh::cut_chunk_rows(q) - r0;
  const int rows = left < R ? (int)left : R;
  const int64_t sbase = dh::cut_src_index(q, g, n, r0, 0);
  const int cnt = rows * q.Cp;
  if (src_vec) {                                           // Cp % 4 == 0 and src 16-byte aligned: so is every tile
    const float4* s4 = reinterpret_cast<const float4*>(src + sbase);
    float4* t4 = reinterpret_cast<float4*>(tile);
    for (int i = threadIdx.x; i < cnt / 4; i += blockDim.x) t4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) tile[i] = src[sbase + i];
  }
  __syncthreads();
  for (int s = 0; s < nseg; ++s) {
    const dh_cut_seg sg = segs[s];
    if (sg.dst == nullptr || !dh::cut_seg_ok(q.Cp, sg.coff, sg.c, sg.ld)) continue;
    if (src_vec && dh::cut_vec4(q.Cp, sg.coff, sg.c, sg.ld, 0, reinterpret_cast<uintptr_t>(sg.dst))) {
      const int c4 = sg.c / 4;
      for (int i = threadIdx.x; i < rows * c4; i += blockDim.x) {
        const int r = i / c4, j = (i - r * c4) * 4;
        const float4 v = *reinterpret_cast<const float4*>(&tile[dh::cut_src_index(q, g, n, r0 + r, sg.coff + j) - sbase]);
        *reinterpret_cast<float4*>(sg.dst + dh::cut_dst_row(q, g, n, r0 + r) * sg.ld + j) = v;
      }
    } else {
      for (int i = threadIdx.x; i < rows * sg.c; i += blockDim.x) {
        const int r = i / sg.c, j = i - r * sg.c;
        sg.dst[dh::cut_dst_row(q, g, n, r0 + r) * sg.ld + j] = tile[dh::cut_src_index(q, g, n, r0 + r, sg.coff + j) - sbase];
      }
    }
  }
}

struct Output { int head; int index; int64_t items; };     // model output k: head output `index` or cut tensor `index`

}  // namespace

struct dh_clip {
  dh_clip_info info = {};
  int rank = 0, n = 0;
  dh_allgather_fn gather = nullptr;
  void* ctx = nullptr;
  dh_plan* frames = nullptr;
  dh_plan* head = nullptr;
  std::vector<int> coff, c;                // the cut table
  std::vector<Output> outs;
  const float* packed = nullptr;           // the frame plan's packed output where it lies (pitch == Cp), else NULL
  float* send = nullptr;                   // dense copy of it otherwise
  float* gbuf = nullptr;                   // [G, n, Tl, P, Cp]; NULL when the packed tensor is read in place (world 1)
  dh_cut_seg* segs_dev = nullptr;
  std::vector<dh_cut_seg> segs, uploaded;  // this call's table, and what segs_dev holds
  std::vector<float*> head_in, head_out;
  // dh_clip_forward_host staging (allocated on first use)
  hipStream_t stream = nullptr;
  void* in_dev = nullptr;
  std::vector<float*> out_dev;
};

namespace {

// the head's inputs in place first (fixed at create), then one segment per wanted pass-through output
void build_segments(dh_clip* cl, float* const* outputs) {
  cl->segs.clear();
  if (cl->head != nullptr)
    for (size_t i = 0; i < cl->c.size(); ++i) cl->segs.push_back({cl->head_in[i], cl->c[i], cl->coff[i], cl->c[i], 0});
  for (size_t k = 0; k < cl->outs.size(); ++k) {
    const Output& o = cl->outs[k];
    if (o.head == 0 && outputs != nullptr && outputs[k] != nullptr)
      cl->segs.push_back({outputs[k], cl->c[o.index], cl->coff[o.index], cl->c[o.index], 0});
  }
}

int upload_segments(dh_clip* cl, hipStream_t s) {
  const size_t nb = cl->segs.size() * sizeof(dh_cut_seg);
  if (cl->segs.size() == cl->uploaded.size() && (nb == 0 || std::memcmp(cl->segs.data(), cl->uploaded.data(), nb) == 0)) return DH_OK;
  cl->uploaded.clear();
  if (nb != 0 && hipMemcpyAsync(cl->segs_dev, cl->segs.data(), nb, hipMemcpyHostToDevice, s) != hipSuccess) return DH_ELAUNCH;
  // the table is pageable host memory: wait until the copy has read it (first call, or new pass-through pointers only)
  if (nb != 0 && hipStreamSynchronize(s) != hipSuccess) return DH_ELAUNCH;
  cl->uploaded = cl->segs;
  return DH_OK;
}

}  // namespace

extern "C" {

int dh_unpack_cut_vec4(int Cp, int coff, int c, int ld, const void* gathered, const void* dst) {
  return dh::cut_vec4(Cp, coff, c, ld, reinterpret_cast<uintptr_t>(gathered), reinterpret_cast<uintptr_t>(dst)) ? 1 : 0;
}

int dh_unpack_cut_host(const float* gathered, int G, int m, int Tl, int64_t P, int Cp, const dh_cut_seg* segs, int nseg) {
  return dh::unpack_cut_host(gathered, G, m, Tl, P, Cp, segs, nseg);
}

int dh_unpack_cut_f32(const float* gathered, int G, int m, int Tl, int64_t P, int Cp, const dh_cut_seg* segs_dev, int nseg,
                      void* stream) {
  if (gathered == nullptr || segs_dev == nullptr || nseg < 1 || dh::cut_geom_check(G, m, Tl, P, Cp) != DH_OK) return DH_EINVAL;
  if (Cp > kCutLdsFloats) return DH_EUNSUPPORTED;
  const CutGeom q = {G, m, Tl, P, Cp};
  const int64_t chunk_rows = dh::cut_chunk_rows(q);
  int R = kCutLdsFloats / Cp;
  if (R > kCutMaxRows) R = kCutMaxRows;
  if (R > chunk_rows) R = (int)chunk_rows;
  const int64_t tiles = (chunk_rows + R - 1) / R, grid = tiles * G * m;
  if (tiles > 0x7fffffff || grid > 0x7fffffff) return DH_EINVAL;
  const int src_vec = (Cp % 4 == 0 && (reinterpret_cast<uintptr_t>(gathered) & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(unpack_cut_kernel, dim3((unsigned)grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), gathered, q,
                     segs_dev, nseg, R, (int)tiles, src_vec);
  return dh::check_launch();
}

int dh_clip_inspect(const void* blob, size_t bytes, dh_clip_info* out) {
  dh::ClipBlob cb;
  if (out == nullptr) return DH_EINVAL;
  const int rc = dh::clip_parse(blob, bytes, &cb);
  if (rc == DH_OK) *out = cb.info;
  return rc;
}

int dh_clip_inspect_cut(const void* blob, size_t bytes, int i, int32_t* channel_offset, int32_t* channels) {
  dh::ClipBlob cb;
  if (channel_offset == nullptr || channels == nullptr || dh::clip_parse(blob, bytes, &cb) != DH_OK) return DH_EINVAL;
  if (i < 0 || i >= cb.info.num_cut) return DH_EINVAL;
  *channel_offset = (int32_t)dh::clip_u32(cb.cut + 8 * i);
  *channels = (int32_t)dh::clip_u32(cb.cut + 8 * i + 4);
  return DH_OK;
}

int dh_clip_inspect_output(const void* blob, size_t bytes, int k, int32_t* is_head, int32_t* index) {
  dh::ClipBlob cb;
  if (is_head == nullptr || index == nullptr || dh::clip_parse(blob, bytes, &cb) != DH_OK) return DH_EINVAL;
  if (k < 0 || k >= cb.info.num_outputs) return DH_EINVAL;
  *is_head = (int32_t)dh::clip_u32(cb.outputs + 8 * k);
  *index = (int32_t)dh::clip_u32(cb.outputs + 8 * k + 4);
  return DH_OK;
}

int dh_clip_create(const void* blob, size_t bytes, int rank, dh_allgather_fn gather, void* ctx, dh_clip** out) {
  dh::ClipBlob cb;
  if (out == nullptr || dh::clip_parse(blob, bytes, &cb) != DH_OK) return DH_EINVAL;
  const dh_clip_info& info = cb.info;
  if (rank < 0 || rank >= info.world || (gather == nullptr && info.world != 1)) return DH_EINVAL;
  if (info.packed_channels > kCutLdsFloats) return DH_EUNSUPPORTED;
  dh_clip* cl = new dh_clip();
  auto fail = [&](int rc) { dh_clip_destroy(cl); return rc; };
  cl->info = info;
  cl->rank = rank;
  cl->gather = gather;
  cl->ctx = ctx;
  const unsigned char* b = static_cast<const unsigned char*>(blob);
  int rc = dh_plan_create(b + info.frames_offset, (size_t)info.frames_bytes, &cl->frames);
  if (rc != DH_OK) return fail(rc);
  if (info.head_bytes != 0 && (rc = dh_plan_create(b + info.head_offset, (size_t)info.head_bytes, &cl->head)) != DH_OK) return fail(rc);
  // the two plans against the cut table: one packed [clips, Tl, P, Cp] output, one dense [clips, T, P, c] input per cut tensor
  cl->n = dh_plan_batch(cl->frames);
  const int Cp = info.packed_channels;
  if (dh::cut_geom_check(info.world, cl->n, info.Tl, info.P, Cp) != DH_OK) return fail(DH_EINVAL);
  int ld = 0, C = 0;
  int64_t npix = 0;
  const float* view = dh::plan_output_view(cl->frames, 0, &ld, &C, &npix);
  if (dh_plan_num_inputs(cl->frames) != 1 || dh_plan_num_outputs(cl->frames) != 1 || view == nullptr || C != Cp ||
      npix != (int64_t)info.Tl * info.P)
    return fail(DH_EINVAL);
  for (int i = 0; i < info.num_cut; ++i) {
    cl->coff.push_back((int)dh::clip_u32(cb.cut + 8 * i));
    cl->c.push_back((int)dh::clip_u32(cb.cut + 8 * i + 4));
  }
  const int64_t TP = (int64_t)info.T * info.P;
  if (cl->head != nullptr) {
    if (dh_plan_batch(cl->head) != cl->n || dh_plan_num_inputs(cl->head) != info.num_cut ||
        dh_plan_num_outputs(cl->head) != info.num_head_outputs)
      return fail(DH_EINVAL);
    for (int i = 0; i < info.num_cut; ++i) {
      float* p = dh_plan_input_ptr(cl->head, i);
      if (p == nullptr || dh_plan_input_items(cl->head, i) != TP * cl->c[i]) return fail(DH_EINVAL);
      cl->head_in.push_back(p);
    }
    cl->head_out.assign((size_t)info.num_head_outputs, nullptr);
  }
  for (int k = 0; k < info.num_outputs; ++k) {
    Output o;
    o.head = (int)dh::clip_u32(cb.outputs + 8 * k);
    o.index = (int)dh::clip_u32(cb.outputs + 8 * k + 4);
    o.items = o.head ? dh_plan_output_items(cl->head, o.index) : TP * cl->c[o.index];
    cl->outs.push_back(o);
  }
  const size_t per_rank = (size_t)cl->n * (size_t)info.Tl * (size_t)info.P * (size_t)Cp * 4;
  if (ld == Cp) cl->packed = view;
  else if (hipMalloc(&cl->send, per_rank) != hipSuccess) return fail(DH_ELAUNCH);
  if (gather != nullptr && hipMalloc(&cl->gbuf, per_rank * (size_t)info.world) != hipSuccess) return fail(DH_ELAUNCH);
  if (hipMalloc(&cl->segs_dev, sizeof(dh_cut_seg) * (size_t)(info.num_cut + info.num_outputs)) != hipSuccess) return fail(DH_ELAUNCH);
  build_segments(cl, nullptr);                      // the head's inputs: uploaded once, here
  if (upload_segments(cl, nullptr) != DH_OK) return fail(DH_ELAUNCH);
  *out = cl;
  return DH_OK;
}

int dh_clip_destroy(dh_clip* cl) {
  if (cl == nullptr) return DH_OK;
  if (cl->stream) hipStreamSynchronize(cl->stream);
  if (cl->in_dev) hipFree(cl->in_dev);
  for (float* q : cl->out_dev) hipFree(q);
  if (cl->stream) hipStreamDestroy(cl->stream);
  if (cl->send) hipFree(cl->send);
  if (cl->gbuf) hipFree(cl->gbuf);
  if (cl->segs_dev) hipFree(cl->segs_dev);
  dh_plan_destroy(cl->frames);
  dh_plan_destroy(cl->head);
  delete cl;
  return DH_OK;
}

int dh_clip_world(const dh_clip* cl) { return cl ? cl->info.world : 0; }
int dh_clip_batch(const dh_clip* cl) { return cl ? cl->n : 0; }
int dh_clip_num_outputs(const dh_clip* cl) { return cl ? (int)cl->outs.size() : 0; }
int64_t dh_clip_output_items(const dh_clip* cl, int k) {
  return (cl && k >= 0 && k < (int)cl->outs.size()) ? cl->outs[k].items : -1;
}
int64_t dh_clip_frame_items(const dh_clip* cl) { return cl ? dh_plan_input_items(cl->frames, 0) : -1; }
int dh_clip_input_is_u8(const dh_clip* cl) { return cl ? dh_plan_input_is_u8(cl->frames, 0) : -1; }

int dh_clip_forward(dh_clip* cl, const void* frames_dev, int m, float* const* outputs, void* stream) {
  if (cl == nullptr || frames_dev == nullptr || outputs == nullptr || m <= 0 || m > cl->n) return DH_EINVAL;
  const dh_clip_info& info = cl->info;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // 1. the frame stage; its packed output stays in the plan's arena when that is dense
  const float* ins[1] = {static_cast<const float*>(frames_dev)};
  float* fouts[1] = {cl->packed != nullptr ? nullptr : cl->send};
  int rc = dh_forward(cl->frames, ins, m, fouts, stream);
  if (rc != DH_OK) return rc;
  const float* packed = cl->packed != nullptr ? cl->packed : cl->send;
  // 2. the host's collective: [m, Tl, P, Cp] of every rank -> [G, m, Tl, P, Cp]
  const float* gathered = packed;
  if (cl->gather != nullptr) {
    if (cl->gather(cl->ctx, packed, cl->gbuf, (int64_t)m * info.Tl * info.P * info.packed_channels, stream) != 0) return DH_ELAUNCH;
    gathered = cl->gbuf;
  }
  // 3. ONE launch: every head input in place, every wanted pass-through output straight to the caller
  build_segments(cl, outputs);
  if ((rc = upload_segments(cl, s)) != DH_OK) return rc;
  if (!cl->segs.empty()) {
    rc = dh_unpack_cut_f32(gathered, info.world, m, info.Tl, info.P, info.packed_channels, cl->segs_dev, (int)cl->segs.size(), stream);
    if (rc != DH_OK) return rc;
  }
  // 4. the temporal head, its outputs in model order
  if (cl->head != nullptr) {
    for (size_t k = 0; k < cl->outs.size(); ++k)
      if (cl->outs[k].head) cl->head_out[(size_t)cl->outs[k].index] = outputs[k];
    rc = dh_forward(cl->head, cl->head_in.data(), m, cl->head_out.data(), stream);
  }
  return rc;
}

int dh_clip_forward_host(dh_clip* cl, const void* frames_host, int m, float* const* outputs_host) {
  if (cl == nullptr || frames_host == nullptr || outputs_host == nullptr || m <= 0 || m > cl->n) return DH_EINVAL;
  const size_t in_item = (size_t)dh_clip_frame_items(cl) * (dh_clip_input_is_u8(cl) ? 1 : 4);
  if (cl->stream == nullptr) {           // staging is committed only when every allocation succeeded (as dh_forward_host)
    hipStream_t st = nullptr;
    void* in_dev = nullptr;
    std::vector<float*> out_dev;
    bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipMalloc(&in_dev, in_item * (size_t)cl->n) == hipSuccess;
    for (size_t k = 0; ok && k < cl->outs.size(); ++k) {
      float* q = nullptr;
      ok = hipMalloc(&q, (size_t)cl->outs[k].items * 4 * (size_t)cl->n) == hipSuccess;
      if (ok) out_dev.push_back(q);
    }
    if (!ok) {
      for (float* q : out_dev) hipFree(q);
      if (in_dev) hipFree(in_dev);
      if (st) hipStreamDestroy(st);
      return DH_ELAUNCH;
    }
    cl->in_dev = in_dev;
    cl->out_dev.swap(out_dev);
    cl->stream = st;
  }
  if (hipMemcpyAsync(cl->in_dev, frames_host, in_item * (size_t)m, hipMemcpyHostToDevice, cl->stream) != hipSuccess) return DH_ELAUNCH;
  std::vector<float*> outs(cl->outs.size(), nullptr);
  for (size_t k = 0; k < outs.size(); ++k) outs[k] = outputs_host[k] != nullptr ? cl->out_dev[k] : nullptr;
  const int rc = dh_clip_forward(cl, cl->in_dev, m, outs.data(), cl->stream);
  if (rc != DH_OK) return rc;
  for (size_t k = 0; k < outs.size(); ++k)
    if (outputs_host[k] != nullptr &&
        hipMemcpyAsync(outputs_host[k], cl->out_dev[k], (size_t)cl->outs[k].items * 4 * (size_t)m, hipMemcpyDeviceToHost, cl->stream) != hipSuccess)
      return DH_ELAUNCH;
  return hipStreamSynchronize(cl->stream) == hipSuccess ? DH_OK : DH_ELAUNCH;
}

}  // extern "C"
