// C-level plan executor: dh_plan_create / dh_forward / dh_forward_host / dh_plan_destroy (include/deephar_hip.h).
// "a plan/execute pair over device pointers ... one plan per device; stream-ordered, no internal threads".
// The blob is written by deephar_amd/engine/serialize.py (format documented there) from a bound, autotuned plan: the
// launch list of Model.predict with every device pointer expressed relative to the activation arena or the weight
// image.  The blob's format lives in plan_blob.h (GPU-free: the step-record table, the parser, the patch loop); this file
// owns the allocations, patches the pointers once and replays the launches in order on the
// caller's stream -- the same C-ABI entry points the Python executor calls, so the results are the same bits.  A version-5
// blob carries the engine's multi-stream schedule: plan_sched.h (GPU-free) turns it into the enqueue program -- the one
// BoundPlan.launch_all walks too -- which dh_forward runs with the caller's stream as stream 0 and the plan's own side streams.  Every
// forward ends with ONE dh_pack_outputs_f32 launch (out_pack.hip) for all wanted outputs.
// dh_frames_* / dh_forward_frames: a uint8 plan fed from full frames and boxes -- the crop program built on the device
// (dh_crop_program_build_dev), ONE crop launch straight into the plan's uint8 input, then the forward with its input copy skipped.
#include <cstring>
#include <vector>
#include "dh_kernels.h"
#include "plan_blob.h"
#include "crop_index.h"
#include "refine_index.h"
#include "posebox_index.h"

namespace {

using namespace dh;             // enum Fn, kRecords, PlanImage
using Out = PlanOut;

struct Step { int fn; std::vector<unsigned char> payload; };    // a copy of the blob's record, its pointers patched
struct In { size_t items; int u8; char* dst; };                 // dst: where dh_forward copies the caller's data (patched)
// floats output o of `items` batch items takes in dh_forward_host's staging buffer: rounded up to whole 16-byte runs
inline size_t stage_floats(const Out& o, int items) { return (o.npix * (size_t)o.C * (size_t)items + 3) & ~(size_t)3; }

}  // namespace

struct dh_plan {
  int n = 0;
  char* arena = nullptr;
  char* weights = nullptr;
  char* bytes = nullptr;        // region 3: uint8 input staging of a uint8-input plan
  std::vector<In> ins;
  std::vector<Out> outs;
  std::vector<Step> steps;
  // version 5: the schedule as an enqueue program (empty: every step in order on the caller's stream), the plan's own side
  // streams (stream k of the program is side[k - 1]) and one sync event per event id of the program
  std::vector<dh_sched_op> ops;
  std::vector<hipStream_t> side;
  std::vector<hipEvent_t> events;
  std::vector<dh_out_seg> segs;  // this call's pack table
  // dh_forward_host staging (allocated on first use): one device buffer per input, ONE device buffer and its pinned host
  // twin for all outputs
  std::vector<float*> in_dev;
  std::vector<float*> out_ptr;   // this call's place of every wanted output inside out_stage
  float* out_stage = nullptr;
  float* out_host = nullptr;
  hipStream_t stream = nullptr;
  // dh_forward_frames (allocated on first use, grown when a call needs more): the device crop program; the device twin of
  // dh_forward_frames_host's job table
  void* crop_prog = nullptr;
  size_t crop_prog_bytes = 0;
  dh_crop_job* crop_jobs = nullptr;
  size_t crop_jobs_n = 0;
  // dh_refine_frames_host (allocated on first use, grown when a call needs more): the box table, the job tables and the
  // builder's status of every iteration, the frame indices and the raw poses of every iteration, in ONE allocation
  char* refine_buf = nullptr;
  size_t refine_bytes = 0;
  // dh_frame_boxes_host (allocated on first use): the float64 boxes, the int32 boxes and the status words of a full batch
  char* boxes_buf = nullptr;
  size_t boxes_bytes = 0;
  std::vector<dh_crop_job> boxes_jobs;                                 // the host job table of the call in flight
};

// full frames resident on the device: dense rows (pitch 3 * W), one allocation per frame, and the source table of the launch
struct dh_frames {
  std::vector<uint8_t*> px;
  dh_crop_src* table = nullptr;
};

namespace {

int run_step(const Step& st, void* stream) {
  const unsigned char* p = st.payload.data();
  auto u = [&](int i) { uint64_t v; std::memcpy(&v, p + 8 * i, 8); return v; };
  auto P = [&](int i) { return reinterpret_cast<float*>(static_cast<uintptr_t>(u(i))); };
  auto I = [&](int i) { return static_cast<int>(static_cast<int64_t>(u(i))); };
  auto Fl = [&](int i) { float f; std::memcpy(&f, p + 8 * i, 4); return f; };
  switch (st.fn) {
    case F_CONV: {
      int64_t cfg;
      std::memcpy(&cfg, p + sizeof(dh_conv_args), 8);
      return dh_conv2d_f32(reinterpret_cast<const dh_conv_args*>(p), (int)cfg, stream);
    }
    case F_SAMCTX: {
      const unsigned char* e = p + sizeof(dh_sam_args);
      int64_t J, nctx, ldy;
      float alpha;
      void* y;
      std::memcpy(&J, e, 8); std::memcpy(&nctx, e + 8, 8); std::memcpy(&alpha, e + 16, 4);
      std::memcpy(&y, e + 24, 8); std::memcpy(&ldy, e + 32, 8);
      return dh_softargmax2d_context_f32(reinterpret_cast<const dh_sam_args*>(p), (int)J, (int)nctx, alpha,
                                         static_cast<float*>(y), (int)ldy, stream);
    }
    case F_DW: return dh_dwconv2d_f32(reinterpret_cast<const dh_dw_args*>(p), stream);
    case F_DWS: return dh_dwconv2d_strided_f32(reinterpret_cast<const dh_dw_strided*>(p), stream);
    case F_CONVT: {
      int64_t cfg;
      std::memcpy(&cfg, p + sizeof(dh_conv_transpose), 8);
      return dh_conv2d_transpose2x2_f32(reinterpret_cast<const dh_conv_transpose*>(p), (int)cfg, stream);
    }
    case F_CONVTS: {
      int64_t parts, cfg;
      std::memcpy(&parts, p + sizeof(dh_conv_transpose), 8);
      std::memcpy(&cfg, p + sizeof(dh_conv_transpose) + 8, 8);
      return dh_conv2d_transpose2x2_split_f32(reinterpret_cast<const dh_conv_transpose*>(p), (int)parts, (int)cfg, stream);
    }
    case F_GROUP:
      return dh_conv2d_dw_group_f32(reinterpret_cast<const dh_conv_args*>(p),
                                    reinterpret_cast<const dh_dw_args*>(p + sizeof(dh_conv_args)), stream);
    case F_PAIR:
      return dh_conv2d_pair_f32(reinterpret_cast<const dh_conv_args*>(p), reinterpret_cast<const dh_conv_args*>(p + sizeof(dh_conv_args)),
                                stream);
    case F_SEG:
      return dh_conv2d_seg_f32(reinterpret_cast<const dh_conv_args*>(p), reinterpret_cast<const dh_conv_seg*>(p + sizeof(dh_conv_args)),
                               stream);
    case F_POOL: return dh_pool2d_f32(reinterpret_cast<const dh_pool_args*>(p), stream);
    case F_ELT: return dh_eltwise_f32(reinterpret_cast<const dh_elt_args*>(p), stream);
    case F_SAM: return dh_softargmax2d_f32(reinterpret_cast<const dh_sam_args*>(p), stream);
    case F_UPADD: return dh_upsample2x_add_f32(P(0), I(1), P(2), I(3), P(4), I(5), I(6), I(7), I(8), I(9), stream);
    case F_CTX: return dh_context_aggregation_f32(P(0), P(1), P(2), P(3), I(4), I(5), I(6), Fl(7), I(8), stream);
    case F_DMEANS: return dh_depth_means_f32(P(0), I(1), P(2), P(3), I(4), I(5), I(6), I(7), stream);
    case F_SAM1D: return dh_softargmax1d_f32(P(0), P(1), P(2), I(3), P(4), I(5), I(6), I(7), stream);
    case F_KRON: return dh_kronecker_f32(P(0), I(1), P(2), I(3), P(4), I(5), I(6), I(7), I(8), I(9), stream);
    case F_GMM: return dh_global_maxmin_softmax_f32(P(0), I(1), P(2), I(3), I(4), I(5), I(6), stream);
    case F_COPY: return dh_copy_channels_f32(P(0), I(1), P(2), I(3), static_cast<int64_t>(u(4)), I(5), stream);
    case F_ZPAD: return dh_zeropad2d_f32(P(0), P(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), stream);
    case F_DFM: return dh_depth_from_maps_f32(P(0), I(1), P(2), I(3), P(4), I(5), I(6), I(7), I(8), stream);
    case F_NORM: return dh_normalize_u8_f32(reinterpret_cast<const uint8_t*>(P(0)), P(1), P(2), static_cast<int64_t>(u(3)),
                                            I(4), stream);
  }
  return DH_EINVAL;
}

}  // namespace

extern "C" {

int dh_plan_inspect(const void* blob, size_t bytes, dh_plan_info* out) {
  PlanImage im;
  if (out == nullptr) return DH_EINVAL;
  const int rc = plan_parse(blob, bytes, &im);
  if (rc == DH_OK) *out = im.info;
  return rc;
}

int dh_plan_record(int fn, const char** name, int* first_version, size_t* payload_bytes, int32_t* offsets, int max_offsets,
                   int* num_offsets) {
  if (fn < 0 || fn >= F_COUNT || name == nullptr || first_version == nullptr || payload_bytes == nullptr || num_offsets == nullptr ||
      max_offsets < 0 || (max_offsets > 0 && offsets == nullptr))
    return DH_EINVAL;
  const Record& rec = kRecords[fn];
  *name = rec.name;
  *first_version = (int)rec.first_version;
  *payload_bytes = rec.bytes;
  *num_offsets = (int)rec.nptr;
  for (int k = 0; k < max_offsets && k < (int)rec.nptr; ++k) offsets[k] = rec.ptr[k];
  return DH_OK;
}

// every malformed blob is refused (DH_EINVAL) before the first allocation; DH_ELAUNCH is a failed HIP call on a well-formed one
int dh_plan_create(const void* blob, size_t blob_bytes, dh_plan** out) {
  PlanImage im;
  if (out == nullptr || plan_parse(blob, blob_bytes, &im) != DH_OK) return DH_EINVAL;
  dh_plan* pl = new dh_plan();
  auto fail = [&](int rc) { dh_plan_destroy(pl); return rc; };
  const dh_plan_info& h = im.info;
  pl->n = h.batch;
  if (hipMalloc(&pl->arena, h.arena_bytes ? h.arena_bytes : 16) != hipSuccess) return fail(DH_ELAUNCH);
  if (hipMalloc(&pl->weights, h.weight_bytes ? h.weight_bytes : 16) != hipSuccess) return fail(DH_ELAUNCH);
  if (h.weight_bytes && hipMemcpy(pl->weights, im.weights, h.weight_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(DH_ELAUNCH);
  if (h.byte_bytes && hipMalloc(&pl->bytes, h.byte_bytes) != hipSuccess) return fail(DH_ELAUNCH);
  for (const PlanIn& in : im.ins)           // float inputs land in the arena, uint8 frames in region 3
    pl->ins.push_back(In{(size_t)in.items, in.u8, (in.u8 ? pl->bytes : pl->arena) + (in.tag & kPlanOffMask)});
  pl->outs = im.outs;
  // copy the step records and patch their pointers (once)
  for (const PlanStep& ps : im.steps) {
    Step st{ps.fn, std::vector<unsigned char>(ps.payload, ps.payload + ps.bytes)};
    if (plan_patch(st.payload.data(), kRecords[ps.fn], pl->arena, pl->weights, pl->bytes) != DH_OK) return fail(DH_EINVAL);
    pl->steps.push_back(std::move(st));
  }
  pl->ops.swap(im.ops);
  // a multi-stream plan's own streams and events: nstreams - 1 non-blocking streams (sched_build bounds nstreams by 4: the
  // hardware queues of a process), fork + joins + one event per recording entry + relays
  for (int k = 1; k < im.info.nstreams; ++k) {
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(DH_ELAUNCH);
    pl->side.push_back(st);
  }
  for (int e = 0; e < im.info.num_events; ++e) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return fail(DH_ELAUNCH);
    pl->events.push_back(ev);
  }
  *out = pl;
  return DH_OK;
}

int dh_plan_destroy(dh_plan* pl) {
  if (pl == nullptr) return DH_OK;
  if (pl->stream) hipStreamSynchronize(pl->stream);
  for (hipStream_t st : pl->side) hipStreamSynchronize(st);
  for (hipEvent_t ev : pl->events) hipEventDestroy(ev);
  for (hipStream_t st : pl->side) hipStreamDestroy(st);
  for (float* q : pl->in_dev) hipFree(q);
  if (pl->out_stage) hipFree(pl->out_stage);
  if (pl->out_host) hipHostFree(pl->out_host);
  if (pl->stream) hipStreamDestroy(pl->stream);
  if (pl->arena) hipFree(pl->arena);
  if (pl->weights) hipFree(pl->weights);
  if (pl->bytes) hipFree(pl->bytes);
  if (pl->crop_prog) hipFree(pl->crop_prog);
  if (pl->crop_jobs) hipFree(pl->crop_jobs);
  if (pl->refine_buf) hipFree(pl->refine_buf);
  if (pl->boxes_buf) hipFree(pl->boxes_buf);
  delete pl;
  return DH_OK;
}

int dh_plan_batch(const dh_plan* pl) { return pl ? pl->n : 0; }
int dh_plan_num_inputs(const dh_plan* pl) { return pl ? (int)pl->ins.size() : 0; }
int dh_plan_num_outputs(const dh_plan* pl) { return pl ? (int)pl->outs.size() : 0; }
int64_t dh_plan_input_items(const dh_plan* pl, int i) {
  return (pl && i >= 0 && i < (int)pl->ins.size()) ? (int64_t)pl->ins[i].items : -1;
}
int dh_plan_input_is_u8(const dh_plan* pl, int i) {
  return (pl && i >= 0 && i < (int)pl->ins.size()) ? pl->ins[i].u8 : -1;
}
int64_t dh_plan_output_items(const dh_plan* pl, int i) {
  return (pl && i >= 0 && i < (int)pl->outs.size()) ? (int64_t)(pl->outs[i].npix * pl->outs[i].C) : -1;
}
int dh_plan_output_channels(const dh_plan* pl, int i) { return (pl && i >= 0 && i < (int)pl->outs.size()) ? pl->outs[i].C : -1; }

float* dh_plan_input_ptr(const dh_plan* pl, int i) {
  return (pl && i >= 0 && i < (int)pl->ins.size() && pl->ins[i].u8 == 0) ? reinterpret_cast<float*>(pl->ins[i].dst) : nullptr;
}

int dh_forward(dh_plan* pl, const float* const* inputs, int m, float* const* outputs, void* stream) {
  if (pl == nullptr || inputs == nullptr || outputs == nullptr || m <= 0 || m > pl->n) return DH_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (size_t i = 0; i < pl->ins.size(); ++i) {
    if (inputs[i] == nullptr) return DH_EINVAL;
    const In& in = pl->ins[i];
    if (reinterpret_cast<const char*>(inputs[i]) == in.dst) continue;     // written in place (dh_plan_input_ptr)
    if (hipMemcpyAsync(in.dst, inputs[i], in.items * (in.u8 ? 1 : 4) * (size_t)m, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return DH_ELAUNCH;
  }
  if (pl->ops.empty()) {
    for (const Step& st : pl->steps) {
      const int rc = run_step(st, stream);
      if (rc != DH_OK) return rc;
    }
  } else {
    // the enqueue program of plan_sched.h: stream 0 is the caller's.  The input copies above and the staging launches at
    // the head of the program run before the fork; the pack launch below runs behind the join.
    auto S = [&](int k) { return k == 0 ? s : pl->side[(size_t)k - 1]; };
    int rc = DH_OK;
    bool forked = false;
    for (const dh_sched_op& op : pl->ops) {
      if (op.kind == DH_SCHED_LAUNCH) rc = run_step(pl->steps[(size_t)op.arg], S(op.stream));
      else if (op.kind == DH_SCHED_RECORD) rc = hipEventRecord(pl->events[(size_t)op.arg], S(op.stream)) == hipSuccess ? DH_OK : DH_ELAUNCH;
      else rc = hipStreamWaitEvent(S(op.stream), pl->events[(size_t)op.arg], 0) == hipSuccess ? DH_OK : DH_ELAUNCH;
      if (rc != DH_OK) break;
      forked = forked || op.kind != DH_SCHED_LAUNCH;          // (the first op that is no launch is the fork's record)
    }
    if (rc != DH_OK) {
      // whatever the side streams were given so far is ordered before the caller's next work: join them anyway
      for (size_t k = 0; forked && k < pl->side.size(); ++k)
        if (hipEventRecord(pl->events[k + 1], pl->side[k]) == hipSuccess) hipStreamWaitEvent(s, pl->events[k + 1], 0);
      return rc;
    }
  }
  pl->segs.clear();
  for (size_t i = 0; i < pl->outs.size(); ++i) {
    const Out& o = pl->outs[i];
    if (outputs[i] == nullptr) continue;                      // an output the caller does not want
    pl->segs.push_back(dh_out_seg{reinterpret_cast<const float*>(pl->arena + o.off), outputs[i], (int64_t)o.npix * m, o.C, o.ld});
  }
  return dh_pack_outputs_f32(pl->segs.data(), (int)pl->segs.size(), stream);
}

int dh_plan_num_streams(const dh_plan* pl) { return pl ? 1 + (int)pl->side.size() : 0; }
void* dh_plan_side_stream(const dh_plan* pl, int k) {
  return (pl && k >= 1 && k <= (int)pl->side.size()) ? pl->side[(size_t)k - 1] : nullptr;
}

int dh_sched_build_ops(int n, const int32_t* step, const int32_t* stream, const int32_t* record, const int32_t* wait_off,
                       const int32_t* waits, int nwaits, int nstreams, int npre, int nsteps, dh_sched_op* ops, int max_ops,
                       int* nops, int* nevents) {
  if (nops == nullptr || nevents == nullptr || max_ops < 0 || (max_ops > 0 && ops == nullptr)) return DH_EINVAL;
  const dh::SchedTable tab = {n, step, stream, record, wait_off, waits, nwaits, nstreams, npre, nsteps};
  dh::SchedProgram prog;
  const int rc = dh::sched_build(tab, &prog);
  if (rc != DH_OK) return rc;
  *nops = (int)prog.ops.size();
  *nevents = prog.nevents;
  for (int i = 0; i < max_ops && i < *nops; ++i) ops[i] = prog.ops[(size_t)i];
  return DH_OK;
}

}  // extern "C"

namespace {

// dh_forward_host / dh_forward_frames_host: the internal stream and the staging buffers, on first use.  Built in locals and
// committed only when every allocation succeeded: a failure part-way leaves the plan as it was (the next call tries again)
// instead of with short in_dev / out_dev vectors
int host_staging(dh_plan* pl) {
  if (pl->stream != nullptr) return DH_OK;
  hipStream_t st = nullptr;
  std::vector<float*> in_dev;
  float* out_stage = nullptr;
  float* out_host = nullptr;
  bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
  for (size_t i = 0; ok && i < pl->ins.size(); ++i) {
    float* q = nullptr;
    ok = hipMalloc(&q, pl->ins[i].items * (pl->ins[i].u8 ? 1 : 4) * (size_t)pl->n) == hipSuccess;
    if (ok) in_dev.push_back(q);
  }
  size_t stage = 0;                                         // floats: every output of a full batch, each from a 16-byte boundary
  for (const Out& o : pl->outs) stage += stage_floats(o, pl->n);
  ok = ok && hipMalloc(&out_stage, stage * 4) == hipSuccess;
  ok = ok && hipHostMalloc(&out_host, stage * 4, hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    for (float* q : in_dev) hipFree(q);
    if (out_stage) hipFree(out_stage);
    if (out_host) hipHostFree(out_host);
    if (st) hipStreamDestroy(st);
    return DH_ELAUNCH;
  }
  pl->in_dev.swap(in_dev);
  pl->out_stage = out_stage;
  pl->out_host = out_host;
  pl->stream = st;
  return DH_OK;
}

// the wanted outputs of THIS call back to back in the staging buffer (the pack launch of dh_forward writes them there);
// returns the floats used
size_t place_outputs(dh_plan* pl, float* const* outputs_host, int m) {
  pl->out_ptr.assign(pl->outs.size(), nullptr);
  size_t used = 0;
  for (size_t i = 0; i < pl->outs.size(); ++i)
    if (outputs_host[i] != nullptr) {
      pl->out_ptr[i] = pl->out_stage + used;
      used += stage_floats(pl->outs[i], m);
    }
  return used;
}

// ONE device-to-host copy of exactly those floats, the wait, then a host-side scatter
int fetch_outputs(dh_plan* pl, float* const* outputs_host, int m, size_t used) {
  if (used != 0 && hipMemcpyAsync(pl->out_host, pl->out_stage, used * 4, hipMemcpyDeviceToHost, pl->stream) != hipSuccess)
    return DH_ELAUNCH;
  if (hipStreamSynchronize(pl->stream) != hipSuccess) return DH_ELAUNCH;
  for (size_t i = 0; i < pl->outs.size(); ++i)
    if (outputs_host[i] != nullptr)
      std::memcpy(outputs_host[i], pl->out_host + (pl->out_ptr[i] - pl->out_stage), pl->outs[i].npix * pl->outs[i].C * 4 * (size_t)m);
  return DH_OK;
}

// a device buffer of the plan that only grows: `*have` elements of `elem` bytes now, at least `need` afterwards.  A failure
// leaves no buffer (the next call tries again).  (hipFree waits for the device: a forward still reading the old one finishes first)
template <typename T>
int grow(T** buf, size_t* have, size_t need, size_t elem) {
  if (*have >= need) return DH_OK;
  if (*buf) hipFree(*buf);
  *buf = nullptr;
  *have = 0;
  if (hipMalloc(reinterpret_cast<void**>(buf), need * elem) != hipSuccess) return DH_ELAUNCH;
  *have = need;
  return DH_OK;
}

// the ONE build -> crop -> forward sequence of dh_forward_frames, dh_refine_frames_host and dh_frame_boxes_host, on `stream`:
// room for the plan's device crop program (one allocation per plan, large enough for a FULL batch of `per_item` frames over the
// frames of `f`), dh_crop_program_build_dev from `njobs` resident jobs (per-job status to `status` unless null), ONE crop
// launch straight into the plan's uint8 input, then the forward of m items with that input in place.
int crop_forward(dh_plan* pl, const dh_frames* f, const dh_crop_job* jobs_dev, int njobs, int per_item, int m, int OH, int OW,
                 int32_t* status, float* const* outputs_dev, void* stream) {
  size_t need = 0;
  int rc = dh_crop_program_max_bytes(pl->n * per_item, (int)f->px.size(), OH, OW, &need);
  if (rc == DH_OK) rc = grow(&pl->crop_prog, &pl->crop_prog_bytes, need, 1);
  if (rc != DH_OK) return rc;
  const In& in = pl->ins[0];
  rc = dh_crop_program_build_dev(f->table, (int)f->px.size(), jobs_dev, njobs, OH, OW, pl->crop_prog, pl->crop_prog_bytes, status,
                                 stream);
  if (rc != DH_OK) return rc;
  rc = dh_crop_resize_u8(pl->crop_prog, njobs, OH, OW, reinterpret_cast<uint8_t*>(in.dst), (int64_t)OH * OW * 3, stream);
  if (rc != DH_OK) return rc;
  const float* inputs[1] = {reinterpret_cast<const float*>(in.dst)};  // written in place: dh_forward skips the input copy
  return dh_forward(pl, inputs, m, outputs_dev, stream);
}

// the plan's device job table, large enough for a FULL batch of `per_item` frames, with `njobs` jobs of the host on their way
int upload_jobs(dh_plan* pl, const dh_crop_job* jobs_host, int njobs, int per_item) {
  const int rc = grow(&pl->crop_jobs, &pl->crop_jobs_n, (size_t)pl->n * (size_t)per_item, sizeof(dh_crop_job));
  if (rc != DH_OK) return rc;
  return hipMemcpyAsync(pl->crop_jobs, jobs_host, (size_t)njobs * sizeof(dh_crop_job), hipMemcpyHostToDevice, pl->stream) == hipSuccess
             ? DH_OK : DH_ELAUNCH;
}

// how a *_host entry point ends: behind a refusal nothing of the call stays in flight; else the wait for its copies (`copies_ok`)
int finish(dh_plan* pl, int rc, bool copies_ok) {
  const bool synced = hipStreamSynchronize(pl->stream) == hipSuccess;
  if (rc != DH_OK) return rc;
  return synced && copies_ok ? DH_OK : DH_ELAUNCH;
}

// dh_forward_frames_shape of this plan: the items `njobs` crops of OH x OW x 3 bytes fill and the frames per item, or DH_EINVAL
int frames_shape(const dh_plan* pl, int njobs, int OH, int OW, int* m, int* per_item) {
  if (pl == nullptr || pl->ins.size() != 1) return DH_EINVAL;
  return dh_forward_frames_shape((int)pl->ins.size(), pl->ins[0].u8, (int64_t)pl->ins[0].items, pl->n, njobs, OH, OW, m, per_item);
}

}  // namespace

extern "C" {

int dh_forward_host(dh_plan* pl, const float* const* inputs_host, int m, float* const* outputs_host) {
  if (pl == nullptr || inputs_host == nullptr || outputs_host == nullptr || m <= 0 || m > pl->n) return DH_EINVAL;
  int rc = host_staging(pl);
  if (rc != DH_OK) return rc;
  for (size_t i = 0; i < pl->ins.size(); ++i)
    if (hipMemcpyAsync(pl->in_dev[i], inputs_host[i], pl->ins[i].items * (pl->ins[i].u8 ? 1 : 4) * (size_t)m,
                       hipMemcpyHostToDevice, pl->stream) != hipSuccess)
      return DH_ELAUNCH;
  const size_t used = place_outputs(pl, outputs_host, m);
  rc = dh_forward(pl, pl->in_dev.data(), m, pl->out_ptr.data(), pl->stream);
  if (rc != DH_OK) return rc;
  return fetch_outputs(pl, outputs_host, m, used);
}

// ---- frames ----------------------------------------------------------------------------------------------------------------
int dh_frames_create(const dh_crop_src* frames_host, int n, dh_frames** out) {
  if (frames_host == nullptr || out == nullptr || n < 1) return DH_EINVAL;
  for (int i = 0; i < n; ++i)
    if (!dh::crop_src_ok(frames_host[i])) return DH_EINVAL;             // before anything is allocated
  dh_frames* f = new dh_frames();
  std::vector<dh_crop_src> table((size_t)n);
  bool ok = true;
  for (int i = 0; ok && i < n; ++i) {
    const dh_crop_src& h = frames_host[i];
    const size_t row = (size_t)3 * (size_t)h.W;
    uint8_t* d = nullptr;
    ok = hipMalloc(&d, row * (size_t)h.H) == hipSuccess;
    if (ok) f->px.push_back(d);
    ok = ok && hipMemcpy2D(d, row, h.ptr, (size_t)h.pitch, row, (size_t)h.H, hipMemcpyHostToDevice) == hipSuccess;
    table[(size_t)i] = dh_crop_src{d, (int64_t)row, h.H, h.W};
  }
  ok = ok && hipMalloc(&f->table, (size_t)n * sizeof(dh_crop_src)) == hipSuccess;
  ok = ok && hipMemcpy(f->table, table.data(), (size_t)n * sizeof(dh_crop_src), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    dh_frames_destroy(f);
    return DH_ELAUNCH;
  }
  *out = f;
  return DH_OK;
}

int dh_frames_destroy(dh_frames* f) {
  if (f == nullptr) return DH_OK;
  for (uint8_t* d : f->px) hipFree(d);
  if (f->table) hipFree(f->table);
  delete f;
  return DH_OK;
}

int dh_frames_count(const dh_frames* f) { return f ? (int)f->px.size() : 0; }
const dh_crop_src* dh_frames_table_dev(const dh_frames* f) { return f ? f->table : nullptr; }

int dh_forward_frames_shape(int num_inputs, int input_is_u8, int64_t input_items, int batch, int njobs, int OH, int OW, int* m,
                            int* per_item) {
  if (num_inputs != 1 || input_is_u8 != 1 || input_items < 1 || batch < 1 || njobs < 1 || OH < 1 || OW < 1 ||
      OH > dh::kCropMaxExtent || OW > dh::kCropMaxExtent)
    return DH_EINVAL;
  const int64_t crop = (int64_t)OH * OW * 3;
  if (input_items % crop != 0) return DH_EINVAL;                         // the input is no stack of [OH, OW, 3] frames
  const int64_t per = input_items / crop;
  if (per > 0x7fffffff / batch || njobs % per != 0 || njobs / per > batch) return DH_EINVAL;
  if (m != nullptr) *m = (int)(njobs / per);
  if (per_item != nullptr) *per_item = (int)per;
  return DH_OK;
}

int dh_forward_frames(dh_plan* pl, const dh_frames* f, const dh_crop_job* jobs_dev, int njobs, int OH, int OW,
                      float* const* outputs_dev, void* stream) {
  if (pl == nullptr || f == nullptr || jobs_dev == nullptr || outputs_dev == nullptr) return DH_EINVAL;
  int m = 0, per_item = 0;
  int rc = frames_shape(pl, njobs, OH, OW, &m, &per_item);
  if (rc != DH_OK) return rc;
  return crop_forward(pl, f, jobs_dev, njobs, per_item, m, OH, OW, nullptr, outputs_dev, stream);
}

int dh_forward_frames_host(dh_plan* pl, const dh_frames* f, const dh_crop_job* jobs_host, int njobs, int OH, int OW,
                           float* const* outputs_host) {
  if (pl == nullptr || f == nullptr || jobs_host == nullptr || outputs_host == nullptr) return DH_EINVAL;
  int m = 0, per_item = 0;
  int rc = frames_shape(pl, njobs, OH, OW, &m, &per_item);
  if (rc != DH_OK) return rc;
  size_t bytes = 0;                                                    // the host builder's answer to this very table, first
  rc = dh::crop_program_bytes(jobs_host, njobs, (int)f->px.size(), OH, OW, &bytes);
  if (rc != DH_OK) return rc;
  rc = host_staging(pl);
  if (rc != DH_OK) return rc;
  rc = upload_jobs(pl, jobs_host, njobs, per_item);
  if (rc != DH_OK) return rc;
  const size_t used = place_outputs(pl, outputs_host, m);
  rc = crop_forward(pl, f, pl->crop_jobs, njobs, per_item, m, OH, OW, nullptr, pl->out_ptr.data(), pl->stream);
  if (rc != DH_OK) return rc;
  return fetch_outputs(pl, outputs_host, m, used);
}

// ---- the box-refinement loop of one batch, boxes resident on the device ----------------------------------------------------------
int dh_refine_frames_host(dh_plan* pl, const dh_frames* f, const int32_t* src, const double* boxes0, int n, int OH, int OW, int outidx,
                          int num_iter, double winsize_scale, double momentum, float* poses_out, dh_crop_job* jobs_out,
                          int32_t* status_out) {
  if (pl == nullptr || f == nullptr || src == nullptr || boxes0 == nullptr || poses_out == nullptr || jobs_out == nullptr ||
      status_out == nullptr || pl->ins.size() != 1 || outidx < 0 || outidx >= (int)pl->outs.size())
    return DH_EINVAL;
  const Out& o = pl->outs[(size_t)outidx];
  int J = 0;
  int rc = dh::refine_frames_shape((int)pl->ins.size(), pl->ins[0].u8, (int64_t)pl->ins[0].items, pl->n, n, OH, OW, (int)pl->outs.size(),
                                   outidx, (int64_t)(o.npix * (size_t)o.C), o.C, num_iter, &J);
  if (rc != DH_OK) return rc;
  if ((int64_t)num_iter * pl->n > 0x7fffffff / 64) return DH_EINVAL;
  rc = host_staging(pl);
  if (rc != DH_OK) return rc;
  // one allocation for a full batch: boxes | jobs of every iteration | status of every iteration | src | poses of every iteration
  const size_t N = (size_t)pl->n, T = (size_t)num_iter;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t pose_floats = stage_floats(o, pl->n);                   // per iteration, a 16-byte multiple
  const size_t off_jobs = up16(32 * N), off_status = off_jobs + up16(sizeof(dh_crop_job) * N * T);
  const size_t off_src = off_status + up16(4 * N * T), off_poses = off_src + up16(4 * N);
  const size_t need = off_poses + pose_floats * 4 * T;
  rc = grow(&pl->refine_buf, &pl->refine_bytes, need, 1);
  if (rc != DH_OK) return rc;
  double* boxes = reinterpret_cast<double*>(pl->refine_buf);
  dh_crop_job* jobs = reinterpret_cast<dh_crop_job*>(pl->refine_buf + off_jobs);
  int32_t* status = reinterpret_cast<int32_t*>(pl->refine_buf + off_status);
  int32_t* src_dev = reinterpret_cast<int32_t*>(pl->refine_buf + off_src);
  float* poses = reinterpret_cast<float*>(pl->refine_buf + off_poses);
  hipStream_t s = pl->stream;
  if (hipMemcpyAsync(boxes, boxes0, 32 * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(src_dev, src, 4 * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess)
    return DH_ELAUNCH;
  rc = dh_jobs_from_boxes_f64(boxes, src_dev, n, jobs, s);
  if (rc != DH_OK) return rc;
  const float* view = reinterpret_cast<const float*>(pl->arena + o.off);
  for (int t = 0; rc == DH_OK && t < num_iter; ++t) {
    dh_crop_job* jt = jobs + (size_t)t * (size_t)n;
    pl->out_ptr.assign(pl->outs.size(), nullptr);                      // only the pose output is packed
    pl->out_ptr[(size_t)outidx] = poses + (size_t)t * pose_floats;
    rc = crop_forward(pl, f, jt, n, 1, n, OH, OW, status + (size_t)t * (size_t)n, pl->out_ptr.data(), s);
    // the next window from the poses where the forward left them: same stream, behind the plan's join -- no event
    if (rc == DH_OK && t + 1 < num_iter)
      rc = dh_refine_boxes_f64(view, (int64_t)o.npix * o.ld, o.ld, J, jt, boxes, n, winsize_scale, momentum, boxes, jt + n, s);
  }
  if (rc != DH_OK) return finish(pl, rc, false);
  const size_t item_floats = o.npix * (size_t)o.C * (size_t)n;
  bool ok = true;
  for (int t = 0; ok && t < num_iter; ++t)
    ok = hipMemcpyAsync(poses_out + (size_t)t * item_floats, poses + (size_t)t * pose_floats, item_floats * 4, hipMemcpyDeviceToHost, s) ==
         hipSuccess;
  ok = ok && hipMemcpyAsync(jobs_out, jobs, sizeof(dh_crop_job) * (size_t)n * T, hipMemcpyDeviceToHost, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(status_out, status, 4 * (size_t)n * T, hipMemcpyDeviceToHost, s) == hipSuccess;
  return finish(pl, DH_OK, ok);
}

// ---- the per-frame person-box pass of one batch: only the boxes and their status leave the device ---------------------------------
int dh_frame_boxes_host(dh_plan* pl, const dh_frames* f, const int32_t* src, const int32_t* windows, int n, int OH, int OW, int outidx,
                        double relsize, int32_t* boxes_out, double* boxes_f64_out, int32_t* status_out) {
  if (pl == nullptr || f == nullptr || src == nullptr || windows == nullptr || boxes_out == nullptr || boxes_f64_out == nullptr ||
      status_out == nullptr || pl->ins.size() != 1 || outidx < 0 || outidx >= (int)pl->outs.size())
    return DH_EINVAL;
  const Out& o = pl->outs[(size_t)outidx];
  int J = 0;
  int rc = dh::frame_boxes_shape((int)pl->ins.size(), pl->ins[0].u8, (int64_t)pl->ins[0].items, pl->n, n, OH, OW, (int)pl->outs.size(),
                                 outidx, (int64_t)(o.npix * (size_t)o.C), o.C, &J);
  if (rc != DH_OK) return rc;
  std::vector<dh_crop_job>& jobs_host = pl->boxes_jobs;                // (outlives the upload: ONE synchronisation, at the end)
  jobs_host.resize((size_t)n);
  for (int i = 0; i < n; ++i)
    jobs_host[(size_t)i] = dh_crop_job{src[i], windows[4 * i], windows[4 * i + 1], windows[4 * i + 2], windows[4 * i + 3], 0};
  size_t bytes = 0;                                                    // the host builder's answer to this very table, first
  rc = dh::crop_program_bytes(jobs_host.data(), n, (int)f->px.size(), OH, OW, &bytes);
  if (rc != DH_OK) return rc;
  rc = host_staging(pl);
  if (rc != DH_OK) return rc;
  // one allocation for a full batch: float64 boxes | int32 boxes | status
  const size_t N = (size_t)pl->n;
  rc = grow(&pl->boxes_buf, &pl->boxes_bytes, 52 * N, 1);
  if (rc != DH_OK) return rc;
  double* boxf = reinterpret_cast<double*>(pl->boxes_buf);
  int32_t* box = reinterpret_cast<int32_t*>(pl->boxes_buf + 32 * N);
  int32_t* status = reinterpret_cast<int32_t*>(pl->boxes_buf + 48 * N);
  hipStream_t s = pl->stream;
  rc = upload_jobs(pl, jobs_host.data(), n, 1);
  if (rc != DH_OK) return rc;
  const float* view = reinterpret_cast<const float*>(pl->arena + o.off);
  pl->out_ptr.assign(pl->outs.size(), nullptr);                        // no output is packed: the poses are read in the arena
  rc = crop_forward(pl, f, pl->crop_jobs, n, 1, n, OH, OW, nullptr, pl->out_ptr.data(), s);
  // the boxes from the poses where the forward left them: same stream, behind the plan's join -- no event
  if (rc == DH_OK)
    rc = dh_pose_boxes_f64(view, (int64_t)o.npix * o.ld, (int64_t)o.npix * o.ld, o.ld, 1, J, o.C - 2, pl->crop_jobs, 1, n, relsize, box,
                           boxf, status, s);
  if (rc != DH_OK) return finish(pl, rc, false);
  bool ok = hipMemcpyAsync(boxes_out, box, 16 * (size_t)n, hipMemcpyDeviceToHost, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(boxes_f64_out, boxf, 32 * (size_t)n, hipMemcpyDeviceToHost, s) == hipSuccess;
  ok = ok && hipMemcpyAsync(status_out, status, 4 * (size_t)n, hipMemcpyDeviceToHost, s) == hipSuccess;
  return finish(pl, DH_OK, ok);
}

}  // extern "C"

namespace dh {

// clip.hip: where output i of a plan lies in its arena ([n * npix, C] floats at pixel pitch ld)
const float* plan_output_view(const dh_plan* pl, int i, int* ld, int* C, int64_t* npix) {
  if (pl == nullptr || i < 0 || i >= (int)pl->outs.size()) return nullptr;
  const Out& o = pl->outs[i];
  *ld = o.ld; *C = o.C; *npix = (int64_t)o.npix;
  return reinterpret_cast<const float*>(pl->arena + o.off);
}

}  // namespace dh
