// The 'DHPL' plan blob (written by deephar_amd/engine/serialize.py, format documented there) as pure functions: the table of
// step records -- one row per function id: entry point, first blob version that knows it, payload bytes, where the payload
// holds pointers -- the parser, and the one loop that turns tagged pointers into addresses.  No HIP header, no allocation on
// a device, no byte read outside the blob.  dh_plan_create (plan.hip) parses with this before its first hipMalloc,
// dh_plan_inspect / dh_plan_record answer the host tests from it, and tools/plan_blob_sweep.cpp runs it stand-alone for a
// sanitizer build, so nobody restates the format.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "deephar_hip.h"
#include "plan_sched.h"

namespace dh {

// function ids of a step record: the index into serialize.ALL_FUNCTIONS
enum Fn { F_CONV, F_DW, F_POOL, F_UPADD, F_ELT, F_SAM, F_CTX, F_DMEANS, F_SAM1D, F_KRON, F_GMM, F_COPY, F_ZPAD, F_DFM, F_SAMCTX, F_NORM, F_GROUP, F_PAIR, F_SEG, F_DWS, F_CONVT, F_CONVTS, F_COUNT };

constexpr int kPlanMaxPtrs = 24;
struct Record {
  const char* name;             // the entry point run_step calls
  uint32_t first_version;       // blobs below it refuse the id
  uint32_t bytes;               // payload: the argument structs back to back, then one u64 per further argument
  uint32_t nptr;
  uint16_t ptr[kPlanMaxPtrs];   // byte offsets of the payload's pointer slots
};

template <typename... Off>
constexpr Record record(const char* name, uint32_t first_version, size_t bytes, Off... ptr) {
  static_assert(sizeof...(Off) <= kPlanMaxPtrs, "kPlanMaxPtrs");
  return Record{name, first_version, (uint32_t)bytes, (uint32_t)sizeof...(Off), {(uint16_t)ptr...}};
}

// the pointer fields of an argument struct that starts at byte `at` of its payload
#define DH_P(T, at, f) ((at) + offsetof(T, f))
#define DH_CONV_PTRS(at)                                                                                                       \
  DH_P(dh_conv_args, at, x), DH_P(dh_conv_args, at, w), DH_P(dh_conv_args, at, y), DH_P(dh_conv_args, at, pre_scale),         \
      DH_P(dh_conv_args, at, pre_shift), DH_P(dh_conv_args, at, post_scale), DH_P(dh_conv_args, at, post_shift),             \
      DH_P(dh_conv_args, at, res1), DH_P(dh_conv_args, at, res2), DH_P(dh_conv_args, at, in_lut), DH_P(dh_conv_args, at, y_pool)
#define DH_DW_PTRS(T, at) DH_P(T, at, x), DH_P(T, at, w), DH_P(T, at, y), DH_P(T, at, pre_scale), DH_P(T, at, pre_shift)
#define DH_CONVT_PTRS DH_DW_PTRS(dh_conv_transpose, 0), DH_P(dh_conv_transpose, 0, res)
#define DH_SAM_PTRS                                                                                                            \
  DH_P(dh_sam_args, 0, h), DH_P(dh_sam_args, 0, gx), DH_P(dh_sam_args, 0, gy), DH_P(dh_sam_args, 0, xy),                      \
      DH_P(dh_sam_args, 0, conf_raw), DH_P(dh_sam_args, 0, conf_prob), DH_P(dh_sam_args, 0, prob), DH_P(dh_sam_args, 0, gmax)

// Row i describes serialize.ALL_FUNCTIONS[i]; tests/test_plan_blob_host.py holds every row against the ctypes signatures the
// writer packs from.  Scalar arguments take 8 bytes each: argument k sits at 8 * k.
inline constexpr Record kRecords[F_COUNT] = {
    record("dh_conv2d_f32", 1, sizeof(dh_conv_args) + 8, DH_CONV_PTRS(0)),                            // + tile_cfg
    record("dh_dwconv2d_f32", 1, sizeof(dh_dw_args), DH_DW_PTRS(dh_dw_args, 0)),
    record("dh_pool2d_f32", 1, sizeof(dh_pool_args), DH_P(dh_pool_args, 0, x), DH_P(dh_pool_args, 0, y)),
    record("dh_upsample2x_add_f32", 1, 8 * 10, 8 * 0, 8 * 2, 8 * 4),                                   // a, lda, b, ldb, y, ldy, N, H, W, C
    record("dh_eltwise_f32", 1, sizeof(dh_elt_args), DH_P(dh_elt_args, 0, a), DH_P(dh_elt_args, 0, b), DH_P(dh_elt_args, 0, c),
           DH_P(dh_elt_args, 0, y), DH_P(dh_elt_args, 0, scale), DH_P(dh_elt_args, 0, shift)),
    record("dh_softargmax2d_f32", 1, sizeof(dh_sam_args), DH_SAM_PTRS),
    record("dh_context_aggregation_f32", 1, 8 * 9, 8 * 0, 8 * 1, 8 * 2, 8 * 3),                         // ys, yc, pc, y, F, J, nctx, alpha, ldy
    record("dh_depth_means_f32", 1, 8 * 8, 8 * 0, 8 * 2, 8 * 3),                                       // h, ldh, hxy, hz, F, HW, D, J
    record("dh_softargmax1d_f32", 1, 8 * 8, 8 * 0, 8 * 1, 8 * 2, 8 * 4),                               // hz, grid, z, ldz, vz, F, D, J
    record("dh_kronecker_f32", 1, 8 * 10, 8 * 0, 8 * 2, 8 * 4),                                        // hm, ldh, x, ldx, f, ldf, B, P, J, C
    record("dh_global_maxmin_softmax_f32", 1, 8 * 7, 8 * 0, 8 * 2),                                    // x, ldx, y, B, P, C, softmax
    record("dh_copy_channels_f32", 1, 8 * 6, 8 * 0, 8 * 2),                                            // x, ldx, y, ldy, npix, C
    record("dh_zeropad2d_f32", 1, 8 * 10, 8 * 0, 8 * 1),                                               // x, y, B, H, W, C, OH, OW, PT, PL
    record("dh_depth_from_maps_f32", 1, 8 * 9, 8 * 0, 8 * 2, 8 * 4),                                   // d, ldd, h, ldh, z, ldz, F, HW, J
    record("dh_softargmax2d_context_f32", 1, sizeof(dh_sam_args) + 8 * 5, DH_SAM_PTRS, sizeof(dh_sam_args) + 8 * 3),   // + J, nctx, agg_alpha, y, ldy
    record("dh_normalize_u8_f32", 1, 8 * 5, 8 * 0, 8 * 1, 8 * 2),                                      // x (bytes), lut, y, n_pixels, C
    record("dh_conv2d_dw_group_f32", 1, sizeof(dh_conv_args) + sizeof(dh_dw_args), DH_CONV_PTRS(0), DH_DW_PTRS(dh_dw_args, sizeof(dh_conv_args))),
    record("dh_conv2d_pair_f32", 1, 2 * sizeof(dh_conv_args), DH_CONV_PTRS(0), DH_CONV_PTRS(sizeof(dh_conv_args))),
    record("dh_conv2d_seg_f32", 1, sizeof(dh_conv_args) + sizeof(dh_conv_seg), DH_CONV_PTRS(0), DH_P(dh_conv_seg, sizeof(dh_conv_args), x2)),
    record("dh_dwconv2d_strided_f32", 3, sizeof(dh_dw_strided), DH_DW_PTRS(dh_dw_strided, 0)),
    record("dh_conv2d_transpose2x2_f32", 3, sizeof(dh_conv_transpose) + 8, DH_CONVT_PTRS),              // + tile_cfg
    record("dh_conv2d_transpose2x2_split_f32", 4, sizeof(dh_conv_transpose) + 8 * 2, DH_CONVT_PTRS),    // + parts, tile_cfg
};
#undef DH_P
#undef DH_CONV_PTRS
#undef DH_DW_PTRS
#undef DH_CONVT_PTRS
#undef DH_SAM_PTRS

// ---- the parsed blob: sizes and tables by value, steps and the weight image as pointers into the caller's bytes ---------------
constexpr uint32_t kPlanMaxVersion = 5;   // 3 = 2 + function ids 19, 20; 4 = 3 + id 21; 5 = 4 + a schedule section behind the steps
constexpr uint64_t kPlanOffMask = (1ull << 60) - 1;

struct PlanIn { uint64_t tag, items; int u8; };          // tag: (region << 60) | offset of the buffer dh_forward copies the input to
struct PlanOut { uint64_t off, npix; int C, ld; };
struct PlanStep { int fn; const unsigned char* payload; uint32_t bytes; };   // not copied; pointers still tagged
struct PlanImage {
  dh_plan_info info;
  std::vector<PlanIn> ins;
  std::vector<PlanOut> outs;
  std::vector<PlanStep> steps;
  std::vector<dh_sched_op> ops;           // version 5: the enqueue program (empty: every step in order on the caller's stream)
  const unsigned char* weights;           // info.weight_bytes bytes: the end of the blob
};

struct PlanReader {
  const unsigned char* p;
  const unsigned char* end;
  bool ok = true;
  template <typename T>
  T get() {
    T v{};
    if ((size_t)(end - p) < sizeof(T)) { ok = false; return v; }
    memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
  }
};

// a tagged pointer of the blob: 0 is NULL, region 1 (arena), 2 (weight image) or 3 (uint8 staging) needs an offset inside it
inline bool plan_tag_ok(uint64_t v, const dh_plan_info& h) {
  const uint64_t size[4] = {0, h.arena_bytes, h.weight_bytes, h.byte_bytes};
  return v == 0 || ((v >> 60) <= 3 && (v & kPlanOffMask) < size[v >> 60]);
}

// The schedule section of a version-5 blob: u32 nstreams | u32 npre | u32 #entries | u32 #waits | per entry u32 step
// (0xffffffff: no launch), u32 stream, u32 flags (bit 0: records an event), u32 #waits of the entry | the waits, entry by
// entry.  Validated and turned into the enqueue program by plan_sched.h.
inline int plan_parse_schedule(PlanReader& r, PlanImage* out) {
  const uint32_t ns = r.get<uint32_t>(), npre = r.get<uint32_t>(), nent = r.get<uint32_t>(), nwaits = r.get<uint32_t>();
  if (!r.ok || nent > (uint32_t)kSchedMaxEntries || ns > 0x7fffffffu || npre > nent || (uint64_t)(r.end - r.p) < 16ull * nent ||
      (uint64_t)(r.end - r.p) - 16ull * nent < 4ull * nwaits)
    return DH_EINVAL;
  std::vector<int32_t> step(nent), stream(nent), record(nent), wait_off(nent + 1, 0), waits(nwaits);
  uint64_t total = 0;
  for (uint32_t i = 0; i < nent; ++i) {
    step[i] = (int32_t)r.get<uint32_t>();
    const uint32_t s = r.get<uint32_t>(), flags = r.get<uint32_t>(), nw = r.get<uint32_t>();
    if (s >= ns || flags > 1 || (total += nw) > nwaits) return DH_EINVAL;
    stream[i] = (int32_t)s;
    record[i] = (int32_t)flags;
    wait_off[i + 1] = (int32_t)total;
  }
  if (total != nwaits) return DH_EINVAL;
  for (uint32_t k = 0; k < nwaits; ++k) waits[k] = (int32_t)r.get<uint32_t>();
  const SchedTable tab = {(int)nent, step.data(), stream.data(), record.data(), wait_off.data(), waits.data(), (int)nwaits,
                          (int)ns, (int)npre, (int)out->steps.size()};
  SchedProgram prog;
  if (!r.ok || sched_build(tab, &prog) != DH_OK) return DH_EINVAL;
  out->ops.swap(prog.ops);
  out->info.nstreams = (int32_t)ns;
  out->info.num_ops = (int32_t)out->ops.size();
  out->info.num_events = prog.nevents;
  return DH_OK;
}

// DH_OK or DH_EINVAL.  Allocates nothing on a device and reads no byte outside [blob, blob + bytes).  The blob is trusted,
// code-equivalent input (it carries launch arguments); these checks catch truncation and mix-ups, they are not a sandbox.
inline int plan_parse(const void* blob, size_t bytes, PlanImage* out) {
  if (blob == nullptr || out == nullptr || bytes < 44) return DH_EINVAL;
  PlanReader r{static_cast<const unsigned char*>(blob), static_cast<const unsigned char*>(blob) + bytes};
  if (memcmp(r.p, "DHPL", 4) != 0) return DH_EINVAL;
  r.p += 4;
  *out = PlanImage();
  dh_plan_info& h = out->info;
  h.version = (int32_t)r.get<uint32_t>();
  if (h.version < 1 || h.version > (int32_t)kPlanMaxVersion) return DH_EINVAL;
  h.batch = r.get<int32_t>();
  h.arena_bytes = r.get<uint64_t>();
  h.weight_bytes = r.get<uint64_t>();
  const uint32_t nin = r.get<uint32_t>(), nout = r.get<uint32_t>(), nsteps = r.get<uint32_t>();
  if (h.version >= 2) h.byte_bytes = r.get<uint64_t>();
  if (!r.ok || h.batch <= 0 || nin == 0 || nout == 0 || nin > 64 || nout > 4096 || nsteps > (1u << 20) || h.byte_bytes > (1ull << 40))
    return DH_EINVAL;
  h.num_inputs = (int32_t)nin; h.num_outputs = (int32_t)nout; h.num_steps = (int32_t)nsteps;
  h.nstreams = 1;
  for (uint32_t i = 0; i < nin; ++i) {
    PlanIn in{};
    in.tag = r.get<uint64_t>();
    in.items = r.get<uint64_t>();
    if (h.version >= 2) {
      in.u8 = (int)r.get<uint32_t>();
      (void)r.get<uint32_t>();
    } else {
      in.tag |= 1ull << 60;        // version 1 stored the bare arena offset
    }
    out->ins.push_back(in);
  }
  for (uint32_t i = 0; i < nout; ++i) {
    PlanOut o;
    o.off = r.get<uint64_t>(); o.npix = r.get<uint64_t>(); o.C = (int)r.get<uint32_t>(); o.ld = (int)r.get<uint32_t>();
    out->outs.push_back(o);
  }
  for (uint32_t i = 0; i < nsteps; ++i) {
    const uint32_t fn = r.get<uint32_t>(), nb = r.get<uint32_t>();
    if (!r.ok || fn >= (uint32_t)F_COUNT || (uint32_t)h.version < kRecords[fn].first_version || nb != kRecords[fn].bytes ||
        (size_t)(r.end - r.p) < nb)
      return DH_EINVAL;
    for (uint32_t k = 0; k < kRecords[fn].nptr; ++k) {
      uint64_t v;
      memcpy(&v, r.p + kRecords[fn].ptr[k], 8);
      if (!plan_tag_ok(v, h)) return DH_EINVAL;
    }
    out->steps.push_back(PlanStep{(int)fn, r.p, nb});
    r.p += nb;
  }
  if (h.version >= 5 && plan_parse_schedule(r, out) != DH_OK) return DH_EINVAL;
  if (!r.ok || (size_t)(r.end - r.p) != h.weight_bytes) return DH_EINVAL;     // the rest is exactly the weight image
  out->weights = r.p;
  // extents, overflow-safe: every factor is bounded by the arena size (in floats) before it is multiplied
  const uint64_t arena_f = h.arena_bytes / 4, nn = (uint64_t)h.batch;
  auto fits = [&](uint64_t off_bytes, uint64_t rows, uint64_t pitch, uint64_t last) {   // off + ((rows-1)*pitch + last)*4
    if (off_bytes % 4 || off_bytes / 4 > arena_f || rows == 0 || pitch > arena_f || last > arena_f || rows > arena_f) return false;
    const uint64_t room = arena_f - off_bytes / 4;
    if (pitch != 0 && rows - 1 > room / pitch) return false;
    return (rows - 1) * pitch + last <= room;
  };
  for (const PlanIn& in : out->ins) {
    const uint64_t region = in.tag >> 60, off = in.tag & kPlanOffMask;
    if (in.u8 == 0) {
      if (region != 1 || in.items == 0 || in.items > arena_f || !fits(off, nn, in.items, in.items)) return DH_EINVAL;
    } else if (in.u8 != 1 || region != 3 || in.items == 0 || in.items > h.byte_bytes || nn > h.byte_bytes / in.items ||
               off > h.byte_bytes - in.items * nn) {                                 // uint8 frames land in region 3
      return DH_EINVAL;
    }
  }
  for (const PlanOut& o : out->outs)
    if (o.C <= 0 || o.ld < o.C || o.npix == 0 || o.npix > arena_f || !fits(o.off, o.npix * nn, (uint64_t)o.ld, (uint64_t)o.C))
      return DH_EINVAL;
  return DH_OK;
}

// The one loop that turns the tagged pointers of a step's payload (a writable copy) into addresses.  plan_parse has checked
// every offset against its region; a region it would have refused is DH_EINVAL here too.
inline int plan_patch(unsigned char* payload, const Record& rec, char* arena, char* weights, char* bytes) {
  char* const base[4] = {nullptr, arena, weights, bytes};
  for (uint32_t k = 0; k < rec.nptr; ++k) {
    uint64_t v;
    memcpy(&v, payload + rec.ptr[k], 8);
    if (v != 0 && (v >> 60 < 1 || v >> 60 > 3)) return DH_EINVAL;
    char* const ptr = v == 0 ? nullptr : base[v >> 60] + (v & kPlanOffMask);
    memcpy(payload + rec.ptr[k], &ptr, 8);
  }
  return DH_OK;
}

}  // namespace dh
