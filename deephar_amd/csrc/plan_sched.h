// The multi-stream schedule of a plan as a pure function: a table of schedule entries (one per bound call of the exporting
// process: which blob step it launches, on which stream, whether it records an event, which earlier entries it waits for)
// -> the enqueue program: LAUNCH / RECORD / WAIT ops in order.  No HIP header, no stream, no event: streams and events are
// small integers here.  Both executors run this one list, so nobody restates the order: dh_plan_create validates the schedule
// section of a version-5 blob with it and dh_forward executes the ops; deephar_amd/engine/executor.py's BoundPlan.launch_all
// asks dh_sched_build_ops for the program of its own calls and walks it (engine/schedule.py: run_program), as the host tests do.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "deephar_hip.h"

namespace dh {

// Every stream a process opens costs one of ROCm's four hardware queues (profiles/r06_hw_queue_collision.md): a plan never
// asks for more streams than that, the caller's included.
constexpr int kSchedMaxStreams = 4;
constexpr int32_t kSchedNoLaunch = -1;            // an entry whose work moved into an earlier grouped / paired launch
constexpr int kSchedMaxEntries = (1 << 20) + 64;

struct SchedTable {
  int n;                        // entries
  const int32_t* step;          // [n] blob step the entry launches, or kSchedNoLaunch
  const int32_t* stream;        // [n]
  const int32_t* record;        // [n] != 0: an event is recorded behind the entry
  const int32_t* wait_off;      // [n + 1] entry i waits for waits[wait_off[i] .. wait_off[i + 1])
  const int32_t* waits;         // [nwaits] indices of earlier entries
  int nwaits;
  int nstreams;
  int npre;                     // leading staging entries: launched on stream 0 in front of the fork
  int nsteps;                   // steps of the blob: the launching entries name 0 .. nsteps - 1, each once, in order
};

struct SchedProgram {
  std::vector<dh_sched_op> ops;
  int nevents = 0;              // event ids: 0 fork | 1 .. nstreams - 1 joins | one per recording entry | relays
};

// DH_OK or DH_EINVAL.  Nothing but the table's own arrays is read.
inline int sched_check(const SchedTable& t) {
  if (t.n < 0 || t.n > kSchedMaxEntries || t.nwaits < 0 || t.nsteps < 0 || t.npre < 0 || t.npre > t.n) return DH_EINVAL;
  if (t.nstreams < 1 || t.nstreams > kSchedMaxStreams) return DH_EINVAL;
  if (t.wait_off == nullptr || (t.n > 0 && (t.step == nullptr || t.stream == nullptr || t.record == nullptr))) return DH_EINVAL;
  if (t.nwaits > 0 && t.waits == nullptr) return DH_EINVAL;
  if (t.wait_off[0] != 0 || t.wait_off[t.n] != t.nwaits) return DH_EINVAL;
  int next = 0;
  for (int i = 0; i < t.n; ++i) {
    const int32_t lo = t.wait_off[i], hi = t.wait_off[i + 1];
    if (lo < 0 || hi < lo || hi > t.nwaits) return DH_EINVAL;
    if (t.stream[i] < 0 || t.stream[i] >= t.nstreams) return DH_EINVAL;
    if (t.step[i] != kSchedNoLaunch && t.step[i] != next++) return DH_EINVAL;
    if (i < t.npre && (t.stream[i] != 0 || hi != lo || t.record[i] != 0 || t.step[i] == kSchedNoLaunch)) return DH_EINVAL;
    for (int32_t k = lo; k < hi; ++k) {
      const int32_t w = t.waits[k];
      if (w < 0 || w >= i || t.record[w] == 0 || t.stream[w] == t.stream[i]) return DH_EINVAL;
    }
  }
  return next == t.nsteps ? DH_OK : DH_EINVAL;
}

// The enqueue program:
//   1. LAUNCH of the staging entries (stream 0)
//   2. RECORD fork on stream 0, WAIT fork on every side stream
//   3. per entry, in order: its WAITs, the LAUNCH (none for an absorbed entry), the RECORD if flagged -- an absorbed entry
//      still records at its own place
//   4. for every side stream: RECORD join on it, WAIT join on stream 0
// Relay rule (ROCm 7.2: two SIDE streams that wait on each other's events in both directions break stream capture, and the
// same order is kept for eager execution): a side stream never waits directly on an event of a higher-numbered side stream;
// stream 0 waits instead and re-records the dependency on a relay event of its own.
inline int sched_build(const SchedTable& t, SchedProgram* out) {
  if (out == nullptr) return DH_EINVAL;
  const int rc = sched_check(t);
  if (rc != DH_OK) return rc;
  out->ops.clear();
  const int S = t.nstreams;
  auto op = [&](int kind, int stream, int arg, int entry) { out->ops.push_back(dh_sched_op{kind, stream, arg, entry}); };
  std::vector<int32_t> event(t.n, -1);
  int nev = S;                                    // fork + joins
  for (int i = 0; i < t.n; ++i)
    if (t.record[i]) event[i] = nev++;
  for (int i = 0; i < t.npre; ++i) op(DH_SCHED_LAUNCH, 0, t.step[i], i);
  if (S > 1) {
    op(DH_SCHED_RECORD, 0, 0, -1);
    for (int k = 1; k < S; ++k) op(DH_SCHED_WAIT, k, 0, -1);
  }
  for (int i = t.npre; i < t.n; ++i) {
    const int s = t.stream[i];
    for (int32_t k = t.wait_off[i]; k < t.wait_off[i + 1]; ++k) {
      const int32_t w = t.waits[k];
      int ev = event[w];
      if (s != 0 && t.stream[w] > s) {
        op(DH_SCHED_WAIT, 0, ev, i);
        ev = nev++;
        op(DH_SCHED_RECORD, 0, ev, i);
      }
      op(DH_SCHED_WAIT, s, ev, i);
    }
    if (t.step[i] != kSchedNoLaunch) op(DH_SCHED_LAUNCH, s, t.step[i], i);
    if (t.record[i]) op(DH_SCHED_RECORD, s, event[i], i);
  }
  for (int k = 1; k < S; ++k) {
    op(DH_SCHED_RECORD, k, k, -1);
    op(DH_SCHED_WAIT, 0, k, -1);
  }
  out->nevents = nev;
  return DH_OK;
}

}  // namespace dh
