// Host-only sweep of the multi-stream schedule module and the output pack's host form (deephar_amd/csrc/plan_sched.h,
// out_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc \
//       tools/sched_sweep.cpp -o /tmp/sched_sweep && /tmp/sched_sweep
//
// 1. dh::sched_build on random well-formed tables (1 - 4 streams, staging entries, absorbed entries, waits in both directions
//    between side streams), every array in a heap block of exactly its length: every WAIT names an event recorded earlier on
//    another stream, no side stream waits directly on a higher-numbered one, every launching entry is launched once on its
//    stream, the joins come last.
// 2. the same tables with one field broken (stream count, a stream index, a wait on a later entry / an entry that does not
//    record / the same stream, a staging entry with a wait, table sizes that do not add up): DH_EINVAL each.
// 3. dh::pack_outputs_host against dst[p * C + c] = src[p * ld + c] written out long-hand, guard floats around every
//    destination, NULL destinations skipped.
// Not a pytest test: nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "out_index.h"
#include "plan_sched.h"

using namespace dh;

static long long n_built = 0, n_refused = 0, n_packed = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("sched_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static uint32_t rng_state = 12345;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}

struct Table {
  std::vector<int32_t> step, stream, record, wait_off, waits;
  int nstreams = 1, npre = 0, nsteps = 0;
  SchedTable view() const {
    return SchedTable{(int)step.size(), step.data(), stream.data(), record.data(), wait_off.data(), waits.data(), (int)waits.size(),
                      nstreams, npre, nsteps};
  }
};

static Table random_table(int n, int nstreams) {
  Table t;
  t.nstreams = nstreams;
  t.npre = (int)rnd(3);
  if (t.npre > n) t.npre = n;
  t.wait_off.push_back(0);
  for (int i = 0; i < n; ++i) {
    const bool pre = i < t.npre;
    const int s = pre ? 0 : (int)rnd((uint32_t)nstreams);
    t.stream.push_back(s);
    t.record.push_back(pre ? 0 : (int)rnd(2));
    t.step.push_back(!pre && rnd(6) == 0 ? kSchedNoLaunch : t.nsteps++);
    if (!pre)
      for (int w = i - 1; w >= 0 && w >= i - 12; --w)
        if (t.record[(size_t)w] && t.stream[(size_t)w] != s && rnd(4) == 0) t.waits.push_back(w);
    t.wait_off.push_back((int32_t)t.waits.size());
  }
  return t;
}

static void check_program(const Table& t, const SchedProgram& p) {
  std::vector<int> recorded_on((size_t)p.nevents, -1);
  std::vector<int> launched(t.step.size(), 0);
  const int S = t.nstreams;
  for (size_t k = 0; k < p.ops.size(); ++k) {
    const dh_sched_op& o = p.ops[k];
    if (o.stream < 0 || o.stream >= S) die("op on a stream the plan does not have", (long long)k, o.stream);
    if (o.kind == DH_SCHED_LAUNCH) {
      if (o.entry < 0 || o.entry >= (int)t.step.size() || t.step[(size_t)o.entry] != o.arg || t.stream[(size_t)o.entry] != o.stream)
        die("launch does not match its entry", (long long)k, o.entry);
      ++launched[(size_t)o.entry];
    } else if (o.kind == DH_SCHED_RECORD) {
      if (o.arg < 0 || o.arg >= p.nevents) die("event id out of range", (long long)k, o.arg);
      recorded_on[(size_t)o.arg] = o.stream;
    } else if (o.kind == DH_SCHED_WAIT) {
      if (o.arg < 0 || o.arg >= p.nevents || recorded_on[(size_t)o.arg] < 0) die("wait for an event nobody recorded", (long long)k, o.arg);
      const int src = recorded_on[(size_t)o.arg];
      if (src == o.stream) die("wait on the own stream", (long long)k, o.arg);
      if (o.stream != 0 && src > o.stream) die("side stream waits on a higher-numbered side stream", o.stream, src);
    } else {
      die("unknown op", (long long)k, o.kind);
    }
  }
  for (size_t i = 0; i < t.step.size(); ++i)
    if (launched[i] != (t.step[i] == kSchedNoLaunch ? 0 : 1)) die("entry launched a wrong number of times", (long long)i, launched[i]);
  const size_t tail = 2 * (size_t)(S - 1);
  if (p.ops.size() < tail) die("no room for the joins");
  for (int k = 1; k < S; ++k) {
    const dh_sched_op& r = p.ops[p.ops.size() - tail + 2 * (size_t)(k - 1)];
    const dh_sched_op& w = p.ops[p.ops.size() - tail + 2 * (size_t)(k - 1) + 1];
    if (r.kind != DH_SCHED_RECORD || r.stream != k || r.arg != k || w.kind != DH_SCHED_WAIT || w.stream != 0 || w.arg != k)
      die("join of a side stream is not at the end", k);
  }
}

static void expect_refused(const Table& t, const char* what) {
  SchedProgram p;
  if (sched_build(t.view(), &p) != DH_EINVAL) die(what);
  ++n_refused;
}

static void sweep_schedules() {
  for (int round = 0; round < 400; ++round) {
    const int n = 1 + (int)rnd(60), S = 1 + (int)rnd(4);
    Table t = random_table(n, S);
    SchedProgram p;
    if (sched_build(t.view(), &p) != DH_OK) die("well-formed table refused", round, n);
    check_program(t, p);
    ++n_built;
    Table b = t;
    b.nstreams = 0;
    expect_refused(b, "nstreams 0 accepted");
    b.nstreams = 5;
    expect_refused(b, "nstreams 5 accepted");
    b = t;
    b.stream[rnd((uint32_t)n)] = S;
    expect_refused(b, "stream index out of range accepted");
    b = t;
    b.wait_off[(size_t)n] += 1;
    expect_refused(b, "wait_off[n] != nwaits accepted");
    b = t;
    b.nsteps += 1;
    expect_refused(b, "missing step accepted");
    if (!t.waits.empty()) {
      const size_t k = rnd((uint32_t)t.waits.size());
      size_t owner = 0;
      while (!((size_t)t.wait_off[owner] <= k && k < (size_t)t.wait_off[owner + 1])) ++owner;
      b = t;
      b.waits[k] = (int32_t)owner;                       // a wait on itself
      expect_refused(b, "wait on the entry itself accepted");
      if (owner + 1 < (size_t)n) {
        b.waits[k] = (int32_t)owner + 1;                 // ... on a later entry
        expect_refused(b, "wait on a later entry accepted");
      }
      b = t;
      b.record[(size_t)t.waits[k]] = 0;
      expect_refused(b, "wait on an entry without an event accepted");
      b = t;
      b.stream[(size_t)t.waits[k]] = t.stream[owner];
      if (t.waits[k] >= t.npre || t.stream[owner] == 0) expect_refused(b, "wait on the same stream accepted");
      b = t;
      b.npre = (int)owner + 1;                           // the waiting entry becomes a staging entry
      expect_refused(b, "staging entry with a wait accepted");
    }
  }
}

static void sweep_pack() {
  const float guard = -7.0f;
  for (int round = 0; round < 300; ++round) {
    const int nseg = 1 + (int)rnd(70);
    std::vector<std::vector<float>> src((size_t)nseg), dst((size_t)nseg);
    std::vector<dh_out_seg> segs((size_t)nseg);
    for (int s = 0; s < nseg; ++s) {
      const int C = 1 + (int)rnd(17), ld = C + (int)rnd(5), npix = 1 + (int)rnd(40);
      src[(size_t)s].resize((size_t)npix * ld);
      for (float& v : src[(size_t)s]) v = (float)rnd(1000);
      dst[(size_t)s].assign((size_t)npix * C + 8, guard);
      segs[(size_t)s] = dh_out_seg{src[(size_t)s].data(), rnd(7) == 0 ? nullptr : dst[(size_t)s].data() + 4, npix, C, ld};
    }
    if (pack_outputs_host(segs.data(), nseg) != DH_OK) die("pack refused", round);
    for (int s = 0; s < nseg; ++s) {
      const dh_out_seg& g = segs[(size_t)s];
      const std::vector<float>& d = dst[(size_t)s];
      for (size_t i = 0; i < d.size(); ++i) {
        const bool inside = g.dst != nullptr && i >= 4 && i < d.size() - 4;
        const float want = inside ? g.src[((i - 4) / (size_t)g.C) * (size_t)g.ld + (i - 4) % (size_t)g.C] : guard;
        if (d[i] != want) die("pack differs", s, (long long)i);
      }
    }
    ++n_packed;
    dh_out_seg bad = segs[0];
    bad.dst = dst[0].data() + 4;
    bad.ld = bad.C - 1;
    if (pack_outputs_host(&bad, 1) != DH_EINVAL) die("pitch below the channels accepted");
    bad = segs[0];
    bad.dst = dst[0].data() + 4;
    bad.npix = 0;
    if (pack_outputs_host(&bad, 1) != DH_EINVAL) die("empty segment accepted");
  }
}

int main() {
  sweep_schedules();
  sweep_pack();
  std::printf("sched_sweep ok: %lld programs built, %lld malformed tables refused, %lld pack cases equal\n", n_built, n_refused, n_packed);
  return 0;
}
