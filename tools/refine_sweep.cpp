// Host-only sweep of the box-refinement index module (deephar_amd/csrc/refine_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc
//       tools/refine_sweep.cpp -o /tmp/refine_sweep && /tmp/refine_sweep
//
// 1. dh::jobs_from_boxes_host over boxes of every kind -- inside, negative, fractional, huge (a corner at 3e9, at +-2^31), NaN,
//    infinite -- each table in a heap block of exactly its length: the window against trunc() of the corners written out
//    long-hand, the empty job for every corner that does not fit int32 (the conversion of such a double is undefined behaviour:
//    the sanitizer build proves it is never reached).
// 2. dh::refine_boxes_host over random sample counts, joint counts, channels per joint, joint and sample strides and channel
//    offsets: poses, jobs and boxes in heap blocks of exactly the extent the strides span, guard values around both outputs;
//    the new job is the window of the new box, the new box is a square around its centre, in-place equals out-of-place bit
//    for bit, a reversed joint order gives the same bits (the device reduces in another order), flipped and empty jobs pass
//    their box through, a NaN coordinate gives the one quiet NaN and the empty job.
// 3. every refusal: NULL pointers, n < 1, J < 1, strides smaller than the extent they span; dh::refine_frames_shape.
// Not a pytest test: nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "refine_index.h"

using namespace dh;

static long long n_windows = 0, n_steps = 0, n_refused = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("refine_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (rnd(1 << 20) / (double)(1 << 20)); }

static bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * 8) == 0; }
static bool same_job(const dh_crop_job& a, const dh_crop_job& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
static bool is_empty(const dh_crop_job& g, int src) { return g.src == src && !g.x0 && !g.y0 && !g.x1 && !g.y1 && !g.hflip; }

static void sweep_windows() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> pool = {0.0, -0.0, 0.5, -0.5, 0.999999, -0.999999, 1.0, -1.0, 17.25, -17.75, 1279.5, 2147483646.5, 2147483647.0,
                              2147483647.5, 2147483648.0, -2147483647.5, -2147483648.0, -2147483649.0, 3e9, -3e9, 1e300, inf, -inf, nan};
  for (int k = 0; k < 400; ++k) pool.push_back(uni(-2000.0, 3000.0));
  for (size_t a = 0; a < pool.size(); a += 1 + rnd(3))
    for (size_t b = 0; b < pool.size(); b += 1 + rnd(3)) {
      const int n = 1 + (int)rnd(5);
      double* boxes = new double[(size_t)4 * n];
      int32_t* src = new int32_t[n];
      dh_crop_job* jobs = new dh_crop_job[n];
      for (int i = 0; i < n; ++i) {
        boxes[4 * i] = pool[a];
        boxes[4 * i + 1] = pool[(b + i) % pool.size()];
        boxes[4 * i + 2] = pool[(a + b + i) % pool.size()];
        boxes[4 * i + 3] = pool[b];
        src[i] = (int32_t)rnd(1000) - 3;
      }
      if (jobs_from_boxes_host(boxes, src, n, jobs) != DH_OK) die("jobs_from_boxes_host refused", n);
      for (int i = 0; i < n; ++i) {
        const double* q = boxes + 4 * i;
        const double cx = (q[0] + q[2]) / 2, cy = (q[1] + q[3]) / 2, w = q[2] - q[0], h = q[3] - q[1];
        const double c[4] = {cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2};
        bool fits = true;
        for (double v : c) fits = fits && std::isfinite(v) && std::fabs(v) < 2147483648.0;
        if (!fits) {
          if (!is_empty(jobs[i], src[i])) die("a corner that does not fit must give the empty job", (long long)a, (long long)b);
        } else if (jobs[i].src != src[i] || jobs[i].x0 != (int32_t)std::trunc(c[0]) || jobs[i].y0 != (int32_t)std::trunc(c[1]) ||
                   jobs[i].x1 != (int32_t)std::trunc(c[2]) || jobs[i].y1 != (int32_t)std::trunc(c[3]) || jobs[i].hflip != 0) {
          die("window", (long long)a, (long long)b);
        }
        ++n_windows;
      }
      delete[] boxes;
      delete[] src;
      delete[] jobs;
    }
}

static void sweep_steps() {
  const float fnan = std::numeric_limits<float>::quiet_NaN();
  const double guard = -12345.678;
  for (int round = 0; round < 3000; ++round) {
    const int n = 1 + (int)rnd(9), J = 1 + (int)rnd(round % 50 == 0 ? 200 : 20), D = 2 + (int)rnd(3);
    const int64_t js = D + (int64_t)rnd(4), ss = (J - 1) * js + 2 + (int64_t)rnd(7);
    const size_t extent = (size_t)(n - 1) * ss + (size_t)(J - 1) * js + 2;               // exactly what the strides span
    float* poses = new float[extent];
    float* reversed = new float[extent];
    for (size_t k = 0; k < extent; ++k) reversed[k] = poses[k] = (float)uni(-0.3, 1.3);
    dh_crop_job* jin = new dh_crop_job[n];
    double* bin = new double[(size_t)4 * n];
    const int special = (int)rnd(8);                                                      // which sample (if < n) is special, and how
    const int kind = (int)rnd(5);
    for (int i = 0; i < n; ++i) {
      const double cx = uni(-200, 1500), cy = uni(-200, 900), w = uni(1.5, 900), h = uni(1.5, 900);
      double* q = bin + 4 * i;
      q[0] = cx - w / 2; q[1] = cy - h / 2; q[2] = cx + w / 2; q[3] = cy + h / 2;
      jin[i] = refine_window(q, i);
      if (i == special) {
        if (kind == 0) jin[i].hflip = 1;
        if (kind == 1) jin[i].x1 = jin[i].x0;
        if (kind == 2) poses[(size_t)i * ss + (size_t)rnd(J) * js + rnd(2)] = fnan;
        if (kind == 3)
          for (int j = 0; j < J; ++j) poses[(size_t)i * ss + j * js] = poses[(size_t)i * ss + j * js + 1] = 0.25f;   // one point
        if (kind == 4) q[2] = 3e9;
      }
      for (int j = 0; j < J; ++j)                                                         // the same joints, last first
        for (int c = 0; c < 2; ++c) reversed[(size_t)i * ss + (size_t)(J - 1 - j) * js + c] = poses[(size_t)i * ss + (size_t)j * js + c];
    }
    const double ws = uni(1.0, 2.0), mom = uni(0.0, 1.0);
    double* bout = new double[(size_t)4 * n + 2];
    dh_crop_job* jout = new dh_crop_job[n + 2];
    bout[0] = bout[4 * n + 1] = guard;
    std::memset(&jout[0], 0x5A, sizeof(dh_crop_job));
    std::memset(&jout[n + 1], 0x5A, sizeof(dh_crop_job));
    if (refine_boxes_host(poses, ss, js, J, jin, bin, n, ws, mom, bout + 1, jout + 1) != DH_OK) die("refine_boxes_host refused", round);
    dh_crop_job pat;
    std::memset(&pat, 0x5A, sizeof pat);
    if (bout[0] != guard || bout[4 * n + 1] != guard || !same_job(jout[0], pat) || !same_job(jout[n + 1], pat)) die("guards", round);
    for (int i = 0; i < n; ++i) {
      const double* o = bout + 1 + 4 * i;
      const dh_crop_job& g = jout[1 + i];
      if (!same_job(g, refine_window(o, jin[i].src)) && !(is_empty(g, jin[i].src))) die("job is not the window of its box", round, i);
      const bool passes = jin[i].hflip != 0 || refine_job_empty(jin[i]);
      if (passes) {
        if (!same_bits(o, bin + 4 * i, 4) || !is_empty(g, jin[i].src)) die("a flipped or empty job passes its box through", round, i);
      } else if (i == special && kind == 2) {
        const double qn = refine_nan();
        for (int c = 0; c < 4; ++c)
          if (std::memcmp(&o[c], &qn, 8) != 0) die("a NaN joint gives the one quiet NaN", round, i);
        if (!is_empty(g, jin[i].src)) die("a NaN joint gives the empty job", round, i);
      } else {
        const double sx = o[2] - o[0], sy = o[3] - o[1];
        if (!(sx >= 0) || std::fabs(sx - sy) > 1e-6 * (1 + std::fabs(sx))) die("the new box is no square", round, i);
        if (i == special && kind == 3 && (sx != 0 || !refine_job_empty(g))) die("all joints at one point: side 0, empty window", round, i);
        if (!(i == special && kind == 4) && !same_job(g, refine_window(o, jin[i].src))) die("window of the new box", round, i);
      }
      ++n_steps;
    }
    // the joints in another order: the same bits
    double* b2 = new double[(size_t)4 * n];
    dh_crop_job* j2 = new dh_crop_job[n];
    if (refine_boxes_host(reversed, ss, js, J, jin, bin, n, ws, mom, b2, j2) != DH_OK) die("refused (reversed)", round);
    if (!same_bits(b2, bout + 1, (size_t)4 * n) || std::memcmp(j2, jout + 1, sizeof(dh_crop_job) * n) != 0) die("joint order moved a bit", round);
    // in place
    if (refine_boxes_host(poses, ss, js, J, jin, bin, n, ws, mom, bin, jin) != DH_OK) die("refused (in place)", round);
    if (!same_bits(bin, bout + 1, (size_t)4 * n) || std::memcmp(jin, jout + 1, sizeof(dh_crop_job) * n) != 0) die("in place differs", round);
    delete[] poses; delete[] reversed; delete[] jin; delete[] bin; delete[] bout; delete[] jout; delete[] b2; delete[] j2;
  }
}

static void sweep_refusals() {
  float poses[2 * 5 * 3] = {};
  dh_crop_job jobs[2] = {{0, 0, 0, 10, 10, 0}, {1, 0, 0, 10, 10, 0}};
  double boxes[8] = {0, 0, 10, 10, 0, 0, 10, 10};
  int32_t src[2] = {0, 1};
  auto want = [](int rc, int code, const char* what) {
    if (rc != code) die(what, rc, code);
    ++n_refused;
  };
  want(jobs_from_boxes_host(nullptr, src, 2, jobs), DH_EINVAL, "NULL boxes");
  want(jobs_from_boxes_host(boxes, nullptr, 2, jobs), DH_EINVAL, "NULL src");
  want(jobs_from_boxes_host(boxes, src, 2, nullptr), DH_EINVAL, "NULL jobs");
  want(jobs_from_boxes_host(boxes, src, 0, jobs), DH_EINVAL, "n = 0");
  want(refine_boxes_host(nullptr, 15, 3, 5, jobs, boxes, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "NULL poses");
  want(refine_boxes_host(poses, 15, 3, 5, nullptr, boxes, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "NULL jobs_in");
  want(refine_boxes_host(poses, 15, 3, 5, jobs, nullptr, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "NULL boxes_in");
  want(refine_boxes_host(poses, 15, 3, 5, jobs, boxes, 2, 1.5, 0.8, nullptr, jobs), DH_EINVAL, "NULL boxes_out");
  want(refine_boxes_host(poses, 15, 3, 5, jobs, boxes, 2, 1.5, 0.8, boxes, nullptr), DH_EINVAL, "NULL jobs_out");
  want(refine_boxes_host(poses, 15, 3, 5, jobs, boxes, 0, 1.5, 0.8, boxes, jobs), DH_EINVAL, "n = 0");
  want(refine_boxes_host(poses, 15, 3, 0, jobs, boxes, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "J = 0");
  want(refine_boxes_host(poses, 15, 1, 5, jobs, boxes, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "joint stride 1");
  want(refine_boxes_host(poses, 13, 3, 5, jobs, boxes, 2, 1.5, 0.8, boxes, jobs), DH_EINVAL, "sample stride 13 < 4 * 3 + 2");
  want(refine_boxes_host(poses, 14, 3, 5, jobs, boxes, 2, 1.5, 0.8, boxes, jobs), DH_OK, "sample stride 14 = 4 * 3 + 2");
  int J = 0;
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, 2, &J), DH_OK, "a good plan");
  if (J != 16) die("J", J);
  want(refine_frames_shape(2, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, 2, &J), DH_EINVAL, "two inputs");
  want(refine_frames_shape(1, 0, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, 2, &J), DH_EINVAL, "a float input");
  want(refine_frames_shape(1, 1, 4 * 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, 2, &J), DH_EINVAL, "a clip plan");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 5, 256, 256, 3, 2, 48, 3, 2, &J), DH_EINVAL, "n above the batch");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 0, 256, 256, 3, 2, 48, 3, 2, &J), DH_EINVAL, "n = 0");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 3, 48, 3, 2, &J), DH_EINVAL, "outidx out of range");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, -1, 48, 3, 2, &J), DH_EINVAL, "outidx negative");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 16, 1, 2, &J), DH_EINVAL, "one channel");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, 0, &J), DH_EINVAL, "num_iter = 0");
  want(refine_frames_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 255, 3, 2, 48, 3, 2, &J), DH_EINVAL, "another crop size");
}

int main() {
  sweep_windows();
  sweep_steps();
  sweep_refusals();
  std::printf("refine_sweep: ok (%lld windows, %lld steps, %lld refusals)\n", n_windows, n_steps, n_refused);
  return 0;
}
