// Host-only sweep of the person-box index module (deephar_amd/csrc/posebox_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc
//       tools/posebox_sweep.cpp -o /tmp/posebox_sweep && /tmp/posebox_sweep
//
// 1. dh::pose_boxes_host over random item counts, frames per item, joint counts, channels per joint, joint, frame and item
//    strides, channel offsets (item 0 starts a few floats into its block), confidence channels and job strides: poses and jobs
//    in heap blocks that end exactly where the strides' span ends, guard values around the three outputs.  A good item's
//    float64 box is ordered, lies within the span of its kept joints enlarged by relsize, and its int32 box is that box
//    truncated; the joints last-first and the frames last-first give the same bits (the device reduces in another order).
// 2. every status on a planted item -- a frame that keeps nothing, a NaN confidence, a NaN joint, an infinite joint, a float32
//    overflow, a corner beyond int32 (the conversion of such a double is undefined behaviour: the sanitizer build proves it is
//    never reached), a flipped, an empty and a reversed window -- with zero boxes behind each, and the precedence 1, 2, 4, 3.
// 3. every refusal: NULL pointers, n < 1, F < 1, J < 1, conf_channel < 0, strides smaller than the extent they span (F = 1
//    included), strides above 2^40, spans above 2^58; dh::frame_boxes_shape.
// Not a pytest test: nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "posebox_index.h"

using namespace dh;

static long long n_items = 0, n_status[5] = {0, 0, 0, 0, 0}, n_refused = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("posebox_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (rnd(1 << 20) / (double)(1 << 20)); }

struct Tables {                                     // the three outputs, one guard row in front of and behind each
  int n;
  int32_t* box;
  double* boxf;
  int32_t* status;
  explicit Tables(int n_) : n(n_), box(new int32_t[4 * (size_t)(n_ + 2)]), boxf(new double[4 * (size_t)(n_ + 2)]), status(new int32_t[n_ + 2]) {
    for (int k = 0; k < 4 * (n + 2); ++k) {
      box[k] = -7777;
      boxf[k] = -777.125;
    }
    for (int k = 0; k < n + 2; ++k) status[k] = 77;
  }
  ~Tables() {
    delete[] box;
    delete[] boxf;
    delete[] status;
  }
  void guards(long long round) const {
    for (int c = 0; c < 4; ++c)
      if (box[c] != -7777 || box[4 * (n + 1) + c] != -7777 || boxf[c] != -777.125 || boxf[4 * (n + 1) + c] != -777.125) die("guards", round);
    if (status[0] != 77 || status[n + 1] != 77) die("status guards", round);
  }
  bool same(const Tables& o) const {
    return std::memcmp(box + 4, o.box + 4, 16 * (size_t)n) == 0 && std::memcmp(boxf + 4, o.boxf + 4, 32 * (size_t)n) == 0 &&
           std::memcmp(status + 1, o.status + 1, 4 * (size_t)n) == 0;
  }
};

static void sweep_items() {
  const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
  for (int round = 0; round < 4000; ++round) {
    const int n = 1 + (int)rnd(9), F = 1 + (int)rnd(4), J = 1 + (int)rnd(round % 50 == 0 ? 200 : 20), D = 2 + (int)rnd(3);
    const int cc = round % 7 == 0 ? (int)rnd(D) : D - 2;
    const int64_t ext = cc < 2 ? 2 : cc + 1;
    const int64_t js = D + (int64_t)rnd(4), fs = (J - 1) * js + ext + (int64_t)rnd(7), its = (F - 1) * fs + (J - 1) * js + ext + (int64_t)rnd(5);
    const int64_t jstride = 1 + (int64_t)rnd(3);
    const size_t extent = (size_t)(n - 1) * its + (size_t)(F - 1) * fs + (size_t)(J - 1) * js + ext;       // exactly what the strides span
    // item 0 starts a random few floats into its block (a channel offset into a wider buffer), the block ends where the
    // strides' span ends; the floats in front are never read
    const size_t base = rnd(6);
    float* poses_block = new float[base + extent];
    float* jrev_block = new float[base + extent];    // the joints of every frame last first
    float* frev_block = new float[base + extent];    // the frames of every item last first
    for (size_t k = 0; k < base; ++k) poses_block[k] = jrev_block[k] = frev_block[k] = std::numeric_limits<float>::quiet_NaN();
    float* poses = poses_block + base;
    float* jrev = jrev_block + base;
    float* frev = frev_block + base;
    for (size_t k = 0; k < extent; ++k) poses[k] = (float)uni(-0.2, 1.2);
    const size_t njobs = (size_t)(n - 1) * jstride + 1;
    dh_crop_job* jobs = new dh_crop_job[njobs];
    std::memset(jobs, 0x5A, sizeof(dh_crop_job) * njobs);
    const int special = (int)rnd(12), kind = (int)rnd(9);                                  // which item (if < n) is special, and how
    const float relsize_d = (float)uni(0.5, 2.5);
    for (int i = 0; i < n; ++i) {
      const int32_t x0 = (int32_t)rnd(1200) - 300, y0 = (int32_t)rnd(800) - 300;
      jobs[(size_t)i * jstride] = dh_crop_job{i, x0, y0, x0 + 32 + (int32_t)rnd(1368), y0 + 32 + (int32_t)rnd(1368), 0};
      float* item = poses + (size_t)i * its;
      for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j) {
          float* p = item + (size_t)f * fs + (size_t)j * js;
          if (cc >= 2) p[cc] = (float)uni(0.0, 1.0);
          if (j == (f % J)) p[cc] = cc < 2 ? 0.5f + (float)uni(0.0, 0.5) : 0.9f;          // every frame keeps at least this joint
        }
      if (i == special) {
        float* p = item + (size_t)rnd(F) * fs;
        float* q = p + (size_t)rnd(J) * js;
        if (kind == 0)
          for (int j = 0; j < J; ++j) p[(size_t)j * js + cc] = 0.25f;                      // a frame keeps nothing
        if (kind == 1)
          for (int j = 0; j < J; ++j) p[(size_t)j * js + cc] = fnan;                       // NaN confidences keep nothing
        if (kind == 2 && cc >= 2) { q[cc] = 0.9f; q[rnd(2)] = fnan; }                      // a kept NaN joint
        if (kind == 3 && cc >= 2) { q[cc] = 0.9f; q[rnd(2)] = rnd(2) ? finf : -finf; }     // a kept infinite joint
        if (kind == 4 && cc >= 2) { q[cc] = 0.9f; q[0] = 1e8f; }                           // a corner beyond int32
        if (kind == 5 && cc >= 2 && J > 1) {                                              // xmax - xmin overflows float32
          p[cc] = p[js + cc] = 0.9f;
          p[0] = 3e38f;
          p[js] = -3e38f;
        }
        if (kind == 6) jobs[(size_t)i * jstride].hflip = 1;
        if (kind == 7) jobs[(size_t)i * jstride].x1 = jobs[(size_t)i * jstride].x0;
        if (kind == 8) jobs[(size_t)i * jstride].y1 = jobs[(size_t)i * jstride].y0 - 5;
      }
    }
    for (size_t k = 0; k < extent; ++k) jrev[k] = frev[k] = poses[k];
    for (int i = 0; i < n; ++i)
      for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j)
          for (int64_t c = 0; c < ext; ++c) {
            const float v = poses[(size_t)i * its + (size_t)f * fs + (size_t)j * js + c];
            jrev[(size_t)i * its + (size_t)f * fs + (size_t)(J - 1 - j) * js + c] = v;
            frev[(size_t)i * its + (size_t)(F - 1 - f) * fs + (size_t)j * js + c] = v;
          }
    Tables t(n), tj(n), tf(n);
    if (pose_boxes_host(poses, its, fs, js, F, J, cc, jobs, jstride, n, relsize_d, t.box + 4, t.boxf + 4, t.status + 1) != DH_OK)
      die("pose_boxes_host refused", round);
    t.guards(round);
    if (pose_boxes_host(jrev, its, fs, js, F, J, cc, jobs, jstride, n, relsize_d, tj.box + 4, tj.boxf + 4, tj.status + 1) != DH_OK)
      die("refused (joints reversed)", round);
    if (!t.same(tj)) die("joint order moved a bit", round);
    if (pose_boxes_host(frev, its, fs, js, F, J, cc, jobs, jstride, n, relsize_d, tf.box + 4, tf.boxf + 4, tf.status + 1) != DH_OK)
      die("refused (frames reversed)", round);
    if (!t.same(tf)) die("frame order moved a bit", round);
    for (int i = 0; i < n; ++i) {
      const int32_t st = t.status[1 + i];
      const int32_t* b = t.box + 4 + 4 * i;
      const double* q = t.boxf + 4 + 4 * i;
      const dh_crop_job& g = jobs[(size_t)i * jstride];
      if (st < 0 || st > 4) die("status out of range", round, i);
      ++n_status[st];
      ++n_items;
      if (i == special) {
        if ((kind == 0 || kind == 1) && st != kPoseBoxNoJoint) die("a frame that keeps nothing: status 1", round, st);
        if (kind == 2 && cc >= 2 && st != kPoseBoxNan) die("a kept NaN joint: status 2", round, st);
        if ((kind == 3 || kind == 4 || kind == 5) && cc >= 2 && (kind != 5 || J > 1) && st != kPoseBoxRange) die("a wild corner: status 3", round, st);
        if (kind >= 6 && st != kPoseBoxWindow && st != kPoseBoxNoJoint && st != kPoseBoxNan) die("a bad window: status 4", round, st);
      }
      if (st != kPoseBoxOk) {
        for (int c = 0; c < 4; ++c)
          if (b[c] != 0 || q[c] != 0.0 || std::signbit(q[c])) die("a non-zero status leaves zero boxes", round, i);
        continue;
      }
      if (!(q[0] <= q[2] && q[1] <= q[3])) die("corners not ordered", round, i);
      for (int c = 0; c < 4; ++c)
        if (!(std::fabs(q[c]) < 2147483648.0) || b[c] != (int32_t)std::trunc(q[c])) die("int box is not the truncated float box", round, i);
      // the box is a square in crop coordinates around the kept joints, so it contains every kept joint mapped to pixels
      const float* item = poses + (size_t)i * its;
      for (int f = 0; f < F; ++f)
        for (int j = 0; j < J; ++j) {
          const float* p = item + (size_t)f * fs + (size_t)j * js;
          if (!(p[cc] > kPoseBoxConfThr) || relsize_d < 1.0f) continue;
          const double X = g.x0 + (double)p[0] * (g.x1 - g.x0), Y = g.y0 + (double)p[1] * (g.y1 - g.y0);
          const double slack = 1e-3 * (1 + (g.x1 - g.x0) + (g.y1 - g.y0));
          if (X < q[0] - slack || X > q[2] + slack || Y < q[1] - slack || Y > q[3] + slack) die("a kept joint lies outside its box", round, i);
        }
    }
    delete[] poses_block; delete[] jrev_block; delete[] frev_block; delete[] jobs;
  }
  for (int s = 0; s < 5; ++s)
    if (n_status[s] == 0) die("a status the sweep never met", s);
}

static void sweep_precedence() {
  const float fnan = std::numeric_limits<float>::quiet_NaN();
  // two frames of two joints [x, y, conf, pad]: frame 0 has a NaN joint, frame 1 keeps nothing, the window is flipped
  float p[2 * 2 * 4] = {fnan, 0.5f, 0.9f, 0, 0.2f, 0.4f, 0.9f, 0, 0.1f, 0.1f, 0.1f, 0, 0.3f, 0.3f, 0.1f, 0};
  dh_crop_job g = {0, 10, 10, 5, 50, 1};
  int32_t b[4], st = -1;
  double q[4];
  auto run = [&]() {
    if (pose_boxes_host(p, 16, 8, 4, 2, 2, 2, &g, 1, 1, 1.5, b, q, &st) != DH_OK) die("precedence: refused");
    return st;
  };
  if (run() != kPoseBoxNoJoint) die("1 comes first", st);
  p[10] = 0.9f;                                       // frame 1 keeps a joint now
  if (run() != kPoseBoxNan) die("then 2", st);
  p[0] = 1e8f;                                        // no NaN any more, but a corner beyond int32
  if (run() != kPoseBoxWindow) die("then 4", st);
  g = dh_crop_job{0, 10, 10, 500, 500, 0};
  if (run() != kPoseBoxRange) die("then 3", st);
  p[0] = 0.6f;
  if (run() != kPoseBoxOk) die("then 0", st);
}

static void sweep_refusals() {
  float poses[2 * 2 * 5 * 3] = {};
  dh_crop_job jobs[4] = {{0, 0, 0, 10, 10, 0}, {1, 0, 0, 10, 10, 0}, {0, 0, 0, 10, 10, 0}, {1, 0, 0, 10, 10, 0}};
  int32_t box[8], status[2];
  double boxf[8];
  const int64_t big = ((int64_t)1 << 40) + 1;
  auto want = [](int rc, int code, const char* what) {
    if (rc != code) die(what, rc, code);
    ++n_refused;
  };
  // two items of two frames of five joints of three channels: joint stride 3, frame stride 15, item stride 30
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_OK, "a good call");
  want(pose_boxes_host(nullptr, 30, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "NULL poses");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, nullptr, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "NULL jobs");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, nullptr, boxf, status), DH_EINVAL, "NULL boxes_out");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, nullptr, status), DH_EINVAL, "NULL boxes_f64_out");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, nullptr), DH_EINVAL, "NULL status_out");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 2, 0, 1.5, box, boxf, status), DH_EINVAL, "n = 0");
  want(pose_boxes_host(poses, 30, 15, 3, 0, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "F = 0");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 0, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "J = 0");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, -1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "conf_channel = -1");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 3, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "conf_channel beyond the joint stride");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, 0, 2, 1.5, box, boxf, status), DH_EINVAL, "job stride 0");
  want(pose_boxes_host(poses, 30, 15, 1, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "joint stride 1");
  want(pose_boxes_host(poses, 30, 13, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "frame stride 13 < 4 * 3 + 2");
  want(pose_boxes_host(poses, 30, 14, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_OK, "frame stride 14 = 4 * 3 + 2");
  want(pose_boxes_host(poses, 28, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "item stride 28 < 15 + 4 * 3 + 2");
  want(pose_boxes_host(poses, 29, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_OK, "item stride 29 = 15 + 4 * 3 + 2");
  want(pose_boxes_host(poses, 13, 14, 3, 1, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "F = 1: item stride 13 < 4 * 3 + 2");
  want(pose_boxes_host(poses, 2, 14, 3, 1, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "F = 1: item stride 2 < 4 * 3 + 2");
  want(pose_boxes_host(poses, 14, 14, 3, 1, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_OK, "F = 1: item stride 14 = 4 * 3 + 2");
  want(pose_boxes_host(poses, big, 15, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "item stride above 2^40");
  want(pose_boxes_host(poses, big - 1, 15, 3, 2, 5, 1, jobs, 2, 0x7fffffff, 1.5, box, boxf, status), DH_EINVAL, "(n - 1) item strides above 2^58");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, big - 1, 0x7fffffff, 1.5, box, boxf, status), DH_EINVAL, "(n - 1) job strides above 2^58");
  want(pose_boxes_host(poses, big, big, 3, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "frame stride above 2^40");
  want(pose_boxes_host(poses, big, big, big, 2, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "joint stride above 2^40");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 5, 1, jobs, big, 2, 1.5, box, boxf, status), DH_EINVAL, "job stride above 2^40");
  want(pose_boxes_host(poses, 30, 15, 3, 2, 0x7fffffff, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "J = 2^31 - 1");
  want(pose_boxes_host(poses, 30, 15, 3, 0x7fffffff, 5, 1, jobs, 2, 2, 1.5, box, boxf, status), DH_EINVAL, "F = 2^31 - 1");
  int J = 0;
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, &J), DH_OK, "a good plan");
  if (J != 16) die("J", J);
  want(frame_boxes_shape(2, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, &J), DH_EINVAL, "two inputs");
  want(frame_boxes_shape(1, 0, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, &J), DH_EINVAL, "a float input");
  want(frame_boxes_shape(1, 1, 4 * 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 48, 3, &J), DH_EINVAL, "a clip plan");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 5, 256, 256, 3, 2, 48, 3, &J), DH_EINVAL, "n above the batch");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 0, 256, 256, 3, 2, 48, 3, &J), DH_EINVAL, "n = 0");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 3, 48, 3, &J), DH_EINVAL, "outidx out of range");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, -1, 48, 3, &J), DH_EINVAL, "outidx negative");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 256, 3, 2, 16, 1, &J), DH_EINVAL, "one channel");
  want(frame_boxes_shape(1, 1, 256 * 256 * 3, 4, 4, 256, 255, 3, 2, 48, 3, &J), DH_EINVAL, "another crop size");
}

int main() {
  sweep_items();
  sweep_precedence();
  sweep_refusals();
  std::printf("posebox_sweep: ok (%lld items: %lld ok, %lld no joint, %lld NaN, %lld range, %lld window; %lld refusals)\n", n_items,
              n_status[0], n_status[1], n_status[2], n_status[3], n_status[4], n_refused);
  return 0;
}
