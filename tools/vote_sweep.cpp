// Host-only sweep of the multi-clip vote's index module (deephar_amd/csrc/vote_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc
//       tools/vote_sweep.cpp -o /tmp/vote_sweep && /tmp/vote_sweep
//
// 1. dh::vote_products_host over random source counts (beyond kVoteMaxSrcs too), class counts, item counts, sequence counts,
//    item strides and channel offsets: every source in a heap block that ends exactly where its strides' span ends, seq, acc,
//    labels and scores in heap blocks of exactly their length.  Checked against a scalar restatement (its arg-max is a plain
//    scan with np.argmax's NaN rule, not the total order), bit for bit; the classes walked last-first and lane-wise in 64
//    strides with a butterfly give the same label (the device reduces in that order); a split into two calls gives the same
//    bits; sequences no item names keep their bits; scores_out = NULL.
// 2. planted values: ties, NaN, +-inf, +-0, negative, float32 and float64 subnormals, products that reach zero, inf * 0.
// 3. items whose seq is out of range: label -1, acc and the item's scores rows untouched.
// 4. every refusal: NULL and misaligned pointers, nb / C / n / nseq < 1, item_stride < C, strides above 2^40, spans above 2^58.
// Not a pytest test: nothing here is loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "vote_index.h"

using namespace dh;

static long long n_items = 0, n_nan_labels = 0, n_skipped = 0, n_refused = 0, n_subnormal = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("vote_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}
static double uni(double lo, double hi) { return lo + (hi - lo) * (rnd(1 << 20) / (double)(1 << 20)); }

static float planted(int kind) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  switch (kind) {
    case 0: return nan;
    case 1: return inf;
    case 2: return -inf;
    case 3: return 0.0f;
    case 4: return -0.0f;
    case 5: return -0.5f;
    case 6: return 1e-40f;                          // a float32 subnormal
    case 7: return 2e-38f;
    case 8: return 0.25f;                           // (ties)
    default: return 3e38f;
  }
}

// np.argmax over a row, as a plain scan: the first NaN if there is one, else the first maximum
static int32_t scan_argmax(const double* row, int C) {
  int best = 0;
  for (int c = 0; c < C; ++c) {
    if (row[c] != row[c]) return c;
    if (row[c] > row[best]) best = c;
  }
  return best;
}

// the device's order: lane l folds classes l, l + 64, ...; then a butterfly over the 64 lanes
static int32_t butterfly_argmax(const double* row, int C) {
  VoteBest lane[kVoteWave];
  for (int l = 0; l < kVoteWave; ++l) {
    lane[l] = vote_best_none();
    for (int c = l; c < C; c += kVoteWave) {
      const VoteBest e = {row[c], c};
      lane[l] = vote_first(lane[l], e);
    }
  }
  for (int d = kVoteWave / 2; d > 0; d >>= 1) {
    VoteBest next[kVoteWave];
    for (int l = 0; l < kVoteWave; ++l) next[l] = vote_first(lane[l], lane[l ^ d]);
    std::memcpy(lane, next, sizeof(lane));
  }
  for (int l = 1; l < kVoteWave; ++l)
    if (lane[l].i != lane[0].i) die("the lanes disagree after the butterfly", l);
  return lane[0].i;
}

static bool same_bits(const double* a, const double* b, size_t n) {
  for (size_t k = 0; k < n; ++k) {
    const bool an = a[k] != a[k], bn = b[k] != b[k];
    if (an != bn) return false;
    if (!an && std::memcmp(a + k, b + k, 8) != 0) return false;
  }
  return true;
}

struct Case {
  int nb, C, n, nseq;
  std::vector<std::unique_ptr<float[]>> blocks;     // one heap block per source, of exactly the span of its strides
  std::vector<dh_vote_src> srcs;
  std::unique_ptr<int32_t[]> seq;
  std::unique_ptr<double[]> acc0;
};

static Case make_case(int round) {
  Case c;
  c.nb = round % 97 == 0 ? kVoteMaxSrcs + 1 + (int)rnd(3) : 1 + (int)rnd(5);
  c.C = round % 53 == 0 ? 64 + (int)rnd(140) : 1 + (int)rnd(20);
  c.n = 1 + (int)rnd(12);
  c.nseq = 1 + (int)rnd(5);
  for (int b = 0; b < c.nb; ++b) {
    const int64_t stride = c.C + (int64_t)rnd(4) * rnd(9), off = rnd(5);
    const size_t extent = (size_t)(c.n - 1) * stride + c.C;
    c.blocks.emplace_back(new float[off + extent]);
    float* base = c.blocks.back().get() + off;
    for (int k = 0; k < c.n; ++k) {
      double sum = 0;
      for (int cc = 0; cc < c.C; ++cc) sum += (base[k * stride + cc] = (float)std::exp(uni(-4, 4)));
      for (int cc = 0; cc < c.C; ++cc) base[k * stride + cc] = (float)(base[k * stride + cc] / sum);
      if (round % 3 == 0)
        for (int t = 0; t < 1 + (int)rnd(3); ++t) base[k * stride + rnd(c.C)] = planted((int)rnd(10));
    }
    c.srcs.push_back(dh_vote_src{base, stride});
  }
  c.seq.reset(new int32_t[c.n]);
  for (int k = 0; k < c.n; ++k) c.seq[k] = (int32_t)rnd(c.nseq);
  const size_t na = (size_t)c.nb * c.nseq * c.C;
  c.acc0.reset(new double[na]);
  for (size_t k = 0; k < na; ++k) c.acc0[k] = round % 5 == 0 ? uni(1e-300, 3e-300) : (round % 2 ? 1.0 : uni(0.5, 2.0));
  return c;
}

static void sweep_items() {
  for (int round = 0; round < 3000; ++round) {
    Case c = make_case(round);
    const size_t na = (size_t)c.nb * c.nseq * c.C, nl = (size_t)c.nb * c.n, ns = nl * c.C;
    if (round % 11 == 0) c.seq[rnd(c.n)] = round % 22 ? -1 - (int32_t)rnd(5) : c.nseq + (int32_t)rnd(5);   // an item out of range
    // the scalar restatement
    std::unique_ptr<double[]> want(new double[na]);
    std::unique_ptr<int32_t[]> want_label(new int32_t[nl]);
    std::memcpy(want.get(), c.acc0.get(), 8 * na);
    for (int b = 0; b < c.nb; ++b)
      for (int k = 0; k < c.n; ++k) {
        const int32_t s = c.seq[k];
        if (s < 0 || s >= c.nseq) {
          want_label[(size_t)b * c.n + k] = -1;
          ++n_skipped;
          continue;
        }
        double* row = want.get() + ((size_t)b * c.nseq + s) * c.C;
        for (int cc = c.C - 1; cc >= 0; --cc) {                             // (last-first: the classes are independent)
          volatile double p = row[cc] * (double)c.srcs[b].p[k * c.srcs[b].item_stride + cc];
          row[cc] = p;
          if (p != 0 && std::fabs(p) < std::numeric_limits<double>::min()) ++n_subnormal;
        }
        const int32_t l = scan_argmax(row, c.C);
        if (butterfly_argmax(row, c.C) != l) die("the butterfly picks another class", round, k);
        if (row[l] != row[l]) ++n_nan_labels;
        want_label[(size_t)b * c.n + k] = l;
        ++n_items;
      }
    // one call
    std::unique_ptr<double[]> acc(new double[na]);
    std::unique_ptr<int32_t[]> label(new int32_t[nl]);
    std::unique_ptr<float[]> scores(new float[ns]);
    std::memcpy(acc.get(), c.acc0.get(), 8 * na);
    for (size_t k = 0; k < ns; ++k) scores[k] = -777.125f;
    if (vote_products_host(c.srcs.data(), c.nb, c.C, c.seq.get(), c.n, c.nseq, acc.get(), label.get(), scores.get()) != DH_OK) die("refused", round);
    if (!same_bits(acc.get(), want.get(), na)) die("acc differs from the scalar loop", round);
    if (std::memcmp(label.get(), want_label.get(), 4 * nl) != 0) die("labels differ from the scalar loop", round);
    for (int b = 0; b < c.nb; ++b)
      for (int k = 0; k < c.n; ++k) {
        const bool skipped = c.seq[k] < 0 || c.seq[k] >= c.nseq;
        for (int cc = 0; cc < c.C; ++cc) {
          const float got = scores[((size_t)b * c.n + k) * c.C + cc], p = c.srcs[b].p[k * c.srcs[b].item_stride + cc];
          if (skipped ? got != -777.125f : std::memcmp(&got, &p, 4) != 0) die("scores", round, k);
        }
      }
    // sequences no item names keep their bits
    for (int s = 0; s < c.nseq; ++s) {
      bool named = false;
      for (int k = 0; k < c.n; ++k) named = named || c.seq[k] == s;
      if (named) continue;
      for (int b = 0; b < c.nb; ++b)
        if (std::memcmp(acc.get() + ((size_t)b * c.nseq + s) * c.C, c.acc0.get() + ((size_t)b * c.nseq + s) * c.C, 8 * (size_t)c.C) != 0)
          die("a sequence no item names moved", round, s);
    }
    // two calls over a split, without scores: the same acc, the same labels
    if (c.n > 1) {
      const int n1 = 1 + (int)rnd(c.n - 1), n2 = c.n - n1;
      std::unique_ptr<double[]> part(new double[na]);
      std::memcpy(part.get(), c.acc0.get(), 8 * na);
      std::unique_ptr<int32_t[]> la(new int32_t[(size_t)c.nb * n1]), lb(new int32_t[(size_t)c.nb * n2]);
      std::vector<dh_vote_src> tail = c.srcs;
      for (auto& g : tail) g.p += n1 * g.item_stride;
      if (vote_products_host(c.srcs.data(), c.nb, c.C, c.seq.get(), n1, c.nseq, part.get(), la.get(), nullptr) != DH_OK ||
          vote_products_host(tail.data(), c.nb, c.C, c.seq.get() + n1, n2, c.nseq, part.get(), lb.get(), nullptr) != DH_OK)
        die("a split call was refused", round);
      if (!same_bits(part.get(), acc.get(), na)) die("split calls differ", round, n1);
      for (int b = 0; b < c.nb; ++b)
        for (int k = 0; k < c.n; ++k)
          if ((k < n1 ? la[(size_t)b * n1 + k] : lb[(size_t)b * n2 + k - n1]) != label[(size_t)b * c.n + k]) die("split labels", round, k);
    }
  }
}

static void sweep_order() {
  // the total order on hand-made pairs, against np.argmax's documented answers
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double a[4] = {1, nan, 3, nan}, b[3] = {2, 2, 1}, c[2] = {0.0, -0.0}, d[2] = {inf, nan}, e[3] = {-inf, -inf, -inf}, f[1] = {nan};
  if (scan_argmax(a, 4) != 1 || butterfly_argmax(a, 4) != 1) die("argmax([1, nan, 3, nan])");
  if (scan_argmax(b, 3) != 0 || butterfly_argmax(b, 3) != 0) die("argmax([2, 2, 1])");
  if (scan_argmax(c, 2) != 0 || butterfly_argmax(c, 2) != 0) die("argmax([0.0, -0.0])");
  if (scan_argmax(d, 2) != 1 || butterfly_argmax(d, 2) != 1) die("argmax([inf, nan])");
  if (scan_argmax(e, 3) != 0 || butterfly_argmax(e, 3) != 0) die("argmax([-inf, -inf, -inf])");
  if (scan_argmax(f, 1) != 0 || butterfly_argmax(f, 1) != 0) die("argmax([nan])");
}

static void sweep_refusals() {
  float p[64];
  int32_t seq[4] = {0, 1, 2, 0}, label[8];
  double acc[2 * 3 * 15];
  float scores[2 * 4 * 15];
  for (float& v : p) v = 0.5f;
  for (double& v : acc) v = 1.0;
  const dh_vote_src good[2] = {{p, 15}, {p + 1, 16}};
  auto call = [&](const dh_vote_src* s, int nb, int C, const int32_t* q, int n, int nseq, double* a, int32_t* l, float* sc) {
    const int rc = vote_products_host(s, nb, C, q, n, nseq, a, l, sc);
    if (rc == DH_EINVAL) ++n_refused;
    return rc;
  };
  if (call(good, 2, 15, seq, 4, 3, acc, label, scores) != DH_OK) die("the good call was refused");
  if (call(good, 2, 15, seq, 4, 3, acc, label, nullptr) != DH_OK) die("the good call without scores was refused");
  auto bad = [&](int rc, int line) {
    if (rc != DH_EINVAL) die("not refused, line", line);
  };
  bad(call(nullptr, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, nullptr, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 3, nullptr, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 3, acc, nullptr, scores), __LINE__);
  bad(call(good, 0, 15, seq, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, -2, 15, seq, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 0, seq, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, -15, seq, 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 0, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, -4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 0, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, -3, acc, label, scores), __LINE__);
  bad(call(good, 2, 16, seq, 4, 3, acc, label, scores), __LINE__);                                  // source 0: item_stride 15 < C
  auto at = [](void* q, int bytes) { return reinterpret_cast<char*>(q) + bytes; };
  bad(call(good, 2, 15, reinterpret_cast<int32_t*>(at(seq, 2)), 4, 3, acc, label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 3, reinterpret_cast<double*>(at(acc, 4)), label, scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 3, acc, reinterpret_cast<int32_t*>(at(label, 1)), scores), __LINE__);
  bad(call(good, 2, 15, seq, 4, 3, acc, label, reinterpret_cast<float*>(at(scores, 2))), __LINE__);
  for (int k = 0; k < 2; ++k) {
    dh_vote_src s[2] = {good[0], good[1]};
    s[k].p = nullptr;
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k].p = reinterpret_cast<const float*>(at(p, 2));
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k] = good[k];
    s[k].item_stride = 14;
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k].item_stride = 0;
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k].item_stride = -15;
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k].item_stride = kVoteMaxStride + 1;
    bad(call(s, 2, 15, seq, 4, 3, acc, label, scores), __LINE__);
    s[k].item_stride = kVoteMaxStride;
    bad(call(s, 2, 15, seq, 0x7fffffff, 3, acc, label, scores), __LINE__);                          // (n - 1) * item_stride above 2^58
  }
  bad(call(good, 2, 0x7fffffff, seq, 4, 0x7fffffff, acc, label, scores), __LINE__);                 // nseq * C above 2^58
  bad(call(good, 0x7fffffff, 15, seq, 4, 0x7fffffff, acc, label, scores), __LINE__);                // nb * nseq * C above 2^58
  bad(call(good, 0x7fffffff, 15, seq, 0x7fffffff, 3, acc, label, scores), __LINE__);                // nb * n * C above 2^58
}

int main() {
  sweep_order();
  sweep_items();
  sweep_refusals();
  if (n_items < 10000 || n_nan_labels < 50 || n_skipped < 100 || n_subnormal < 100 || n_refused < 30) {
    std::printf("vote_sweep: thin coverage: %lld items, %lld NaN labels, %lld skipped, %lld subnormal products, %lld refusals\n", n_items,
                n_nan_labels, n_skipped, n_subnormal, n_refused);
    return 1;
  }
  std::printf("vote_sweep: ok (%lld items, %lld NaN labels, %lld skipped, %lld subnormal products, %lld refusals)\n", n_items, n_nan_labels,
              n_skipped, n_subnormal, n_refused);
  return 0;
}
