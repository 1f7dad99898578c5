// The arithmetic of the multi-clip action vote (dh_vote_products_f64, vote.hip) as pure functions: the running PRODUCT of the
// per-clip class probabilities of every sequence and the running arg-max label behind every clip.  It restates the inner loop of
// deephar_amd/evaltools/action.py:_multiclip (exp/common/penn_tools.py:85-163, exp/common/ntu_tools.py:53-152 in the reference)
//     a_pred[b, i, :] *= pred[b][0];   np.argmax(a_pred[-1, i])
// with a float64 a_pred and a float32 pred.  No HIP header, no stream.  The kernel, the host twin, tools/vote_sweep.cpp and the
// host tests use these.
//
// An ITEM k is one clip's result: nb probability rows p_b[k, 0:C] (float32, one per action output b) of sequence seq[k].  For
// k = 0 .. n-1 IN THAT ORDER and every b:
//     acc[b, seq[k], c] = acc[b, seq[k], c] * (double)p_b[k, c]          one IEEE double multiply, nothing else
//     label[b, k]       = argmax_c acc[b, seq[k], :]                     np.argmax's rule, its NaN rule included
//     scores[b, k, c]   = p_b[k, c]                                       (a plain copy, if wanted)
// Like posebox_index.h, the arithmetic runs on the host AND on the device and both must give the same bits.  The conversion
// float -> double is exact and the product is one operation with nothing to contract into (DH_CROP_NO_CONTRACT stands anyway).
// What could still differ between the two sides is pinned here:
//   order     : only the order of the ITEMS matters, and both sides walk them serially.  The classes of one item are
//               independent products.
//   arg-max   : np.argmax takes the first maximum, a NaN beats every number, the first NaN wins.  That is the minimum of a TOTAL
//               order on (value, index) pairs -- NaN first, then the larger value (+0 and -0 compare equal), then the lower
//               index -- so the host's scan in ascending c and the device's cross-lane butterfly pick the same pair whatever the
//               order of the reduction.  Only the INDEX leaves: the bits of a NaN (x86 and gfx950 do not make the same NaN from
//               inf * 0) stay in acc, where each side keeps its own; every comparison treats all NaNs alike.
//   denormals : products may go subnormal and reach zero exactly as numpy's do.  Neither side flushes double denormals (the
//               build has no flag that would; a test holds the device to it).
// There is no status word: every input has a defined result.  An item whose seq[k] is outside [0, nseq) is skipped: label -1,
// acc and its scores rows untouched.
#pragma once
#include <stdint.h>
#include <string.h>
#include "crop_index.h"

namespace dh {

constexpr int kVoteWave = 64;                     // lanes over the classes of one item
constexpr int kVoteMaxSrcs = 32;                  // sources (action outputs b) one launch takes by value
constexpr int64_t kVoteMaxStride = (int64_t)1 << 40;
constexpr int64_t kVoteMaxSpan = (int64_t)1 << 58;      // (n - 1) * item_stride, and the elements of acc and of scores_out

// a candidate of the arg-max: the product and its class
struct VoteBest {
  double v;
  int32_t i;
};
// what a lane without a class holds: every real candidate (index < 2^31 - 1) beats it, -inf included
DH_CROP_HD inline VoteBest vote_best_none() {
  const uint64_t bits = 0xfff0000000000000ull;    // -inf
  VoteBest e;
  memcpy(&e.v, &bits, 8);
  e.i = 0x7fffffff;
  return e;
}
// the total order: does a come before b?  NaN first, then the larger value, then the lower index
DH_CROP_HD inline bool vote_before(const VoteBest& a, const VoteBest& b) {
  const bool an = a.v != a.v, bn = b.v != b.v;
  if (an != bn) return an;
  if (!an) {
    if (a.v > b.v) return true;
    if (a.v < b.v) return false;
  }
  return a.i < b.i;
}
DH_CROP_HD inline VoteBest vote_first(const VoteBest& a, const VoteBest& b) { return vote_before(b, a) ? b : a; }

// classes c0, c0 + step, ... of one item of one output: the products into `arow` (the sequence's row of acc), the copy into
// `srow` if given; returns the first of them in the total order
DH_CROP_HD inline VoteBest vote_item(const float* row, double* arow, float* srow, int C, int c0, int step) {
  DH_CROP_NO_CONTRACT
  VoteBest best = vote_best_none();
  for (int c = c0; c < C; c += step) {
    const float p = row[c];
    VoteBest e;
    e.v = arow[c] * (double)p;
    e.i = c;
    arow[c] = e.v;
    if (srow != nullptr) srow[c] = p;
    best = vote_first(best, e);
  }
  return best;
}

// ---- argument checks the launch and the host twin share ---------------------------------------------------------------------
// item_stride is in floats and lies in [C, 2^40]; (n - 1) * item_stride, nb * nseq * C and nb * n * C lie in [0, 2^58], so no
// offset in the kernel or the twin, nor its byte offset, can leave int64.
inline int vote_args(const dh_vote_src* srcs, int nb, int C, const int32_t* seq, int n, int nseq, const double* acc,
                     const int32_t* label_out, const float* scores_out) {
  if (srcs == nullptr || seq == nullptr || acc == nullptr || label_out == nullptr || nb < 1 || C < 1 || n < 1 || nseq < 1)
    return DH_EINVAL;
  if (((uintptr_t)seq & 3) != 0 || ((uintptr_t)acc & 7) != 0 || ((uintptr_t)label_out & 3) != 0 || ((uintptr_t)scores_out & 3) != 0)
    return DH_EINVAL;
  if ((int64_t)nseq > kVoteMaxSpan / C || (int64_t)nb > kVoteMaxSpan / ((int64_t)nseq * C)) return DH_EINVAL;
  if ((int64_t)n > kVoteMaxSpan / C || (int64_t)nb > kVoteMaxSpan / ((int64_t)n * C)) return DH_EINVAL;
  for (int b = 0; b < nb; ++b) {
    const dh_vote_src& g = srcs[b];
    if (g.p == nullptr || ((uintptr_t)g.p & 3) != 0 || g.item_stride < C || g.item_stride > kVoteMaxStride ||
        (int64_t)(n - 1) > kVoteMaxSpan / g.item_stride)
      return DH_EINVAL;
  }
  return DH_OK;
}

// ---- the host twin -----------------------------------------------------------------------------------------------------------
inline int vote_products_host(const dh_vote_src* srcs, int nb, int C, const int32_t* seq, int n, int nseq, double* acc,
                              int32_t* label_out, float* scores_out) {
  const int rc = vote_args(srcs, nb, C, seq, n, nseq, acc, label_out, scores_out);
  if (rc != DH_OK) return rc;
  for (int64_t b = 0; b < nb; ++b) {
    const dh_vote_src g = srcs[b];
    double* accb = acc + b * nseq * C;
    for (int64_t k = 0; k < n; ++k) {
      const int32_t s = seq[k];
      if (s < 0 || s >= nseq) {
        label_out[b * n + k] = -1;
        continue;
      }
      float* srow = scores_out != nullptr ? scores_out + (b * n + k) * C : nullptr;
      label_out[b * n + k] = vote_item(g.p + k * g.item_stride, accb + (int64_t)s * C, srow, C, 0, 1).i;
    }
  }
  return DH_OK;
}

}  // namespace dh
