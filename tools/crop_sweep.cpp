// Host-only sweep of the crop front end's index module (deephar_amd/csrc/crop_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc
//       tools/crop_sweep.cpp -o /tmp/crop_sweep && /tmp/crop_sweep
//
// 1. dh::crop_axis_coeffs over a grid of (in, out): tables in heap blocks of exactly their length; first / count inside the
//    axis, count <= taps, every k >= 0, the k of an output sum to 2^22 within one unit per tap.  dh::crop_axis_output, the
//    per-output function the device builder runs one lane per index of, called for single indices in DESCENDING order into
//    blocks of their own: the same table, and nothing outside row i is touched.
// 2. crop programs over a grid of image sizes, output sizes and windows (inside, overhanging every edge, fully outside, one
//    pixel wide, scale exactly 16), several jobs and sources per program, row pitches above 3 W: program, sources and
//    destination each in a heap block of exactly its length, guard bytes around every destination item; dh::crop_resize_host
//    against the two passes written out long-hand with a materialised crop and a materialised horizontal intermediate.
//    dh::crop_program_max_bytes covers every one of them, is reached exactly by a table of jobs at the scale cap, and the 4
//    bytes behind a table of odd length are written (0) whatever the buffer held.
// 3. refusals: scale above 16 (DH_EUNSUPPORTED, nothing written), empty boxes, bad source index, short pitch, short program
//    buffer, and programs with one field broken (DH_EINVAL each, destination untouched).
// Not a pytest test: nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crop_index.h"

using namespace dh;

static long long n_axes = 0, n_jobs = 0, n_refused = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("crop_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (rng_state >> 8) % n;
}

struct Axis {
  int taps;
  std::vector<int32_t> first, count, k;
  Axis(int in, int out) : taps(crop_axis_taps(in, out)), first(out), count(out), k((size_t)out * taps) {
    crop_axis_coeffs(in, out, taps, first.data(), count.data(), k.data());
  }
};

static void sweep_axes() {
  for (int out : {1, 2, 3, 5, 8, 31, 64, 256})
    for (int in = 1; in <= 16 * out && in <= 1300; in += (in < 70 ? 1 : 37)) {
      Axis a(in, out);
      if (a.taps > kCropMaxTaps) die("taps above the bound", in, out);
      for (int i = 0; i < out; ++i) {
        if (a.first[i] < 0 || a.count[i] < 1 || a.count[i] > a.taps || a.first[i] + a.count[i] > in) die("axis bounds", in, out);
        long long sum = 0;
        for (int j = 0; j < a.taps; ++j) {
          const int32_t k = a.k[(size_t)i * a.taps + j];
          if (k < 0 || (j >= a.count[i] && k != 0)) die("coefficient", in, out);
          sum += k;
        }
        if (sum < (1 << 22) - a.taps || sum > (1 << 22) + a.taps) die("coefficients do not sum to one", in, out);
      }
      // one output at a time, last index first, into tables filled with a sentinel
      const int32_t mark = -77;
      std::vector<int32_t> first(out, mark), count(out, mark), k((size_t)out * a.taps, mark);
      const CropAxis ax = crop_axis_setup(in, out);
      for (int i = out - 1; i >= 0; --i) {
        crop_axis_output(ax, in, a.taps, i, first.data(), count.data(), k.data());
        for (int r = 0; r < i; ++r)
          if (first[r] != mark || count[r] != mark || k[(size_t)r * a.taps] != mark || k[(size_t)(r + 1) * a.taps - 1] != mark)
            die("crop_axis_output wrote outside its row", in, out);
      }
      if (first != a.first || count != a.count || k != a.k) die("per-output tables differ from the axis loop", in, out);
      ++n_axes;
    }
}

struct Image {
  int H, W;
  int64_t pitch;
  std::vector<uint8_t> px;
  Image(int h, int w, int extra) : H(h), W(w), pitch(3 * w + extra), px((size_t)h * (3 * w + extra)) {
    for (auto& b : px) b = (uint8_t)rnd(256);
  }
};

// the two passes with everything materialised: crop, horizontal intermediate (uint8), vertical pass, mirror
static std::vector<uint8_t> long_hand(const Image& im, const dh_crop_job& g, int OH, int OW) {
  const int cw = g.x1 - g.x0, ch = g.y1 - g.y0;
  std::vector<uint8_t> crop((size_t)ch * cw * 3, 0);
  for (int y = 0; y < ch; ++y)
    for (int x = 0; x < cw; ++x) {
      const int sy = g.y0 + y, sx = g.x0 + x;
      if (sy < 0 || sy >= im.H || sx < 0 || sx >= im.W) continue;
      for (int c = 0; c < 3; ++c) crop[((size_t)y * cw + x) * 3 + c] = im.px[(size_t)sy * im.pitch + (size_t)sx * 3 + c];
    }
  Axis ax(cw, OW), ay(ch, OH);
  std::vector<uint8_t> mid((size_t)ch * OW * 3), out((size_t)OH * OW * 3);
  for (int y = 0; y < ch; ++y)
    for (int ox = 0; ox < OW; ++ox)
      for (int c = 0; c < 3; ++c) {
        int32_t acc = 1 << 21;
        for (int j = 0; j < ax.count[ox]; ++j) acc += ax.k[(size_t)ox * ax.taps + j] * crop[((size_t)y * cw + ax.first[ox] + j) * 3 + c];
        const int v = acc >> 22;
        mid[((size_t)y * OW + ox) * 3 + c] = (uint8_t)(v > 255 ? 255 : v);
      }
  for (int oy = 0; oy < OH; ++oy)
    for (int ox = 0; ox < OW; ++ox)
      for (int c = 0; c < 3; ++c) {
        int32_t acc = 1 << 21;
        for (int j = 0; j < ay.count[oy]; ++j) acc += ay.k[(size_t)oy * ay.taps + j] * mid[((size_t)(ay.first[oy] + j) * OW + ox) * 3 + c];
        const int v = acc >> 22;
        const int dx = g.hflip ? OW - 1 - ox : ox;
        out[((size_t)oy * OW + dx) * 3 + c] = (uint8_t)(v > 255 ? 255 : v);
      }
  return out;
}

static dh_crop_job random_job(int nsrc, const std::vector<Image>& ims, int OH, int OW, int kind) {
  dh_crop_job g = {};
  g.src = (int)rnd((uint32_t)nsrc);
  const Image& im = ims[g.src];
  int cw = 1 + (int)rnd((uint32_t)(16 * OW < im.W + 12 ? 16 * OW : im.W + 12));
  int ch = 1 + (int)rnd((uint32_t)(16 * OH < im.H + 12 ? 16 * OH : im.H + 12));
  switch (kind) {
    case 0: g.x0 = (int)rnd((uint32_t)im.W) - 6; g.y0 = (int)rnd((uint32_t)im.H) - 6; break;       // anywhere around the image
    case 1: g.x0 = im.W + (int)rnd(5); g.y0 = (int)rnd((uint32_t)im.H); break;                     // fully outside, right
    case 2: g.x0 = -cw - (int)rnd(5); g.y0 = -ch; break;                                           // fully outside, top left
    case 3: cw = 1; g.x0 = (int)rnd((uint32_t)im.W); g.y0 = -3; break;                             // one pixel wide
    case 4: cw = 16 * OW; ch = 16 * OH; g.x0 = -(int)rnd(9); g.y0 = -(int)rnd(9); break;           // the cap
    default: cw = OW; ch = OH; g.x0 = (int)rnd(4); g.y0 = (int)rnd(4); break;                      // identity in both passes
  }
  g.x1 = g.x0 + cw;
  g.y1 = g.y0 + ch;
  g.hflip = (int)rnd(2);
  return g;
}

static void sweep_programs() {
  const int guard = 24;
  for (int round = 0; round < 160; ++round) {
    const int OH = 1 + (int)rnd(round % 8 == 0 ? 40 : 12), OW = 1 + (int)rnd(round % 8 == 1 ? 40 : 12);
    const int nsrc = 1 + (int)rnd(3), njobs = 1 + (int)rnd(5);
    std::vector<Image> ims;
    for (int s = 0; s < nsrc; ++s) ims.emplace_back(1 + (int)rnd(40), 1 + (int)rnd(40), (int)rnd(2) ? (int)rnd(20) : 0);
    std::vector<dh_crop_src> srcs;
    for (const Image& im : ims) srcs.push_back(dh_crop_src{im.px.data(), im.pitch, im.H, im.W});
    std::vector<dh_crop_job> jobs;
    for (int j = 0; j < njobs; ++j) jobs.push_back(random_job(nsrc, ims, OH, OW, (round + j) % 6));
    size_t bytes = 0;
    if (crop_program_bytes(jobs.data(), njobs, nsrc, OH, OW, &bytes) != DH_OK) die("size query refused a good table", round);
    std::vector<uint64_t> store(bytes / 8);                                    // exactly the program, 8-byte aligned
    if (bytes % 8) die("program size is no multiple of 8", (long long)bytes);
    if (crop_program_max_bytes(njobs, nsrc, OH, OW) < bytes) die("capacity below a program", round);
    std::fill(store.begin(), store.end(), 0xCDCDCDCDCDCDCDCDull);             // the padding behind odd tables must be written
    if (crop_program_build(srcs.data(), nsrc, jobs.data(), njobs, OH, OW, store.data(), bytes) != DH_OK) die("builder refused", round);
    for (int j = 0; j < njobs; ++j) {
      const CropJobView v = crop_job_view(store.data(), j, OH, OW);
      if (crop_axis_table_pad(OW, v.rec.xtaps) && v.xk[(size_t)OW * v.rec.xtaps] != 0) die("x table padding", round, j);
      if (crop_axis_table_pad(OH, v.rec.ytaps) && v.yk[(size_t)OH * v.rec.ytaps] != 0) die("y table padding", round, j);
    }
    const int64_t item = (int64_t)OH * OW * 3 + guard;
    std::vector<uint8_t> y((size_t)(item * njobs), 0xCD);
    if (crop_resize_host(store.data(), bytes, njobs, OH, OW, y.data(), item) != DH_OK) die("host twin refused", round);
    for (int j = 0; j < njobs; ++j) {
      const std::vector<uint8_t> want = long_hand(ims[jobs[j].src], jobs[j], OH, OW);
      if (std::memcmp(want.data(), y.data() + (size_t)j * item, want.size()) != 0) die("host twin differs from the long-hand passes", round, j);
      for (int g = 0; g < guard; ++g)
        if (y[(size_t)j * item + want.size() + g] != 0xCD) die("guard byte overwritten", round, j);
      ++n_jobs;
    }
    // one broken field at a time: the twin refuses and leaves the destination alone
    CropHeader h;
    std::memcpy(&h, store.data(), sizeof(h));
    struct Patch { size_t off; uint32_t val; };
    const size_t jo = h.job_off;
    const Patch patches[] = {{0, 0u}, {4, 0u}, {8, 0u}, {12, (uint32_t)OH + 1}, {20, 8u}, {28, (uint32_t)bytes + 8},
                             {jo + 0, (uint32_t)nsrc}, {jo + 12, (uint32_t)jobs[0].x0}, {jo + 24, 0u}, {jo + 28, 99u},
                             {jo + 32, 0u}, {jo + 36, (uint32_t)bytes}, {jo + 40, 4u}};
    for (const Patch& p : patches) {
      std::vector<uint64_t> bad(store);
      std::memcpy(reinterpret_cast<uint8_t*>(bad.data()) + p.off, &p.val, 4);
      std::vector<uint8_t> y2((size_t)(item * njobs), 0xCD);
      const int rc = crop_resize_host(bad.data(), bytes, njobs, OH, OW, y2.data(), item);
      if (rc != DH_EINVAL) die("a broken program was not refused", round, (long long)p.off);
      for (uint8_t b : y2)
        if (b != 0xCD) die("a refused program wrote", round, (long long)p.off);
      ++n_refused;
    }
    if (crop_resize_host(store.data(), bytes - 8, njobs, OH, OW, y.data(), item) != DH_EINVAL) die("truncated program accepted", round);
    if (crop_resize_host(store.data(), bytes, njobs, OH, OW, y.data(), item - guard - 1) != DH_EINVAL) die("short item pitch accepted", round);
    n_refused += 2;
  }
}

static void sweep_capacity() {
  for (int OH : {1, 4, 7, 256})
    for (int OW : {1, 5, 8, 256})
      for (int njobs : {1, 3, 64}) {
        std::vector<dh_crop_job> jobs((size_t)njobs, dh_crop_job{0, -3, 2, -3 + 16 * OW, 2 + 16 * OH, 0});   // every job at the cap
        size_t bytes = 0;
        if (crop_program_bytes(jobs.data(), njobs, 2, OH, OW, &bytes) != DH_OK) die("cap table refused", OH, OW);
        if (crop_program_max_bytes(njobs, 2, OH, OW) != bytes) die("capacity is not the program at the cap", OH, OW);
        jobs[0].x1 = jobs[0].x0 + 1;                                                                          // one job up-scaled: 3 taps
        if (crop_program_bytes(jobs.data(), njobs, 2, OH, OW, &bytes) != DH_OK || crop_program_max_bytes(njobs, 2, OH, OW) <= bytes)
          die("capacity does not exceed a smaller program", OH, OW);
      }
  if (crop_program_max_bytes(0, 1, 8, 8) != 0 || crop_program_max_bytes(1, 0, 8, 8) != 0 || crop_program_max_bytes(1, 1, 0, 8) != 0 ||
      crop_program_max_bytes(1, 1, 8, kCropMaxExtent + 1) != 0)
    die("capacity of a bad argument");
  n_refused += 4;
}

static void sweep_refusals() {
  Image im(70, 70, 0);
  const dh_crop_src src = {im.px.data(), im.pitch, im.H, im.W};
  size_t bytes = 0;
  std::vector<uint64_t> out(1 << 12, 0);
  const auto untouched = [&] {
    for (uint64_t v : out)
      if (v != 0) die("a refused build wrote");
  };
  const dh_crop_job over_x = {0, 0, 0, 65, 64, 0}, over_y = {0, 0, 0, 64, 65, 0}, cap = {0, 0, 0, 64, 64, 0};
  if (crop_program_bytes(&over_x, 1, 1, 4, 4, &bytes) != DH_EUNSUPPORTED || crop_program_bytes(&over_y, 1, 1, 4, 4, &bytes) != DH_EUNSUPPORTED)
    die("scale above 16 not refused");
  if (crop_program_build(&src, 1, &over_x, 1, 4, 4, out.data(), out.size() * 8) != DH_EUNSUPPORTED) die("builder: scale above 16");
  untouched();
  if (crop_program_bytes(&cap, 1, 1, 4, 4, &bytes) != DH_OK) die("scale 16 refused");
  const dh_crop_job bad_jobs[] = {{0, 5, 0, 5, 9, 0}, {0, 0, 9, 4, 9, 0}, {0, 8, 0, 2, 4, 0}, {1, 0, 0, 4, 4, 0}, {-1, 0, 0, 4, 4, 0}};
  for (const dh_crop_job& g : bad_jobs) {
    if (crop_program_bytes(&g, 1, 1, 8, 8, &bytes) != DH_EINVAL) die("bad job accepted");
    if (crop_program_build(&src, 1, &g, 1, 8, 8, out.data(), out.size() * 8) != DH_EINVAL) die("builder: bad job accepted");
    ++n_refused;
  }
  const dh_crop_job ok = {0, 0, 0, 32, 32, 0};
  const dh_crop_src bad_srcs[] = {{nullptr, 210, 70, 70}, {im.px.data(), 209, 70, 70}, {im.px.data(), 210, 0, 70}, {im.px.data(), 210, 70, 0}};
  for (const dh_crop_src& s : bad_srcs) {
    if (crop_program_build(&s, 1, &ok, 1, 8, 8, out.data(), out.size() * 8) != DH_EINVAL) die("bad source accepted");
    ++n_refused;
  }
  if (crop_program_bytes(&ok, 1, 1, 8, 8, &bytes) != DH_OK) die("good job refused");
  if (crop_program_build(&src, 1, &ok, 1, 8, 8, out.data(), bytes - 1) != DH_EINVAL) die("short buffer accepted");
  if (crop_program_build(nullptr, 1, &ok, 1, 8, 8, out.data(), bytes) != DH_EINVAL || crop_program_build(&src, 1, &ok, 1, 8, 8, nullptr, bytes) != DH_EINVAL ||
      crop_program_build(&src, 1, nullptr, 1, 8, 8, out.data(), bytes) != DH_EINVAL)
    die("NULL accepted");
  if (crop_program_build(&src, 1, &ok, 1, 8, 8, reinterpret_cast<uint8_t*>(out.data()) + 4, bytes) != DH_EINVAL) die("misaligned buffer accepted");
  untouched();
  // a very wide output: the rows one output row reads do not fit LDS
  const dh_crop_job wide = {0, 0, 0, 70, 60, 0};
  if (crop_program_bytes(&wide, 1, 1, 4, 30000, &bytes) != DH_OK) die("wide size query");
  std::vector<uint64_t> big(bytes / 8 + 1, 0);
  if (crop_program_build(&src, 1, &wide, 1, 4, 30000, big.data(), bytes) != DH_EUNSUPPORTED) die("wide output accepted");
  n_refused += 6;
}

int main() {
  sweep_axes();
  sweep_programs();
  sweep_capacity();
  sweep_refusals();
  std::printf("crop_sweep: %lld axes, %lld jobs equal to the long-hand passes, %lld refusals -- clean\n", n_axes, n_jobs, n_refused);
  return 0;
}
