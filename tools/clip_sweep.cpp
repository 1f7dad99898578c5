// Host-only sweep of the clip boundary (deephar_amd/csrc/cut_index.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc \
//       tools/clip_sweep.cpp -o /tmp/clip_sweep && /tmp/clip_sweep
//
// 1. dh::clip_parse on containers assembled here around stub plan blobs, each copied into a heap block of exactly its length
//    (a read past the end is an AddressSanitizer report): the well-formed one parses and gives its fields back, every
//    truncation length and every single corrupted header field or table entry is DH_EINVAL.
// 2. dh::unpack_cut_host against a gather written out long-hand (dst[n, g * Tl + t, p, j] = src[g, n, t, p, coff + j]) over
//    G x m x Tl x P x Cp and segment sets with narrow and wide segments, pitches ld == c and ld > c; the guard columns
//    behind c and the guard floats around every destination must keep their value.
// Not a pytest test: nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cut_index.h"

using namespace dh;

static long long n_parsed = 0, n_refused = 0, n_unpacked = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("clip_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

static void put32(std::vector<unsigned char>& v, size_t at, uint32_t x) { std::memcpy(v.data() + at, &x, 4); }
static void put64(std::vector<unsigned char>& v, size_t at, uint64_t x) { std::memcpy(v.data() + at, &x, 8); }

struct Spec {
  uint32_t world, T, Tl, Cp;
  uint64_t P;
  std::vector<uint32_t> cut;       // offset, channels, ...
  std::vector<uint32_t> outs;      // kind, index, ...
  size_t frames_bytes, head_bytes;
};

static std::vector<unsigned char> assemble(const Spec& s) {
  const size_t tables = kClipHeader + 4 * s.cut.size() + 4 * s.outs.size();
  const size_t foff = (size_t)clip_align(tables), hoff = (size_t)clip_align(foff + s.frames_bytes);
  std::vector<unsigned char> v(hoff + s.head_bytes, 0);
  std::memcpy(v.data(), "DHCL", 4);
  put32(v, 4, kClipVersion); put32(v, 8, s.world); put32(v, 12, s.T); put32(v, 16, s.Tl); put32(v, 20, s.Cp);
  put64(v, 24, s.P); put32(v, 32, (uint32_t)(s.cut.size() / 2)); put32(v, 36, (uint32_t)(s.outs.size() / 2));
  put64(v, 40, foff); put64(v, 48, s.frames_bytes); put64(v, 56, hoff); put64(v, 64, s.head_bytes);
  for (size_t i = 0; i < s.cut.size(); ++i) put32(v, kClipHeader + 4 * i, s.cut[i]);
  for (size_t i = 0; i < s.outs.size(); ++i) put32(v, kClipHeader + 4 * s.cut.size() + 4 * i, s.outs[i]);
  for (size_t i = 4; i < s.frames_bytes; ++i) v[foff + i] = (unsigned char)(i * 7);
  std::memcpy(v.data() + foff, "DHPL", 4);
  if (s.head_bytes) {
    for (size_t i = 4; i < s.head_bytes; ++i) v[hoff + i] = (unsigned char)(i * 11);
    std::memcpy(v.data() + hoff, "DHPL", 4);
  }
  return v;
}

// parse a copy that owns exactly `len` bytes
static int parse_exact(const std::vector<unsigned char>& v, size_t len, ClipBlob* cb) {
  unsigned char* p = static_cast<unsigned char*>(std::malloc(len ? len : 1));
  std::memcpy(p, v.data(), len);
  ClipBlob local;
  const int rc = clip_parse(p, len, &local);
  if (rc == DH_OK && cb) {
    *cb = local;
    cb->cut = nullptr;             // (they point into the freed copy)
    cb->outputs = nullptr;
  }
  std::free(p);
  return rc;
}

static void expect_refused(std::vector<unsigned char> v, size_t at, uint32_t value, const char* what) {
  put32(v, at, value);
  if (parse_exact(v, v.size(), nullptr) != DH_EINVAL) die(what, (long long)at, value);
  ++n_refused;
}

static void container_sweep(const Spec& s) {
  const std::vector<unsigned char> v = assemble(s);
  ClipBlob cb;
  if (parse_exact(v, v.size(), &cb) != DH_OK) die("well-formed container refused", (long long)v.size());
  ++n_parsed;
  const dh_clip_info& o = cb.info;
  uint32_t nhead = 0;
  for (size_t k = 0; k < s.outs.size(); k += 2) nhead += s.outs[k] == 1;
  if (o.version != 1 || (uint32_t)o.world != s.world || (uint32_t)o.T != s.T || (uint32_t)o.Tl != s.Tl ||
      (uint32_t)o.packed_channels != s.Cp || (uint64_t)o.P != s.P || (size_t)o.num_cut != s.cut.size() / 2 ||
      (size_t)o.num_outputs != s.outs.size() / 2 || (uint32_t)o.num_head_outputs != nhead || o.frames_bytes != s.frames_bytes ||
      o.head_bytes != s.head_bytes || o.frames_offset % 256 || o.head_offset % 256 || o.head_offset + o.head_bytes != v.size())
    die("fields do not round-trip");
  for (size_t len = 0; len < v.size(); ++len) {
    if (parse_exact(v, len, nullptr) != DH_EINVAL) die("truncated container accepted", (long long)len);
    ++n_refused;
  }
  std::vector<unsigned char> longer = v;
  longer.push_back(0);
  if (parse_exact(longer, longer.size(), nullptr) != DH_EINVAL) die("trailing byte accepted");
  // header fields
  expect_refused(v, 0, 0x4c434844u ^ 1u, "magic");
  expect_refused(v, 4, 2, "version");
  expect_refused(v, 8, 0, "world 0");
  expect_refused(v, 8, s.T + 1, "world not dividing T");
  if (s.T > 1 && s.T % (s.world + 1) != 0) expect_refused(v, 8, s.world + 1, "world not dividing T");
  expect_refused(v, 12, 0, "T 0");
  expect_refused(v, 16, s.Tl + 1, "Tl != T / world");
  expect_refused(v, 20, 0, "Cp 0");
  expect_refused(v, 24, 0, "P 0 (low word)");
  expect_refused(v, 28, 0x80000000u, "P huge");
  expect_refused(v, 32, 0, "no cut tensor");
  expect_refused(v, 32, 0xffffffffu, "cut count");
  expect_refused(v, 36, 0, "no output");
  expect_refused(v, 36, 0xffffffffu, "output count");
  for (size_t at = 40; at < kClipHeader; at += 8) {
    std::vector<unsigned char> w = v;
    uint64_t x;
    for (int64_t d : {-256, -1, 1, 256}) {
      if (at == 48 && (d == 1 || d == -1)) continue;      // (a frames blob one byte longer or shorter inside its padding is well formed)
      std::memcpy(&x, v.data() + at, 8);
      put64(w, at, x + (uint64_t)d);
      if (parse_exact(w, w.size(), nullptr) != DH_EINVAL) die("blob extent accepted", (long long)at, d);
      ++n_refused;
    }
    put64(w, at, ~0ull);
    if (parse_exact(w, w.size(), nullptr) != DH_EINVAL) die("blob extent ~0 accepted", (long long)at);
    put64(w, at, 1ull << 63);
    if (parse_exact(w, w.size(), nullptr) != DH_EINVAL) die("blob extent 2^63 accepted", (long long)at);
    n_refused += 2;
  }
  // every table entry, one at a time
  for (size_t i = 0; i < s.cut.size() / 2; ++i) {
    const size_t at = kClipHeader + 8 * i;
    expect_refused(v, at, s.Cp - s.cut[2 * i + 1] + 1, "offset + channels > Cp");
    expect_refused(v, at, 0xffffffffu, "offset wraps");
    expect_refused(v, at + 4, s.Cp - s.cut[2 * i] + 1, "offset + channels > Cp");
    expect_refused(v, at + 4, 0, "channels 0");
    expect_refused(v, at + 4, 0xffffffffu, "channels wrap");
  }
  for (size_t k = 0; k < s.outs.size() / 2; ++k) {
    const size_t at = kClipHeader + 4 * s.cut.size() + 8 * k;
    expect_refused(v, at, 2, "output kind");
    expect_refused(v, at + 4, s.outs[2 * k] == 0 ? (uint32_t)(s.cut.size() / 2) : nhead, "output index out of range");
    expect_refused(v, at + 4, 0xffffffffu, "output index out of range");
  }
  // the plan blobs' magic
  expect_refused(v, (size_t)o.frames_offset, 0, "frames plan magic");
  if (s.head_bytes) expect_refused(v, (size_t)o.head_offset, 0, "head plan magic");
}

// ---- unpack ---------------------------------------------------------------------------------------------------------------
struct SegSpec { int coff, c, ld; };

static void unpack_case(int G, int m, int Tl, int64_t P, int Cp, const std::vector<SegSpec>& specs) {
  const int64_t T = (int64_t)G * Tl, total = (int64_t)G * m * Tl * P * Cp;
  std::vector<float> src((size_t)total);
  for (int64_t i = 0; i < total; ++i) src[(size_t)i] = (float)(i % 8191) + 0.25f;
  const int guard = 3;
  std::vector<std::vector<float>> dst(specs.size()), want(specs.size());
  std::vector<dh_cut_seg> segs;
  for (size_t s = 0; s < specs.size(); ++s) {
    const int64_t rows = m * T * P;
    dst[s].assign((size_t)(rows * specs[s].ld + 2 * guard), -7.f);
    want[s] = dst[s];
    segs.push_back({dst[s].data() + guard, specs[s].ld, specs[s].coff, specs[s].c, 0});
    for (int g = 0; g < G; ++g)
      for (int n = 0; n < m; ++n)
        for (int t = 0; t < Tl; ++t)
          for (int64_t p = 0; p < P; ++p)
            for (int j = 0; j < specs[s].c; ++j)
              want[s][(size_t)(guard + ((n * T + g * Tl + t) * P + p) * specs[s].ld + j)] =
                  src[(size_t)(((((int64_t)g * m + n) * Tl + t) * P + p) * Cp + specs[s].coff + j)];
  }
  if (unpack_cut_host(src.data(), G, m, Tl, P, Cp, segs.data(), (int)segs.size()) != DH_OK) die("unpack refused", Cp, (long long)specs.size());
  for (size_t s = 0; s < specs.size(); ++s)
    if (std::memcmp(dst[s].data(), want[s].data(), dst[s].size() * 4) != 0) die("unpack differs", Cp, (long long)s);
  ++n_unpacked;
}

static std::vector<SegSpec> segment_set(int Cp, int start, bool padded) {
  std::vector<SegSpec> v;
  const int widths[] = {1, 2, 3, 4, 5, 16};
  int off = start;
  for (int w : widths) {
    if (off + w > Cp) break;
    v.push_back({off, w, padded ? w + (w % 4 == 0 ? 4 : 3) : w});
    off += w;
  }
  if (off < Cp) v.push_back({off, Cp - off, padded ? Cp - off + 4 : Cp - off});      // the remainder: the wide segment
  return v;
}

int main() {
  // containers: merge-like (head + pass-through), pose-only (no head), one cut tensor used twice, many segments
  container_sweep({2, 8, 4, 581, 16, {0, 2, 2, 1, 3, 576, 579, 2}, {0, 0, 0, 1, 1, 0, 1, 1}, 300, 200});
  container_sweep({1, 4, 4, 24, 1, {0, 3, 3, 1}, {0, 0, 0, 1}, 44, 0});
  container_sweep({3, 3, 1, 7, 5, {0, 7}, {1, 0, 0, 0, 0, 0}, 257, 44});
  {
    Spec s = {4, 16, 4, 200, 34, {}, {}, 512, 256};
    for (uint32_t i = 0; i < 100; ++i) { s.cut.push_back(2 * i); s.cut.push_back(2); }
    for (uint32_t i = 0; i < 100; ++i) { s.outs.push_back(i % 2); s.outs.push_back(i % 2 ? i / 2 : i); }
    container_sweep(s);
  }
  for (int G : {1, 2, 3})
    for (int m : {1, 2})
      for (int Tl : {1, 3})
        for (int64_t P : {1, 5, 16})
          for (int Cp : {7, 24, 581})
            for (int start : {0, 1, 4})
              for (bool padded : {false, true}) unpack_case(G, m, Tl, P, Cp, segment_set(Cp, start, padded));
  // refused requests touch nothing
  float one = 1.f, d = 0.f;
  dh_cut_seg bad[4] = {{&d, 1, 7, 1, 0}, {&d, 1, -1, 1, 0}, {&d, 0, 0, 1, 0}, {nullptr, 1, 0, 1, 0}};
  for (const dh_cut_seg& b : bad)
    if (unpack_cut_host(&one, 1, 1, 1, 1, 7, &b, 1) != DH_EINVAL) die("bad segment accepted");
  if (unpack_cut_host(&one, 0, 1, 1, 1, 7, bad, 0) != DH_EINVAL || unpack_cut_host(&one, 1 << 20, 1 << 20, 1 << 20, 1, 7, bad, 0) != DH_EINVAL)
    die("bad geometry accepted");
  std::printf("clip_sweep ok: %lld containers parsed, %lld malformed ones refused, %lld unpack cases equal\n", n_parsed, n_refused,
              n_unpacked);
  return 0;
}
