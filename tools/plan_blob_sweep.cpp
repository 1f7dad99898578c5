// Host-only sweep of the plan blob's parser (deephar_amd/csrc/plan_blob.h: no HIP header) for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Ideephar_amd/csrc \
//       tools/plan_blob_sweep.cpp -o /tmp/plan_blob_sweep && /tmp/plan_blob_sweep model.dhplan
//
// model.dhplan: a 'DHPL' blob (Model.export_plan, or serialize.pack_plan without a device).  Every run of dh::plan_parse gets a
// copy of the blob in a heap block of exactly its length (a read past the end is an AddressSanitizer report):
// 1. the blob itself parses; every step's payload, copied, goes through dh::plan_patch against three fake regions, and every
//    patched pointer is NULL or lies inside the region its tag named;
// 2. every proper prefix and the blob plus one byte are DH_EINVAL;
// 3. every single-byte change of the part in front of the weight image (each byte xor 0x01, xor 0x80 and set to 0xff) parses
//    to DH_OK or DH_EINVAL without leaving the block; a change the parser accepts still patches inside the regions.
// Not a pytest test: nothing here is loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plan_blob.h"

using namespace dh;

static long long n_parsed = 0, n_refused = 0, n_patched = 0;

static void die(const char* what, long long a = 0, long long b = 0) {
  std::printf("plan_blob_sweep: %s (%lld, %lld)\n", what, a, b);
  std::exit(1);
}

// every step of a parsed image through plan_patch, with the regions at three fake addresses
static void patch_all(const PlanImage& im) {
  char* const arena = reinterpret_cast<char*>(uintptr_t(1) << 40);
  char* const weights = reinterpret_cast<char*>(uintptr_t(2) << 40);
  char* const bytes = reinterpret_cast<char*>(uintptr_t(3) << 40);
  const dh_plan_info& h = im.info;
  for (const PlanStep& ps : im.steps) {
    const Record& rec = kRecords[ps.fn];
    if (ps.bytes != rec.bytes) die("payload size", ps.fn, ps.bytes);
    std::vector<unsigned char> copy(ps.payload, ps.payload + ps.bytes);
    if (plan_patch(copy.data(), rec, arena, weights, bytes) != DH_OK) die("plan_patch refused a parsed step", ps.fn);
    for (uint32_t k = 0; k < rec.nptr; ++k) {
      uint64_t tag;
      char* ptr;
      std::memcpy(&tag, ps.payload + rec.ptr[k], 8);
      std::memcpy(&ptr, copy.data() + rec.ptr[k], 8);
      const bool inside = (ptr >= arena && (uint64_t)(ptr - arena) < h.arena_bytes && tag >> 60 == 1) ||
                          (ptr >= weights && (uint64_t)(ptr - weights) < h.weight_bytes && tag >> 60 == 2) ||
                          (ptr >= bytes && (uint64_t)(ptr - bytes) < h.byte_bytes && tag >> 60 == 3);
      if (!(tag == 0 ? ptr == nullptr : inside)) die("patched pointer leaves its region", ps.fn, k);
      ++n_patched;
    }
  }
}

// parse a copy that owns exactly `len` bytes
static int parse_exact(const unsigned char* src, size_t len, bool patch) {
  unsigned char* p = static_cast<unsigned char*>(std::malloc(len ? len : 1));
  std::memcpy(p, src, len);
  PlanImage im;
  const int rc = plan_parse(p, len, &im);
  if (rc != DH_OK && rc != DH_EINVAL) die("plan_parse answers DH_OK or DH_EINVAL", rc);
  if (rc == DH_OK) {
    if (im.weights + im.info.weight_bytes != p + len) die("the weight image is not the end of the blob");
    if (patch) patch_all(im);
    ++n_parsed;
  } else {
    ++n_refused;
  }
  std::free(p);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 2) die("usage: plan_blob_sweep <blob file>");
  std::FILE* f = std::fopen(argv[1], "rb");
  if (f == nullptr) die("cannot open the blob");
  std::vector<unsigned char> v;
  unsigned char buf[1 << 16];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  if (parse_exact(v.data(), v.size(), true) != DH_OK) die("the blob itself is refused", (long long)v.size());
  PlanImage whole;
  plan_parse(v.data(), v.size(), &whole);
  const size_t front = v.size() - (size_t)whole.info.weight_bytes;
  for (size_t len = 0; len < v.size(); ++len)
    if (parse_exact(v.data(), len, false) != DH_EINVAL) die("a truncated blob is accepted", (long long)len);
  std::vector<unsigned char> w = v;
  w.push_back(0);
  if (parse_exact(w.data(), w.size(), false) != DH_EINVAL) die("a trailing byte is accepted");
  w.pop_back();
  for (size_t at = 0; at < front; ++at) {
    for (int how = 0; how < 3; ++how) {
      w[at] = how == 0 ? v[at] ^ 0x01 : (how == 1 ? v[at] ^ 0x80 : 0xff);
      if (w[at] != v[at]) parse_exact(w.data(), w.size(), true);
    }
    w[at] = v[at];
  }
  std::printf("plan_blob_sweep: ok (%zu bytes, %zu in front of the image; %lld parsed, %lld refused, %lld pointers patched)\n", v.size(),
              front, n_parsed, n_refused, n_patched);
  return 0;
}
