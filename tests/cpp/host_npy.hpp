// host_npy.hpp -- what the programs that run kernel code on the host (tests/cpp/*_host_main.cpp) share on the data side:
// reading the .npy dumps of a test (numpy's format, version 1, C order, little endian; the header is skipped and the payload
// size checked; tests/host_run.py: dump_case writes them) into allocations of EXACTLY the payload, so that the sanitizers see
// a load past the end, and comparing a result with the definition's byte for byte.  No HIP in it.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static bool read_npy(const std::string& path, size_t bytes, std::unique_ptr<uint8_t[]>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  uint8_t head[10];
  bool ok = f && fread(head, 1, 10, f) == 10 && !memcmp(head, "\x93NUMPY\x01", 7);
  const size_t hlen = ok ? (size_t)head[8] | ((size_t)head[9] << 8) : 0;
  ok = ok && fseek(f, 0, SEEK_END) == 0 && (size_t)ftell(f) == 10 + hlen + bytes && fseek(f, (long)(10 + hlen), SEEK_SET) == 0;
  out->reset(new uint8_t[bytes ? bytes : 1]());  // exactly sized (one byte where the dump is empty)
  ok = ok && fread(out->get(), 1, bytes, f) == bytes;
  if (f) fclose(f);
  if (!ok) fprintf(stderr, "cannot read %zu payload bytes from %s\n", bytes, path.c_str());
  return ok;
}

// `count` elements from `from` into an allocation of exactly `count` elements: nothing in front, nothing behind
template <typename T>
static std::unique_ptr<T[]> exact_copy(const void* from, size_t count) {
  std::unique_ptr<T[]> q(new T[count]);
  if (count) memcpy(q.get(), from, count * sizeof(T));
  return q;
}

// The dumps of one case: a directory of <name>.npy.  A read that fails says so on stderr, sets `failed` and hands out zeros
// of the size asked for, so that a main reads all it needs and then returns 2 once.
struct Case {
  std::string dir;
  bool failed = false;
  explicit Case(const char* path) : dir(std::string(path) + "/") {}

  // the payload as bytes: what differ() compares with, and what exact_copy() takes planes from
  std::unique_ptr<uint8_t[]> raw(const char* name, size_t bytes) {
    std::unique_ptr<uint8_t[]> out;
    failed |= !read_npy(dir + name + ".npy", bytes, &out);
    return out;
  }
  // the payload as `count` elements of T in an allocation of exactly that size
  template <typename T>
  std::unique_ptr<T[]> read(const char* name, size_t count) {
    return exact_copy<T>(raw(name, count * sizeof(T)).get(), count);
  }
  // the `n` doubles of params.npy
  std::vector<double> params(int n) {
    const std::unique_ptr<double[]> p = read<double>("params", (size_t)n);
    return std::vector<double>(p.get(), p.get() + n);
  }
};

// a motion X' = R X + t from twelve consecutive doubles of params.npy: R[9] row-major, then t[3]
static inline void read_motion(const double* m, double R[9], double t[3]) {
  memcpy(R, m, 9 * sizeof(double));
  memcpy(t, m + 9, 3 * sizeof(double));
}

// 0: equal; 1: the first differing byte is named on stderr, followed by " (<pass>)" where a pass is named
static int differ(const char* what, const void* got, const void* want, size_t bytes, const char* pass = nullptr) {
  if (!memcmp(got, want, bytes)) return 0;
  const uint8_t* g = (const uint8_t*)got;
  const uint8_t* w = (const uint8_t*)want;
  size_t at = 0;
  while (g[at] == w[at]) ++at;
  fprintf(stderr, "%s differs from the definition at byte %zu of %zu%s%s%s\n", what, at, bytes, pass ? " (" : "", pass ? pass : "",
          pass ? ")" : "");
  return 1;
}
