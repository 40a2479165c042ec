// host_npy.hpp -- what the programs that run kernel code on the host (tests/cpp/*_host_main.cpp) share: reading the .npy
// dumps of a test (numpy's format, version 1, C order, little endian; the header is skipped and the payload size checked)
// into allocations of EXACTLY the payload, so that the sanitizers see a load past the end, and comparing a result with the
// definition's byte for byte.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

static bool read_npy(const std::string& path, size_t bytes, std::unique_ptr<uint8_t[]>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  uint8_t head[10];
  bool ok = fread(head, 1, 10, f) == 10 && !memcmp(head, "\x93NUMPY\x01", 7);
  const size_t hlen = ok ? (size_t)head[8] | ((size_t)head[9] << 8) : 0;
  ok = ok && fseek(f, 0, SEEK_END) == 0 && (size_t)ftell(f) == 10 + hlen + bytes && fseek(f, (long)(10 + hlen), SEEK_SET) == 0;
  if (ok) {
    out->reset(new uint8_t[bytes ? bytes : 1]);  // exactly sized (one byte where the dump is empty)
    ok = fread(out->get(), 1, bytes, f) == bytes;
  }
  fclose(f);
  if (!ok) fprintf(stderr, "cannot read %zu payload bytes from %s\n", bytes, path.c_str());
  return ok;
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
