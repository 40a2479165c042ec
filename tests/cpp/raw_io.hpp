// raw_io.hpp -- how the caller programs of tests/cpp/ exchange arrays with the Python tests: headerless files of exactly
// the elements, in memory order.  A read fills storage the caller has sized; it is false where the file is missing or short.
#pragma once

#include <fstream>
#include <string>

#include "patchmatch_gpu.hpp"

template <typename T>
inline bool read_raw(const std::string& path, T* data, size_t count) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  f.read(reinterpret_cast<char*>(data), (std::streamsize)(sizeof(T) * count));
  return (bool)f;
}
template <typename T>
inline bool read_raw(const std::string& path, bm::core::Image<T>& im) {
  return read_raw(path, im.data(), (size_t)im.rows * im.cols);
}

template <typename T>
inline void write_raw(const std::string& path, const T* data, size_t count) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(data), (std::streamsize)(sizeof(T) * count));
}
template <typename T>
inline void write_raw(const std::string& path, const bm::core::Image<T>& im) {
  write_raw(path, im.data(), (size_t)im.rows * im.cols);
}
