// Stand-in for glog: CHECK / CHECK_GT abort with their message when the condition fails, LOG swallows its text.
#pragma once

#include <cstdlib>
#include <iostream>

namespace glog_standin {

struct Sink {
  template <typename T> Sink& operator<<(const T&) { return *this; }
  Sink& operator<<(std::ostream& (*)(std::ostream&)) { return *this; }
};

struct Fatal {
  Fatal(const char* file, int line, const char* what) {
    std::cerr << file << ":" << line << ": check failed: " << what << " ";
  }
  [[noreturn]] ~Fatal() {
    std::cerr << std::endl;
    std::abort();
  }
  template <typename T> Fatal& operator<<(const T& v) {
    std::cerr << v;
    return *this;
  }
  Fatal& operator<<(std::ostream& (*m)(std::ostream&)) {
    std::cerr << m;
    return *this;
  }
};

}  // namespace glog_standin

#define CHECK(cond) \
  if (cond) {       \
  } else            \
    ::glog_standin::Fatal(__FILE__, __LINE__, #cond)
#define CHECK_GT(a, b) CHECK((a) > (b))
#define CHECK_GE(a, b) CHECK((a) >= (b))
#define CHECK_LT(a, b) CHECK((a) < (b))
#define CHECK_LE(a, b) CHECK((a) <= (b))
#define CHECK_EQ(a, b) CHECK((a) == (b))
#define LOG(severity) ::glog_standin::Sink()
