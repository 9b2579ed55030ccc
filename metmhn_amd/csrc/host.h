// Host-side plumbing shared by the engine and its helpers: error type and checks, owning device arrays, the device
// guard of the ABI entry points and the readers of the MMHN_* environment knobs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

namespace mmhn {

struct Fail {
  std::string msg;
};
#define HIPCHECK(expr)                                                                       \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      throw Fail{std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                 std::to_string(__LINE__) + ")"};                                            \
  } while (0)
#define REQUIRE(cond, text) \
  do {                      \
    if (!(cond)) throw Fail{std::string(text)}; \
  } while (0)

template <typename U>
struct DevArr {
  U* p = nullptr;
  size_t n = 0;
  void alloc(size_t count) {
    if (count <= n && p) return;
    release();
    if (count == 0) return;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(U)));
    n = count;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  ~DevArr() { release(); }
  DevArr() = default;
  DevArr(const DevArr&) = delete;
  DevArr& operator=(const DevArr&) = delete;
  DevArr(DevArr&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevArr& operator=(DevArr&& o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
};

// Every ABI entry runs with the engine's GPU current and puts the caller's device back on exit, so engines on
// different GPUs can live in one process (and a handle may be used from a thread whose current device differs).
struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) HIPCHECK(hipSetDevice(dev));
    else prev = -1;
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

// MMHN_* environment knobs: an integer (fallback when unset), a switch (any value but 0 turns it on), a keyword
inline bool env_set(const char* name) { return std::getenv(name) != nullptr; }
inline long long env_int(const char* name, long long fallback) {
  const char* v = std::getenv(name);
  return v ? std::atoll(v) : fallback;
}
inline bool env_flag(const char* name, bool fallback) { return env_int(name, fallback ? 1 : 0) != 0; }
inline bool env_is(const char* name, const char* word) {
  const char* v = std::getenv(name);
  return v && std::strcmp(v, word) == 0;
}

}  // namespace mmhn
