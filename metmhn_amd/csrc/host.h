// Host-side plumbing shared by the engine and its helpers: error type and checks, owning device arrays, the device
// guard of the ABI entry points, the lanes, the kernel timer and the readers of the MMHN_* environment knobs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/metmhn_amd.h"

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

// A stream of the engine with what belongs to it.  Every launch helper takes the lane it issues on, so the stream, the flag
// set of a cooperative launch and the events a stage waits for cannot come apart.
// flags: index of the CoopState::flags[] set (tsolve_host.h) its cooperative launches use, which also picks their CoopCtl slots
// (flags * 4 + ...); -1: the lane carries none.  Launches of two lanes may be in flight together, so two lanes that both
// issue cooperative launches never share a set.
// fork / join: a side lane waits for a point of the main lane (begin), and the main lane later for the side lane's last
// launch (end on the side lane, join on the main one).  The host needs ~25 us for a fork, the launches and the join
// record, so the point to wait for may be recorded ahead of time (record_fork) and launches of the critical chain be issued
// before those of the side lane.
struct Lane {
  hipStream_t s = nullptr;
  int flags = -1;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;     // (created once, hipEventDisableTiming)
  bool forked = false;                                 // launches of an evaluation in flight that the main lane has not joined
  bool fork_recorded = false;                          // ev_fork was recorded ahead of time
  void record_fork(const Lane& main) {
    HIPCHECK(hipEventRecord(ev_fork, main.s));
    fork_recorded = true;
  }
  void begin(const Lane& main) {
    if (!fork_recorded) HIPCHECK(hipEventRecord(ev_fork, main.s));
    fork_recorded = false;
    HIPCHECK(hipStreamWaitEvent(s, ev_fork, 0));
    forked = true;
  }
  void end() { HIPCHECK(hipEventRecord(ev_join, s)); }
  void join(const Lane& main) {
    if (forked) HIPCHECK(hipStreamWaitEvent(main.s, ev_join, 0));
    forked = false;
  }
  // (an evaluation that threw between a fork and its join must not leave its flags to the next one: the side stream
  // would wait for the previous evaluation's event and start before this one's parameters are up)
  void reset() { forked = fork_recorded = false; }
};

// The times of the dominant kernels for the counters (mmhn_get_counters): HIP events around a launch, read when the
// evaluation is complete.  An event record costs ~5 us of host time, which a short evaluation cannot afford (it is bound by
// the host's issue rate): the engine turns the timer on per batch, for batches of at least 2^26 states
// (MMHN_TIME_KERNELS=1: every batch).  Off, a timed launch is the launch and its error check.
struct KernelTimer {
  bool on = true;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  size_t used = 0;
  std::vector<double> bytes;
  std::vector<int> slot;              // MMHN_K_* class of the timed launch
  // the events are recorded on the lane of the launch (they are not created with hipEventDisableTiming - evaluate() keeps
  // a timed batch on the main lane)
  template <typename F>
  void timed(const Lane& L, int slot_, double alg_bytes, F&& launch) {
    if (!on) {
      launch();
      HIPCHECK(hipGetLastError());
      return;
    }
    if (used == pool.size()) {
      hipEvent_t a, b;
      HIPCHECK(hipEventCreate(&a));
      HIPCHECK(hipEventCreate(&b));
      pool.push_back({a, b});
    }
    hipEvent_t e0 = pool[used].first, e1 = pool[used].second;
    ++used;
    bytes.push_back(alg_bytes);
    slot.push_back(slot_);
    HIPCHECK(hipEventRecord(e0, L.s));
    launch();
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(e1, L.s));
  }
  // after the lanes have been synchronised
  void collect(mmhn_counters& cnt) {
    for (size_t i = 0; i < used; ++i) {
      float ms = 0;
      HIPCHECK(hipEventElapsedTime(&ms, pool[i].first, pool[i].second));
      mmhn_kernel_counter& c = cnt.kernel[slot[i]];
      c.ms += ms;
      c.launches += 1;
      c.alg_bytes += bytes[i];
    }
    used = 0;
    bytes.clear();
    slot.clear();
  }
  void release() {
    for (auto& e : pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    pool.clear();
  }
};

// Run-time booleans as compile-time arguments of a generic lambda, to pick a template instantiation:
//   with_flags([&](auto tr, auto jac) { launch k<T, tr(), jac()> }, transposed, lidg != nullptr);
template <typename F>
void with_flags(F&& f) { f(); }
template <typename F, typename... Bs>
void with_flags(F&& f, bool b, Bs... rest) {
  if (b) with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}

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
