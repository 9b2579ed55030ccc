// Measurement entry points of the C ABI: mmhn_bench_stream (plain stream, the denominator of the HBM-bound kernels) and
// mmhn_bench_kronvec (the launch sequence of the batched Kronecker product).
#pragma once
#include "host.h"
#include "prims.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// plain stream for mmhn_bench_stream: the denominator the HBM-bound kernels are compared with.  Four 16-byte
// accesses per lane in flight per trip, one contiguous 4 KiB run per wave and trip.
__global__ __launch_bounds__(256) void k_stream(double2* __restrict__ a, const double2* __restrict__ b,
                                                const double2* __restrict__ c, size_t n16, int kind) {
  constexpr int U = 4;
  const size_t lane = threadIdx.x & 63, wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const size_t nwave = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t base = wave * (64 * U); base < n16; base += nwave * (64 * U)) {
    double2 u[U], v[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const size_t i = base + q * 64 + lane;
      if (i < n16) { u[q] = b[i]; if (kind == 1) v[q] = c[i]; }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const size_t i = base + q * 64 + lane;
      if (i < n16) a[i] = kind == 0 ? u[q] : make_double2(u[q].x + 3.0 * v[q].x, u[q].y + 3.0 * v[q].y);
    }
  }
}

// achieved device-memory bandwidth of this GPU for a plain E.stream: kind 0 copy (b = a), 1 triad (a = b + s c);
// 16 bytes per lane, `bytes` per array (>> Infinity Cache), HIP events around `iters` launches; GB/s of the
// bytes the kernel is asked to move (copy 2 x, triad 3 x bytes)
template <typename T>
double bench_stream(Engine<T>& E, size_t bytes, int iters, int kind) {
  REQUIRE(bytes >= (1u << 20) && iters >= 1 && (kind == 0 || kind == 1), "bench_stream: bad arguments");
  const size_t n16 = bytes / 16;
  DevArr<double2> a, b, c;
  a.alloc(n16); b.alloc(n16);
  if (kind == 1) c.alloc(n16);
  HIPCHECK(hipMemsetAsync(a.p, 0, n16 * 16, E.stream));
  HIPCHECK(hipMemsetAsync(b.p, 0, n16 * 16, E.stream));
  if (kind == 1) HIPCHECK(hipMemsetAsync(c.p, 0, n16 * 16, E.stream));
  auto run = [&]() {
    hipLaunchKernelGGL(k_stream, dim3(E.cfg.stream_blocks), dim3(256), 0, E.stream, a.p, b.p, c.p, n16, kind);
  };
  run();
  hipEvent_t e0, e1;
  HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
  HIPCHECK(hipEventRecord(e0, E.stream));
  for (int i = 0; i < iters; ++i) run();
  HIPCHECK(hipEventRecord(e1, E.stream));
  HIPCHECK(hipEventSynchronize(e1));
  HIPCHECK(hipGetLastError());
  float ms = 0;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return (double)(kind == 0 ? 2 : 3) * (double)(n16 * 16) * iters / ((double)ms * 1e6);
}
// tiles[0] = tiles where Q_off has entries, tiles[1] = tiles per launch (both over the whole batch)
template <typename T>
double bench_kronvec(Engine<T>& E, const Desc& d0, long long batch, int iters, bool tr, bool jacobi, long long* tiles) {
  REQUIRE(batch >= 1 && iters >= 1, "batch and iters must be positive");
  KvBatch<T> kb; kv_setup(E, kb, d0, batch);
  const long long V = kb.V;
  if (tiles) { tiles[0] = kb.nlive; tiles[1] = kb.ntiles; }
  DevArr<T> a, b, c, r;
  a.alloc((size_t)(batch * V)); b.alloc((size_t)(batch * V));
  std::vector<T> host((size_t)V);
  for (long long i = 0; i < V; ++i) host[(size_t)i] = (T)(1.0 / (double)(1 + (i % 97)));
  for (long long i = 0; i < batch; ++i)
    HIPCHECK(hipMemcpy(a.p + i * V, host.data(), (size_t)V * sizeof(T), hipMemcpyHostToDevice));
  HIPCHECK(hipMemsetAsync(b.p, 0xFF, (size_t)(batch * V) * sizeof(T), E.stream));   // y starts as NaNs: the launch writes all of it
  if (jacobi) {
    c.alloc((size_t)(batch * V)); r.alloc((size_t)(batch * V));
    E.launch_diag(E.main, kb.dd.p, kb.map.p, kb.ntiles, nullptr, c.p, nullptr, KD_LIDG);
    HIPCHECK(hipMemcpyAsync(r.p, a.p, (size_t)(batch * V) * sizeof(T), hipMemcpyDeviceToDevice, E.stream));
  }
  // the timed launch is exactly the one mmhn_kronvec_batched issues (plain product), or the fused Jacobi step
  auto run = [&]() {
    if (jacobi) kv_launch(E, kb, tr, a.p, b.p, c.p, r.p);
    else kv_launch(E, kb, tr, a.p, b.p);
  };
  run(); run();
  hipEvent_t e0, e1;
  HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
  HIPCHECK(hipEventRecord(e0, E.stream));
  for (int i = 0; i < iters; ++i) run();
  HIPCHECK(hipEventRecord(e1, E.stream));
  HIPCHECK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return (double)ms / iters;
}

}  // namespace mmhn
