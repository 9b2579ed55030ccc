// Host side of the Gillespie sampler (sampler.h): mmhn_simulate, mmhn_simulate_summary and mmhn_simulate_pairs on the stream
// `st` of an engine.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host.h"
#include "sampler.h"

namespace mmhn {

// n_sim trajectories: dat_out[n_sim][2 n + 2], orders_out (optional) [n_sim][2 N + 2]
static void simulate(hipStream_t st, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int n, int64_t n_sim,
                     uint64_t seed, int8_t* dat_out, int8_t* orders_out) {
  const int N = n + 1;
  if (n_sim > 0) {
    const size_t W = (size_t)2 * n + 2, L = (size_t)2 * N + 2;
    DevArr<double> d_lt, d_dp, d_dm;
    DevArr<int8_t> d_dat, d_ord;
    d_lt.alloc((size_t)N * N); d_dp.alloc(N); d_dm.alloc(N); d_dat.alloc((size_t)n_sim * W);
    if (orders_out) d_ord.alloc((size_t)n_sim * L);
    HIPCHECK(hipMemcpy(d_lt.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dp.p, pt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dm.p, mt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((n_sim + SIM_BLOCK - 1) / SIM_BLOCK);
    hipLaunchKernelGGL(k_gillespie, dim3(grid), dim3(SIM_BLOCK), 0, st, d_lt.p, d_dp.p, d_dm.p, N, (long long)n_sim, seed,
                       d_dat.p, orders_out ? d_ord.p : nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipMemcpy(dat_out, d_dat.p, (size_t)n_sim * W, hipMemcpyDeviceToHost));
    if (orders_out) HIPCHECK(hipMemcpy(orders_out, d_ord.p, (size_t)n_sim * L, hipMemcpyDeviceToHost));
  }
}

// the summary counts of trajectories first .. first + n_sim - 1, computed in chunks of MMHN_SIM_CHUNK samples per launch
static void simulate_summary(hipStream_t st, int device, long long sim_chunk, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int n, int64_t first,
                             int64_t n_sim, uint64_t seed, int64_t* counts) {
  const int N = n + 1;
  const int C = SIM_HEAD + 5 * n;
  std::fill(counts, counts + C, (int64_t)0);
  if (n_sim > 0) {
    DevArr<double> d_lt, d_dp, d_dm;
    DevArr<unsigned long long> d_cnt;
    d_lt.alloc((size_t)N * N); d_dp.alloc(N); d_dm.alloc(N); d_cnt.alloc(C);
    HIPCHECK(hipMemcpy(d_lt.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dp.p, pt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dm.p, mt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long) * C, st));
    int n_cu = 1;
    HIPCHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    // a grid-stride loop over the chunk: enough workgroups to fill the chip (7 resident per CU), few global atomics
    const long long max_grid = 8ll * std::max(1, n_cu);
    for (int64_t done = 0; done < n_sim; done += sim_chunk) {
      const long long cnt = (long long)std::min<int64_t>(sim_chunk, n_sim - done);
      const unsigned grid = (unsigned)std::min<long long>((cnt + SIM_BLOCK - 1) / SIM_BLOCK, max_grid);
      hipLaunchKernelGGL(k_gillespie_summary, dim3(grid), dim3(SIM_BLOCK), 0, st, d_lt.p, d_dp.p, d_dm.p, N,
                         (long long)(first + done), cnt, seed, d_cnt.p);
      HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipMemcpyAsync(counts, d_cnt.p, sizeof(int64_t) * C, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
  }
}

// the pair and burden tables of trajectories first .. first + n_sim - 1 (k_gillespie_pairs), chunked and sized as
// simulate_summary: n_class [3], pairs [3][B][B] (the device counts the upper triangle, mirrored here), burden [3][5][n + 1]
static void simulate_pairs(hipStream_t st, int device, long long sim_chunk, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int n, int64_t first,
                           int64_t n_sim, uint64_t seed, int64_t* n_class, int64_t* pairs, int64_t* burden) {
  const int N = n + 1, B = 2 * n, P = B * (B + 1) / 2, H = SIM_CLASSES * SIM_BURDEN_KINDS * (n + 1);
  const int C = sim_pairs_counts(n);
  std::fill(n_class, n_class + SIM_CLASSES, (int64_t)0);
  std::fill(pairs, pairs + (size_t)SIM_CLASSES * B * B, (int64_t)0);
  std::fill(burden, burden + H, (int64_t)0);
  if (n_sim > 0) {
    DevArr<double> d_lt, d_dp, d_dm;
    DevArr<unsigned long long> d_cnt;
    d_lt.alloc((size_t)N * N); d_dp.alloc(N); d_dm.alloc(N); d_cnt.alloc(C);
    HIPCHECK(hipMemcpy(d_lt.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dp.p, pt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_dm.p, mt_d_ef, sizeof(double) * N, hipMemcpyHostToDevice));
    HIPCHECK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long) * C, st));
    int n_cu = 1;
    HIPCHECK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    const long long max_grid = 8ll * std::max(1, n_cu);
    // the kernel's per-workgroup counters are 32 bits wide and take at most SIM_BLOCK per pass: at most
    // SIM_PAIRS_MAX_PASSES passes per launch (2^31 per counter), whatever MMHN_SIM_CHUNK says
    const long long per_launch = std::min(sim_chunk, max_grid * SIM_BLOCK * SIM_PAIRS_MAX_PASSES);
    for (int64_t done = 0; done < n_sim; done += per_launch) {
      const long long cnt = (long long)std::min<int64_t>(per_launch, n_sim - done);
      const unsigned grid = (unsigned)std::min<long long>((cnt + SIM_BLOCK - 1) / SIM_BLOCK, max_grid);
      hipLaunchKernelGGL(k_gillespie_pairs, dim3(grid), dim3(SIM_BLOCK), 0, st, d_lt.p, d_dp.p, d_dm.p, N,
                         (long long)(first + done), cnt, seed, d_cnt.p);
      HIPCHECK(hipGetLastError());
    }
    std::vector<int64_t> h(C);
    HIPCHECK(hipMemcpyAsync(h.data(), d_cnt.p, sizeof(int64_t) * C, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    std::copy(h.begin(), h.begin() + SIM_CLASSES, n_class);
    for (int c = 0; c < SIM_CLASSES; ++c) {
      const int64_t* tri = h.data() + SIM_CLASSES + (size_t)c * P;
      int64_t* full = pairs + (size_t)c * B * B;
      for (int a = 0, p = 0; a < B; ++a)
        for (int b = a; b < B; ++b, ++p) full[a * B + b] = full[b * B + a] = tri[p];
    }
    std::copy(h.begin() + SIM_CLASSES + SIM_CLASSES * P, h.end(), burden);
  }
}

}  // namespace mmhn
