// Host side of the Gillespie sampler (sampler.h): mmhn_simulate and mmhn_simulate_summary on the stream `st` of an engine.
#pragma once
#include <algorithm>
#include <cstdint>

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

}  // namespace mmhn
