// Host side of the seeding forecasts (forecast.h: k_forecast_level, k_forecast_reduce): the genotypes decoded and
// checked, cut into batches by the workspace limit as opr_rows cuts a cohort (rows in call order while their lattices and
// partials fit; a row that does not fit on its own is MMHN_ORD_TOO_LARGE), the workspace allocated once for the largest
// batch; per batch the (row, tile) map, one launch per level and the reduction on the engine's stream, one copy back.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "forecast.h"
#include "host.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// gen [R][n]: 1 = the tumour holds the mutation.  until: 0 the seeding, 1 the seeding or the clock of the first observation.
// p_seed, time [R]; before, with_seed [R][n] (NaN for a held mutation); n_before [R][n+1] (0 past the row's free events).
template <typename T>
void seeding_forecasts(Engine<T>& E, const double* lt, const double* obs1, const int8_t* gen, long long R, int until,
                       double* p_seed, double* time, double* before, double* with_seed, double* n_before, int32_t* status) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the forecast kernels (n_mut <= 31)");
  REQUIRE(until == 0 || until == 1, "until must be 0 (the seeding) or 1 (the seeding or the observation)");
  const int n = E.n, N = E.N;
  const double nan = std::nan("");
  std::fill(p_seed, p_seed + R, nan);
  std::fill(time, time + R, nan);
  std::fill(before, before + R * n, nan);
  std::fill(with_seed, with_seed + R * n, nan);
  std::fill(n_before, n_before + R * N, nan);
  if (until == 0) {
    double s = lt[n * N + n];
    for (int i = 0; i < n; ++i) s += lt[n * N + i];
    REQUIRE(std::exp(s) > 0.0, "seeding forecasts until the seeding: the seeding rate of the full genotype underflows to 0, "
                               "so the chain has a state without exit (a model fitted without a seeded sample?); use until = observation");
  }
  const long long limit = (long long)E.cfg.plan.ws_limit;
  std::vector<FRow> todo;
  std::vector<long long> src;
  for (long long i = 0; i < R; ++i) {
    const int8_t* g = gen + i * n;
    FRow r{};
    bool bad = false;
    for (int j = 0; j < n && !bad; ++j) {
      if (g[j] == 0) { if (r.f < 32) r.ev[r.f] = (int8_t)j; ++r.f; }
      else if (g[j] != 1) bad = true;
    }
    if (bad) { status[i] = MMHN_ORD_INVALID | (MMHN_ORD_BAD_ENTRY << 16); continue; }
    if (r.f > MAXK || fc_doubles(r.f) * (long long)sizeof(double) > limit) { status[i] = MMHN_ORD_TOO_LARGE; continue; }
    status[i] = MMHN_ORD_OK;
    r.c = fc_chunk_bits(r.f); r.tb = fc_tile_bits(r.f); r.until = until;
    r.tiles = 1 << (r.f - r.c - r.tb);
    // the exponents' share of the diagonal and the held events, in ascending event order
    for (int j = 0; j < r.f + 2; ++j) {
      const int e = j < r.f ? r.ev[j] : n;
      double b = j <= r.f ? lt[e * N + e] : 0.0;
      for (int k = 0; k < n; ++k)
        if (g[k] == 1) b += j <= r.f ? lt[e * N + k] : obs1[k];
      r.base[j] = b;
    }
    todo.push_back(r);
    src.push_back(i);
  }
  if (todo.empty()) return;
  std::vector<size_t> cut{0};
  long long used = 0, most = 0;
  for (size_t j = 0; j < todo.size(); ++j) {
    const long long d = fc_doubles(todo[j].f);
    if (j > cut.back() && (used + d) * (long long)sizeof(double) > limit) { cut.push_back(j); used = 0; }
    used += d;
    most = std::max(most, used);
  }
  cut.push_back(todo.size());
  DevArr<double> par, ws, d_out;
  DevArr<FRow> d_rows;
  DevArr<int2> d_map;
  par.alloc((size_t)N * N + N);
  HIPCHECK(hipMemcpyAsync(par.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N, obs1, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  ws.alloc((size_t)most);
  for (size_t b = 0; b + 1 < cut.size(); ++b) {
    const size_t nr = cut[b + 1] - cut[b];
    std::vector<FRow> rows(todo.begin() + cut[b], todo.begin() + cut[b + 1]);
    std::vector<int2> map;
    long long off = 0, ooff = 0;
    int fmax = 0;
    for (size_t j = 0; j < nr; ++j) {
      FRow& r = rows[j];
      r.goff = off;
      r.poff = off + (1ll << r.f);
      r.ooff = ooff;
      r.row = (int)j;
      off += fc_doubles(r.f);
      ooff += fc_block(r.f);
      fmax = std::max(fmax, r.f);
      for (int t = 0; t < r.tiles; ++t) map.push_back(make_int2((int)j, t));
    }
    REQUIRE((size_t)off <= ws.n, "forecast kernels: batch larger than its workspace");
    REQUIRE(map.size() < ((size_t)1 << 31), "forecast kernels: too many tiles in a batch");
    d_rows.alloc(nr); d_map.alloc(map.size()); d_out.alloc((size_t)ooff);
    HIPCHECK(hipMemcpyAsync(d_rows.p, rows.data(), nr * sizeof(FRow), hipMemcpyHostToDevice, E.stream));
    HIPCHECK(hipMemcpyAsync(d_map.p, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
    for (int lev = 0; lev <= fmax; ++lev) {
      hipLaunchKernelGGL(k_forecast_level, dim3((unsigned)map.size()), dim3(FC_KB), 0, E.stream, d_rows.p, d_map.p, par.p,
                         par.p + N * N, N, lev, ws.p);
      HIPCHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_forecast_reduce, dim3((unsigned)nr), dim3(FC_KB), 0, E.stream, d_rows.p, ws.p, d_out.p);
    HIPCHECK(hipGetLastError());
    std::vector<double> out((size_t)ooff);
    HIPCHECK(hipMemcpyAsync(out.data(), d_out.p, (size_t)ooff * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipStreamSynchronize(E.stream));
    for (size_t j = 0; j < nr; ++j) {
      const FRow& r = rows[j];
      const long long i = src[cut[b] + j];
      const double* o = out.data() + r.ooff;
      p_seed[i] = o[0];
      time[i] = o[1];
      for (int a = 0; a < r.f; ++a) {
        before[i * n + r.ev[a]] = o[2 + a];
        with_seed[i * n + r.ev[a]] = o[2 + r.f + a];
      }
      for (int m = 0; m < N; ++m) n_before[i * N + m] = m <= r.f ? o[2 + 2 * r.f + m] : 0.0;
    }
  }
}

}  // namespace mmhn
