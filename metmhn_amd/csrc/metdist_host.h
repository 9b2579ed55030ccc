// Host side of the genotype distribution of the metastasis and its founder (metdist.h: k_metdist_level, k_metdist_tile,
// k_metdist_gather; genodist.h's k_genodist_summary; the tables are landscape.h's k_landscape_tables, launched once with
// obs1 and once with obs2): the query genotypes decoded to codes and checked, the workspace - three planes of 2^n
// doubles, the two sets of tables, the tile list and, for the summary, the tiles' partial sums - refused as a whole when
// it does not fit the workspace limit (there is no partial distribution), the tiles sorted by the popcount of their
// number, one launch per popcount, ascending, on the engine's stream, one launch over every tile that turns the planes
// into Z, M, C and folds the tiles' sums of Z and M, the summary, the queried codes gathered on the device and, on request,
// the three planes copied out.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "genodist_host.h"                      // gd_summary_doubles, gd_summary_items
#include "host.h"
#include "landscape_host.h"                     // ls_decode_queries, ls_tile_levels
#include "metdist.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// bytes of workspace a distribution over n mutations takes: 24 B a genotype, the two sets of tables, 4 B a tile and, with
// the summary, 2 GD_FEAT doubles a tile and the summary itself
inline long long md_bytes(int n, bool summary) {
  const long long nt = 1ll << (n - ls_tile_bits(n));
  return (24ll << n) + 2 * (long long)sizeof(LsTables) + 4 * nt +
         (summary ? (long long)sizeof(double) * (2 * GD_FEAT * nt + gd_summary_doubles(n)) : 0);
}

// gen [R][n]: 1 = held (R may be 0).  values [R][3]: Z, M, C of every query; summary: nullptr or [2][1 + n * n + n + 1],
// the founder plane Z and then the metastasis plane M; full: nullptr or [3][2^n], every genotype by code.
template <typename T>
void metastasis_distribution(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* gen,
                             long long R, double* values, int32_t* status, double* summary, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the metastasis distribution kernels (n_mut <= 31)");
  const int n = E.n, N = E.N, c = ls_tile_bits(n);
  std::fill(values, values + 3 * R, std::nan(""));
  const long long need = md_bytes(n, summary != nullptr), limit = (long long)E.cfg.plan.ws_limit;
  if (need > limit)
    throw Fail{"metastasis distribution: " + std::to_string(n) + " mutations need " + std::to_string(need) +
               " bytes of workspace (24 B x 2^n_mut, the rate tables, the tile list and the tiles' partial sums), the "
               "workspace limit is " + std::to_string(limit) + " bytes; there is no partial distribution"};
  std::vector<uint32_t> codes;
  std::vector<long long> src;
  ls_decode_queries(gen, R, n, status, codes, src);
  // the tiles by the popcount of their number, ascending
  const int hb = n - c;
  const size_t nt = (size_t)1 << hb;
  std::vector<uint32_t> tiles;
  std::vector<size_t> first;                           // first[l]: where the tiles of popcount l start
  ls_tile_levels(hb, false, tiles, first);
  DevArr<double> par, V, part, d_sum, d_out;
  DevArr<LsTables> tabs;                               // [0]: of (theta, obs1), [1]: of (theta, obs2)
  DevArr<uint32_t> d_tiles, d_codes;
  par.alloc((size_t)N * N + 2 * N);
  V.alloc((size_t)3 << n);
  tabs.alloc(2);
  d_tiles.alloc(nt);
  const double *d_lt = par.p, *d_o1 = par.p + N * N, *d_o2 = par.p + N * N + N;
  HIPCHECK(hipMemcpyAsync(par.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N, obs1, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N + N, obs2, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(d_tiles.p, tiles.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
  hipLaunchKernelGGL(k_landscape_tables, dim3(1), dim3(LS_KB), 0, E.stream, d_lt, d_o1, N, c, tabs.p);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_landscape_tables, dim3(1), dim3(LS_KB), 0, E.stream, d_lt, d_o2, N, c, tabs.p + 1);
  HIPCHECK(hipGetLastError());
  for (int l = 0; l <= hb; ++l) {
    hipLaunchKernelGGL(k_metdist_level, dim3((unsigned)(first[l + 1] - first[l])), dim3(LS_KB), 0, E.stream, tabs.p,
                       tabs.p + 1, d_tiles.p + first[l], d_lt, d_o1, d_o2, N, c, V.p);
    HIPCHECK(hipGetLastError());
  }
  if (summary) {
    part.alloc((size_t)2 * GD_FEAT * nt);
    d_sum.alloc((size_t)gd_summary_doubles(n));
    hipLaunchKernelGGL(k_metdist_tile<true>, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, tabs.p, tabs.p + 1, d_lt, d_o2, N,
                       c, V.p, part.p, (long long)nt);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_genodist_summary, dim3((unsigned)(2 * gd_summary_items(n))), dim3(LS_KB), 0, E.stream, part.p,
                       (long long)nt, n, c, d_sum.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(summary, d_sum.p, sizeof(double) * gd_summary_doubles(n), hipMemcpyDeviceToHost, E.stream));
  } else {
    hipLaunchKernelGGL(k_metdist_tile<false>, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, tabs.p, tabs.p + 1, d_lt, d_o2, N,
                       c, V.p, (double*)nullptr, (long long)nt);
    HIPCHECK(hipGetLastError());
  }
  std::vector<double> out(3 * codes.size());
  if (!codes.empty()) {
    d_codes.alloc(codes.size()); d_out.alloc(out.size());
    HIPCHECK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_metdist_gather, dim3((unsigned)((codes.size() + LS_KB - 1) / LS_KB)), dim3(LS_KB), 0, E.stream,
                       d_codes.p, (long long)codes.size(), V.p, n, d_out.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
  }
  if (full) HIPCHECK(hipMemcpyAsync(full, V.p, sizeof(double) * ((size_t)3 << n), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
  for (size_t j = 0; j < codes.size(); ++j)
    for (int k = 0; k < 3; ++k) values[3 * src[j] + k] = out[3 * j + k];
}

}  // namespace mmhn
