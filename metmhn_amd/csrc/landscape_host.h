// Host side of the seeding landscape (landscape.h: k_landscape_tables, k_landscape_level, k_landscape_gather): the query
// genotypes decoded to codes and checked, the workspace - four planes of 2^n doubles, the model's tables and the tile list -
// refused as a whole when it does not fit the workspace limit (there is no partial landscape), the tiles sorted by the
// popcount of their number, one launch per popcount, descending, on the engine's stream, the queried codes gathered on
// the device and, on request, the four planes copied out.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "host.h"
#include "landscape.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// bytes of workspace a landscape over n mutations takes: 32 B a genotype, the tables, 4 B a tile
inline long long ls_bytes(int n) {
  return (32ll << n) + (long long)sizeof(LsTables) + (4ll << (n - ls_tile_bits(n)));
}

// the query genotypes gen [R][n] (1 = held) as codes: the status of every row, the codes of the valid rows and the rows they
// came from (shared with genodist_host.h and metdist_host.h)
inline void ls_decode_queries(const int8_t* gen, long long R, int n, int32_t* status, std::vector<uint32_t>& codes,
                              std::vector<long long>& src) {
  for (long long i = 0; i < R; ++i) {
    const int8_t* g = gen + i * n;
    uint32_t x = 0;
    bool bad = false;
    for (int j = 0; j < n && !bad; ++j) {
      if (g[j] == 1) x |= 1u << j;
      else if (g[j] != 0) bad = true;
    }
    if (bad) { status[i] = MMHN_ORD_INVALID | (MMHN_ORD_BAD_ENTRY << 16); continue; }
    status[i] = MMHN_ORD_OK;
    codes.push_back(x);
    src.push_back(i);
  }
}

// the 2^hb tile numbers in levels by popcount - level l holds the tiles of popcount hb - l (descending) or l -, ascending
// within a level; first[l]: where level l starts, first[hb + 1] the number of tiles (shared with genodist_host.h and metdist_host.h)
inline void ls_tile_levels(int hb, bool descending, std::vector<uint32_t>& tiles, std::vector<size_t>& first) {
  const size_t nt = (size_t)1 << hb;
  auto level = [&](size_t t) { const int pc = __builtin_popcountll(t); return descending ? hb - pc : pc; };
  first.assign(hb + 2, 0);
  for (size_t t = 0; t < nt; ++t) ++first[level(t) + 1];
  for (int l = 0; l <= hb; ++l) first[l + 1] += first[l];
  tiles.resize(nt);
  std::vector<size_t> at(first.begin(), first.end() - 1);
  for (size_t t = 0; t < nt; ++t) tiles[at[level(t)]++] = (uint32_t)t;
}

// gen [R][n]: 1 = held (R may be 0).  until: 0 the seeding, 1 the seeding or the clock of the first observation.
// values [R][4]: p_seed, time, new_events, seed_events of every query; full: nullptr or [4][2^n], every genotype by code.
template <typename T>
void seeding_landscape(Engine<T>& E, const double* lt, const double* obs1, int until, const int8_t* gen, long long R,
                       double* values, int32_t* status, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the landscape kernels (n_mut <= 31)");
  REQUIRE(until == 0 || until == 1, "until must be 0 (the seeding) or 1 (the seeding or the observation)");
  const int n = E.n, N = E.N, c = ls_tile_bits(n);
  std::fill(values, values + 4 * R, std::nan(""));
  if (until == 0) {
    double s = lt[n * N + n];
    for (int i = 0; i < n; ++i) s += lt[n * N + i];
    REQUIRE(std::exp(s) > 0.0, "seeding landscape until the seeding: the seeding rate of the full genotype underflows to 0, "
                               "so the chain has a state without exit (a model fitted without a seeded sample?); use until = observation");
  }
  const long long need = ls_bytes(n), limit = (long long)E.cfg.plan.ws_limit;
  if (need > limit)
    throw Fail{"seeding landscape: " + std::to_string(n) + " mutations need " + std::to_string(need) +
               " bytes of workspace (32 B x 2^n_mut, the rate tables and the tile list), the workspace limit is " +
               std::to_string(limit) + " bytes; there is no partial landscape"};
  std::vector<uint32_t> codes;
  std::vector<long long> src;
  ls_decode_queries(gen, R, n, status, codes, src);
  // the tiles by the popcount of their number, descending
  const int hb = n - c;
  const size_t nt = (size_t)1 << hb;
  std::vector<uint32_t> tiles;
  std::vector<size_t> first;                           // first[l]: where the tiles of popcount hb - l start
  ls_tile_levels(hb, true, tiles, first);
  DevArr<double> par, V, d_out;
  DevArr<LsTables> tabs;
  DevArr<uint32_t> d_tiles, d_codes;
  par.alloc((size_t)N * N + N);
  V.alloc((size_t)4 << n);
  tabs.alloc(1);
  d_tiles.alloc(nt);
  HIPCHECK(hipMemcpyAsync(par.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N, obs1, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(d_tiles.p, tiles.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
  hipLaunchKernelGGL(k_landscape_tables, dim3(1), dim3(LS_KB), 0, E.stream, par.p, par.p + N * N, N, c, tabs.p);
  HIPCHECK(hipGetLastError());
  for (int l = 0; l <= hb; ++l) {
    hipLaunchKernelGGL(k_landscape_level, dim3((unsigned)(first[l + 1] - first[l])), dim3(LS_KB), 0, E.stream, tabs.p,
                       d_tiles.p + first[l], par.p, par.p + N * N, N, c, until, V.p);
    HIPCHECK(hipGetLastError());
  }
  std::vector<double> out(4 * codes.size());
  if (!codes.empty()) {
    d_codes.alloc(codes.size()); d_out.alloc(out.size());
    HIPCHECK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_landscape_gather, dim3((unsigned)((codes.size() + LS_KB - 1) / LS_KB)), dim3(LS_KB), 0, E.stream,
                       d_codes.p, (long long)codes.size(), V.p, n, d_out.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
  }
  if (full) HIPCHECK(hipMemcpyAsync(full, V.p, sizeof(double) * ((size_t)4 << n), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
  for (size_t j = 0; j < codes.size(); ++j)
    for (int k = 0; k < 4; ++k) values[4 * src[j] + k] = out[4 * j + k];
}

}  // namespace mmhn
