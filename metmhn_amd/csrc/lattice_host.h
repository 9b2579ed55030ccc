// Host side of the sweeps over all 2^n genotypes (lattice.h; landscape_host.h, genodist_host.h and metdist_host.h hold what
// differs): lattice_sweep decodes and checks the query genotypes, refuses as a whole a workspace - K planes of 2^n doubles,
// the model's tables, the tile list and, for a summary, the tiles' partial sums - that does not fit the workspace limit
// (there is no partial sweep), sorts the tiles by the popcount of their number, launches the sweep's level kernel once
// per popcount on the engine's stream, runs the sweep's finishing step, gathers the queried codes on the device and, on
// request, copies the K planes out.  lattice_summary is the finishing step of the sweeps that have a summary.
// partner_host.h loops over queries on one workspace and calls the pieces itself: ls_check_workspace, ls_decode_queries,
// ls_tile_levels, ls_upload_model and, for the tiles under a query's high bits, ls_tile_levels_under.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "genodist.h"                           // GD_FEAT, k_genodist_summary: the summary of a sweep's first two planes
#include "host.h"
#include "lattice.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// what a sweep is, its arithmetic apart
struct LatticeSpec {
  const char* name;                             // the refusal: "<name>: <n> mutations need ... (<8 K> B x 2^n_mut<holds>), ...
  const char* holds;                            // ...; there is no partial <whole>"
  const char* whole;
  int sets;                                     // sets of tables: 1 of (theta, obs1), 2 and of (theta, obs2)
  bool descending;                              // the levels by popcount of the tile number, descending or ascending
};

// a sweep under way, as its level launch and its finishing step see it (pointers on the device)
struct LatticeRun {
  int n, N, c;
  size_t nt;                                    // tiles
  hipStream_t stream;
  const double *lt, *obs1, *obs2;               // obs2 with two sets of tables
  const LsTables* tabs;                         // [sets]
  double* V;                                    // [K][2^n]
  DevArr<double> part, d_sum;                   // lattice_summary's
};

// doubles of the summary: per plane mass, pairs [n][n], burden [n + 1]
inline long long gd_summary_doubles(int n) { return 2ll * (1 + (long long)n * n + n + 1); }

// bytes of workspace a sweep over n mutations takes: 8 B a plane and genotype, the sets of tables, 4 B a tile and, with the
// summary, 2 GD_FEAT doubles a tile and the summary itself
inline long long lattice_bytes(int n, int planes, int sets, bool summary) {
  const long long nt = 1ll << (n - ls_tile_bits(n));
  return ((8ll * planes) << n) + sets * (long long)sizeof(LsTables) + 4 * nt +
         (summary ? (long long)sizeof(double) * (2 * GD_FEAT * nt + gd_summary_doubles(n)) : 0);
}

// the query genotypes gen [R][n] (1 = held) as codes: the status of every row, the codes of the valid rows and the rows they
// came from
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
// within a level; first[l]: where level l starts, first[hb + 1] the number of tiles
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

// the refusal of a sweep of K planes whose `need` bytes of workspace exceed the limit
inline void ls_check_workspace(const LatticeSpec& spec, int n, int K, long long need, long long limit) {
  if (need > limit)
    throw Fail{std::string(spec.name) + ": " + std::to_string(n) + " mutations need " + std::to_string(need) +
               " bytes of workspace (" + std::to_string(8 * K) + " B x 2^n_mut" + spec.holds + "), the workspace limit is " +
               std::to_string(limit) + " bytes; there is no partial " + spec.whole};
}

// the model and the tile list to the device - par: theta [N][N], then `sets` obs vectors [N] - and the sets of tables
inline void ls_upload_model(hipStream_t stream, int N, int c, int sets, const double* lt, const double* const* obs,
                            const std::vector<uint32_t>& tiles, double* par, uint32_t* d_tiles, LsTables* tabs) {
  HIPCHECK(hipMemcpyAsync(par, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, stream));
  for (int s = 0; s < sets; ++s)
    HIPCHECK(hipMemcpyAsync(par + N * N + s * N, obs[s], sizeof(double) * N, hipMemcpyHostToDevice, stream));
  HIPCHECK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  for (int s = 0; s < sets; ++s) {
    hipLaunchKernelGGL(k_landscape_tables, dim3(1), dim3(LS_KB), 0, stream, par, par + N * N + s * N, N, c, tabs + s);
    HIPCHECK(hipGetLastError());
  }
}

// the tile numbers that are subsets of `mask` in levels by popcount, ascending within a level: level l holds the subsets
// of popcount l, first[l] where it starts, first[popcount(mask) + 1] their number (partner_host.h's restricted list)
inline void ls_tile_levels_under(uint32_t mask, std::vector<uint32_t>& tiles, std::vector<size_t>& first) {
  const int k = __builtin_popcount(mask);
  first.assign(k + 2, 0);
  tiles.resize((size_t)1 << k);
  uint32_t t = 0;
  do { ++first[__builtin_popcount(t) + 1]; t = (t - mask) & mask; } while (t);
  for (int l = 0; l <= k; ++l) first[l + 1] += first[l];
  std::vector<size_t> at(first.begin(), first.end() - 1);
  do { tiles[at[__builtin_popcount(t)]++] = t; t = (t - mask) & mask; } while (t);
}

// One sweep of K planes.  gen [R][n]: 1 = held (R may be 0); values [R][K] of every query (NaN for a row that is not
// valid); full: nullptr or [K][2^n], every genotype by code; summary: whether the workspace holds lattice_summary's.
// level(X, blocks, tiles) launches the level kernel over the `blocks` tile numbers at `tiles` (on the device);
// finish(X) launches what follows the last level.
template <int K, typename T, typename Level, typename Finish>
void lattice_sweep(Engine<T>& E, const LatticeSpec& spec, const double* lt, const double* obs1, const double* obs2,
                   bool summary, const int8_t* gen, long long R, double* values, int32_t* status, double* full, Level level,
                   Finish finish) {
  const int n = E.n, N = E.N, c = ls_tile_bits(n);
  std::fill(values, values + K * R, std::nan(""));
  ls_check_workspace(spec, n, K, lattice_bytes(n, K, spec.sets, summary), (long long)E.cfg.plan.ws_limit);
  std::vector<uint32_t> codes;
  std::vector<long long> src;
  ls_decode_queries(gen, R, n, status, codes, src);
  const int hb = n - c;
  const size_t nt = (size_t)1 << hb;
  std::vector<uint32_t> tiles;
  std::vector<size_t> first;                           // first[l]: where the tiles of level l start
  ls_tile_levels(hb, spec.descending, tiles, first);
  DevArr<double> par, V, d_out;
  DevArr<LsTables> tabs;
  DevArr<uint32_t> d_tiles, d_codes;
  par.alloc((size_t)N * N + spec.sets * N);
  V.alloc((size_t)K << n);
  tabs.alloc(spec.sets);
  d_tiles.alloc(nt);
  const double* obs[2] = {obs1, obs2};
  ls_upload_model(E.stream, N, c, spec.sets, lt, obs, tiles, par.p, d_tiles.p, tabs.p);
  LatticeRun X{n, N, c, nt, E.stream, par.p, par.p + N * N, spec.sets > 1 ? par.p + N * N + N : nullptr, tabs.p, V.p, {}, {}};
  for (int l = 0; l <= hb; ++l) {
    level(X, (unsigned)(first[l + 1] - first[l]), d_tiles.p + first[l]);
    HIPCHECK(hipGetLastError());
  }
  finish(X);
  std::vector<double> out(K * codes.size());
  if (!codes.empty()) {
    d_codes.alloc(codes.size()); d_out.alloc(out.size());
    HIPCHECK(hipMemcpyAsync(d_codes.p, codes.data(), codes.size() * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
    hipLaunchKernelGGL(k_lattice_gather<K>, dim3((unsigned)((codes.size() + LS_KB - 1) / LS_KB)), dim3(LS_KB), 0, E.stream,
                       d_codes.p, (long long)codes.size(), V.p, n, d_out.p);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
  }
  if (full) HIPCHECK(hipMemcpyAsync(full, V.p, sizeof(double) * ((size_t)K << n), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
  for (size_t j = 0; j < codes.size(); ++j)
    for (int k = 0; k < K; ++k) values[K * src[j] + k] = out[K * j + k];
}

// The finishing step of a sweep with a summary: tile(sums, part) launches the sweep's tile kernel over every tile - it
// turns the planes into probabilities in place and, with sums (std::true_type), folds the GD_FEAT partial sums of the
// first two planes into part -, k_genodist_summary adds the tiles' partials into summary [2][1 + n * n + n + 1] (nullptr:
// no sums).
template <typename Tile>
void lattice_summary(LatticeRun& X, double* summary, Tile tile) {
  if (!summary) {
    tile(std::false_type{}, (double*)nullptr);
    HIPCHECK(hipGetLastError());
    return;
  }
  X.part.alloc((size_t)2 * GD_FEAT * X.nt);
  X.d_sum.alloc((size_t)gd_summary_doubles(X.n));
  tile(std::true_type{}, X.part.p);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_genodist_summary, dim3((unsigned)(2 * gd_summary_items(X.n))), dim3(LS_KB), 0, X.stream, X.part.p,
                     (long long)X.nt, X.n, X.c, X.d_sum.p);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(summary, X.d_sum.p, sizeof(double) * gd_summary_doubles(X.n), hipMemcpyDeviceToHost, X.stream));
}

}  // namespace mmhn
