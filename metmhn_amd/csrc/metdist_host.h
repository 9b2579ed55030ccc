// Host side of the genotype distribution of the metastasis and its founder (metdist.h: k_metdist_level, k_metdist_tile;
// genodist.h's k_genodist_summary): lattice_host.h's sweep with three planes, two sets of tables - of (theta, obs1) and of
// (theta, obs2) -, the levels ascending and, behind them, one launch over every tile that turns the planes into Z, M, C and
// folds the tiles' sums of Z and M, and the summary.
#pragma once
#include "lattice_host.h"
#include "metdist.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// gen [R][n]: 1 = held (R may be 0).  values [R][3]: Z, M, C of every query; summary: nullptr or [2][1 + n * n + n + 1],
// the founder plane Z and then the metastasis plane M; full: nullptr or [3][2^n], every genotype by code.
template <typename T>
void metastasis_distribution(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* gen,
                             long long R, double* values, int32_t* status, double* summary, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the metastasis distribution kernels (n_mut <= 31)");
  static const LatticeSpec spec{"metastasis distribution", ", the rate tables, the tile list and the tiles' partial sums",
                                "distribution", 2, false};
  lattice_sweep<3>(
      E, spec, lt, obs1, obs2, summary != nullptr, gen, R, values, status, full,
      [](const LatticeRun& X, unsigned blocks, const uint32_t* tiles) {
        hipLaunchKernelGGL(k_metdist_level, dim3(blocks), dim3(LS_KB), 0, X.stream, X.tabs, X.tabs + 1, tiles, X.lt, X.obs1,
                           X.obs2, X.N, X.c, X.V);
      },
      [&](LatticeRun& X) {
        lattice_summary(X, summary, [&](auto sums, double* part) {
          hipLaunchKernelGGL(k_metdist_tile<decltype(sums)::value>, dim3((unsigned)X.nt), dim3(LS_KB), 0, X.stream, X.tabs,
                             X.tabs + 1, X.lt, X.obs2, X.N, X.c, X.V, part, (long long)X.nt);
        });
      });
}

}  // namespace mmhn
