// Host side of the genotype distribution (genodist.h: k_genodist_level, k_genodist_tile, k_genodist_summary):
// lattice_host.h's sweep with two planes, one set of tables, the levels ascending and, behind them, one launch over every
// tile that turns the planes into probabilities and folds the tiles' sums, and the summary.
#pragma once
#include "genodist.h"
#include "lattice_host.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// gen [R][n]: 1 = held (R may be 0).  values [R][2]: U, S of every query; summary: nullptr or [2][1 + n * n + n + 1];
// full: nullptr or [2][2^n], every genotype by code.
template <typename T>
void genotype_distribution(Engine<T>& E, const double* lt, const double* obs1, const int8_t* gen, long long R,
                           double* values, int32_t* status, double* summary, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the genotype distribution kernels (n_mut <= 31)");
  static const LatticeSpec spec{"genotype distribution", ", the rate tables, the tile list and the tiles' partial sums",
                                "distribution", 1, false};
  lattice_sweep<2>(
      E, spec, lt, obs1, nullptr, summary != nullptr, gen, R, values, status, full,
      [](const LatticeRun& X, unsigned blocks, const uint32_t* tiles) {
        hipLaunchKernelGGL(k_genodist_level, dim3(blocks), dim3(LS_KB), 0, X.stream, X.tabs, tiles, X.lt, X.obs1, X.N, X.c, X.V);
      },
      [&](LatticeRun& X) {
        lattice_summary(X, summary, [&](auto sums, double* part) {
          hipLaunchKernelGGL(k_genodist_tile<decltype(sums)::value>, dim3((unsigned)X.nt), dim3(LS_KB), 0, X.stream, X.tabs,
                             X.obs1, X.N, X.c, X.V, part, (long long)X.nt);
        });
      });
}

}  // namespace mmhn
