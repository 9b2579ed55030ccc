// Host side of the seeding landscape (landscape.h: k_landscape_level): lattice_host.h's sweep with four planes, one set of
// tables, the levels descending and no finishing step.
#pragma once
#include <cmath>

#include "landscape.h"
#include "lattice_host.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// gen [R][n]: 1 = held (R may be 0).  until: 0 the seeding, 1 the seeding or the clock of the first observation.
// values [R][4]: p_seed, time, new_events, seed_events of every query; full: nullptr or [4][2^n], every genotype by code.
template <typename T>
void seeding_landscape(Engine<T>& E, const double* lt, const double* obs1, int until, const int8_t* gen, long long R,
                       double* values, int32_t* status, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the landscape kernels (n_mut <= 31)");
  REQUIRE(until == 0 || until == 1, "until must be 0 (the seeding) or 1 (the seeding or the observation)");
  if (until == 0) {
    const int n = E.n, N = E.N;
    double s = lt[n * N + n];
    for (int i = 0; i < n; ++i) s += lt[n * N + i];
    REQUIRE(std::exp(s) > 0.0, "seeding landscape until the seeding: the seeding rate of the full genotype underflows to 0, "
                               "so the chain has a state without exit (a model fitted without a seeded sample?); use until = observation");
  }
  static const LatticeSpec spec{"seeding landscape", ", the rate tables and the tile list", "landscape", 1, true};
  lattice_sweep<4>(
      E, spec, lt, obs1, nullptr, false, gen, R, values, status, full,
      [&](const LatticeRun& X, unsigned blocks, const uint32_t* tiles) {
        hipLaunchKernelGGL(k_landscape_level, dim3(blocks), dim3(LS_KB), 0, X.stream, X.tabs, tiles, X.lt, X.obs1, X.N, X.c,
                           until, X.V);
      },
      [](LatticeRun&) {});
}

}  // namespace mmhn
