// Host side of the posterior order samples of a cohort (ordersample.h: k_order_sample): orderpost_host.h's decoding, limits,
// batching and launches (opr_rows) with the kernel's further arguments, its int8 block of orders beside the block of
// log-probabilities, and the outputs counted in the batch cut - the samples of a row (n_samples x (2 N - 1 + 8) bytes) can
// outweigh its lattice.
#pragma once
#include "orderprec_host.h"
#include "ordersample.h"

namespace mmhn {

// orders [npat][n_samples][2n+1] padded with -1, log_prob [npat][n_samples]: -1 / NaN throughout where status is not 0.
// Rows of more than OPO_CB joint events are turned away as in opr_move_rows (the unseeded states are in LDS).
template <typename T>
void order_samples(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                   int ncols, long long first, long long n_samples, uint64_t seed, double* log_ev, int8_t* orders,
                   double* log_prob, int32_t* status) {
  const long long L = 2 * E.n + 1;
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status,
           [=](bool big, size_t grid, hipStream_t stream, const ORow* rows, const double* par, int N, double* tab, double* le,
               double* lp, int8_t* ord) {
             hipLaunchKernelGGL(big ? k_order_sample<1024> : k_order_sample<256>, dim3(grid), dim3(big ? 1024 : 256), 0, stream,
                                rows, par, par + N * N, par + N * N + N, N, tab, le, first, n_samples, seed, lp, ord, (int)L);
           },
           [](const ORow& r) { return opost_doubles(r); }, [=](const ORow&) { return n_samples; },
           [=](const ORow&) { return n_samples * L; }, true,
           [](const ORow& r) { return __builtin_popcount(r.joint) <= OPO_CB; },
           [&](const ORow&, long long i, const double* lp, const int8_t* ord) {
             std::memcpy(log_prob + i * n_samples, lp, sizeof(double) * n_samples);
             std::memcpy(orders + i * n_samples * L, ord, (size_t)(n_samples * L));
           });
  for (long long i = 0; i < npat; ++i)          // (only the rows no kernel wrote: the orders are the largest array of the call)
    if (status[i] != MMHN_ORD_OK) {
      std::fill(orders + i * n_samples * L, orders + (i + 1) * n_samples * L, (int8_t)-1);
      std::fill(log_prob + i * n_samples, log_prob + (i + 1) * n_samples, std::nan(""));
    }
}

}  // namespace mmhn
