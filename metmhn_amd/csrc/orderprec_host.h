// Host side of the pairwise precedence posteriors of a cohort (orderprec.h: k_order_prec): orderpost_host.h's decoding,
// limits, batching and launches (opr_rows) with the workspace, the block and the limit of the kernels that sum move masses
// (opr_move_rows; orderpos_host.h calls it too), and the scatter of a row's compact slot matrix to the event codes.
#pragma once
#include "orderpost_host.h"
#include "orderprec.h"

namespace mmhn {

// opr_rows for k_order_prec / k_order_pos (orderpos.h): chunk partials behind the tables (the thread count of the row's
// launch sizes them), a compact k x k block per row, and at most OPO_CB joint events - with more, 23 slots or more, the
// unseeded states would not fit the kernels' LDS
template <typename T, class Scatter>
void opr_move_rows(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                   int ncols, double* log_ev, int32_t* status, OprKernel k256, OprKernel k1024, Scatter scatter) {
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, opr_launch(k256, k1024),
           [](const ORow& r) { return oprec_doubles(r, r.k >= ORD_BIG_K ? 1024 : 256); },
           [](const ORow& r) { return (long long)r.k * r.k; }, [](const ORow&) { return 0ll; }, false,
           [](const ORow& r) { return __builtin_popcount(r.joint) <= OPO_CB; },
           [&](const ORow& r, long long i, const double* in, const int8_t*) { scatter(r, i, in); });
}

// prec [npat][2n+1][2n+1] over the event codes: NaN where a code is not in the row.
template <typename T>
void order_precedences(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                       int ncols, double* log_ev, double* prec, int32_t* status) {
  const long long L = 2 * E.n + 1;
  std::fill(prec, prec + npat * L * L, std::nan(""));
  opr_move_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, k_order_prec<256>, k_order_prec<1024>,
                [&](const ORow& r, long long i, const double* in) {
                  double* out = prec + i * L * L;
                  for (int a = 0; a < r.k; ++a)
                    for (int b = 0; b < r.k; ++b) out[r.code[a] * L + r.code[b]] = in[a * r.k + b];
                });
}

}  // namespace mmhn
