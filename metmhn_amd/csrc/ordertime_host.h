// Host side of the posterior event and observation times of a cohort (ordertime.h: k_order_time): orderpost_host.h's
// decoding, limits, batching and launches (opr_rows) with this kernel's workspace and block - 1 or 2 vectors of partials
// behind the tables and k + 3 doubles per row, where opr_move_rows fixes k vectors and a k x k block; the same limit of
// OPO_CB joint events -, and the scatter of a row's times to the event codes.
#pragma once
#include "orderprec_host.h"
#include "ordertime.h"

namespace mmhn {

// time [npat][2n+1] over the event codes: NaN where a code is not in the row.  obs [npat][2]: the first and the second
// observation (NaN: a one-tumour row has one).  pt_first [npat]: NaN in the one-tumour rows.
template <typename T>
void order_times(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                 int ncols, double* log_ev, double* time, double* obs, double* pt_first, int32_t* status) {
  const long long L = 2 * E.n + 1;
  std::fill(time, time + npat * L, std::nan(""));
  std::fill(obs, obs + npat * 2, std::nan(""));
  std::fill(pt_first, pt_first + npat, std::nan(""));
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, opr_launch(k_order_time<256>, k_order_time<1024>),
           [](const ORow& r) { return otime_doubles(r, r.k >= ORD_BIG_K ? 1024 : 256); },
           [](const ORow& r) { return (long long)r.k + 3; }, [](const ORow&) { return 0ll; }, false,
           [](const ORow& r) { return __builtin_popcount(r.joint) <= OPO_CB; },
           [&](const ORow& r, long long i, const double* in, const int8_t*) {
             for (int d = 0; d < r.k; ++d) time[i * L + r.code[d]] = in[d];
             obs[2 * i] = in[r.k]; obs[2 * i + 1] = in[r.k + 1];
             pt_first[i] = in[r.k + 2];
           });
}

}  // namespace mmhn
