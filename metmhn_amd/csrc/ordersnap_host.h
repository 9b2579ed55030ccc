// Host side of the posterior genotypes at the first observation of a cohort (ordersnap.h: k_order_snap): orderpost_host.h's
// decoding, limits, batching and launches (opr_rows) with this kernel's workspace and block - 2 vectors of partials behind
// the tables and 4 k + 3 doubles per paired row, nothing but the evidence of a one-tumour row; no limit on the joint events,
// the row predicate is order_posteriors' -, and the scatter of a row's block to the event codes.
#pragma once
#include "orderpos_host.h"
#include "ordersnap.h"

namespace mmhn {

// held [npat][2][2n+1] over the event codes: NaN where a code is not in the row.  late [npat][2][n+1].  map_state
// [npat][2n+1]: 1 held, 0 carried and still to come, -1 not in the row; map_first [npat]; map_prob [npat].  Rows without a
// first observation (one tumour) keep NaN / -1 throughout.
template <typename T>
void order_snapshots(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat,
                     long long npat, int ncols, double* log_ev, double* held, double* late, int8_t* map_state,
                     int32_t* map_first, double* map_prob, int32_t* status) {
  const long long L = 2 * E.n + 1, N = E.N;
  std::fill(held, held + npat * 2 * L, std::nan(""));
  std::fill(late, late + npat * 2 * N, std::nan(""));
  std::fill(map_state, map_state + npat * L, (int8_t)-1);
  std::fill(map_first, map_first + npat, -1);
  std::fill(map_prob, map_prob + npat, std::nan(""));
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, opr_launch(k_order_snap<256>, k_order_snap<1024>),
           [](const ORow& r) { return osnap_doubles(r, r.k >= ORD_BIG_K ? 1024 : 256); },
           [](const ORow& r) { return osnap_block(r); }, [](const ORow&) { return 0ll; }, false,
           [](const ORow&) { return true; },
           [&](const ORow& r, long long i, const double* in, const int8_t*) {
             if (r.mode != ORD_PAIRED) return;
             const int k = r.k;
             const uint32_t x = (uint32_t)in[4 * k + 1];
             for (int t = 0; t < 2; ++t) {
               for (int d = 0; d < k; ++d) held[(2 * i + t) * L + r.code[d]] = in[t * k + d];
               // (the other tumour has at most n slots: the entries past them are zeros in the block too)
               for (int j = 0; j < N; ++j) late[(2 * i + t) * N + j] = j < k ? in[2 * k + t * k + j] : 0.0;
             }
             for (int d = 0; d < k; ++d) map_state[i * L + r.code[d]] = (int8_t)((x >> d) & 1u);
             map_first[i] = (int32_t)in[4 * k];
             map_prob[i] = in[4 * k + 2];
           });
}

}  // namespace mmhn
