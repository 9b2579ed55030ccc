// Host side of the posterior event positions of a cohort (orderpos.h: k_order_pos): orderprec_host.h's decoding, limits,
// batching and launches (opr_move_rows; the kernel's workspace is never larger than k_order_prec's, so the same rows fit), and
// the scatter of a row's compact slot x position matrix to the events of the two lineages.
#pragma once
#include "orderpos.h"
#include "orderprec_host.h"

namespace mmhn {

// pos_pt / pos_mt [npat][n+1][n+1] (event, position; event n: the seeding): NaN for an event the row does not carry in
// that lineage, 0 at the positions past the lineage's length.
template <typename T>
void order_positions(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                     int ncols, double* log_ev, double* pos_pt, double* pos_mt, int32_t* status) {
  const long long N = E.N;
  std::fill(pos_pt, pos_pt + npat * N * N, std::nan(""));
  std::fill(pos_mt, pos_mt + npat * N * N, std::nan(""));
  opr_move_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, k_order_pos<256>, k_order_pos<1024>,
                [&](const ORow& r, long long i, const double* in) {
                  auto put = [&](double* pos, int d) {
                    double* out = pos + (i * N + r.ev[d]) * N;
                    for (int j = 0; j < N; ++j) out[j] = j < r.k ? in[d * r.k + j] : 0.0;
                  };
                  for (int d = 0; d < r.k; ++d) {
                    // the seeding is an entry of every lineage the row has
                    const bool in_pt = r.kind[d] == ORD_K_PT || (r.kind[d] == ORD_K_SEED && r.mode != ORD_MT);
                    const bool in_mt = r.kind[d] == ORD_K_MT || (r.kind[d] == ORD_K_SEED && r.mode != ORD_PT);
                    if (in_pt) put(pos_pt, d);
                    if (in_mt) put(pos_mt, d);
                  }
                });
}

}  // namespace mmhn
