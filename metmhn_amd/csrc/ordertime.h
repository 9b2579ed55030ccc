// Posterior event and observation times of a cohort: the device form of metmhn_amd/model.py MetMHN.order_time, on the row
// set-up, tables and passes of orderpass.h (every order kernel's) and the backward passes over every state and the bit
// sums of orderprec.h (k_order_prec's).
//
// Given a path, the chain holds in a state x for an Exp(den[x]) time that does not depend on the move that follows, so the
// posterior mean of a time is a sum of (posterior probability that the chain passes through x in regime r) / den_r[x]:
//   one tumour    h(x)  = F[x] G[x]                       (F carries 1 / den[x], G = B / den: occupancy / den)
//   both tumours  hu(x) = F[x]_a Bu[x] / den[x]           unseeded x whose tumours agree
//                 ha(x) = F[x]_a B[x]_a / den[x]          seeded x, no observation made yet
//                 hb(x) = bP B[x]_P / den_mt[x] + bM B[x]_M / den_pt[x]   seeded x, (a, bP, bM) = _settle(F[x]): the first
//                         observation made, the other tumour runs on alone (each term under its diagnosis-order flag only:
//                         den_mt / den_pt are not written otherwise)
//   output        time of slot d = (1 / Z) sum of h over the states WITHOUT bit d (the event is still to come); the first
//                 observation (1 / Z) (sum hu + sum ha), the second that plus (1 / Z) sum hb; one tumour: its one observation
//                 (1 / Z) sum h.  pt_first = bP(full) o2[full] / Z = P(the primary tumour was observed first | the row):
//                 exactly 1 / 0 where the row's diagnosis order says so, since the other term of Z is an exact zero.
//
// The reduction.  One vector h over the m = k index bits of a one-tumour row, two (ha, hb) over the m = k - 1 index bits
// of the seeded half of a paired one (x = idx | top).  opr_bit_sums gives the sums over the idx WITH a bit set; it is
// handed val(t, idx ^ (2^m - 1)), so bit d's sum is the sum of h over the states with bit d clear - no subtraction from
// the total, no cancellation.  The unseeded states (at most 2^10, B in LDS behind bu): one wave per joint event q (the
// states without q) and one for the total, lanes striding e, then opo_wave_sum.  Every value is written once, every sum has
// a shape fixed by k and the thread count, no atomics: a row's result does not depend on the batch or the run.
//
// Workspace of a row: opost_doubles + oprec_part_doubles(nt, m, c) with nt = 1, m = k (one tumour) or nt = 2, m = k - 1
// (paired) - from 4 slots on less than k_order_prec's k vectors of m - 1 bits.  Output: k times in slot order, the first
// observation, the second (NaN: one tumour), pt_first (NaN: one tumour) - k + 3 doubles; the host side scatters the times to
// the event codes.  fp64 only.
#pragma once
#include "orderprec.h"

namespace mmhn {

// index bits of the vectors k_order_time reduces, and how many there are
inline int otime_bits(const ORow& r) { return r.mode == ORD_PAIRED ? r.k - 1 : r.k; }
inline int otime_vectors(const ORow& r) { return r.mode == ORD_PAIRED ? 2 : 1; }

// workspace of a row in doubles (kb: threads of the row's launch)
inline long long otime_doubles(const ORow& r, int kb) {
  const int m = otime_bits(r);
  return opost_doubles(r) + oprec_part_doubles(otime_vectors(r), m, opo_chunk_bits(m, kb));
}

// ha of the seeded state x: the time the chain spends there before any observation, times Z
__device__ __forceinline__ double otm_before(const OprPaired& P, uint32_t x) {
  return P.F[3ll * x] * P.B[3ll * (x ^ P.top)] / P.den[x];
}

// hb of the seeded state x: the time the remaining tumour spends there after the first observation, times Z
__device__ __forceinline__ double otm_after(const ORow& r, const OprPaired& P, uint32_t x) {
  const OrdTab t{P.o1, P.o2, P.dmt, P.dpt};
  double fa = P.F[3ll * x], fp = P.F[3ll * x + 1], fm = P.F[3ll * x + 2];
  ord_settle(r, t, x, fa, fp, fm);
  const double* g = P.B + 3ll * (x ^ P.top);
  double w = 0.0;
  if (r.pt_first) w += fp * g[1] / P.dmt[x];
  if (r.mt_first) w += fm * g[2] / P.dpt[x];
  return w;
}

// hu of the unseeded state of the joint events e
__device__ __forceinline__ double otm_unseeded(const OprRow& S, const OprPaired& P, const double* bu, uint32_t e) {
  const uint32_t x = opr_joint_state(S, e);
  return P.F[3ll * x] * bu[e] / P.den[x];
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), coff chunk partials, foff the row's k + 3 doubles of out_time.  out_le [row]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_time(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                   const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                   double* tab, double* out_le, double* out_time) {
  __shared__ OprRow S;
  __shared__ double bu[1 << OPO_CB];           // paired: B of the unseeded state of the joint events e
  __shared__ double Rs[2][33];                 // Rs[t][j]: vector t summed over the states without slot j; Rs[t][m] its total
  __shared__ double Ru[OPO_CB + 1];            // paired, before the seeding: hu summed over the states without joint event
                                               // q; Ru[kj] its total
  const int tid = threadIdx.x;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const int k = r.k;
  double* den = tab + opr_uniform(r.toff);
  double* part = tab + opr_uniform(r.coff);
  double* O = out_time + opr_uniform(r.foff);
  const double nan = __builtin_nan("");

  if (r.mode != ORD_PAIRED) {
    double* F = den + (1ll << k);
    const double Z = opr_single_passes<KB>(S, N, den, F);
    if (tid == 0) {
      out_le[r.row] = log(Z);
      O[k + 1] = nan; O[k + 2] = nan;
      if (k == 0) O[0] = 1.0 / den[0];         // the empty row: the chain held in the event-free state until it was seen
    }
    if (k == 0) return;
    const uint32_t all = (1u << k) - 1u;
    const double* G = den;
    opr_bit_sums<KB>(1, k, opo_chunk_bits(k, KB), part,
        [&](int, uint32_t idx) { const uint32_t x = idx ^ all; return F[x] * G[x]; },
        [&](int, int j, double s) { Rs[0][j] = s; });
    for (int i = tid; i <= k; i += KB) O[i] = Rs[0][i] / Z;
    return;
  }

  const OprPaired T = opr_paired_tables(r, den);
  const double Z = opr_paired_passes<KB>(S, N, T);
  opr_unseeded_backward<KB>(S, N, T, bu);
  const int kj = T.kj, m = k - 1;
  const uint32_t all = (1u << m) - 1u;
  // after the seeding: x = idx | top holds the seeding; vector 0 before, vector 1 after the first observation
  opr_bit_sums<KB>(2, m, opo_chunk_bits(m, KB), part,
      [&](int t, uint32_t idx) {
        const uint32_t x = (idx ^ all) | T.top;
        return t == 0 ? otm_before(T, x) : otm_after(r, T, x);
      },
      [&](int t, int j, double s) { Rs[t][j] = s; });
  // before the seeding: one wave per joint event (the states without it) and one for the total, the lanes stride the states
  {
    const int wave = tid >> 6, lane = tid & 63;
    const uint32_t EJ = 1u << kj;
    for (int q = wave; q <= kj; q += KB / 64) {
      double s = 0.0;
      for (uint32_t e = lane; e < EJ; e += 64)
        if (q == kj || !((e >> q) & 1u)) s += otm_unseeded(S, T, bu, e);
      s = opo_wave_sum(s);
      if (lane == 0) Ru[q] = s;
    }
  }
  __syncthreads();
  for (int d = tid; d < k; d += KB) {
    // the seeding's own time: every unseeded state; a slot of one tumour alone is in no unseeded state
    double s = Ru[d < m && S.jev[d] >= 0 ? S.jev[d] : kj];
    if (d < m) s += Rs[0][d] + Rs[1][d];
    O[d] = s / Z;
  }
  if (tid == 0) {
    const uint32_t full = (1u << k) - 1u;
    const OrdTab t{T.o1, T.o2, T.dmt, T.dpt};
    double fa = T.F[3ll * full], fp = T.F[3ll * full + 1], fm = T.F[3ll * full + 2];
    ord_settle(r, t, full, fa, fp, fm);
    const double first = Ru[kj] + Rs[0][m];
    out_le[r.row] = log(Z);
    O[k] = first / Z;
    O[k + 1] = (first + Rs[1][m]) / Z;
    O[k + 2] = fp * T.o2[full] / Z;
  }
}

}  // namespace mmhn
