// Posterior genotypes at the first observation of a cohort's paired rows: the device form of metmhn_amd/model.py
// MetMHN.order_snapshot, on the row set-up, tables and passes of orderpass.h (every order kernel's), the bit sums of
// orderprec.h (k_order_prec's) and the popcount-class sums of orderpos.h (k_order_pos').
//
// The first observation of a paired row falls in a seeded state x that holds every slot of the tumour it is made of.  With
// F, B and Z of opr_paired_passes (F unsettled, B[x]_P / B[x]_M the weights the rest of the order gives the two settled
// components, which _settle's transpose leaves alone):
//   sP(x) = [pt_first and x holds every PT slot]  F[x]_a o1[x] / den_mt[x] B[x]_P
//   sM(x) = [mt_first and x holds every MT slot]  F[x]_a o2[x] / den_pt[x] B[x]_M
// are Z times the posterior probability that the first observation was of the primary tumour (the metastasis) AND found
// the chain in x.  The observation lies in the seeded half: no backward pass over the unseeded states, so neither their
// LDS array nor the limit of OPO_CB joint events of k_order_prec / k_order_pos / k_order_time.
//   held[t][d]  = (1 / Z) sum of s_t over the states holding slot d; the seeding's entry is the total of s_t
//   late[t][j]  = (1 / Z) sum of s_t over the states that lack j slots of the other tumour
//   snapshot    the (t, x) of largest s_t; of equal masses t = 0 before t = 1, then the smaller x - a total order, so the
//               result does not depend on the shape of the reduction
//
// The reduction.  Two vectors (sP, sM) over the m = k - 1 index bits of the seeded half (x = idx | top), structural zeros
// where the state lacks a slot of the observed tumour or the diagnosis order excludes the regime - a test of two masks in
// registers, no memory read.  opr_bit_sums gives held (sums over the idx WITH a bit set: no complement), opp_class_sums the
// sums by popcount(idx & the other tumour's slots) in the same chunk partials once the bit sums are done, and a plain
// strided loop keeps every thread's best (mass, t, x), reduced over the wave with shuffles and over the waves through LDS.
// A state's mass is formed three times (three reads of F, B and two tables for the 2^(slots of the other tumour) states
// that have one); next to the passes (k moves with an exp each per state and pass) that is under 1 / k of the work.
// Every value is written once, every sum has a shape fixed by k, the thread count and the row's masks, no atomics: a row's
// result does not depend on the batch or the run.
//
// Workspace of a row: paired opost_doubles + oprec_part_doubles(2, k - 1, c); one tumour opost_doubles (the evidence only).
// Output of a paired row: held [2][k] in slot order, late [2][k], the snapshot's t, its x and its probability - 4 k + 3
// doubles (x < 2^32 fits a double exactly); none of a one-tumour row.  The host side scatters the block to the event
// codes.  fp64 only.
#pragma once
#include "orderpos.h"

namespace mmhn {

// workspace of a row in doubles (kb: threads of the row's launch)
inline long long osnap_doubles(const ORow& r, int kb) {
  if (r.mode != ORD_PAIRED) return opost_doubles(r);
  const int m = r.k - 1;
  return opost_doubles(r) + oprec_part_doubles(2, m, opo_chunk_bits(m, kb));
}

// doubles of a row's output block
inline long long osnap_block(const ORow& r) { return r.mode == ORD_PAIRED ? 4ll * r.k + 3 : 0; }

// s_t of the seeded state x (t = 0: the primary tumour observed first, 1: the metastasis)
__device__ __forceinline__ double osn_mass(const ORow& r, const OprPaired& P, int t, uint32_t x) {
  const bool pt = t == 0;
  const uint32_t own = pt ? r.pt_mask : r.mt_mask;
  if (!(pt ? r.pt_first : r.mt_first) || (x & own) != own) return 0.0;
  const double* o = pt ? P.o1 : P.o2;
  const double* dn = pt ? P.dmt : P.dpt;
  return P.F[3ll * x] * o[x] / dn[x] * P.B[3ll * (x ^ P.top) + (pt ? 1 : 2)];
}

// the order of the snapshots: the larger mass, then the smaller key = t << 31 | idx
__device__ __forceinline__ bool osn_better(double s, uint32_t key, double best, uint32_t best_key) {
  return s > best || (s == best && key < best_key);
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), coff chunk partials, foff the row's 4 k + 3 doubles of out_snap.  out_le [row]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_snap(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                   const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                   double* tab, double* out_le, double* out_snap) {
  __shared__ OprRow S;
  __shared__ double Hs[2][33];                 // Hs[t][j]: s_t summed over the states holding slot j; Hs[t][m] its total
  __shared__ double Ls[2][33];                 // Ls[t][q]: s_t summed over the states holding q slots of the other tumour
  __shared__ double wbest[KB / 64];            // the waves' best snapshots
  __shared__ uint32_t wkey[KB / 64];
  const int tid = threadIdx.x;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const int k = r.k;
  double* den = tab + opr_uniform(r.toff);

  if (r.mode != ORD_PAIRED) {                  // one tumour has one observation: the evidence only
    const double Z = opr_single_passes<KB>(S, N, den, den + (1ll << k));
    if (tid == 0) out_le[r.row] = log(Z);
    return;
  }

  double* part = tab + opr_uniform(r.coff);
  double* O = out_snap + opr_uniform(r.foff);
  const OprPaired T = opr_paired_tables(r, den);
  const double Z = opr_paired_passes<KB>(S, N, T);
  const int m = k - 1, c = opo_chunk_bits(m, KB);
  const auto mass = [&](int t, uint32_t idx) { return osn_mass(r, T, t, idx | T.top); };
  opr_bit_sums<KB>(2, m, c, part, mass, [&](int t, int j, double s) { Hs[t][j] = s; });
  // by the slots of the other tumour the state holds; the chunk partials are free again
  opp_class_sums<KB>(2, m, c, part, mass, [&](int t) { return t == 0 ? r.mt_mask : r.pt_mask; },
                     [&](int t, int q, double s) { Ls[t][q] = s; });
  // the snapshot of largest mass: every thread's best over the states it visits, then the wave's, then the row's
  double best = -1.0;
  uint32_t key = 0xFFFFFFFFu;
  for (int t = 0; t < 2; ++t) {
    if (!(t == 0 ? r.pt_first : r.mt_first)) continue;
    const uint32_t own = t == 0 ? r.pt_mask : r.mt_mask;
    for (uint32_t idx = tid; idx < (1u << m); idx += KB) {
      if ((idx & own) != own) continue;
      const double s = mass(t, idx);
      const uint32_t ky = ((uint32_t)t << 31) | idx;
      if (osn_better(s, ky, best, key)) { best = s; key = ky; }
    }
  }
  for (int d = 32; d; d >>= 1) {
    const double ob = __shfl_xor(best, d, 64);
    const uint32_t ok = __shfl_xor(key, d, 64);
    if (osn_better(ob, ok, best, key)) { best = ob; key = ok; }
  }
  if ((tid & 63) == 0) { wbest[tid >> 6] = best; wkey[tid >> 6] = key; }
  __syncthreads();
  for (int i = tid; i < 2 * k; i += KB) {
    const int t = i / k, d = i - t * k;
    // (a probability: the quotient of two roundings may pass 1)
    O[i] = fmin(Hs[t][d] / Z, 1.0);            // d = m: the seeding, which every state of the sum holds - the total
    const int q = __builtin_popcount(t == 0 ? r.mt_mask : r.pt_mask) - d;      // d slots of the other tumour still to come
    O[2 * k + i] = q >= 0 ? fmin(Ls[t][q] / Z, 1.0) : 0.0;
  }
  if (tid == 0) {
    for (int w = 0; w < KB / 64; ++w)
      if (osn_better(wbest[w], wkey[w], best, key)) { best = wbest[w]; key = wkey[w]; }
    out_le[r.row] = log(Z);
    O[4 * k] = (double)(key >> 31);
    O[4 * k + 1] = (double)((key & 0x7FFFFFFFu) | T.top);
    O[4 * k + 2] = fmin(best / Z, 1.0);
  }
}

}  // namespace mmhn
