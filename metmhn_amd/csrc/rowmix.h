// Row groups (mmhn_set_row_groups): a group is a list of cohort rows that are alternatives of one patient - the completions
// of a row with unobserved entries.  Its likelihood is the sum of theirs,
//   lp_g = log sum_{r in g} exp(lp_r)      grad_g = sum_{r in g} rho_{g,r} grad_r      rho_{g,r} = exp(lp_r - lp_g),
// so the cohort sums are those of the per-row values with the mixing weights
//   omega_r = sum_{g holds r} w_g rho_{g,r}  (elements e >= 1)      lambda_r = sum_{g holds r} w_g rho_{g,r} lp_g  (element 0).
// Everything here is fp64 whatever the engine's dtype (lp and out are double), and every sum has a fixed order: no atomics.
#pragma once
#include "common.h"

namespace mmhn {

constexpr int MIX_WAVE = 64;                       // one wave per group
constexpr int MIX_WAVES = BLOCK / MIX_WAVE;        // groups per workgroup of k_group_lse

// device view of the groups held by an engine: the group lists (CSR over the groups, rows = cohort rows), the transposed
// lists (CSR over the cohort rows, mgrp = the groups a row belongs to, in group order) and the per-evaluation arrays
struct MixDev {
  const long long* gptr; const int* grows; const double* gw; int n_groups;
  const long long* mptr; const int* mgrp; int n_rows;
  double* lpc;                                     // [n_rows]   lp by COHORT row (the batches write their rows)
  double* lpg;                                     // [n_groups] lp_g
  double* omega; double* lambda;                   // [n_rows]
};

// lpc[cohort row] = element 0 of the batch's assembled rows
__global__ __launch_bounds__(BLOCK) void k_mix_gather(const PatRec* __restrict__ pats, int npat, const double* __restrict__ out,
                                                      int stride, double* __restrict__ lpc) {
  const int i = blockIdx.x * BLOCK + threadIdx.x;
  if (i < npat) lpc[pats[i].row] = out[(long long)i * stride];
}

// butterfly over the wave: every lane ends with the same bits (a + b and b + a round alike), the tree is fixed
__device__ __forceinline__ double mix_wave_max(double v) {
#pragma unroll
  for (int o = MIX_WAVE / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, MIX_WAVE));
  return v;
}
__device__ __forceinline__ double mix_wave_sum(double v) {
#pragma unroll
  for (int o = MIX_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, MIX_WAVE);
  return v;
}

// lp_g of every group: one wave per group.  Lane l takes the alternatives l, l + 64, ... of the list in that order (a group
// longer than a wave strides through it), the lanes are joined by the butterfly.  The maximum is subtracted, so an alternative
// more than ~745 below it adds exactly 0 and nothing overflows.  rho (optional, mmhn_group_posteriors): rho[ptr[g] + s].
__global__ __launch_bounds__(BLOCK) void k_group_lse(MixDev m, double* __restrict__ rho) {
  const int lane = threadIdx.x % MIX_WAVE;
  const int g = blockIdx.x * MIX_WAVES + threadIdx.x / MIX_WAVE;
  if (g >= m.n_groups) return;                     // (uniform over the wave)
  const long long a = m.gptr[g], b = m.gptr[g + 1];
  double mx = -INFINITY;
  for (long long k = a + lane; k < b; k += MIX_WAVE) mx = fmax(mx, m.lpc[m.grows[k]]);
  mx = mix_wave_max(mx);
  double s = 0;
  for (long long k = a + lane; k < b; k += MIX_WAVE) s += exp(m.lpc[m.grows[k]] - mx);
  s = mix_wave_sum(s);
  const double lg = mx + log(s);
  if (lane == 0) m.lpg[g] = lg;
  if (rho)
    for (long long k = a + lane; k < b; k += MIX_WAVE) rho[k] = exp(m.lpc[m.grows[k]] - lg);
}

// omega_r, lambda_r of every cohort row from its memberships, in list order (= group order).  A membership in a group of
// weight 0 is selected out, not multiplied: that group's rows may hold anything.
__global__ __launch_bounds__(BLOCK) void k_mix_weights(MixDev m) {
  const int r = blockIdx.x * BLOCK + threadIdx.x;
  if (r >= m.n_rows) return;
  double om = 0, la = 0;
  const double lr = m.lpc[r];
  for (long long k = m.mptr[r]; k < m.mptr[r + 1]; ++k) {
    const int g = m.mgrp[k];
    const double w = m.gw[g];
    if (w == 0.0) continue;
    const double lg = m.lpg[g];
    const double t = w * exp(lr - lg);
    om += t;
    la += t * lg;
  }
  m.omega[r] = om;
  m.lambda[r] = la;
}

// k_reduce_rows_w with the mixing weights in the place of the row weights: the same rows in the same order, chunks and part[]
// layout; the addend of row r is omega_r * v for e >= 1 and lambda_r for e = 0 (out is not read there).  A row with
// omega_r == 0 (in no group, only in groups of weight 0, or with every rho underflowed) is selected out.
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_mix(const PatRec* __restrict__ pats, int npat, int per,
                                                           const double* __restrict__ out, int stride, int nelem,
                                                           const double* __restrict__ omega, const double* __restrict__ lambda,
                                                           double* __restrict__ part) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= nelem) return;
  const int i0 = blockIdx.y * per, i1 = min(npat, i0 + per);
  double acc0 = 0, acc1 = 0;
#pragma unroll 4
  for (int i = i0; i < i1; ++i) {
    const int kd = pats[i].kind, r = pats[i].row;
    const double om = omega[r];
    double a = 0.0;
    if (om != 0.0) a = e == 0 ? lambda[r] : om * out[(long long)i * stride + e];
    if (kd == 0 || kd >= 4) acc1 += a; else acc0 += a;
  }
  part[((long long)blockIdx.y * 2 + 0) * stride + e] = acc0;
  part[((long long)blockIdx.y * 2 + 1) * stride + e] = acc1;
}

}  // namespace mmhn
