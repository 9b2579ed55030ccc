// Pre-seeding posteriors of a cohort: the sum-product twin of orders.h (k_orders), the device form of
// metmhn_amd/model.py MetMHN.order_posterior, on the tables and passes of orderpass.h.
//   edges     w(x) = B[x | top]_a * F[x]_a * num_top / den[x | top]       the mass of the orders that seed at x
//   outputs   log Z; pre[m] = sum of w over the x that hold m, seed_pos[j] = sum of w over the x with j events, both
//             over Z
// One tumour: opr_single_forward over k - 1 walked bits, then its own backward pass over the seeded half, in F's place.
// Both tumours: opr_paired_passes, whose B over the seeded half is all the edges need - no unseeded backward pass, no
// limit on the joint events.  The reductions have a fixed shape: no atomics, the result of a row does not depend on the
// batch, the launch geometry or the run.  fp64 only.
#pragma once
#include "orderpass.h"

namespace mmhn {

// The edge masses w[e * stride], e in [0, 2^ne), bit i of e = event evb[i]: pre and seed_pos of the row.  One wave per
// output, the lanes stride over e, one tree per output.
template <int KB>
__device__ __forceinline__ void opo_reduce(const double* w, int stride, int ne, const int8_t* evb, double Z, int n,
                                           double* pre, double* sp) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t E = 1u << ne;
  for (int o = wave; o < 2 * ne + 1; o += KB / 64) {
    double s = 0.0;
    for (uint32_t e = lane; e < E; e += 64) {
      const bool in = o < ne ? (e >> o) & 1u : __builtin_popcount(e) == o - ne;
      if (in) s += w[(long long)e * stride];
    }
    s = opo_wave_sum(s);
    if (lane == 0) {
      if (o < ne) pre[evb[o]] = s / Z;
      else sp[o - ne] = s / Z;
    }
  }
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), foff the row's block of out: pre [n], then seed_pos [n + 1].  out_le [row]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_post(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                   const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                   double* tab, double* out_le, double* out) {
  __shared__ OprRow S;
  __shared__ int8_t evb[32];                   // event of bit i of an edge index
  const int tid = threadIdx.x;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const double* lt = S.lt;
  const int n = N - 1, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  double* den = tab + opr_uniform(r.toff);
  double* pre = out + opr_uniform(r.foff);
  double* sp = pre + n;
  for (int i = tid; i < n; i += KB) pre[i] = 0.0;
  for (int i = tid; i < N; i += KB) sp[i] = 0.0;

  if (r.mode != ORD_PAIRED) {
    const bool pt = r.mode == ORD_PT;
    double* F = den + V;
    const bool sd = r.seeded_top && k > 0;
    double fin;
    const double Z = opr_single_forward<KB>(S, N, den, F, sd ? k - 1 : k, fin);   // the seeding stays out of a chunk's pattern bits
    if (tid == 0) out_le[r.row] = log(Z);
    if (!sd) return;                            // "absent": no seeding to place (the host side reports NaN)
    // backward over the seeded half, in F's place: the forward values there are spent (Z is in registers)
    const int c = S.L.c;
    const uint32_t top = 1u << (k - 1);
    __syncthreads();                            // every thread has read F[full]
    if (tid == 0) F[full] = fin;
    __syncthreads();
    for (int lev = k - 1; lev >= 1; --lev) {
      opo_level<KB>(S.L, top >> c, V >> c, lev, [&](uint32_t x) {
        double s = 0.0;
        for (uint32_t m = full & ~x; m; m &= m - 1) {
          const int b = __builtin_ctz(m);
          const uint32_t y = x | (1u << b);
          s += F[y] * ord_num(lt, N, r, r.ev[b], y, pt) / den[y];
        }
        F[x] = s;
      });
      __syncthreads();
    }
    // edge masses into den's unseeded half (read for the last time by this very thread)
    for (uint32_t x = tid; x < top; x += KB) {
      const uint32_t y = x | top;
      den[x] = F[x] * ord_num(lt, N, r, r.ev[k - 1], y, pt) / den[y] * F[y];
    }
    for (int i = tid; i < k - 1; i += KB) evb[i] = r.ev[i];
    __syncthreads();
    opo_reduce<KB>(den, 1, k - 1, evb, Z, n, pre, sp);
    return;
  }

  const OprPaired T = opr_paired_tables(r, den);
  const double Z = opr_paired_passes<KB>(S, N, T);
  const int kj = T.kj;
  double *F = T.F, *B = T.B;
  // edge masses into the b_P entry of the unseeded states (zero in the forward pass and never read as anything else)
  for (uint32_t e = tid; e < (1u << kj); e += KB) {
    const uint32_t x = opr_joint_state(S, e), y = x | T.top;
    const double va = F[3ll * x] * ord_num(lt, N, r, r.ev[k - 1], y & T.in_mt, false) / den[y];
    F[3ll * e + 1] = B[3ll * x] * va;
  }
  for (int i = tid; i < kj; i += KB) evb[i] = r.ev[S.jslot[i]];
  __syncthreads();
  if (tid == 0) out_le[r.row] = log(Z);
  opo_reduce<KB>(F + 1, 3, kj, evb, Z, n, pre, sp);
}

}  // namespace mmhn
