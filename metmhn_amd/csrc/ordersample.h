// Posterior samples of the event orders of a cohort: the device form of metmhn_amd/model.py MetMHN.sample_order, on the row
// set-up, tables and passes of orderpass.h and the backward passes over every state and the edges of orderprec.h (both
// unchanged).
//
// The passes leave the backward weight of every sub-state the chain can be in.  A sample is a path of moves from the empty
// sub-state to the full one; the candidates of a move are visited in a fixed order and their weights w - the factor of the
// move times the backward weight of the state it leads to - summed in that order to `total`.  One uniform u in [0, 1) per
// move; the move taken is the first candidate whose cumulative weight exceeds u total (the last candidate with w > 0 if
// rounding lets the loop fall through: gillespie_step's rule); log_prob accumulates log(w / total).  An order is drawn with
// the probability likelihood(order) / Z.
//   one tumour              from x every slot b not in x, ascending: w = ord_num(ev[b], x | b) G[x | b]
//   paired, before seeding  from the joint events e: opr_joint_edge of every event not in e, ascending, then opr_seed_edge -
//                           the terms and the order of opr_unseeded_backward, so total = bu[e]
//   paired, after seeding   the path carries its own prefix vector f in F's place: at x, (fa, fp, fm) = ord_settle(x, f);
//                           every slot b < k - 1 not in x, ascending, y = x | b: g = (fa num / den[y], [pt_first, MT slot]
//                           fp num / dmt[y], [mt_first, PT slot] fm num / dpt[y]), w = B[y] . g - the three terms of
//                           opr_seeded_mass - and f = g / w after the choice, so that the next total is 1 up to rounding.
//                           The seeding is a choice like any other and leaves f = (1 / B[y]_a, 0, 0)
// Random numbers: Philox4x32-10 (sampler.h), key = the 64-bit seed, counter = (sample index low word, high word, move number,
// cohort row + 1); the uniform as in gillespie_step.  Counter word 3 = 0 is the Gillespie sampler's stream.  A sample depends
// on (seed, cohort row, sample index) only - not on n_samples, the batch or the launch.
//
// One workgroup per row.  After the passes thread t walks the samples first + t, first + t + KB, ...; a block of KB walks
// leaves its orders as slot numbers in LDS (OSM_STRIDE bytes per walk: a stride of 9 dwords, no two lanes of a store on one
// bank), then the whole workgroup writes the block's codes, padded with -1, as consecutive bytes of the row's output - no
// lane writes a byte per move to memory.  Static LDS: OprRow 11 KB + bu 8 KB + KB x 36 B (36 KB with 1024 threads).
// Workspace of a row: opost_doubles; output n_samples x (L + 8) bytes, L = 2 N - 1.  No atomics, fp64 only.
#pragma once
#include "orderprec.h"
#include "sampler.h"

namespace mmhn {

constexpr int OSM_STRIDE = 36;                  // bytes of a walk's slots in LDS (k <= MAXK = 30)
static_assert(MAXK <= OSM_STRIDE, "a walk's slots do not fit their LDS row");

// the uniform of move `move` of sample `id` of cohort row `crow`
__device__ __forceinline__ double osm_uniform(uint64_t seed, int crow, uint64_t id, int move) {
  uint32_t r[4];
  philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), (uint32_t)move, (uint32_t)(crow + 1), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  return (double)(((uint64_t)(r[0] >> 5) << 26) | (uint64_t)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
}

// The draw: weight(c) of the candidates c = 0 .. nc - 1 in visiting order (0: not a candidate).  Returns the candidate taken,
// its weight in w; lp accumulates log(w / total).
template <class Weight>
__device__ __forceinline__ int osm_draw(int nc, double u01, Weight weight, double& w, double& lp) {
#pragma clang fp contract(off)                  // the host's sums and products, one rounding each
  double total = 0.0;
  for (int c = 0; c < nc; ++c) total += weight(c);
  const double u = u01 * total;
  double cum = 0.0, wl = 0.0;
  int pick = -1, last = 0;
  for (int c = 0; c < nc; ++c) {
    const double v = weight(c);
    if (v > 0.0) { last = c; wl = v; }
    cum += v;
    if (cum > u) { pick = c; w = v; break; }
  }
  if (pick < 0) { pick = last; w = wl; }        // rounding at the upper end
  lp += log(w / total);
  return pick;
}

// one-tumour walk of sample id: slots into st[0 .. k - 1]; returns log_prob
__device__ __forceinline__ double osm_walk_single(const OprRow& S, int N, const double* G, uint64_t seed, uint64_t id,
                                                  uint8_t* st) {
  const ORow& r = S.r;
  const int k = r.k;
  const bool pt = r.mode == ORD_PT;
  uint32_t x = 0;
  double lp = 0.0, w = 0.0;
  for (int move = 0; move < k; ++move) {
    const int b = osm_draw(k, osm_uniform(seed, r.pad_, id, move), [&](int c) {
#pragma clang fp contract(off)
      const uint32_t y = x | (1u << c);
      return ((x >> c) & 1u) ? 0.0 : ord_num(S.lt, N, r, r.ev[c], y, pt) * G[y];
    }, w, lp);
    st[move] = (uint8_t)b;
    x |= 1u << b;
  }
  return lp;
}

// the vector g of the seeded move x -> y = x | b from the settled prefix vector (fa, fp, fm); returns w = B[y] . g
__device__ __forceinline__ double osm_seeded_weight(const OprRow& S, int N, const OprPaired& P, uint32_t x, int b, double fa,
                                                    double fp, double fm, double (&g)[3]) {
#pragma clang fp contract(off)
  const ORow& r = S.r;
  const uint32_t y = x | (1u << b);
  const bool pt_ev = r.kind[b] == ORD_K_PT;
  const double num = ord_num(S.lt, N, r, r.ev[b], y & (pt_ev ? r.pt_mask : P.in_mt), false);
  const double* by = P.B + 3ll * (y ^ P.top);
  g[0] = fa * num / P.den[y]; g[1] = 0.0; g[2] = 0.0;
  double w = by[0] * g[0];
  if (r.pt_first && !pt_ev) { g[1] = fp * num / P.dmt[y]; w += by[1] * g[1]; }
  if (r.mt_first && pt_ev) { g[2] = fm * num / P.dpt[y]; w += by[2] * g[2]; }
  return w;
}

// paired walk of sample id: slots into st[0 .. k - 1] (a joint move writes its PT slot, then its MT slot); returns log_prob
__device__ __forceinline__ double osm_walk_paired(const OprRow& S, int N, const OprPaired& P, const double* bu, uint64_t seed,
                                                  uint64_t id, uint8_t* st) {
  const ORow& r = S.r;
  const OrdTab t{P.o1, P.o2, P.dmt, P.dpt};
  const int k = r.k, kj = P.kj;
  const uint32_t full = (1u << k) - 1u;
  double lp = 0.0, w = 0.0;
  int move = 0, held = 0;
  // before the seeding: the joint events e
  uint32_t e = 0, x;
  for (;;) {
    x = opr_joint_state(S, e);
    const int q = osm_draw(kj + 1, osm_uniform(seed, r.pad_, id, move++), [&](int c) {
      if (c == kj) return opr_seed_edge(S, N, P, x);
      return ((e >> c) & 1u) ? 0.0 : opr_joint_edge(S, N, P, bu, e, c);
    }, w, lp);
    if (q == kj) break;
    const int b = S.jslot[q];
    st[held++] = (uint8_t)b;
    st[held++] = (uint8_t)(b + 1);
    e |= 1u << q;
  }
  st[held++] = (uint8_t)(k - 1);
  x |= P.top;
  double f0 = 1.0 / P.B[3ll * (x ^ P.top)], f1 = 0.0, f2 = 0.0;
  while (x != full) {
    double fa = f0, fp = f1, fm = f2, g[3];
    ord_settle(r, t, x, fa, fp, fm);
    const int b = osm_draw(k - 1, osm_uniform(seed, r.pad_, id, move++), [&](int c) {
      return ((x >> c) & 1u) ? 0.0 : osm_seeded_weight(S, N, P, x, c, fa, fp, fm, g);
    }, w, lp);
    osm_seeded_weight(S, N, P, x, b, fa, fp, fm, g);
    f0 = g[0] / w; f1 = g[1] / w; f2 = g[2] / w;
    st[held++] = (uint8_t)b;
    x |= 1u << b;
  }
  return lp;
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), foff the row's first sample in out_lp [.. n_samples] and out_orders
// [.. n_samples][L], pad_ the cohort row.  out_le [row].  Samples first ... first + n_samples - 1.
template <int KB>
__global__ __launch_bounds__(KB) void k_order_sample(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                     const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                     double* tab, double* out_le, long long first, long long n_samples,
                                                     uint64_t seed, double* out_lp, int8_t* out_orders, int L) {
  __shared__ OprRow S;
  __shared__ double bu[1 << OPO_CB];           // paired: B of the unseeded state of the joint events e
  __shared__ uint8_t stage[KB * OSM_STRIDE];   // the slots of the block's walks
  const int tid = threadIdx.x;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const int k = r.k;
  double* den = tab + opr_uniform(r.toff);
  const long long foff = opr_uniform(r.foff);
  const bool paired = r.mode == ORD_PAIRED;
  OprPaired T{};
  double Z;
  if (!paired) {
    Z = opr_single_passes<KB>(S, N, den, den + (1ll << k));
  } else {
    T = opr_paired_tables(r, den);
    Z = opr_paired_passes<KB>(S, N, T);
    opr_unseeded_backward<KB>(S, N, T, bu);
  }
  if (tid == 0) out_le[r.row] = log(Z);
  __syncthreads();
  for (long long base = 0; base < n_samples; base += KB) {
    const long long i = base + tid;
    if (i < n_samples) {
      const uint64_t id = (uint64_t)first + (uint64_t)i;
      uint8_t* st = stage + tid * OSM_STRIDE;
      out_lp[foff + i] = paired ? osm_walk_paired(S, N, T, bu, seed, id, st) : osm_walk_single(S, N, den, seed, id, st);
    }
    __syncthreads();
    const long long left = n_samples - base;
    const int cnt = left < KB ? (int)left : KB;
    int8_t* o = out_orders + (foff + base) * L;
    for (int j = tid; j < cnt * L; j += KB) {
      const int s = j / L, p = j - s * L;
      o[j] = p < k ? r.code[stage[s * OSM_STRIDE + p]] : (int8_t)-1;
    }
    __syncthreads();
  }
}

}  // namespace mmhn
