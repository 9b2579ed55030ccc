// Pre-seeding posteriors of a cohort: the sum-product twin of orders.h (k_orders), the device form of
// metmhn_amd/model.py MetMHN.order_posterior.
//
// One workgroup per row; the row's lattice of 2^k sub-states lives in the batch workspace.  Where k_orders keeps a
// Pareto front of candidates per sub-state, the sum keeps ONE prefix vector: the recurrences _advance / _settle /
// _total of model.py are linear in (a, b_P, b_M).
//   forward   F[y] = sum over the predecessors x of y of A(x, b) F[x]      (3 doubles per sub-state; 1 for one tumour)
//   backward  B[x] = S(x)^T sum over b not in x of D(x, b) B[x | b]        (seeded half only), B[full] = S(full)^T t
//             with A(x, b) = D(x, b) S(x), S = _settle, D the diagonal of the three rate factors, t = _total
//   edges     w(x) = B[x | top]_a * F[x]_a * num_top / den[x | top]       the mass of the orders that seed at x
//   outputs   log Z = log t(S(full) F[full]); pre[m] = sum of w over the x that hold m, seed_pos[j] = sum of w over the
//             x with j events, both over Z
// Tables (den, o1, o2, den_mt, den_pt) and numerators exactly as k_orders forms them (the same device functions).
// Every sum runs over its terms in ascending bit, every value is written once and the reductions have a fixed shape:
// no atomics, the result of a row does not depend on the batch, the launch geometry or the run.
//
// Level walk.  A level (popcount) is enumerated in chunks of 2^c consecutive indices (c = 10 at most): one wave owns a
// chunk, its high bits h are wave-uniform (scalar registers), and the lanes take the low patterns of the popcount the
// level needs from a table sorted by popcount (LDS), so the lanes of a wave are dense on every level instead of one
// in C(6, j) / 64.  fp64 only.
#pragma once
#include "orders.h"

namespace mmhn {

constexpr int OPO_CB = 10;                      // index bits of a chunk of the level walk

// workspace of a row in doubles: paired den, o1, o2, den_mt, den_pt, F (3 per state), B (3 per seeded state);
// one tumour den (the edge masses once the forward pass is done), F (the seeded half becomes B)
inline long long opost_doubles(const ORow& r) {
  const long long V = 1ll << r.k;
  return r.mode == ORD_PAIRED ? 8 * V + 3 * (V / 2) : 2 * V;
}

struct OpoLevels {
  uint16_t pat[1 << OPO_CB];                    // the c-bit patterns sorted by (popcount, value)
  int off[OPO_CB + 2];                          // first pattern of every popcount
  int c;
};

// the table of the level walk for chunks of c bits (every thread of the workgroup; ends with a barrier)
template <int KB>
__device__ __forceinline__ void opo_levels_init(OpoLevels& L, int c) {
  // binomials C(i, t), i <= OPO_CB: rank of a pattern among those of its popcount (combinatorial number system)
  auto binom = [](int i, int t) {
    int v = 1;
    if (t < 0 || t > i) return 0;
    for (int s = 1; s <= t; ++s) v = v * (i - t + s) / s;
    return v;
  };
  if (threadIdx.x == 0) {
    L.c = c;
    int o = 0;
    for (int j = 0; j <= c; ++j) { L.off[j] = o; o += binom(c, j); }
    L.off[c + 1] = o;
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < (1u << c); p += KB) {
    int rank = 0, t = 0;
    for (uint32_t m = p; m; m &= m - 1) rank += binom(__builtin_ctz(m), ++t);
    L.pat[L.off[__builtin_popcount(p)] + rank] = (uint16_t)p;
  }
  __syncthreads();
}

// chunk bits for a walk over kk index bits: every wave of the workgroup gets a chunk where the row is large enough,
// chunks of at least one wave's width otherwise
template <int KB>
__device__ __forceinline__ int opo_chunk_bits(int kk) {
  int lg = 0;
  while ((64 << lg) < KB) ++lg;
  int c = kk - lg;
  c = c < 6 ? 6 : c;
  c = c > OPO_CB ? OPO_CB : c;
  return c < kk ? c : (kk > 0 ? kk : 0);
}

// fn(x) for every index x in [hlo << c, hhi << c) of popcount lev
template <int KB, class Fn>
__device__ __forceinline__ void opo_level(const OpoLevels& L, uint32_t hlo, uint32_t hhi, int lev, Fn fn) {
  const int c = L.c;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  for (uint32_t h = hlo + wave; h < hhi; h += KB / 64) {
    const int j = lev - __builtin_popcount(h);
    if (j < 0 || j > c) continue;
    for (int i = L.off[j] + (int)lane; i < L.off[j + 1]; i += 64) fn((h << c) | L.pat[i]);
  }
}

// sum of v over the 64 lanes, the same tree on every run
__device__ __forceinline__ double opo_wave_sum(double v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

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
// out_le [row], out_pre [row][n], out_sp [row][n + 1]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_post(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                   const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                   double* tab, double* out_le, double* out_pre, double* out_sp) {
  __shared__ double lt[ORD_MAXN * ORD_MAXN];
  __shared__ double o1w[ORD_MAXN], o2w[ORD_MAXN];
  __shared__ ORow r;
  __shared__ OpoLevels L;
  __shared__ int8_t evb[32];                   // event of bit i of an edge index
  __shared__ int8_t jslot[32];                 // paired: slot of the i-th joint event
  __shared__ double zsh;
  const int tid = threadIdx.x;
  for (int i = tid; i < N * N; i += KB) lt[i] = g_lt[i];
  for (int i = tid; i < N; i += KB) { o1w[i] = g_o1[i]; o2w[i] = g_o2[i]; }
  if (tid == 0) r = rows[blockIdx.x];
  __syncthreads();
  const int n = N - 1, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  double* den = tab + r.toff;
  double* pre = out_pre + (long long)r.row * n;
  double* sp = out_sp + (long long)r.row * N;
  for (int i = tid; i < n; i += KB) pre[i] = 0.0;
  for (int i = tid; i < N; i += KB) sp[i] = 0.0;

  if (r.mode != ORD_PAIRED) {
    // ---------------------------------------------------------------- one tumour: _single_tables, sums for the maxima
    const bool pt = r.mode == ORD_PT;
    const double* after = pt ? o1w : o2w;
    double* F = den + V;
    const bool sd = r.seeded_top && k > 0;
    const int c = opo_chunk_bits<KB>(sd ? k - 1 : k);    // the seeding stays out of a chunk's pattern bits
    opo_levels_init<KB>(L, c);
    for (uint32_t x = tid; x < V; x += KB) {
      const bool sd = r.seeded_top && ((x >> (k - 1)) & 1u);
      const double ob = exp(sd ? ord_obs_sum(after, r, x) : ord_obs_sum(o1w, r, x));
      den[x] = ob - ord_single_diag(lt, N, r, full, x, N, pt);
    }
    __syncthreads();
    if (tid == 0) F[0] = 1.0 / den[0];
    __syncthreads();
    for (int lev = 1; lev <= k; ++lev) {
      opo_level<KB>(L, 0u, V >> c, lev, [&](uint32_t x) {
        double s = 0.0;
        for (uint32_t m = x; m; m &= m - 1) {
          const int b = __builtin_ctz(m);
          s += F[x ^ (1u << b)] * ord_num(lt, N, r, r.ev[b], x, pt);
        }
        F[x] = s / den[x];
      });
      __syncthreads();
    }
    const double fin = exp(sd ? ord_obs_sum(after, r, full) : ord_obs_sum(o1w, r, full));
    const double Z = F[full] * fin;
    if (tid == 0) out_le[r.row] = log(Z);
    if (!sd) return;                            // "absent": no seeding to place (the host side reports NaN)
    // backward over the seeded half, in F's place: the forward values there are spent (Z is in registers)
    const uint32_t top = 1u << (k - 1);
    __syncthreads();                            // every thread has read F[full]
    if (tid == 0) F[full] = fin;
    __syncthreads();
    for (int lev = k - 1; lev >= 1; --lev) {
      opo_level<KB>(L, top >> c, V >> c, lev, [&](uint32_t x) {
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

  // ---------------------------------------------------------------- both tumours: _paired_tables (as k_orders)
  double* o1 = den + V;
  double* o2 = o1 + V;
  double* dmt = o2 + V;
  double* dpt = dmt + V;
  double* F = dpt + V;
  double* B = F + 3ll * V;                      // B[3 (x ^ top)] of the seeded x
  const uint32_t top = 1u << (k - 1);
  const uint32_t in_mt = r.mt_mask | top;
  const int c = opo_chunk_bits<KB>(k - 1);
  opo_levels_init<KB>(L, c);
  if (tid == 0) {
    int kj = 0;
    for (uint32_t m = r.joint; m; m &= m - 1) { jslot[kj] = (int8_t)__builtin_ctz(m); evb[kj] = r.ev[__builtin_ctz(m)]; ++kj; }
  }
  for (uint32_t x = tid; x < V; x += KB) {
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t m = x; m; m &= m - 1) {
      const int j = __builtin_ctz(m);
      if (r.kind[j] != ORD_K_MT) s1 += o1w[r.ev[j]];
      if (r.kind[j] != ORD_K_PT) s2 += o2w[r.ev[j]];
    }
    const double e1 = exp(s1), e2 = exp(s2);
    o1[x] = e1; o2[x] = e2;
    den[x] = (e1 + ((x & top) ? e2 : 0.0)) - den[x];
    if (r.pt_first) dmt[x] = e2 - ord_single_diag(lt, N, r, in_mt, x, N, false);
    if (r.mt_first) dpt[x] = e1 - ord_single_diag(lt, N, r, r.pt_mask, x, n, false);
  }
  const OrdTab t{o1, o2, dmt, dpt};
  const int kj = __builtin_popcount(r.joint);
  const uint32_t EJ = 1u << kj;
  // state of the compact index e over the joint events: both slots of every event in e
  auto joint_state = [&](uint32_t e) {
    uint32_t x = 0;
    for (uint32_t m = e; m; m &= m - 1) x |= 3u << jslot[__builtin_ctz(m)];
    return x;
  };
  __syncthreads();
  if (tid == 0) { F[0] = 1.0 / den[0]; F[1] = 0.0; F[2] = 0.0; }
  __syncthreads();
  // before the seeding: the states whose tumours agree, joint moves only (at most 2^((k-1)/2) of them)
  for (int lev = 1; lev <= kj; ++lev) {
    for (uint32_t e = tid; e < EJ; e += KB) {
      if (__builtin_popcount(e) != lev) continue;
      const uint32_t y = joint_state(e);
      double a = 0.0;
      for (uint32_t m = e; m; m &= m - 1) {
        const int b = jslot[__builtin_ctz(m)];
        a += F[3ll * (y ^ (3u << b))] * ord_num(lt, N, r, r.ev[b], y & r.pt_mask, false) / den[y];
      }
      F[3ll * y] = a; F[3ll * y + 1] = 0.0; F[3ll * y + 2] = 0.0;
    }
    __syncthreads();
  }
  // seeded half, level by level: every move
  for (int lev = 1; lev <= k; ++lev) {
    opo_level<KB>(L, top >> c, V >> c, lev, [&](uint32_t y) {
      double a = 0.0, bp = 0.0, bm = 0.0;
      for (uint32_t m = y; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        const uint32_t x = y ^ (1u << b);
        if (b == k - 1) {                       // the seeding itself, from a state whose tumours agree
          const uint32_t lo = x & r.joint;
          if (x != (lo | lo << 1)) continue;
          a += F[3ll * x] * ord_num(lt, N, r, r.ev[b], y & in_mt, false) / den[y];
          continue;
        }
        const bool pt_ev = r.kind[b] == ORD_K_PT;
        const double num = ord_num(lt, N, r, r.ev[b], y & (pt_ev ? r.pt_mask : in_mt), false);
        double fa = F[3ll * x], fp = F[3ll * x + 1], fm = F[3ll * x + 2];
        ord_settle(r, t, x, fa, fp, fm);                                   // _advance
        if (r.pt_first && !pt_ev) bp += fp * num / dmt[y];
        if (r.mt_first && pt_ev) bm += fm * num / dpt[y];
        a += fa * num / den[y];
      }
      F[3ll * y] = a; F[3ll * y + 1] = bp; F[3ll * y + 2] = bm;
    });
    __syncthreads();
  }
  // _settle's two coefficients at a seeded x (transposed: they carry the b's weights back to a)
  auto settle_t = [&](uint32_t x, double& ga, double gp, double gm) {
    if (r.pt_first && (x & r.pt_mask) == r.pt_mask) ga = ga + gp * (o1[x] / dmt[x]);
    if (r.mt_first && (x & r.mt_mask) == r.mt_mask) ga = ga + gm * (o2[x] / dpt[x]);
  };
  if (tid == 0) {
    double a = F[3ll * full], bp = F[3ll * full + 1], bm = F[3ll * full + 2];
    ord_settle(r, t, full, a, bp, bm);
    zsh = bp * o2[full] + bm * o1[full];                                   // _total
    double ga = 0.0;
    settle_t(full, ga, o2[full], o1[full]);
    double* bf = B + 3ll * (full ^ top);
    bf[0] = ga; bf[1] = o2[full]; bf[2] = o1[full];
  }
  __syncthreads();
  const double Z = zsh;
  for (int lev = k - 1; lev >= 1; --lev) {
    opo_level<KB>(L, top >> c, V >> c, lev, [&](uint32_t x) {
      double ga = 0.0, gp = 0.0, gm = 0.0;
      for (uint32_t m = full & ~x; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        const uint32_t y = x | (1u << b);
        const bool pt_ev = r.kind[b] == ORD_K_PT;
        const double num = ord_num(lt, N, r, r.ev[b], y & (pt_ev ? r.pt_mask : in_mt), false);
        const double* by = B + 3ll * (y ^ top);
        ga += by[0] * num / den[y];
        if (r.pt_first && !pt_ev) gp += by[1] * num / dmt[y];
        if (r.mt_first && pt_ev) gm += by[2] * num / dpt[y];
      }
      settle_t(x, ga, gp, gm);
      double* bx = B + 3ll * (x ^ top);
      bx[0] = ga; bx[1] = gp; bx[2] = gm;
    });
    __syncthreads();
  }
  // edge masses into the b_P entry of the unseeded states (zero in the forward pass and never read as anything else)
  for (uint32_t e = tid; e < EJ; e += KB) {
    const uint32_t x = joint_state(e), y = x | top;
    const double va = F[3ll * x] * ord_num(lt, N, r, r.ev[k - 1], y & in_mt, false) / den[y];
    F[3ll * e + 1] = B[3ll * x] * va;
  }
  __syncthreads();
  if (tid == 0) out_le[r.row] = log(Z);
  opo_reduce<KB>(F + 1, 3, kj, evb, Z, n, pre, sp);
}

}  // namespace mmhn
