// What the three sum-product kernels over a row's lattice of sub-states share - k_order_post (orderpost.h), k_order_prec
// (orderprec.h), k_order_pos (orderpos.h): the level walk, the row in LDS, the tables and the passes of model.py's
// _single_tables / _paired_passes.  One workgroup per row, the lattice of 2^k sub-states in the batch workspace.
//
// Where k_orders keeps a Pareto front of candidates per sub-state, the sum keeps ONE prefix vector: the recurrences
// _advance / _settle / _total of model.py are linear in (a, b_P, b_M).
//   forward   F[y] = sum over the predecessors x of y of A(x, b) F[x]      (3 doubles per sub-state; 1 for one tumour)
//   backward  B[x] = S(x)^T sum over b not in x of D(x, b) B[x | b]        (seeded half only), B[full] = S(full)^T t
//             with A(x, b) = D(x, b) S(x), S = _settle, D the diagonal of the three rate factors, t = _total
//   evidence  Z = t(S(full) F[full])
// Tables (den, o1, o2, den_mt, den_pt) and numerators exactly as k_orders forms them (the same device functions).
// Every sum runs over its terms in ascending bit and every value is written once.
//   one tumour   opr_single_forward: den and F over the walked bits.  The backward pass is the caller's: k_order_post
//                runs it over the seeded half only, opr_single_passes (orderprec.h) over the whole lattice - two forms
//                that round differently, as model.py's _posterior_single and _single_passes do
//   both tumours opr_paired_passes: the tables, the joint-move and the seeded-half forward pass, Z, B over the seeded
//                half (model.py _paired_passes).  The unseeded backward pass (_unseeded_backward) is orderprec.h's
//
// Level walk.  A level (popcount) is enumerated in chunks of 2^c consecutive indices (c = 10 at most): one wave owns a
// chunk, its high bits h are wave-uniform (scalar registers), and the lanes take the low patterns of the popcount the
// level needs from a table sorted by popcount (LDS), so the lanes of a wave are dense on every level instead of one
// in C(6, j) / 64.  fp64 only.
#pragma once
#include "orders.h"

namespace mmhn {

constexpr int OPO_CB = 10;                      // index bits of a chunk of the level walk

// tables and passes of a row in doubles: paired den, o1, o2, den_mt, den_pt, F (3 per state), B (3 per seeded state);
// one tumour den, F
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

// chunk bits for a walk over kk index bits by a workgroup of kb threads: every wave of the workgroup gets a chunk where
// the row is large enough, chunks of at least one wave's width otherwise (host and device: the workspace sizes need it)
__host__ __device__ inline int opo_chunk_bits(int kk, int kb) {
  int lg = 0;
  while ((64 << lg) < kb) ++lg;
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

// LDS of a row
struct OprRow {
  double lt[ORD_MAXN * ORD_MAXN];
  double o1w[ORD_MAXN], o2w[ORD_MAXN];
  ORow r;
  OpoLevels L;
  int8_t jslot[32];                            // paired: slot of the i-th joint event
  int8_t jev[32];                              // paired: joint event of a slot, -1 none
  double zsh;
};

// a value every lane of the wave holds, moved to scalar registers (the offsets of a row come from LDS, in vector ones)
__device__ __forceinline__ long long opr_uniform(long long v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// the parameters and rows[blockIdx.x] into LDS (every thread of the workgroup; ends with a barrier)
template <int KB>
__device__ __forceinline__ void opr_load(OprRow& S, const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                         const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N) {
  const int tid = threadIdx.x;
  for (int i = tid; i < N * N; i += KB) S.lt[i] = g_lt[i];
  for (int i = tid; i < N; i += KB) { S.o1w[i] = g_o1[i]; S.o2w[i] = g_o2[i]; }
  if (tid == 0) S.r = rows[blockIdx.x];
  __syncthreads();
}

// One tumour (_single_tables, every slot alike): den and the forward pass into F, the level walk set up for kk index
// bits (k, or k - 1 where the caller keeps the seeding out of a chunk's pattern bits).  Returns Z, fin = the
// observation factor of the full state (the backward passes start from it); ends with a barrier.
template <int KB>
__device__ __forceinline__ double opr_single_forward(OprRow& S, int N, double* den, double* F, int kk, double& fin) {
  const ORow& r = S.r;
  const double* lt = S.lt;
  const int tid = threadIdx.x, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  const bool pt = r.mode == ORD_PT;
  const double* after = pt ? S.o1w : S.o2w;
  const bool sd = r.seeded_top && k > 0;
  const int c = opo_chunk_bits(kk, KB);
  opo_levels_init<KB>(S.L, c);
  for (uint32_t x = tid; x < V; x += KB) {
    const bool sx = r.seeded_top && ((x >> (k - 1)) & 1u);
    const double ob = exp(sx ? ord_obs_sum(after, r, x) : ord_obs_sum(S.o1w, r, x));
    den[x] = ob - ord_single_diag(lt, N, r, full, x, N, pt);
  }
  __syncthreads();
  if (tid == 0) F[0] = 1.0 / den[0];
  __syncthreads();
  for (int lev = 1; lev <= k; ++lev) {
    opo_level<KB>(S.L, 0u, V >> c, lev, [&](uint32_t x) {
      double s = 0.0;
      for (uint32_t m = x; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        s += F[x ^ (1u << b)] * ord_num(lt, N, r, r.ev[b], x, pt);
      }
      F[x] = s / den[x];
    });
    __syncthreads();
  }
  fin = exp(sd ? ord_obs_sum(after, r, full) : ord_obs_sum(S.o1w, r, full));
  return F[full] * fin;
}

// the tables of a paired row in its workspace (_paired_tables)
struct OprPaired {
  double *den, *o1, *o2, *dmt, *dpt, *F, *B;    // B[3 (x ^ top)] of the seeded x
  uint32_t top, in_mt;
  int kj;                                       // joint events
};

__device__ __forceinline__ OprPaired opr_paired_tables(const ORow& r, double* den) {
  const long long V = 1ll << r.k;
  OprPaired P;
  P.den = den; P.o1 = den + V; P.o2 = P.o1 + V; P.dmt = P.o2 + V; P.dpt = P.dmt + V; P.F = P.dpt + V; P.B = P.F + 3 * V;
  P.top = 1u << (r.k - 1);
  P.in_mt = r.mt_mask | P.top;
  P.kj = __builtin_popcount(r.joint);
  return P;
}

// state of the compact index e over the joint events: both slots of every event in e
__device__ __forceinline__ uint32_t opr_joint_state(const OprRow& S, uint32_t e) {
  uint32_t x = 0;
  for (uint32_t m = e; m; m &= m - 1) x |= 3u << S.jslot[__builtin_ctz(m)];
  return x;
}

// Both tumours (_paired_passes): the tables, the forward pass - the states whose tumours agree, then the seeded half -
// and the backward pass over the seeded half.  diagJ is in den already (k_diag, KD_DQ).  Returns Z; ends with a barrier.
template <int KB>
__device__ __forceinline__ double opr_paired_passes(OprRow& S, int N, const OprPaired& P) {
  const ORow& r = S.r;
  const double* lt = S.lt;
  const int tid = threadIdx.x, n = N - 1, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  double *den = P.den, *o1 = P.o1, *o2 = P.o2, *dmt = P.dmt, *dpt = P.dpt, *F = P.F, *B = P.B;
  const uint32_t top = P.top, in_mt = P.in_mt;
  const int c = opo_chunk_bits(k - 1, KB);
  opo_levels_init<KB>(S.L, c);
  if (tid == 0) {
    int kj = 0;
    for (int b = 0; b < 32; ++b) S.jev[b] = -1;
    for (uint32_t m = r.joint; m; m &= m - 1) {
      const int b = __builtin_ctz(m);
      S.jslot[kj] = (int8_t)b; S.jev[b] = S.jev[b + 1] = (int8_t)kj; ++kj;
    }
  }
  for (uint32_t x = tid; x < V; x += KB) {
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t m = x; m; m &= m - 1) {
      const int j = __builtin_ctz(m);
      if (r.kind[j] != ORD_K_MT) s1 += S.o1w[r.ev[j]];
      if (r.kind[j] != ORD_K_PT) s2 += S.o2w[r.ev[j]];
    }
    const double e1 = exp(s1), e2 = exp(s2);
    o1[x] = e1; o2[x] = e2;
    den[x] = (e1 + ((x & top) ? e2 : 0.0)) - den[x];
    if (r.pt_first) dmt[x] = e2 - ord_single_diag(lt, N, r, in_mt, x, N, false);
    if (r.mt_first) dpt[x] = e1 - ord_single_diag(lt, N, r, r.pt_mask, x, n, false);
  }
  const OrdTab t{o1, o2, dmt, dpt};
  const int kj = P.kj;
  const uint32_t EJ = 1u << kj;
  __syncthreads();
  if (tid == 0) { F[0] = 1.0 / den[0]; F[1] = 0.0; F[2] = 0.0; }
  __syncthreads();
  // before the seeding: the states whose tumours agree, joint moves only (at most 2^((k-1)/2) of them)
  for (int lev = 1; lev <= kj; ++lev) {
    for (uint32_t e = tid; e < EJ; e += KB) {
      if (__builtin_popcount(e) != lev) continue;
      const uint32_t y = opr_joint_state(S, e);
      double a = 0.0;
      for (uint32_t m = e; m; m &= m - 1) {
        const int b = S.jslot[__builtin_ctz(m)];
        a += F[3ll * (y ^ (3u << b))] * ord_num(lt, N, r, r.ev[b], y & r.pt_mask, false) / den[y];
      }
      F[3ll * y] = a; F[3ll * y + 1] = 0.0; F[3ll * y + 2] = 0.0;
    }
    __syncthreads();
  }
  // seeded half, level by level: every move
  for (int lev = 1; lev <= k; ++lev) {
    opo_level<KB>(S.L, top >> c, V >> c, lev, [&](uint32_t y) {
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
    S.zsh = bp * o2[full] + bm * o1[full];                                 // _total
    double ga = 0.0;
    settle_t(full, ga, o2[full], o1[full]);
    double* bf = B + 3ll * (full ^ top);
    bf[0] = ga; bf[1] = o2[full]; bf[2] = o1[full];
  }
  __syncthreads();
  for (int lev = k - 1; lev >= 1; --lev) {
    opo_level<KB>(S.L, top >> c, V >> c, lev, [&](uint32_t x) {
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
  return S.zsh;
}

}  // namespace mmhn
