// Pairwise event-precedence posteriors of a cohort: the device form of metmhn_amd/model.py MetMHN.order_precedence, on the
// tables, forward vectors F, backward vectors B and level walk of orderpass.h, which k_order_post (orderpost.h) calls too.
//
// Every admissible order of a row is a path of moves x -> y over the row's lattice of 2^k sub-states (slot b = bit b).
//   mass of a move   m(x, b) = B[y] . A(x, b) F[x]   (a scalar product of 3-vectors on the seeded half of a paired row, a
//                    product of scalars elsewhere): the summed likelihood of the orders that make this move
//   output           P[c][d] = (1 / Z) sum of m(x, b) over the moves that add slot d from a state x that holds slot c
//                    = P(c happened strictly earlier than d | the row); a joint move (before the seeding of a paired row)
//                    adds both of its slots, so neither of the two precedes the other
// One tumour: the whole lattice, B as G[x] = B[x] / den[x] in den's place once the forward pass is done.  Both tumours: B
// over the seeded half as opr_paired_passes forms it, then the scalar B of the unseeded states whose tumours agree (joint moves
// and the seeding edge; at most 2^((k-1)/2) states, LDS: the host side turns a row of more than 10 joint events away).
// The move masses are recomputed from F, B and the tables - a k x 2^(k-1) edge array would not fit.
//
// The reduction.  For a target slot d the moves that add d are indexed by the other slots: idx of m bits (m = k - 1 for
// one tumour, k - 2 on the seeded half, where the seeding is always held).  The k - 1 sums "over the x that hold c" are the
// sums over the idx with one bit set.  The vector of masses is folded along one index bit at a time: the upper half's sum
// is that bit's answer, lower + upper goes on to the next bit.  A wave folds a chunk of 2^c consecutive idx (c = the chunk
// bits of the level walk): bits 9..6 in registers (lane l holds idx l + 64 i), bits 5..0 with one xor-shuffle each - in
// step j a lane whose highest set bit is j keeps its value and from then on collects that bit's answer, every other lane
// adds its partner - and writes the chunk's c bit sums and its total.  The totals of the chunks are a vector over the
// high bits and are folded the same way (a second level; a third from m = 21 on), the bit sums of the chunks are added by
// one wave per sum, lanes striding the chunks.  Every value is written once, every sum has a fixed shape, no atomics: a
// row's result does not depend on the batch, the launch geometry (a function of k alone) or the run.
//
// Workspace of a row in doubles: opost_doubles (paired 8 x 2^k + 3 x 2^(k-1), one tumour 2 x 2^k) + the chunk partials
// k x sum over the levels of (c_l + 1) 2^(m_l - c_l), m_0 = m, c_0 = c, m_(l+1) = m_l - c_l, c_l = min(m_l, 10) - that is
// k (c + 1) 2^(m - c) + k (m - c + 1) up to m = 20, under 3 % of the lattice.  Output: the compact k x k matrix in slot
// order (row c, column d, diagonal 0); the host side scatters it to the event codes.  fp64 only.
#pragma once
#include "orderpass.h"

namespace mmhn {

// index bits of the vector of moves that add one slot
inline int oprec_bits(const ORow& r) {
  const int m = r.mode == ORD_PAIRED ? r.k - 2 : r.k - 1;
  return m > 0 ? m : 0;
}

// chunk partials of nt vectors of 2^m values whose first level has chunks of c bits, in doubles
__host__ __device__ inline long long oprec_part_doubles(int nt, int m, int c) {
  long long s = 0;
  for (;;) {
    s += (long long)nt * (c + 1) << (m - c);
    if (m == c) return s;
    m -= c;
    c = m < OPO_CB ? m : OPO_CB;
  }
}

// workspace of a row in doubles (kb: threads of the row's launch)
inline long long oprec_doubles(const ORow& r, int kb) {
  const int m = oprec_bits(r);
  return opost_doubles(r) + oprec_part_doubles(r.k, m, opo_chunk_bits(m, kb));
}

// idx with a zero inserted at bit d
__device__ __forceinline__ uint32_t opr_ins0(uint32_t idx, int d) { return ((idx >> d) << (d + 1)) | (idx & ((1u << d) - 1u)); }

// The fold of one chunk by one wave.  In: v[i] = the value of chunk index lane + 64 i (0 past the chunk).  Out: t = the
// chunk's total on lane 0 and the sum over the indices with bit j set on lane 2^j (j < 6); hi[j] = the sum over the
// indices with bit 6 + j set, on every lane.
__device__ __forceinline__ void opr_fold(double (&v)[1 << (OPO_CB - 6)], double& t, double (&hi)[OPO_CB - 6]) {
#pragma unroll
  for (int j = OPO_CB - 7; j >= 0; --j) {
    const int h = 1 << j;
    double u = v[h];
#pragma unroll
    for (int i = 1; i < h; ++i) u += v[h + i];
#pragma unroll
    for (int i = 0; i < h; ++i) v[i] += v[h + i];
    hi[j] = opo_wave_sum(u);
  }
  t = v[0];
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int j = 5; j >= 0; --j) {
    const double u = __shfl_xor(t, 1 << j, 64);
    if ((lane >> j) != 1u) t += u;              // the lanes [2^j, 2^(j+1)) hold the upper half: bit j's answer from here on
  }
}

// Bit sums of nt vectors of 2^m values val(t, idx): out(t, j, s) with s = the sum over the idx with bit j set (j < m)
// and out(t, m, s) with the total.  c0: chunk bits of the first level; part: oprec_part_doubles(nt, m, c0) doubles.
// Every thread of the workgroup; starts from values the caller has fenced with a barrier, ends with a barrier.
template <int KB, class Val, class Out>
__device__ __forceinline__ void opr_bit_sums(int nt, int m, int c0, double* part, Val val, Out out) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  int ml = m, cl = c0, lo = 0, pc = 0;
  long long pnh = 0;
  double* pl = part;
  const double* prev = nullptr;                 // the level below: its chunks' totals are this level's values
  for (;;) {
    const long long nh = 1ll << (ml - cl);
    for (long long task = wave; task < nt * nh; task += KB / 64) {
      const int t = (int)(task / nh);
      const long long h = task - t * nh;
      double v[1 << (OPO_CB - 6)], tot, hi[OPO_CB - 6];
#pragma unroll
      for (int i = 0; i < (1 << (OPO_CB - 6)); ++i) {
        const uint32_t p = lane + 64u * i;
        v[i] = 0.0;
        if (p < (1u << cl)) {
          const long long idx = (h << cl) | p;
          v[i] = prev ? prev[(t * pnh + idx) * (pc + 1) + pc] : val(t, (uint32_t)idx);
        }
      }
      opr_fold(v, tot, hi);
      double* o = pl + (t * nh + h) * (cl + 1);
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (lane == (1u << j) && j < cl) o[j] = tot;
      if (lane == 0) {
        for (int j = 6; j < cl; ++j) o[j] = hi[j - 6];
        o[cl] = tot;
      }
    }
    __syncthreads();
    // this level's bit sums over its chunks: one wave per sum, lanes stride the chunks
    for (int task = wave; task < nt * cl; task += KB / 64) {
      const int t = task / cl, j = task - t * cl;
      double s = 0.0;
      for (long long h = lane; h < nh; h += 64) s += pl[(t * nh + h) * (cl + 1) + j];
      s = opo_wave_sum(s);
      if (lane == 0) out(t, lo + j, s);
    }
    if (nh == 1) {
      for (int t = threadIdx.x; t < nt; t += KB) out(t, m, pl[t * (cl + 1) + cl]);
      break;
    }
    prev = pl; pc = cl; pnh = nh;
    pl += nt * nh * (cl + 1);
    lo += cl; ml -= cl;
    cl = ml < OPO_CB ? ml : OPO_CB;
  }
  __syncthreads();
}

// ---- what k_order_prec and k_order_pos (orderpos.h) share on top of orderpass.h: the backward pass over every state the
// chain can be in, the masses of the moves

// One tumour (_single_passes): opr_single_forward over every bit and - unless the row is empty - the backward pass over the
// whole lattice, G[x] = B[x] / den[x] in den's place.  Returns Z; ends with a barrier.
template <int KB>
__device__ __forceinline__ double opr_single_passes(OprRow& S, int N, double* den, double* F) {
  const ORow& r = S.r;
  const double* lt = S.lt;
  const int tid = threadIdx.x, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  const bool pt = r.mode == ORD_PT;
  double fin;
  const double Z = opr_single_forward<KB>(S, N, den, F, k, fin);
  const int c = S.L.c;
  if (k == 0) return Z;
  // (den[x] is read for the last time by the thread that writes G[x])
  double* G = den;
  if (tid == 0) G[full] = fin / den[full];
  __syncthreads();
  for (int lev = k - 1; lev >= 0; --lev) {
    opo_level<KB>(S.L, 0u, V >> c, lev, [&](uint32_t x) {
      double s = 0.0;
      for (uint32_t m = full & ~x; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        const uint32_t y = x | (1u << b);
        s += G[y] * ord_num(lt, N, r, r.ev[b], y, pt);
      }
      G[x] = s / den[x];
    });
    __syncthreads();
  }
  return Z;
}

// mass of the one-tumour move that adds slot d from the state of the other slots idx
__device__ __forceinline__ double opr_single_mass(const OprRow& S, int N, const double* G, const double* F, int d, uint32_t idx) {
  const uint32_t x = opr_ins0(idx, d), y = x | (1u << d);
  return F[x] * ord_num(S.lt, N, S.r, S.r.ev[d], y, S.r.mode == ORD_PT) * G[y];
}

// the seeding edge of the unseeded state x: the factor that takes F[x]_a to its mass
__device__ __forceinline__ double opr_seed_edge(const OprRow& S, int N, const OprPaired& P, uint32_t x) {
  const uint32_t y = x | P.top;
  return ord_num(S.lt, N, S.r, S.r.ev[S.r.k - 1], y & P.in_mt, false) / P.den[y] * P.B[3ll * x];
}

// the same for the joint move of event q from the unseeded state of the joint events e
__device__ __forceinline__ double opr_joint_edge(const OprRow& S, int N, const OprPaired& P, const double* bu, uint32_t e, int q) {
  const uint32_t y = opr_joint_state(S, e | (1u << q));
  return ord_num(S.lt, N, S.r, S.r.ev[S.jslot[q]], y & S.r.pt_mask, false) / P.den[y] * bu[e | (1u << q)];
}

// mass of the move that adds slot d < k - 1 from the seeded state of the other slots idx (k - 2 bits)
__device__ __forceinline__ double opr_seeded_mass(const OprRow& S, int N, const OprPaired& P, int d, uint32_t idx) {
  const ORow& r = S.r;
  const OrdTab t{P.o1, P.o2, P.dmt, P.dpt};
  const uint32_t x = opr_ins0(idx, d) | P.top, y = x | (1u << d);
  const bool pt_ev = r.kind[d] == ORD_K_PT;
  const double num = ord_num(S.lt, N, r, r.ev[d], y & (pt_ev ? r.pt_mask : P.in_mt), false);
  double fa = P.F[3ll * x], fp = P.F[3ll * x + 1], fm = P.F[3ll * x + 2];
  ord_settle(r, t, x, fa, fp, fm);                                     // _advance
  const double* by = P.B + 3ll * (y ^ P.top);
  double w = by[0] * (fa * num / P.den[y]);
  if (r.pt_first && !pt_ev) w += by[1] * (fp * num / P.dmt[y]);
  if (r.mt_first && pt_ev) w += by[2] * (fm * num / P.dpt[y]);
  return w;
}

// Both tumours, after opr_paired_passes (_unseeded_backward): the scalar B of the unseeded states whose tumours agree, into
// bu[e] of the state of the joint events e (1 << OPO_CB doubles of LDS) - joint moves in ascending event, then the seeding
// edge.  Ends with a barrier.
template <int KB>
__device__ __forceinline__ void opr_unseeded_backward(const OprRow& S, int N, const OprPaired& P, double* bu) {
  const int tid = threadIdx.x, kj = P.kj;
  const uint32_t EJ = 1u << kj;
  for (int lev = kj; lev >= 0; --lev) {
    for (uint32_t e = tid; e < EJ; e += KB) {
      if (__builtin_popcount(e) != lev) continue;
      double s = 0.0;
      for (uint32_t m = (EJ - 1u) & ~e; m; m &= m - 1) s += opr_joint_edge(S, N, P, bu, e, __builtin_ctz(m));
      bu[e] = s + opr_seed_edge(S, N, P, opr_joint_state(S, e));
    }
    __syncthreads();
  }
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), coff chunk partials, foff the row's k x k block of out_prec.  out_le [row]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_prec(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                   const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                   double* tab, double* out_le, double* out_prec) {
  __shared__ OprRow S;
  __shared__ double bu[1 << OPO_CB];           // paired: B of the unseeded state of the joint events e
  __shared__ double Rs[32][32];                // Rs[d][c]: summed masses of the moves that add d from a state holding c
  __shared__ double Rj[OPO_CB + 1][OPO_CB + 1]; // paired, before the seeding: Rj[t][q] target joint event t (kj: the
                                               // seeding), held joint event q
  __shared__ double pj[(OPO_CB + 1) * (OPO_CB + 1)];   // chunk partials of the sums before the seeding (one chunk each)
  const int tid = threadIdx.x;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const int k = r.k;
  double* den = tab + opr_uniform(r.toff);
  double* part = tab + opr_uniform(r.coff);
  double* P = out_prec + opr_uniform(r.foff);

  if (r.mode != ORD_PAIRED) {
    double* F = den + (1ll << k);
    const double Z = opr_single_passes<KB>(S, N, den, F);
    if (tid == 0) out_le[r.row] = log(Z);
    if (k == 0) return;
    const int m = k - 1;
    opr_bit_sums<KB>(k, m, opo_chunk_bits(m, KB), part,
        [&](int d, uint32_t idx) { return opr_single_mass(S, N, den, F, d, idx); },
        [&](int d, int j, double s) { if (j < m) Rs[d][j < d ? j : j + 1] = s; });
    for (int i = tid; i < k * k; i += KB) {
      const int cc = i / k, d = i - cc * k;
      P[i] = cc == d ? 0.0 : fmin(Rs[d][cc] / Z, 1.0);     // a probability: the quotient of two roundings may pass 1
    }
    return;
  }

  const OprPaired T = opr_paired_tables(r, den);
  const double Z = opr_paired_passes<KB>(S, N, T);
  opr_unseeded_backward<KB>(S, N, T, bu);
  const int kj = T.kj;
  if (tid == 0) out_le[r.row] = log(Z);
  // after the seeding: target slot d < k - 1, the moves from the seeded x without d
  const int m = k >= 2 ? k - 2 : 0;
  opr_bit_sums<KB>(k - 1, m, opo_chunk_bits(m, KB), part,
      [&](int d, uint32_t idx) { return opr_seeded_mass(S, N, T, d, idx); },
      [&](int d, int j, double s) { Rs[d][j < m ? (j < d ? j : j + 1) : k - 1] = s; });   // every seeded x holds the seeding
  // before the seeding: the joint move of event q from the states without it, then the seeding from every such state
  opr_bit_sums<KB>(kj, kj > 0 ? kj - 1 : 0, kj > 0 ? kj - 1 : 0, pj,
      [&](int q, uint32_t idx) {
        const uint32_t e = opr_ins0(idx, q);
        return T.F[3ll * opr_joint_state(S, e)] * opr_joint_edge(S, N, T, bu, e, q);
      },
      [&](int q, int j, double s) { if (j < kj - 1) Rj[q][j < q ? j : j + 1] = s; });
  opr_bit_sums<KB>(1, kj, kj, pj,
      [&](int, uint32_t e) {
        const uint32_t x = opr_joint_state(S, e);
        return T.F[3ll * x] * opr_seed_edge(S, N, T, x);
      },
      [&](int, int j, double s) { if (j < kj) Rj[kj][j] = s; });
  for (int i = tid; i < k * k; i += KB) {
    const int cc = i / k, d = i - cc * k;
    double s = 0.0;
    if (cc != d) {
      if (d < k - 1) s = Rs[d][cc];
      const int q = S.jev[cc], td = d == k - 1 ? kj : S.jev[d];
      if (q >= 0 && td >= 0 && td != q) s += Rj[td][q];
    }
    P[i] = fmin(s / Z, 1.0);
  }
}

}  // namespace mmhn
