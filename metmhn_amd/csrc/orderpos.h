// Posterior event positions of a cohort: the device form of metmhn_amd/model.py MetMHN.order_position, on the row set-up,
// tables and passes of orderpass.h (every order kernel's) and the backward passes over every state and the move masses
// m(x, b) of orderprec.h (k_order_prec's and this kernel's).
//
// An order has two lineages: the metastasis' (the joint events before the seeding, the seeding, the metastasis' own events)
// and the primary tumour's (the joint events, the seeding, the primary tumour's own events).
//   output   pos[d][j] = (1 / Z) sum of m(x, d) over the moves that add slot d from a state x with
//            popcount(x & mask_d) = j: P(slot d's event is the j-th entry of its lineage | the row); mask_d = the slots of
//            d's lineage (PT slot: pt_mask | top, MT slot: mt_mask | top; one tumour: every slot)
// Before the seeding of a paired row both tumours agree: a joint move or the seeding edge from the unseeded state of the
// joint events e has the position popcount(e) in both lineages (at most 2^10 states; summed in LDS, one wave per output).
//
// The reduction.  For a target slot d the moves that add d are indexed by the other slots (idx of m bits, as in
// orderprec.h); mask_d without bit d, packed to the index bits, is mk.  A wave owns a chunk of 2^c consecutive idx
// (c = opo_chunk_bits): the class popcount(idx & mk) splits into popcount(h & mk_hi) of the chunk's number h
// (wave-uniform) and popcount(p & mk_lo) of the index p = lane + 64 i in the chunk, which splits again into the lane's part
// and popcount(i & (mk_lo >> 6)) (wave-uniform per i).  A lane adds its masses into five sums by that last part - no array
// of masses in registers -, then the wave does one opo_wave_sum tree per class of the chunk and writes c + 1 partials.
// One wave per (d, class) then adds the chunks' partials, lanes striding the chunks.  Every value is written once, every
// sum has a shape fixed by k, the thread count and the row's masks, no atomics: a row's result does not depend on the batch
// or the run.
//
// Workspace of a row: opost_doubles + nt (c + 1) 2^(m - c) doubles of partials (nt = k one tumour, k - 1 paired) - the first
// level of oprec_part_doubles, so never more than oprec_doubles.  Output: the compact k x k matrix (row slot d, column
// position j); the host side scatters it to the events of the two lineages.  fp64 only.
#pragma once
#include "orderprec.h"

namespace mmhn {

// bits of a slot mask as index bits of the moves that add slot d (bit d removed), the m low ones
__device__ __forceinline__ uint32_t opp_index_mask(uint32_t mask, int d, int m) {
  const uint32_t mk = ((mask >> (d + 1)) << d) | (mask & ((1u << d) - 1u));
  return mk & ((1u << m) - 1u);
}

// Class sums of nt vectors of 2^m values val(t, idx): out(t, q, s) with s = the sum over the idx with
// popcount(idx & msk(t)) = q, for every q in 0 .. m.  c: chunk bits; part: nt (c + 1) 2^(m - c) doubles.
// Every thread of the workgroup; starts from values the caller has fenced with a barrier, ends with a barrier.
template <int KB, class Val, class Msk, class Out>
__device__ __forceinline__ void opp_class_sums(int nt, int m, int c, double* part, Val val, Msk msk, Out out) {
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const long long nh = 1ll << (m - c);
  const uint32_t cm = (1u << c) - 1u;
  const int per_lane = c > 6 ? 1 << (c - 6) : 1;
  for (long long task = wave; task < nt * nh; task += KB / 64) {
    const int t = (int)(task / nh);
    const long long h = task - t * nh;
    const uint32_t lo = __builtin_amdgcn_readfirstlane(msk(t)) & cm;
    const int mine = __builtin_popcount(lane & lo), most = __builtin_popcount(lo);
    double acc[OPO_CB - 5];
#pragma unroll
    for (int q = 0; q < OPO_CB - 5; ++q) acc[q] = 0.0;
    for (int i = 0; i < per_lane; ++i) {
      const uint32_t p = lane + 64u * i;
      const double v = p <= cm ? val(t, (uint32_t)((h << c) | p)) : 0.0;
      const int ci = __builtin_popcount((uint32_t)i & (lo >> 6));           // wave-uniform
#pragma unroll
      for (int q = 0; q < OPO_CB - 5; ++q) acc[q] += ci == q ? v : 0.0;
    }
    double* o = part + (t * nh + h) * (c + 1);
    for (int q = 0; q <= c; ++q) {
      double s = 0.0;
      if (q <= most) {                            // (no index of the chunk has more of the mask's bits)
#pragma unroll
        for (int u = 0; u < OPO_CB - 5; ++u) s += mine + u == q ? acc[u] : 0.0;
        s = opo_wave_sum(s);
      }
      if (lane == 0) o[q] = s;
    }
  }
  __syncthreads();
  for (int task = wave; task < nt * (m + 1); task += KB / 64) {
    const int t = task / (m + 1), q = task - t * (m + 1);
    const uint32_t hi = __builtin_amdgcn_readfirstlane(msk(t)) >> c;
    double s = 0.0;
    for (long long h = lane; h < nh; h += 64) {
      const int j = q - __builtin_popcount((uint32_t)h & hi);
      if (j >= 0 && j <= c) s += part[(t * nh + h) * (c + 1) + j];
    }
    s = opo_wave_sum(s);
    if (lane == 0) out(t, q, s);
  }
  __syncthreads();
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// Row fields: toff tables (opost_doubles), coff chunk partials, foff the row's k x k block of out_pos.  out_le [row]
template <int KB>
__global__ __launch_bounds__(KB) void k_order_pos(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                                  const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                                  double* tab, double* out_le, double* out_pos) {
  __shared__ OprRow S;
  __shared__ double bu[1 << OPO_CB];           // paired: B of the unseeded state of the joint events e
  __shared__ double Rs[32][32];                // Rs[d][j]: summed masses of the moves that put slot d at position j
  __shared__ double Rj[OPO_CB + 1][OPO_CB + 1]; // paired, before the seeding: Rj[t][j] target joint event t (kj: the
                                               // seeding) from a state of j joint events
  const int tid = threadIdx.x;
  for (int i = tid; i < 32 * 32; i += KB) (&Rs[0][0])[i] = 0.0;
  opr_load<KB>(S, rows, g_lt, g_o1, g_o2, N);
  const ORow& r = S.r;
  const int k = r.k;
  double* den = tab + opr_uniform(r.toff);
  double* part = tab + opr_uniform(r.coff);
  double* P = out_pos + opr_uniform(r.foff);

  if (r.mode != ORD_PAIRED) {
    double* F = den + (1ll << k);
    const double Z = opr_single_passes<KB>(S, N, den, F);
    if (tid == 0) out_le[r.row] = log(Z);
    if (k == 0) return;
    const int m = k - 1;
    opp_class_sums<KB>(k, m, opo_chunk_bits(m, KB), part,
        [&](int d, uint32_t idx) { return opr_single_mass(S, N, den, F, d, idx); },
        [&](int) { return (1u << m) - 1u; },
        [&](int d, int j, double s) { Rs[d][j] = s; });
    for (int i = tid; i < k * k; i += KB) P[i] = fmin(Rs[i / k][i % k] / Z, 1.0);
    return;
  }

  const OprPaired T = opr_paired_tables(r, den);
  const double Z = opr_paired_passes<KB>(S, N, T);
  opr_unseeded_backward<KB>(S, N, T, bu);
  const int kj = T.kj;
  if (tid == 0) out_le[r.row] = log(Z);
  // after the seeding: target slot d < k - 1, the moves from the seeded x without d; x holds the seeding, an entry of
  // both lineages
  const int m = k >= 2 ? k - 2 : 0;
  opp_class_sums<KB>(k - 1, m, opo_chunk_bits(m, KB), part,
      [&](int d, uint32_t idx) { return opr_seeded_mass(S, N, T, d, idx); },
      [&](int d) { return opp_index_mask(r.kind[d] == ORD_K_PT ? r.pt_mask : r.mt_mask, d, m); },
      [&](int d, int j, double s) { Rs[d][j + 1] = s; });
  // before the seeding: one wave per (target, joint events held), the lanes stride the states
  {
    const int wave = tid >> 6, lane = tid & 63;
    const uint32_t EJ = 1u << kj;
    for (int task = wave; task < (kj + 1) * (kj + 1); task += KB / 64) {
      const int q = task / (kj + 1), j = task - q * (kj + 1);
      double s = 0.0;
      for (uint32_t e = lane; e < EJ; e += 64) {
        if (__builtin_popcount(e) != j || (q < kj && ((e >> q) & 1u))) continue;
        const uint32_t x = opr_joint_state(S, e);
        s += T.F[3ll * x] * (q < kj ? opr_joint_edge(S, N, T, bu, e, q) : opr_seed_edge(S, N, T, x));
      }
      s = opo_wave_sum(s);
      if (lane == 0) Rj[q][j] = s;
    }
  }
  __syncthreads();
  for (int i = tid; i < k * k; i += KB) {
    const int d = i / k, j = i - d * k;
    const int q = d == k - 1 ? kj : S.jev[d];
    double s = d < k - 1 ? Rs[d][j] : 0.0;
    if (q >= 0 && j <= kj) s += Rj[q][j];
    P[i] = fmin(s / Z, 1.0);
  }
}

}  // namespace mmhn
