// Genotype distribution of one tumour given the other: for a primary tumour observed seeded with the genotype x the joint
// probability with EVERY genotype y of the metastasis (given PT), or for a metastasis observed with y the joint probability
// with every genotype of the primary tumour (given MT) - one row or column of the (PT x MT) table, exp(lp) of the paired
// row (type 3) with unknown order of observation for all 2^n partners at once (metmhn_amd/model.py
// MetMHN.partner_distribution has the definition on the host).
//
// After the seeding the two tumours are independent absorbing chains, each stopped by its own clock, so the joint
// factorises through the founder z.  With genodist.h's and metdist.h's symbols, kappa1 = kappa0 exp(obs1[n]),
// den1 = L + kappa1, denm = Lm + kappam, the query q, the GIVEN chain's rates rho_j (lambda_j for PT, mu_j for MT), clock
// kq (kappa1 / kappam) and den dq, the PARTNER chain's rates, clock kp and den dp:
//   G0(z), z in q:      genodist.h's F0 / G0 (a subset's G0 reads subsets only)
//   B(q) = kq(q) / dq(q),   B(z) = sum over j in q - z of rho_j(z) B(z + j) / dq(z)     z a proper subset of q
//   W(z) = sigma(z) G0(z) B(z) for z in q, 0 elsewhere            = P(founder z, the given tumour observed as q)
//   F(y) = W(y) + sum_b G(y - b) rate_b(y - b),   G = F / dp,   J(y) = kp(y) G(y)
//   sum W = sum J = P(the given tumour is observed as q, seeded)
// dq takes EVERY mutation z lacks, the ones q does not hold included: they leave the sub-lattice and are lost.
//
// Layout.  TWO planes of 2^n doubles, PLANAR as in the siblings: plane 0 the founder (B, then W), plane 1 the partner.
// Plane 1 is free until the full sweep starts, so G0 of the subsets of q lives there first: 16 B x 2^n.
//
// Shape, per query, on lattice.h's tiling and by stream order alone (no cooperative launch, no flags, no atomics).  ql /
// qh are the low c and the high bits of q; the RESTRICTED tiles are the 2^popcount(qh) tile numbers that are subsets of
// qh, a host-built list sorted by popcount that the first two passes walk in opposite directions.
// The three level kernels are lattice.h's tile solve with a recursion each.
//   1. k_partner_back, restricted tiles, levels DESCENDING: B into plane 0.  Every free bit is a term of den, only the ones
//      q holds are pulled (from the finished tile T | bit); states whose low bits are not a subset of ql are 0.
//   2. k_partner_seed, restricted tiles, levels ASCENDING: F0 / G0 on the subsets of q, pulled from and written to plane 1,
//      and plane 0 from B to W = sigma G0 B in place.
//   3. k_partner_level, EVERY tile, levels ascending: F / G with the partner chain's rates and clock into plane 1.  The
//      source W is read only where tile and state are subsets of q - the masks are tested before the load, so plane 0
//      outside the sub-lattice is never read - and a tile overwrites the G0 it may hold only after its own pulls, which
//      read finished tiles of F.
//   4. k_partner_tile, every tile: plane 1 times the partner's clock in place, and the GD_FEAT partial sums of founder and
//      partner with genodist.h's gd_tile_fold.  The founder outside the sub-lattice is SUBSTITUTED BY MASK, not memset:
//      the kernel folds an exact 0 there without reading plane 0 and, for the `full` output only (ZERO), stores the 0.
//   5. k_genodist_summary, unchanged, when summaries are asked for; k_partner_values: `mass` = the sum over the tiles, in
//      k_genodist_summary's order (thread t the tiles t, t + 256, ... ascending, then the one ls_block_sum both call), of the
//      fold's tile masses of the partner plane - the summary's mass[1] by construction, formed whether or not summaries are
//      asked for - and the two planes at the row's target.
// The chain is a kernel parameter (PartnerChain), not a second copy: its tables (the rate columns are the same in both
// sets, the clock column is obs1's or obs2's), its obs vector and whether a rate takes the factor exp(theta[j][n]).
// Every rate comes in O(1) from the tile's factor and the two 32-entry tables.
//
// Every shape depends on n and the query alone: no byte of a query's outputs depends on the other queries or an earlier call.
// fp64 only.
//
// LDS of a workgroup of the three level kernels: 2 x 8 KiB (the value and the partial den of 2^10 states) + 16.5 KiB of
// rate tables + 2 KiB of patterns + the tile's factors: four workgroups a CU, against metdist.h's two.
//
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_partner_back 64 VGPRs, 0 AGPRs, 76 SGPRs, scratch 0, LDS
// 35 928 B, 4 waves / SIMD (four workgroups a CU, by LDS); k_partner_seed 46 VGPRs, 57 SGPRs, scratch 0, LDS 35 656 B, 4 waves
// / SIMD; k_partner_level 66 VGPRs, 0 AGPRs, 48 SGPRs, scratch 0, LDS 35 928 B, 4 waves / SIMD; k_partner_tile<true> / <false>
// 34 VGPRs, 52 SGPRs, scratch 0, LDS 51 200 B, 3 waves / SIMD; k_partner_values 12 VGPRs, 26 SGPRs, scratch 0, LDS 2 048 B,
// 8 waves / SIMD.  genodist.h has k_genodist_summary's, lattice.h the tables'.
#pragma once
#include "genodist.h"

namespace mmhn {

// one of the two chains behind the seeding, as a kernel sees it
struct PartnerChain {
  const LsTables* tabs;                         // the tables of (theta, obs): obs1 for the primary tumour, obs2 for the metastasis
  const double* obs;                            // [N]; the clock is exp(obs[n]) times column n + 1
  int met;                                      // 0: lambda_j, 1: mu_j = lambda_j exp(theta[j][n])
};

// what the kernels of a chain add to ls_tile_prologue, every thread: EM[j] the factor of rate j.  Returns exp(obs[n]).
__device__ __forceinline__ double pt_chain_prologue(LsTables& S, double (&HF)[LS_COLS], double (&EM)[ORD_MAXN + 1],
                                                    const PartnerChain& ch, const double* __restrict__ g_lt, int N, int c,
                                                    uint32_t T) {
  ls_tile_prologue(S, HF, ch.tabs, g_lt, ch.obs, N, c, T);
  ls_seeded_factors(EM, g_lt, N, ch.met != 0);
  return exp(ch.obs[N - 1]);
}

// what the two recursions of a chain share: the one rate of a move is the chain's, its clock is column n + 1 times ek
struct PartnerChainRecursion : LsRecursion {
  const LsTables& S;
  const double (&HF)[LS_COLS];
  const double (&EM)[ORD_MAXN + 1];
  int n;
  double ek;
  __device__ __forceinline__ double column(int j) const { return EM[j]; }
  __device__ __forceinline__ void rates(double r, double em, double (&rt)[1]) const { rt[0] = r * em; }
  __device__ __forceinline__ double clock(uint32_t lo, uint32_t hi) const { return ls_rate(S, HF[n + 1], n + 1, lo, hi) * ek; }
};

// B of the given chain: every free bit a term of den, the ones q holds pulled; 0 outside the subsets of q, the clock at q
struct PartnerBackRecursion : PartnerChainRecursion {
  uint32_t q, ql;
  bool top;                                     // the tile of q
  __device__ __forceinline__ bool pulls(int j) const { return (q >> j) & 1u; }
  __device__ __forceinline__ bool live(uint32_t p) const { return !(p & ~ql); }
  __device__ __forceinline__ void finish(uint32_t p, uint32_t lo, uint32_t hi, double (&f)[1], const double (&L)[1]) const {
    const double kap = clock(lo, hi);
    f[0] = ((top && p == ql) ? kap : f[0]) / (L[0] + kap);
  }
};

// 1. one level of restricted tiles, descending: workgroup b finishes B of the tile tiles[b] (a subset of q's high bits);
// every tile tiles[b] | bit with the bit in q is finished (earlier launches)
__global__ __launch_bounds__(LS_KB) void k_partner_back(PartnerChain ch, const uint32_t* __restrict__ tiles,
                                                        const double* __restrict__ g_lt, int N, int c, uint32_t q, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];
  __shared__ double EM[ORD_MAXN + 1];
  __shared__ double W[2][1 << LS_TILE_BITS];    // 0: B of the tile's states (partial sums until a state is finished), 1: its partial den
  const int n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c, ql = q & (Vt - 1u);
  const double ek = pt_chain_prologue(S, HF, EM, ch, g_lt, N, c, T);
  __syncthreads();
  ls_tile_solve<1, 1, false>(PartnerBackRecursion{{{}, S, HF, EM, n, ek}, q, ql, T == q >> c}, S, HF, W, n, c, T, V, 0);
  ls_write_tile<1>(W, Vt, V, (long long)T << c, 1ll << n);
}

// F0 / G0 on the subsets of q
struct PartnerSeedRecursion : LsRecursion {
  const LsTables& S;
  const double (&HF)[LS_COLS];
  int n;
  uint32_t T, ql;
  __device__ __forceinline__ void source(uint32_t p, double (&f)[1]) const {
    if (T == 0u && p == 0u) f[0] = 1.0;         // F0 of the empty genotype
  }
  __device__ __forceinline__ bool live(uint32_t p) const { return !(p & ~ql); }
  __device__ __forceinline__ void finish(uint32_t, uint32_t lo, uint32_t hi, double (&f)[1], const double (&L)[1]) const {
    f[0] = f[0] / (L[0] + ls_rate(S, HF[n], n, lo, hi) + ls_rate(S, HF[n + 1], n + 1, lo, hi));
  }
};

// 2. one level of restricted tiles, ascending: G0 of the tile tiles[b] into plane 1 and plane 0 from B to W = sigma G0 B;
// every tile tiles[b] - bit is finished (earlier launches).  tabs: the tables of (theta, obs1)
__global__ __launch_bounds__(LS_KB) void k_partner_seed(const LsTables* __restrict__ tabs, const uint32_t* __restrict__ tiles,
                                                        const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                        int N, int c, uint32_t q, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];
  __shared__ double W[2][1 << LS_TILE_BITS];    // 0: F0 of the tile's states (partial until a state is finished, then G0), 1: its partial L
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c, ql = q & (Vt - 1u);
  const long long plane = 1ll << n, base = (long long)T << c;
  ls_tile_prologue(S, HF, tabs, g_lt, g_o1, N, c, T);
  __syncthreads();
  ls_tile_solve<1, 1, true>(PartnerSeedRecursion{{}, S, HF, n, T, ql}, S, HF, W, n, c, T, V + plane, 0);   // G0 lives in plane 1
  for (uint32_t p = tid; p < Vt; p += LS_KB) {
    double* o = V + base + p;
    const double g0 = W[0][p];
    o[0] = (p & ~ql) ? 0.0 : (ls_rate(S, HF[n], n, p & 31u, p >> LS_HALF) * g0) * o[0];
    o[plane] = g0;
  }
}

// F / G of the partner chain; the source W is read only where tile and state are subsets of q, the masks tested before the load
struct PartnerLevelRecursion : PartnerChainRecursion {
  const double* src;                            // plane 0 of the tile
  bool sub;                                     // the tile is a subset of q's high bits
  uint32_t ql;
  __device__ __forceinline__ void source(uint32_t p, double (&f)[1]) const {
    if (sub && !(p & ~ql)) f[0] = src[p];
  }
  __device__ __forceinline__ void finish(uint32_t, uint32_t lo, uint32_t hi, double (&f)[1], const double (&L)[1]) const {
    f[0] = f[0] / (L[0] + clock(lo, hi));
  }
};

// 3. one level of ALL tiles, ascending: workgroup b finishes G = F / den of the partner chain in plane 1 of the tile tiles[b];
// every tile tiles[b] - bit is finished (earlier launches).  The source W (plane 0) is read on the subsets of q only
__global__ __launch_bounds__(LS_KB) void k_partner_level(PartnerChain ch, const uint32_t* __restrict__ tiles,
                                                         const double* __restrict__ g_lt, int N, int c, uint32_t q, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];
  __shared__ double EM[ORD_MAXN + 1];
  __shared__ double W[2][1 << LS_TILE_BITS];    // 0: F of the tile's states (partial until a state is finished, then G), 1: its partial L
  const int n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c, ql = q & (Vt - 1u), qh = q >> c;
  const long long plane = 1ll << n, base = (long long)T << c;
  const double ek = pt_chain_prologue(S, HF, EM, ch, g_lt, N, c, T);
  __syncthreads();
  ls_tile_solve<1, 1, true>(PartnerLevelRecursion{{{}, S, HF, EM, n, ek}, V + base, (T & ~qh) == 0u, ql}, S, HF, W, n, c, T,
                            V + plane, 0);
  ls_write_tile<1>(W, Vt, V + plane, base, plane);
}

// 4. every tile once all levels are finished (workgroup = tile number): plane 1 from G to J = clock G in place, and the
// GD_FEAT partial sums of the tile's founder and partner at part[(s * GD_FEAT + f) * nt + T].  The founder outside the
// subsets of q is an exact 0 that is not read; with ZERO it is stored too (the `full` output)
template <bool ZERO>
__global__ __launch_bounds__(LS_KB) void k_partner_tile(PartnerChain ch, int N, int c, uint32_t q, double* V,
                                                        double* __restrict__ part, long long nt) {
  __shared__ double KL[1 << LS_HALF], KH[1 << LS_HALF];
  const LsColumn KC{KL, KH};                    // the chain's clock
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = blockIdx.x;
  const uint32_t Vt = 1u << c, ql = q & (Vt - 1u), qh = q >> c;
  const long long plane = 1ll << n, base = (long long)T << c;
  KC.load(ch.tabs, n + 1);
  const double k0 = LsColumn::factor(ch.obs, 0.0, c, T), ek = exp(ch.obs[n]);
  const bool sub = (T & ~qh) == 0u;
  __syncthreads();
  double u[LS_SPT], w[LS_SPT];
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    u[s] = w[s] = 0.0;
    if (p < Vt) {
      double* o = V + base + p;
      if (sub && !(p & ~ql)) u[s] = o[0];
      else if constexpr (ZERO) o[0] = 0.0;
      w[s] = (KC.at(k0, p & 31u, p >> LS_HALF) * ek) * o[plane];
      o[plane] = w[s];
    }
  }
  gd_tile_fold(u, w, part, nt, T);
}

// 5. a query's rows (workgroup b = row first + b of the sorted rows): out[row] = the mass of the partner plane - the tiles'
// masses added as k_genodist_summary adds them -, W and J at the row's target (NaN without targets)
__global__ __launch_bounds__(LS_KB) void k_partner_values(const double* __restrict__ part, long long nt, int n, uint32_t q,
                                                          const uint32_t* __restrict__ targets, long long first,
                                                          const double* __restrict__ V, double* __restrict__ out) {
  __shared__ double red[LS_KB];
  const int tid = threadIdx.x;
  const double* pc = part + (long long)GD_FEAT * nt;
  double acc = 0.0;
  for (long long T = tid; T < nt; T += LS_KB) acc += pc[T];
  const double mass = ls_block_sum(red, acc);
  if (tid == 0) {
    const long long i = first + blockIdx.x;
    double* o = out + 3 * i;
    o[0] = mass;
    o[1] = o[2] = __builtin_nan("");
    if (targets) {
      const uint32_t t = targets[i];
      o[1] = (t & ~q) ? 0.0 : V[t];
      o[2] = V[(1ll << n) + t];
    }
  }
}

}  // namespace mmhn
