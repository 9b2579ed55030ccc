// Genotype distribution of the metastasis and of its founder: the probability of EVERY genotype to be the one the seeding
// cell holds (Z), to be the metastasis' observed one (M), and M weighted by how many of its mutations the founder already
// held (C), in one forward sweep over the full lattice - genodist.h's sweep with a third plane and the metastasis' own
// rates behind the seeding (metmhn_amd/model.py MetMHN.metastasis_distribution has the definition on the host).
//
// The metastasis is an autonomous chain: up to the seeding it is the common lineage, which leaves by seeding or by the
// primary tumour's first clock; from the seeding on it runs with its own rates, which carry the seeding's effect
// theta[j][n], until its own clock obs2.  x, y, z are genotype codes, j over the mutations a code does not hold, b over the
// ones it holds; lambda, sigma, kappa0, L as in genodist.h and
//   mu_j(z) = lambda_j(z) exp(theta[j][n]),  Lm(z) = sum_j mu_j(z),  kappam(z) = exp(obs2[n] + sum over i in z of obs2[i])
//   F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                       G0 = F0 / (L + sigma + kappa0)
//                   FM(y) = G0(y) sigma(y)      + sum_b GM(y - b) mu_b(y - b),     GM = FM / (Lm + kappam)
//                   FC(y) = G0(y) sigma(y) |y|  + sum_b GC(y - b) mu_b(y - b),     GC = FC / (Lm + kappam)
//   Z = sigma G0,  M = kappam GM (exp(lp) of the cohort row of type 2),  C = kappam GC  (C / M: the expected number of
//   the metastasis' mutations that the founder held)
//
// Layout.  PLANAR: three vectors of 2^n doubles in the workspace, plane s of code x at V[s * 2^n + x], G0, GM, GC during
// the sweep; k_metdist_tile turns them into Z, M, C in place once every level is finished - the layout of `full`.
//
// Shape.  k_genodist_level's: lattice.h's tiling and its tile solve forwards, one launch of k_metdist_level per popcount
// of the tile number, ASCENDING.  This file's own is the recursion (MetdistRecursion), with TWO rates per move: r = HF[j]
// TL[j] TH[j] is formed once, r exp(theta[j][n]) (the factor from lattice.h's ls_seeded_factors, a 33-entry table in LDS)
// serves GM, GC and Lm; G0 of a state before its FM and FC, which take G0 sigma of the same state; |y| = popcount(T) +
// popcount(p).
//
// kappa0 is column n + 1 of the obs1 tables, as in genodist.h.  kappam needs the same column of obs2: the host launches
// lattice.h's k_landscape_tables a SECOND time with obs2 in place of obs1 and a tile copies ONLY the clock column of
// that second set (an LsColumn, 2 x 32 doubles) into LDS - no table kernel of its own; the second set's rate columns equal
// the first's and are not read.
//
// LDS of a workgroup of k_metdist_level: 5 x 8 KiB (F0, FM, FC, the partial L and Lm of 2^10 states) + 16.5 KiB of rate
// tables + 2 KiB of patterns + the tile's factors, exp(theta[j][n]) and the obs2 clock column: the landscape's footprint,
// two workgroups a CU.  256 threads, 4 states per thread in step 1: 20 accumulators.
//
// Summary.  k_metdist_tile<SUMS> forms the GD_FEAT = 67 partial sums of the planes Z and M per tile with genodist.h's
// three-stage fold (gd_tile_fold, the one copy both kernels call); k_genodist_summary then adds the tiles' partials,
// unchanged: summary plane 0 is the founder, plane 1 the metastasis.
//
// Every shape depends on n alone: no byte of an output depends on the queries, the grid or an earlier call.  fp64 only.
//
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_metdist_level 82 VGPRs, 0 AGPRs, 52 SGPRs, scratch 0,
// LDS 61 024 B, 2 waves / SIMD (two workgroups a CU, by LDS; the registers would allow 5); k_metdist_tile<true> 40 VGPRs,
// 54 SGPRs, scratch 0, LDS 51 712 B, 3 waves / SIMD; k_metdist_tile<false> 26 VGPRs, 48 SGPRs, scratch 0, LDS 1 024 B.
// (k_genodist_tile<true>, the other caller of gd_tile_fold: 36 VGPRs, 50 SGPRs, scratch 0, LDS 51 200 B - the 512 B between
// the two are the sigma tables.)  lattice.h has the tables' and the gather's.
#pragma once
#include "genodist.h"

namespace mmhn {

// the recursion of F0 / FM / FC: two rates per move, lambda_j for F0 and L, mu_j for FM, FC and Lm; G0 of a state before its
// FM and FC, which take G0 sigma of the same state; |y| = popcount(T) + popcount(p)
struct MetdistRecursion : LsRecursion {
  const LsTables& S;
  const double (&HF)[LS_COLS];
  const double (&EM)[ORD_MAXN + 1];
  LsColumn MC;
  int n;
  uint32_t T;
  int pcT;
  double km;
  __device__ __forceinline__ double column(int j) const { return EM[j]; }
  __device__ __forceinline__ void rates(double r, double em, double (&rt)[2]) const { rt[0] = r; rt[1] = r * em; }
  __device__ __forceinline__ void move(double (&f)[3], const double (&rt)[2], const double (&v)[3]) const {
    f[0] += rt[0] * v[0];
    f[1] += rt[1] * v[1];
    f[2] += rt[1] * v[2];
  }
  __device__ __forceinline__ void source(uint32_t p, double (&f)[3]) const {
    if (T == 0u && p == 0u) f[0] = 1.0;         // F0 of the empty genotype
  }
  __device__ __forceinline__ void finish(uint32_t p, uint32_t lo, uint32_t hi, double (&f)[3], const double (&L)[2]) const {
    const double sig = ls_rate(S, HF[n], n, lo, hi);
    const double kap = ls_rate(S, HF[n + 1], n + 1, lo, hi);
    const double g0 = f[0] / (L[0] + sig + kap);
    const double seeded = g0 * sig;
    const double denm = L[1] + MC.at(km, lo, hi);
    f[0] = g0;
    f[1] = (seeded + f[1]) / denm;
    f[2] = (seeded * (double)(pcT + __builtin_popcount(p)) + f[2]) / denm;
  }
};

// one level of tiles: workgroup b finishes the tile tiles[b]; every tile tiles[b] - bit is finished (earlier launches).
// tabs: the tables of (theta, obs1); tabm: the tables of (theta, obs2), of which only the clock column is read
__global__ __launch_bounds__(LS_KB) void k_metdist_level(const LsTables* __restrict__ tabs, const LsTables* __restrict__ tabm,
                                                         const uint32_t* __restrict__ tiles, const double* __restrict__ g_lt,
                                                         const double* __restrict__ g_o1, const double* __restrict__ g_o2,
                                                         int N, int c, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];                // column j: exp(diagonal + the effects of the tile's high bits)
  __shared__ double EM[ORD_MAXN + 1];           // exp(theta[j][n]): mu_j = lambda_j EM[j]
  __shared__ double ML[1 << LS_HALF], MH[1 << LS_HALF];
  const LsColumn MC{ML, MH};                    // the clock column of the obs2 tables
  __shared__ double KM;                         // its factor of the tile, with exp(obs2[n])
  __shared__ double W[5][1 << LS_TILE_BITS];    // 0 / 1 / 2: F0 / FM / FC of the tile's states (partial until a state is finished, then G), 3 / 4: its partial L / Lm
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const long long plane = 1ll << n;
  ls_tile_prologue(S, HF, tabs, g_lt, g_o1, N, c, T);
  ls_seeded_factors(EM, g_lt, N, true);
  MC.load(tabm, n + 1);
  if (tid == LS_KB - 1) KM = LsColumn::factor(g_o2, g_o2[n], c, T);
  __syncthreads();
  ls_tile_solve<3, 2, true>(MetdistRecursion{{}, S, HF, EM, MC, n, T, __builtin_popcount(T), KM}, S, HF, W, n, c, T, V, plane);
  ls_write_tile<3>(W, 1u << c, V, (long long)T << c, plane);
}

// every tile once all levels are finished (workgroup = tile number): G to Z = sigma G0, M = kappam GM, C = kappam GC in
// place and, with SUMS, the GD_FEAT partial sums of the tile's Z and M at part[(s * GD_FEAT + f) * nt + T]
template <bool SUMS>
__global__ __launch_bounds__(LS_KB) void k_metdist_tile(const LsTables* __restrict__ tabs, const LsTables* __restrict__ tabm,
                                                        const double* __restrict__ g_lt, const double* __restrict__ g_o2,
                                                        int N, int c, double* V, double* __restrict__ part, long long nt) {
  __shared__ double SL[1 << LS_HALF], SH[1 << LS_HALF], ML[1 << LS_HALF], MH[1 << LS_HALF];
  const LsColumn SC{SL, SH}, MC{ML, MH};        // sigma; the clock column of the obs2 tables
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = blockIdx.x;
  const uint32_t Vt = 1u << c;
  const long long plane = 1ll << n, base = (long long)T << c;
  SC.load(tabs, n);
  MC.load(tabm, n + 1);
  const double sf = LsColumn::factor(g_lt + n * N, g_lt[n * N + n], c, T), km = LsColumn::factor(g_o2, g_o2[n], c, T);
  __syncthreads();
  double u[LS_SPT], w[LS_SPT];
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    u[s] = w[s] = 0.0;
    if (p < Vt) {
      const uint32_t lo = p & 31u, hi = p >> LS_HALF;
      const double sig = SC.at(sf, lo, hi);
      const double kap = MC.at(km, lo, hi);
      double* o = V + base + p;
      u[s] = sig * o[0];
      w[s] = kap * o[plane];
      o[0] = u[s]; o[plane] = w[s];
      o[2 * plane] = kap * o[2 * plane];
    }
  }
  if constexpr (SUMS) gd_tile_fold(u, w, part, nt, T);
}

}  // namespace mmhn
