// Exact PT x MT co-occurrence and joint burden tables: P(the primary tumour holds mutation i, the metastasis holds mutation j,
// seeded) for every i, j and P(|PT| = k, |MT| = l, seeded) for every k, l - the second moments of the (PT x MT) table of which
// partner.h gives one row or column per sweep (metmhn_amd/lattice_host.py _cross_host has the definition on the host).
//
// After the seeding the two tumours are independent absorbing chains, each stopped by its own clock (partner.h), so every
// BILINEAR statistic of the pair factorises through the founder z:
//   E[phi(PT) psi(MT); seeded] = sum_z Z(z) a_phi(z) b_psi(z)
// Z = sigma G0 is metdist.h's founder plane, a_phi(z) = E[phi(PT at its observation) | founder z] the value function
//   a_phi(z) = (kappa1(z) phi(z) + sum over j not in z of lambda_j(z) a_phi(z + j)) / den1(z),   den1 = L + kappa1
// from the full genotype down, b_psi the same with the metastasis' mu_j, kappam, denm = Lm + kappam.  The FEATURES of a
// chain, in this order: the n gene indicators [mutation i held], then the n + 1 burden indicators [|x| = k]; without the
// burden only the first n.  Gene x gene is `cross`, burden x burden `burden`, the mixed products `gene_burden`, Z a_f and
// Z b_g alone the marginals `pt` and `mt`.
//
// Layout.  PLANAR as in the siblings, planes of 2^n doubles: one plane of G0 / Z and BLOCKS of four planes, a block the value
// functions of four consecutive features of one chain (CrossBlock).  The last block is padded with features that are
// identically 0: their planes are exact zeros and their sums are discarded on the host.
//
// Shape, on lattice.h's tiling and by stream order alone (no cooperative launch, no flags, no atomics):
//   1. k_cross_seed, every tile, levels ASCENDING: genodist.h's F0 / G0 through partner.h's PartnerSeedRecursion with the full
//      mask (every state live), one plane, pulled from and written to itself.
//   2. k_cross_founder, every tile (workgroup = tile number), once per call: G0 to Z = sigma G0 in place - k_metdist_tile's
//      product, so metdist.h's founder plane byte for byte - and the tile's mass of Z.
//   3. k_cross_back, one level of tiles, levels DESCENDING, per block: ls_tile_solve<4, 1, false> with CrossBackRecursion, a
//      PartnerChainRecursion (the chain is a kernel parameter, PartnerChain): every free bit is pulled and is a term of den,
//      finish forms (clock phi_f(state) + sum) / den for the block's four features.  phi_f is decided from the descriptor:
//      bit f of the code (of the low offset or of the tile number) or popcount(tile number) + popcount(low offset) == k.
//   4. k_cross_fold, every tile (workgroup = tile number), per PAIR of a PT block and an MT block: Z and the 4 + 4 planes
//      read once, the tile's 16 sums of (Z a_f) b_g, 4 of Z a_f and 4 of Z b_g, each one ls_block_sum in a fixed order, to
//      part[s * nt + T].
//   5. k_cross_reduce, a workgroup per sum: the tiles' partials in k_genodist_summary's order (thread t the tiles t, t + 256,
//      ... ascending, then the one ls_block_sum) into the device's table; the same kernel adds the tile masses of step 2.
// A state's sums run over the high bits ascending, then the low bits ascending, as in every sweep of lattice.h.
//
// Every shape depends on n alone and a block's planes on the model and its features alone: no byte of an output depends on
// the workspace limit, on how many PT blocks were held or recomputed (cross_host.h), or on an earlier call.  fp64 only.
//
// LDS of a workgroup of k_cross_back: 5 x 8 KiB (four values and the partial den of 2^10 states) + 16.5 KiB of rate tables +
// 2 KiB of patterns + the tile's factors and exp(theta[j][n]): the landscape's footprint, two workgroups a CU.
//
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_cross_back 82 VGPRs, 0 AGPRs, 95 SGPRs, scratch 0, LDS
// 60 504 B, 2 waves / SIMD (two workgroups a CU, by LDS; the registers would allow 5); k_cross_seed 46 VGPRs, 50 SGPRs, scratch
// 0, LDS 35 656 B, 4 waves / SIMD; k_cross_founder 15 VGPRs, 26 SGPRs, scratch 0, LDS 2 560 B; k_cross_fold 72 VGPRs, 28 SGPRs,
// scratch 0, LDS 2 048 B, 7 waves / SIMD; k_cross_reduce 12 VGPRs, 22 SGPRs, scratch 0, LDS 2 048 B.  lattice.h has the tables'.
#pragma once
#include "partner.h"

namespace mmhn {

constexpr int CX_BLOCK = 4;                     // features of a block: the planes of one backward sweep
constexpr int CX_SUMS = CX_BLOCK * CX_BLOCK + 2 * CX_BLOCK;   // sums of a tile and pair of blocks: (Z a_f) b_g, Z a_f, Z b_g

// four consecutive features of a chain: feature first + k is the gene indicator of bit first + k below `genes`, the burden
// indicator of popcount first + k - genes below `count`, and identically 0 from there (the padding of the last block)
struct CrossBlock {
  int first, genes, count;
};

// the value functions of a block's features: every free bit pulled and a term of den, the clock times the feature at the state
struct CrossBackRecursion : PartnerChainRecursion {
  CrossBlock blk;
  uint32_t T;
  int c;
  __device__ __forceinline__ bool feature(int k, uint32_t p) const {
    const int f = blk.first + k;
    if (f < blk.genes) return f < c ? (p >> f) & 1u : (T >> (f - c)) & 1u;
    if (f < blk.count) return __builtin_popcount(T) + __builtin_popcount(p) == f - blk.genes;
    return false;
  }
  __device__ __forceinline__ void finish(uint32_t p, uint32_t lo, uint32_t hi, double (&f)[CX_BLOCK], const double (&L)[1]) const {
    const double kap = clock(lo, hi);
    const double den = L[0] + kap;
#pragma unroll
    for (int k = 0; k < CX_BLOCK; ++k) f[k] = ((feature(k, p) ? kap : 0.0) + f[k]) / den;   // kap phi + sum: phi is 0 or 1
  }
};

// 1. one level of ALL tiles, ascending: G0 of the tile tiles[b], pulled from and written to the one plane V; every tile
// tiles[b] - bit is finished (earlier launches).  tabs: the tables of (theta, obs1)
__global__ __launch_bounds__(LS_KB) void k_cross_seed(const LsTables* __restrict__ tabs, const uint32_t* __restrict__ tiles,
                                                      const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                      int N, int c, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];
  __shared__ double W[2][1 << LS_TILE_BITS];    // 0: F0 of the tile's states (partial until a state is finished, then G0), 1: its partial L
  const int n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c;
  ls_tile_prologue(S, HF, tabs, g_lt, g_o1, N, c, T);
  __syncthreads();
  ls_tile_solve<1, 1, true>(PartnerSeedRecursion{{}, S, HF, n, T, Vt - 1u}, S, HF, W, n, c, T, V, 0);
  ls_write_tile<1>(W, Vt, V, (long long)T << c, 1ll << n);
}

// 2. every tile once all levels of G0 are finished (workgroup = tile number): G0 to Z = sigma G0 in place and the tile's mass
// of Z at mass[T]
__global__ __launch_bounds__(LS_KB) void k_cross_founder(const LsTables* __restrict__ tabs, const double* __restrict__ g_lt,
                                                         int N, int c, double* V, double* __restrict__ mass) {
  __shared__ double SL[1 << LS_HALF], SH[1 << LS_HALF];
  __shared__ double red[LS_KB];
  const LsColumn SC{SL, SH};                    // sigma
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = blockIdx.x;
  const uint32_t Vt = 1u << c;
  const long long base = (long long)T << c;
  SC.load(tabs, n);
  const double sf = LsColumn::factor(g_lt + n * N, g_lt[n * N + n], c, T);
  __syncthreads();
  double acc = 0.0;
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    if (p < Vt) {
      const double z = SC.at(sf, p & 31u, p >> LS_HALF) * V[base + p];
      V[base + p] = z;
      acc += z;
    }
  }
  const double sum = ls_block_sum(red, acc);
  if (tid == 0) mass[T] = sum;
}

// 3. one level of tiles, descending: workgroup b finishes the four value functions of block blk in the tile tiles[b] of the
// four planes at V; every tile tiles[b] | bit is finished (earlier launches)
__global__ __launch_bounds__(LS_KB) void k_cross_back(PartnerChain ch, CrossBlock blk, const uint32_t* __restrict__ tiles,
                                                      const double* __restrict__ g_lt, int N, int c, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];
  __shared__ double EM[ORD_MAXN + 1];
  __shared__ double W[CX_BLOCK + 1][1 << LS_TILE_BITS];   // the four values of the tile's states (partial sums until a state is finished), 4: its partial den
  const int n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const long long plane = 1ll << n;
  const double ek = pt_chain_prologue(S, HF, EM, ch, g_lt, N, c, T);
  __syncthreads();
  ls_tile_solve<CX_BLOCK, 1, false>(CrossBackRecursion{{{}, S, HF, EM, n, ek}, blk, T, c}, S, HF, W, n, c, T, V, plane);
  ls_write_tile<CX_BLOCK>(W, 1u << c, V, (long long)T << c, plane);
}

// 4. every tile (workgroup = tile number): the tile's sums over its states of (Z a_f) b_g at part[(4 f + g) * nt + T], of
// Z a_f at part[(16 + f) * nt + T] and of Z b_g at part[(20 + g) * nt + T]; A / B: the four planes of a PT / an MT block.
// Thread t adds its offsets t, t + 256, ... ascending, then one ls_block_sum per sum
__global__ __launch_bounds__(LS_KB) void k_cross_fold(const double* __restrict__ Z, const double* __restrict__ A,
                                                      const double* __restrict__ B, int n, int c, double* __restrict__ part,
                                                      long long nt) {
  __shared__ double red[LS_KB];
  const int tid = threadIdx.x;
  const uint32_t T = blockIdx.x;
  const uint32_t Vt = 1u << c;
  const long long plane = 1ll << n, base = (long long)T << c;
  double acc[CX_SUMS];
#pragma unroll
  for (int i = 0; i < CX_SUMS; ++i) acc[i] = 0.0;
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    if (p < Vt) {
      const double z = Z[base + p];
      double b[CX_BLOCK];
#pragma unroll
      for (int g = 0; g < CX_BLOCK; ++g) {
        b[g] = B[g * plane + base + p];
        acc[CX_BLOCK * CX_BLOCK + CX_BLOCK + g] += z * b[g];
      }
#pragma unroll
      for (int f = 0; f < CX_BLOCK; ++f) {
        const double za = z * A[f * plane + base + p];
        acc[CX_BLOCK * CX_BLOCK + f] += za;
#pragma unroll
        for (int g = 0; g < CX_BLOCK; ++g) acc[CX_BLOCK * f + g] += za * b[g];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CX_SUMS; ++i) {
    const double sum = ls_block_sum(red, acc[i]);
    if (tid == 0) part[(long long)i * nt + T] = sum;
    __syncthreads();                            // red is written again by the next sum
  }
}

// 5. the tiles' partials of one sum per workgroup, in k_genodist_summary's order: thread t adds the tiles t, t + 256, ...
// ascending, then the one block sum.  Of a fold over the PT block at feature fa and the MT block at feature fb (workgroup
// s < CX_SUMS, fa >= 0): tab[(fa + f) * FP + fb + g], the marginals behind the FP * FP products: Z a at tab[FP * FP + fa + f],
// Z b at tab[FP * FP + FP + fb + g].  Of the founder's tile masses (one workgroup, fa < 0): tab[FP * FP + 2 * FP]
__global__ __launch_bounds__(LS_KB) void k_cross_reduce(const double* __restrict__ part, long long nt, int fa, int fb, int FP,
                                                        double* __restrict__ tab) {
  __shared__ double red[LS_KB];
  const int tid = threadIdx.x, s = blockIdx.x;
  const double* pc = part + (long long)s * nt;
  double acc = 0.0;
  for (long long T = tid; T < nt; T += LS_KB) acc += pc[T];
  const double sum = ls_block_sum(red, acc);
  if (tid == 0) {
    const int pp = FP * FP;
    if (fa < 0) tab[pp + 2 * FP] = sum;
    else if (s < CX_BLOCK * CX_BLOCK) tab[(fa + s / CX_BLOCK) * FP + fb + s % CX_BLOCK] = sum;
    else if (s < CX_BLOCK * CX_BLOCK + CX_BLOCK) tab[pp + fa + s - CX_BLOCK * CX_BLOCK] = sum;
    else tab[pp + FP + fb + s - CX_BLOCK * CX_BLOCK - CX_BLOCK] = sum;
  }
}

}  // namespace mmhn
