// Seeding landscape: the four forecast scalars of EVERY genotype of a model in one backward sweep over the full lattice -
// the value functions behind metmhn_amd/model.py MetMHN.seeding_landscape (forecast.h answers the same question forwards,
// one genotype at a time).
//
// x is a genotype code (bit j = mutation j held), the primary tumour's theta, j runs over the mutations x does not hold:
//   lambda_j(x) = exp(theta[j][j] + sum over i in x of theta[j][i]),  sigma(x) the same with row n,
//   kappa(x) = exp(sum over i in x of obs1[i]) (0 until the seeding),  den = sum of lambda_j + sigma + kappa
//   p_seed(x)      = (sigma(x) + sum_j lambda_j(x) p_seed(x + j)) / den(x)
//   time(x)        = (1        + sum_j lambda_j(x) time(x + j)) / den(x)
//   new_events(x)  = (           sum_j lambda_j(x) (1 + new_events(x + j))) / den(x)
//   seed_events(x) = (           sum_j lambda_j(x) (p_seed(x + j) + seed_events(x + j))) / den(x)
// The full genotype has no j and is the first state.
//
// Layout.  Four planes of 2^n doubles in the workspace, value k of code x at V[k * 2^n + x] - the layout of the entry
// point's `full` output, so that is one copy.
//
// Shape.  lattice.h's tiling (the tiles, the rate tables and a tile's prologue are shared with genodist.h and metdist.h),
// the levels DESCENDING: tile T needs the tiles T | bit and itself.  Inside a tile
//   1. the moves along the high bits, ascending: thread t adds lambda_j(x) v(x + j) for every high bit j not in T, v read
//      from the finished tile T | j at the same offset; the partial sums and the partial den go to LDS;
//   2. the backward substitution over the low bits in LDS, by popcount of the low part, descending, the low moves added in
//      ascending bit.
// So a state's sums run over the high bits ascending, then the low bits ascending.  A rate is computed once per move and
// shared by the four values.  This is lattice.h's ls_tile_solve<4, 1, false> WRITTEN OUT: on the shared solve the kernel gave
// the same bytes and the same instruction counts but 20.1 against 19.9 ms per LUAD-28 sweep in three rounds of three, more
// than the parent's spread of 0.1 ms, so the one sweep that is bound by its stream keeps its own copy of the skeleton.
//
// LDS of a workgroup: 5 x 8 KiB (four values and the partial den of 2^10 states) + 16.5 KiB of rate tables + 2 KiB of
// patterns + the tile's factors = 58.8 KiB, so two workgroups share a CU's 160 KiB and one streams its neighbour tiles
// while the other solves on the chip.  4 states per thread in step 1: 20 accumulators (40 VGPRs); a rate lives for one
// move, not n of them.  These figures are those of lattice.h's `constexpr int LS_TILE_BITS = 10;` (asserted below).
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_landscape_level 66 VGPRs, 0 AGPRs, 56 SGPRs, scratch 0,
// LDS 60 232 B, 2 waves / SIMD (two workgroups a CU, by LDS; the registers would allow 7).  lattice.h has the tables' and the
// gather's.
//
// Every shape depends on n alone: a genotype's four values do not depend on the queries, the grid or an earlier call.
// fp64 only.
#pragma once
#include "lattice.h"

namespace mmhn {

static_assert(LS_TILE_BITS == 10, "the LDS budget and the resources in this file's comment are worked out for tiles of 10 bits");

// one level of tiles: workgroup b finishes the tile tiles[b]; every tile tiles[b] | bit is finished (earlier launches)
__global__ __launch_bounds__(LS_KB) void k_landscape_level(const LsTables* __restrict__ tabs, const uint32_t* __restrict__ tiles,
                                                           const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                           int N, int c, int clock, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];                // column j: exp(diagonal + the effects of the tile's high bits)
  __shared__ double W[5][1 << LS_TILE_BITS];    // the four values of the tile's states (partial sums until a state is finished), 4: its partial den
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c;
  const long long plane = 1ll << n, base = (long long)T << c;
  ls_tile_prologue(S, HF, tabs, g_lt, g_o1, N, c, T, clock != 0);
  __syncthreads();

  // 1. the moves along the high bits
  {
    double a0[LS_SPT], a1[LS_SPT], a2[LS_SPT], a3[LS_SPT], dn[LS_SPT];
#pragma unroll
    for (int s = 0; s < LS_SPT; ++s) a0[s] = a1[s] = a2[s] = a3[s] = dn[s] = 0.0;
    for (int j = c; j < n; ++j) {
      if ((T >> (j - c)) & 1u) continue;
      const double hf = HF[j];
      const double* q = V + base + (1ll << j);
#pragma unroll
      for (int s = 0; s < LS_SPT; ++s) {
        const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
        if (p < Vt) {
          const double r = ls_rate(S, hf, j, p & 31u, p >> LS_HALF);
          const double v0 = q[p], v1 = q[plane + p], v2 = q[2 * plane + p], v3 = q[3 * plane + p];
          a0[s] += r * v0;
          a1[s] += r * v1;
          a2[s] += r * (1.0 + v2);
          a3[s] += r * (v0 + v3);
          dn[s] += r;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < LS_SPT; ++s) {
      const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
      if (p < Vt) { W[0][p] = a0[s]; W[1][p] = a1[s]; W[2][p] = a2[s]; W[3][p] = a3[s]; W[4][p] = dn[s]; }
    }
  }
  __syncthreads();

  // 2. the backward substitution over the low bits
  const uint32_t chunks = Vt >> S.L.c;
  for (int lev = c; lev >= 0; --lev) {
    opo_level<LS_KB>(S.L, 0u, chunks, lev, [&](uint32_t p) {
      const uint32_t lo = p & 31u, hi = p >> LS_HALF;
      double n0 = W[0][p], n1 = W[1][p], n2 = W[2][p], n3 = W[3][p], den = W[4][p];
#pragma unroll
      for (int j = 0; j < LS_TILE_BITS; ++j) {
        if (j < c && !((p >> j) & 1u)) {
          const double r = ls_rate(S, HF[j], j, lo, hi);
          const uint32_t y = p | (1u << j);
          const double v0 = W[0][y];
          n0 += r * v0;
          n1 += r * W[1][y];
          n2 += r * (1.0 + W[2][y]);
          n3 += r * (v0 + W[3][y]);
          den += r;
        }
      }
      const double sig = ls_rate(S, HF[n], n, lo, hi);
      den += sig;
      if (clock) den += ls_rate(S, HF[n + 1], n + 1, lo, hi);
      W[0][p] = (sig + n0) / den;
      W[1][p] = (1.0 + n1) / den;
      W[2][p] = n2 / den;
      W[3][p] = n3 / den;
    });
    __syncthreads();
  }
  ls_write_tile<4>(W, Vt, V, base, plane);
}

}  // namespace mmhn
