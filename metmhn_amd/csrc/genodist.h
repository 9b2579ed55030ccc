// Genotype distribution of the primary tumour: the probability of EVERY genotype to be the one observed, unseeded (U) and
// seeded by then (S), in one forward sweep over the full lattice - the forward counterpart of landscape.h on lattice.h's
// tiling (metmhn_amd/model.py MetMHN.genotype_distribution has the definition on the host).
//
// x is a genotype code (bit j = mutation j held), the primary tumour's theta, j over the mutations x does not hold, b over
// the ones it holds:
//   lambda_j(x) = exp(theta[j][j] + sum over i in x of theta[j][i]),  sigma(x) the same with row n,
//   kappa0(x) = exp(sum over i in x of obs1[i]),  kappa1(x) = kappa0(x) exp(obs1[n]),  L(x) = sum_j lambda_j(x)
//   F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                       G0 = F0 / (L + sigma + kappa0)
//                   F1(y) = G0(y) sigma(y) + sum_b G1(y - b) lambda_b(y - b),      G1 = F1 / (L + kappa1)
//   U = kappa0 G0,  S = kappa1 G1
//
// Layout.  PLANAR: two vectors of 2^n doubles in the workspace, plane s of code x at V[s * 2^n + x].  During the sweep
// the planes hold G (what a successor pulls); k_genodist_tile turns them into U and S in place once every level is
// finished - the layout of the entry point's `full` output, so that is one copy - and folds the tile's sums on the way.
//
// Shape.  lattice.h's tiling and its tile solve forwards, one launch of k_genodist_level per popcount of the tile number,
// ASCENDING: tile T needs the tiles T - bit and itself.  This file's own is the recursion (GenodistRecursion): the rate of
// a move is shared by the two planes; G0 of a state before its F1, which takes G0 sigma of the same state.
//
// den.  A state's den needs its OUTGOING rates, which are not the moves it pulls.  L(x) is FORMED IN THE TILE, not
// carried: column b of the rate tables does not read bit b (ls_eff), so lambda_b(x - b) is the product HF[b] TL[b] TH[b]
// at x's own offsets.  A state therefore takes the n column products at its own offsets once: a column it holds is the
// rate of the move it pulls, a column it does not hold is a term of L (the forward rule of ls_tile_solve).  n products per
// state from LDS, no memory traffic for den and no third plane (carrying L would cost a plane of 8 B x 2^n written and read
// once per state, and the pushes to n - |x| successors).
//
// LDS of a workgroup of k_genodist_level: 3 x 8 KiB (the two values and the partial L of 2^10 states) + 16.5 KiB of rate
// tables + 2 KiB of patterns + the tile's factors = 42.8 KiB: three workgroups share a CU's 160 KiB.  256 threads, 4 states
// per thread in step 1: 12 accumulators.
// What -Rpass-analysis=kernel-resource-usage reports is under RESOURCES below.
//
// Summary.  mass[s] = sum_x P_s(x), pairs[s][i][j] = sum_x P_s(x) x_i x_j (marginals on the diagonal),
// burden[s][m] = sum over |x| = m of P_s(x).  k_genodist_tile (a workgroup per tile, every tile in one launch) forms per
// plane the GD_FEAT = 67 sums of its tile: mass, the c low-bit marginals, the low-low pair sums, the histogram by low
// popcount - a fold in LDS (gd_tile_fold, which metdist.h's k_metdist_tile calls too) in three stages (the low 5 bits in pieces of 8 offsets, the four pieces, the next 5 bits), every
// sum in ascending order.  k_genodist_summary (a workgroup per output) then adds the tiles' partials: a high bit of a tile
// is constant over the tile, so high-high = the sum over the tiles that hold both bits of the tile mass, high-low = the sum
// over the tiles that hold the high bit of the low marginal, burden is shifted by the popcount of the tile number.  Thread
// t adds the tiles t, t + 256, ... ascending, lattice.h's ls_block_sum adds the 256 threads.  No atomics; the partials are indexed by
// the tile number, not by the place in the list.  Longest chain of additions behind an output: 8 + 4 + 32 in the tile,
// ceil(tiles / 256) + 8 across tiles.
//
// Every shape depends on n alone: no byte of an output depends on the queries, the grid or an earlier call.  fp64 only.
//
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_genodist_level 56 VGPRs, 0 AGPRs, 50 SGPRs, scratch 0,
// LDS 43 848 B, 3 waves / SIMD (three workgroups a CU, by LDS; the registers would allow 8); k_genodist_tile<true> 36 VGPRs,
// 50 SGPRs, scratch 0, LDS 51 200 B, 3 waves / SIMD; k_genodist_tile<false> 18 VGPRs, 46 SGPRs, scratch 0, LDS 512 B;
// k_genodist_summary 12 VGPRs, 32 SGPRs, scratch 0, LDS 2 048 B.  lattice.h has the tables' and the gather's.
#pragma once
#include "lattice.h"

namespace mmhn {

constexpr int GD_PAIRS = LS_TILE_BITS * (LS_TILE_BITS - 1) / 2;           // low-low pairs of a tile
constexpr int GD_FEAT = 1 + LS_TILE_BITS + GD_PAIRS + LS_TILE_BITS + 1;   // partial sums of a tile and plane: mass, marginals, pairs, histogram
constexpr int GD_F_MARG = 1, GD_F_PAIR = 1 + LS_TILE_BITS, GD_F_HIST = GD_F_PAIR + GD_PAIRS;
constexpr int GD_ROW = (1 << LS_HALF) + 1;      // doubles of a row of 2^LS_HALF offsets in the fold (padded: no bank conflicts)
constexpr int GD_S1 = 11;                       // sums of a piece of 8 offsets: all, bits 0 1 2, pairs 01 02 12, popcounts 0 - 3
constexpr int GD_S2 = 1 + LS_HALF + LS_HALF * (LS_HALF - 1) / 2 + LS_HALF + 1;   // sums over the low 5 bits: 22
static_assert(LS_TILE_BITS == 10 && LS_HALF == 5 && LS_KB == 256, "the fold of k_genodist_tile is written for tiles of 5 + 5 bits and 256 threads");

// pair (i, j), i < j, at j (j - 1) / 2 + i
__host__ __device__ inline int gd_pair_index(int i, int j) { return j * (j - 1) / 2 + i; }
__host__ __device__ inline void gd_pair_of(int idx, int& i, int& j) {
  j = 1;
  while (j * (j + 1) / 2 <= idx) ++j;
  i = idx - j * (j - 1) / 2;
}

// the recursion of F0 / F1: G0 of a state before its F1, which takes G0 sigma of the same state
struct GenodistRecursion : LsRecursion {
  const LsTables& S;
  const double (&HF)[LS_COLS];
  int n;
  uint32_t T;
  double e1;
  __device__ __forceinline__ void source(uint32_t p, double (&f)[2]) const {
    if (T == 0u && p == 0u) f[0] = 1.0;         // F0 of the empty genotype
  }
  __device__ __forceinline__ void finish(uint32_t, uint32_t lo, uint32_t hi, double (&f)[2], const double (&L)[1]) const {
    const double sig = ls_rate(S, HF[n], n, lo, hi);
    const double kap = ls_rate(S, HF[n + 1], n + 1, lo, hi);
    const double g0 = f[0] / (L[0] + sig + kap);
    f[0] = g0;
    f[1] = (g0 * sig + f[1]) / (L[0] + kap * e1);
  }
};

// one level of tiles: workgroup b finishes the tile tiles[b]; every tile tiles[b] - bit is finished (earlier launches)
__global__ __launch_bounds__(LS_KB) void k_genodist_level(const LsTables* __restrict__ tabs, const uint32_t* __restrict__ tiles,
                                                          const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                          int N, int c, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];                // column j: exp(diagonal + the effects of the tile's high bits)
  __shared__ double W[3][1 << LS_TILE_BITS];    // 0 / 1: F0 / F1 of the tile's states (partial until a state is finished, then G), 2: its partial L
  const int n = N - 1;
  const uint32_t T = tiles[blockIdx.x];
  const long long plane = 1ll << n;
  ls_tile_prologue(S, HF, tabs, g_lt, g_o1, N, c, T);
  const double e1 = exp(g_o1[n]);               // kappa1 = kappa0 e1
  __syncthreads();
  ls_tile_solve<2, 1, true>(GenodistRecursion{{}, S, HF, n, T, e1}, S, HF, W, n, c, T, V, plane);
  ls_write_tile<2>(W, 1u << c, V, (long long)T << c, plane);
}

// the GD_FEAT partial sums of a tile's two planes to part[(s * GD_FEAT + f) * nt + T]: u / w hold the planes' values at the
// thread's offsets tid + s * LS_KB (0 past the tile); every thread of the workgroup calls it (k_genodist_tile and metdist.h's
// k_metdist_tile share this one copy)
__device__ __forceinline__ void gd_tile_fold(const double (&u)[LS_SPT], const double (&w)[LS_SPT], double* __restrict__ part,
                                             long long nt, uint32_t T) {
  const int tid = threadIdx.x;
  __shared__ double P[2][(1 << LS_HALF) * GD_ROW];   // the tile's two planes, offset (hi, lo) at hi * GD_ROW + lo; 0 past the tile
  __shared__ double Q[GD_S1][4][64];                 // stage 1: per piece of 8 offsets of a row
  __shared__ double R[GD_S2][64];                    // stage 2: per row (plane, hi): all, bit i, pair (i, j), popcount a of the low 5 bits
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    P[0][(p >> LS_HALF) * GD_ROW + (p & 31u)] = u[s];
    P[1][(p >> LS_HALF) * GD_ROW + (p & 31u)] = w[s];
  }
  __syncthreads();
  {
    const int row = tid & 63, piece = tid >> 6;
    const double* x = &P[row >> 5][(row & 31) * GD_ROW + piece * 8];
    double b = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, m01 = 0.0, m02 = 0.0, m12 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
      const double t = x[l];
      b += t;
      if (l & 1) m0 += t;
      if (l & 2) m1 += t;
      if (l & 4) m2 += t;
      if ((l & 3) == 3) m01 += t;
      if ((l & 5) == 5) m02 += t;
      if ((l & 6) == 6) m12 += t;
      const int pc = (l & 1) + ((l >> 1) & 1) + ((l >> 2) & 1);
      if (pc == 0) c0 += t; else if (pc == 1) c1 += t; else if (pc == 2) c2 += t; else c3 += t;
    }
    Q[0][piece][row] = b; Q[1][piece][row] = m0; Q[2][piece][row] = m1; Q[3][piece][row] = m2;
    Q[4][piece][row] = m01; Q[5][piece][row] = m02; Q[6][piece][row] = m12;
    Q[7][piece][row] = c0; Q[8][piece][row] = c1; Q[9][piece][row] = c2; Q[10][piece][row] = c3;
  }
  __syncthreads();
  // stage 2: the four pieces of a row, ascending.  The piece number is the bits 3, 4 of the offset.
  for (int it = tid; it < GD_S2 * 64; it += LS_KB) {
    const int k = it >> 6, row = it & 63;
    double r = 0.0;
    if (k < 1 + LS_HALF + LS_HALF * (LS_HALF - 1) / 2) {
      uint32_t bits = 0u;
      if (k >= 1 + LS_HALF) { int i, j; gd_pair_of(k - 1 - LS_HALF, i, j); bits = (1u << i) | (1u << j); }
      else if (k >= 1) bits = 1u << (k - 1);
      const uint32_t sl = bits & 7u, sh = bits >> 3;
      const int qi = sl == 0u ? 0 : sl == 1u ? 1 : sl == 2u ? 2 : sl == 4u ? 3 : sl == 3u ? 4 : sl == 5u ? 5 : 6;
      for (uint32_t piece = 0; piece < 4; ++piece)
        if ((piece & sh) == sh) r += Q[qi][piece][row];
    } else {
      const int a = k - (1 + LS_HALF + LS_HALF * (LS_HALF - 1) / 2);
      for (int piece = 0; piece < 4; ++piece) {
        const int d = a - __builtin_popcount(piece);
        if (d >= 0 && d <= 3) r += Q[7 + d][piece][row];
      }
    }
    R[k][row] = r;
  }
  __syncthreads();
  // stage 3: the 32 rows of a plane, ascending
  if (tid < 2 * GD_FEAT) {
    const int s = tid / GD_FEAT, f = tid % GD_FEAT;
    double r = 0.0;
    if (f < GD_F_HIST) {
      uint32_t bits = 0u;
      if (f >= GD_F_PAIR) { int i, j; gd_pair_of(f - GD_F_PAIR, i, j); bits = (1u << i) | (1u << j); }
      else if (f >= GD_F_MARG) bits = 1u << (f - GD_F_MARG);
      const uint32_t sl = bits & 31u, sh = bits >> LS_HALF;
      const int pc = __builtin_popcount(sl);
      const int k = pc == 0 ? 0 : pc == 1 ? 1 + __builtin_ctz(sl) : 1 + LS_HALF + gd_pair_index(__builtin_ctz(sl), 31 - __builtin_clz(sl));
      for (uint32_t hi = 0; hi < 32u; ++hi)
        if ((hi & sh) == sh) r += R[k][s * 32 + hi];
    } else {
      const int m = f - GD_F_HIST;
      for (int hi = 0; hi < 32; ++hi) {
        const int d = m - __builtin_popcount(hi);
        if (d >= 0 && d <= LS_HALF) r += R[1 + LS_HALF + LS_HALF * (LS_HALF - 1) / 2 + d][s * 32 + hi];
      }
    }
    part[((long long)s * GD_FEAT + f) * nt + T] = r;
  }
}

// every tile once all levels are finished (workgroup = tile number): G to U = kappa0 G0 and S = kappa1 G1 in place and,
// with SUMS, the GD_FEAT partial sums of the tile and plane at part[(s * GD_FEAT + f) * nt + T]
template <bool SUMS>
__global__ __launch_bounds__(LS_KB) void k_genodist_tile(const LsTables* __restrict__ tabs, const double* __restrict__ g_o1,
                                                         int N, int c, double* V, double* __restrict__ part, long long nt) {
  __shared__ double KL[1 << LS_HALF], KH[1 << LS_HALF];
  const LsColumn KC{KL, KH};                    // the clock
  const int tid = threadIdx.x, n = N - 1;
  const uint32_t T = blockIdx.x;
  const uint32_t Vt = 1u << c;
  const long long plane = 1ll << n, base = (long long)T << c;
  KC.load(tabs, n + 1);
  const double k0 = LsColumn::factor(g_o1, 0.0, c, T), e1 = exp(g_o1[n]);
  __syncthreads();
  double u[LS_SPT], w[LS_SPT];
#pragma unroll
  for (int s = 0; s < LS_SPT; ++s) {
    const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
    u[s] = w[s] = 0.0;
    if (p < Vt) {
      const double kap = KC.at(k0, p & 31u, p >> LS_HALF);
      double* o = V + base + p;
      u[s] = kap * o[0];
      w[s] = (kap * e1) * o[plane];
      o[0] = u[s]; o[plane] = w[s];
    }
  }
  if constexpr (SUMS) gd_tile_fold(u, w, part, nt, T);
}

// outputs of a plane's summary that k_genodist_summary forms: mass, the pairs i <= j, burden
inline int gd_summary_items(int n) { return 1 + n * (n + 1) / 2 + n + 1; }

// the summary from the tiles' partials: workgroup (s, q) forms one output of plane s - q = 0 mass, then the pairs i <= j at
// j (j + 1) / 2 + i (written to [i][j] and [j][i]), then burden[m].  out [2][1 + n * n + n + 1]
__global__ __launch_bounds__(LS_KB) void k_genodist_summary(const double* __restrict__ part, long long nt, int n, int c,
                                                            double* __restrict__ out) {
  __shared__ double red[LS_KB];
  const int tid = threadIdx.x;
  const int items = 1 + n * (n + 1) / 2 + n + 1, len = 1 + n * n + n + 1;
  const int s = blockIdx.x / items, q = blockIdx.x % items;
  const double* ps = part + (long long)s * GD_FEAT * nt;
  double acc = 0.0;
  int oi = -1, oj = -1;
  if (q < 1 + n * (n + 1) / 2) {
    uint32_t mask = 0u;                           // the tile-number bits a tile has to hold
    int col = 0;
    if (q > 0) {
      int idx = q - 1;
      oj = 0;
      while ((oj + 1) * (oj + 2) / 2 <= idx) ++oj;
      oi = idx - oj * (oj + 1) / 2;               // oi <= oj
      if (oj >= c) mask |= 1u << (oj - c);
      if (oi >= c) mask |= 1u << (oi - c);
      if (oi < c) col = (oj < c && oi != oj) ? GD_F_PAIR + gd_pair_index(oi, oj) : GD_F_MARG + oi;
    }
    const double* pc = ps + (long long)col * nt;
    for (long long T = tid; T < nt; T += LS_KB)
      if (((uint32_t)T & mask) == mask) acc += pc[T];
  } else {
    const int m = q - 1 - n * (n + 1) / 2;
    for (long long T = tid; T < nt; T += LS_KB) {
      const int d = m - __builtin_popcountll(T);
      if (d >= 0 && d <= c) acc += ps[(long long)(GD_F_HIST + d) * nt + T];
    }
  }
  const double sum = ls_block_sum(red, acc);
  if (tid == 0) {
    double* o = out + (long long)s * len;
    if (q == 0) o[0] = sum;
    else if (oi >= 0) { o[1 + oi * n + oj] = sum; o[1 + oj * n + oi] = sum; }
    else o[1 + n * n + (q - 1 - n * (n + 1) / 2)] = sum;
  }
}

}  // namespace mmhn
