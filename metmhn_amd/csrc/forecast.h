// Seeding forecasts from a tumour's genotype: the device form of metmhn_amd/model.py MetMHN.seeding_forecast.
//
// From a genotype x that has not seeded, the primary tumour's chain before the seeding (or the clock of the first
// observation) is an absorbing chain on the supersets y of x: a lattice over the f FREE events of the row (bit b = the
// b-th mutation x does not hold, ascending), not over the held ones as the order kernels' lattices.
//   r_j(y) = exp(base_j + sum over the bits i of y, i != j, of theta[j, i])     base_j = theta[j, j] + the held events' effects
//            j not in y: the rate lambda_j(y) of the move y -> y + j;  j in y: lambda_j(y - j), the rate of the move INTO y
//   sigma(y), kappa(y)   the same sum-products for the seeding (row n of theta) and the clock (obs1; 0 for "until seeding")
//   den(y) = sum over j not in y of r_j(y) + sigma(y) + kappa(y)
//   F(x) = 1,  F(y) = sum over b in y of G(y - b) r_b(y),   G(y) = F(y) / den(y)    (occupancy / den: the expected time in y)
// Outputs (a row's block of fc_block(f) doubles): [0] p_seed = sum G sigma, [1] time = sum G, [2 + j] before[j] = sum over
// y without j of G r_j, [2 + f + j] with_seed[j] = sum over y with j of G sigma, [2 + 2f + m] n_before[m] = sum over |y| = m
// of G sigma.  Every sum runs over its terms in ascending bit.
//
// Shape.  A row spreads over the whole GPU: ONE launch of k_forecast_level per level (popcount) covers that level of every
// row of the batch, so the levels are ordered by kernel boundaries alone - no cooperative launch, no flags, no atomics.  A
// lattice holds one double per state (G).  The walk is orderpass.h's: chunks of 2^c consecutive indices (c = min(f, 10)),
// the chunk's high bits wave-uniform, the lanes dense on the level through the popcount-sorted pattern table.  A workgroup
// takes one TILE of a row, 2^tb consecutive chunks (tb = min(f - c, 4): fixed by the row, not by the grid), through the
// host-built map (row, tile); a tile whose high bits cannot reach the level exits at once.
//
// Rates in O(1) per entry: r_j(y) = HF[chunk][j] * TL[j][low 5 pattern bits] * TH[j][high 5 pattern bits] - a factor of
// the chunk's high bits, once per chunk, and two LDS tables of 32 entries per column (column f the seeding, f + 1 the clock).
// A product of three exponentials rounds differently from the exponential of the sum: each factor carries its own
// rounding, the bound of tests/test_seeding_forecasts.py allows for it.
//
// A state is finished in one visit: pull F from the |y| predecessors' G, form den, write G, add the state's terms to the
// thread's partials (2f + 2 registers; the level's n_before entry is the level's share of p_seed).  Reduction: lanes by
// opo_wave_sum, the four waves in order, then the tile's block of partials in the row's workspace: written whole on the
// tile's first level (popcount of its high bits, which every tile has), added to on the later ones.  k_forecast_reduce adds
// the tiles of a row up, thread t the tiles t, t + 256, ..., then the same wave and workgroup sums.  Every shape is fixed
// by f alone, so a row's bits do not depend on the batch, the other rows or the grid.
//
// S, the longest chain of additions behind an output: a thread adds at most 4 chunks x 4 states per level, + 6 (wave) + 3
// (waves) + 1 (tile block) = 26 per level, at most tb + c + 1 = 15 levels per tile: 390; the reduction adds at most
// 2^(f - 14) / 256 <= 256 tiles per thread + 6 + 3 = 265.  S <= 655 for every f <= 30, S <= 400 for f <= 22.  fp64 only.
#pragma once
#include "orderpass.h"

namespace mmhn {

constexpr int FC_KB = 256;                      // threads of a workgroup, both kernels
constexpr int FC_TB = 4;                        // chunk bits of a tile at most
constexpr int FC_COLS = 32;                     // columns of the rate tables: f <= MAXK free events, the seeding, the clock
constexpr int FC_HALF = 5;                      // pattern bits of the low table
static_assert(MAXK + 2 <= FC_COLS, "the rate tables hold a column per free event, the seeding and the clock");
static_assert(2 * FC_HALF >= OPO_CB, "two tables of 2^FC_HALF entries cover a chunk's pattern bits");

struct FRow {
  long long goff;                               // the row's lattice G in the workspace (doubles)
  long long poff;                               // its tiles' blocks of partials
  long long ooff;                               // its block of the batch's output
  int f, c, tb, until;                          // free events, chunk bits, tile bits; 1: the clock runs
  int tiles, row;
  int8_t ev[32];                                // the free events, ascending: lattice bit b is event ev[b]
  double base[FC_COLS];                         // column j < f: theta[j, j] + the held events' effects; f the seeding, f + 1 the clock
};

__host__ __device__ inline int fc_block(int f) { return 3 * f + 3; }
inline int fc_chunk_bits(int f) { return opo_chunk_bits(f, 64); }
inline int fc_tile_bits(int f) { const int c = fc_chunk_bits(f); return f - c < FC_TB ? f - c : FC_TB; }
// workspace of a row in doubles: the lattice and the tiles' partials
inline long long fc_doubles(int f) {
  const int c = fc_chunk_bits(f), tb = fc_tile_bits(f);
  return (1ll << f) + (1ll << (f - c - tb)) * fc_block(f);
}

// level `lev` of every row of the batch: workgroup b takes the tile map[b] = (row, tile)
__global__ __launch_bounds__(FC_KB) void k_forecast_level(const FRow* __restrict__ rows, const int2* __restrict__ map,
                                                          const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                          int N, int lev, double* ws) {
  __shared__ OpoLevels L;
  __shared__ double eff[FC_COLS][32];           // eff[j][b]: what bit b adds to column j's exponent
  __shared__ double TL[FC_COLS][32], TH[FC_COLS][32];
  __shared__ double HF[1 << FC_TB][FC_COLS];    // per chunk of the tile
  __shared__ double red[FC_KB / 64][2 * MAXK + 2];
  const int tid = threadIdx.x;
  const int2 m = map[blockIdx.x];
  const FRow& r = rows[m.x];
  const int f = r.f, c = r.c, tb = r.tb;
  const uint32_t tlo = (uint32_t)m.y << tb, thi = tlo + (1u << tb);
  const int first = __builtin_popcount((uint32_t)m.y);
  if (lev < first || lev > first + tb + c) return;      // the tile's high bits cannot reach the level
  const bool clock = r.until != 0;
  const int n = N - 1, cols = f + 2;
  opo_levels_init<FC_KB>(L, c);
  for (int i = tid; i < FC_COLS * 32; i += FC_KB) {
    const int j = i >> 5, b = i & 31;
    double v = 0.0;
    if (b < f) {
      if (j < f) v = b == j ? 0.0 : g_lt[(int)r.ev[j] * N + (int)r.ev[b]];
      else if (j == f) v = g_lt[n * N + (int)r.ev[b]];
      else if (j == f + 1) v = g_o1[(int)r.ev[b]];
    }
    eff[j][b] = v;
  }
  __syncthreads();
  for (int i = tid; i < FC_COLS * 32; i += FC_KB) {
    const int j = i >> 5, p = i & 31;
    double sl = 0.0, sh = 0.0;
    for (int b = 0; b < FC_HALF; ++b)
      if ((p >> b) & 1) {
        if (b < c) sl += eff[j][b];
        if (b + FC_HALF < c) sh += eff[j][b + FC_HALF];
      }
    TL[j][p] = exp(sl); TH[j][p] = exp(sh);
  }
  for (int i = tid; i < (1 << tb) * FC_COLS; i += FC_KB) {
    const int s = i >> 5, j = i & 31;
    const uint32_t h = tlo + (uint32_t)s;
    double e = 0.0;
    if (j < cols) {
      double v = r.base[j];
      for (uint32_t mm = h; mm; mm &= mm - 1) v += eff[j][c + __builtin_ctz(mm)];
      e = (j == f + 1 && !clock) ? 0.0 : exp(v);
    }
    HF[s][j] = e;
  }
  __syncthreads();

  double* G = ws + opr_uniform(r.goff);
  double ab[MAXK], aw[MAXK], a_seed = 0.0, a_time = 0.0;
#pragma unroll
  for (int j = 0; j < MAXK; ++j) { ab[j] = 0.0; aw[j] = 0.0; }
  const uint32_t pmask = (1u << c) - 1u;
  opo_level<FC_KB>(L, tlo, thi, lev, [&](uint32_t y) {
    const uint32_t s = (y >> c) - tlo, p = y & pmask, lo = p & 31u, hi = p >> FC_HALF;
    double rj[MAXK], F = 0.0, den = 0.0;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      if (j < f) {
        const double v = HF[s][j] * TL[j][lo] * TH[j][hi];
        rj[j] = v;
        if ((y >> j) & 1u) F += G[y ^ (1u << j)] * v;
        else den += v;
      }
    }
    if (lev == 0) F = 1.0;
    const double sig = HF[s][f] * TL[f][lo] * TH[f][hi];
    den += sig;
    if (clock) den += HF[s][f + 1] * TL[f + 1][lo] * TH[f + 1][hi];
    const double g = F / den, gs = g * sig;
    G[y] = g;
    a_seed += gs;
    a_time += g;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      if (j < f) {
        if ((y >> j) & 1u) aw[j] += gs;
        else ab[j] += g * rj[j];
      }
    }
  });

  // lanes, then waves, then the tile's block
  const int wave = tid >> 6, lane = tid & 63;
  {
    const double s0 = opo_wave_sum(a_seed), s1 = opo_wave_sum(a_time);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; }
  }
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    if (j < f) {
      const double sb = opo_wave_sum(ab[j]), sw = opo_wave_sum(aw[j]);
      if (lane == 0) { red[wave][2 + j] = sb; red[wave][2 + f + j] = sw; }
    }
  }
  __syncthreads();
  const int PS = fc_block(f);
  double* P = ws + opr_uniform(r.poff) + (long long)m.y * PS;
  auto waves = [&](int q) { return ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q]; };
  for (int q = tid; q < PS; q += FC_KB) {
    const int slot = q - (2 + 2 * f);           // >= 0: n_before's entry of level `slot`, the level's share of p_seed
    if (slot >= 0) {
      if (slot == lev) P[q] = waves(0);
      else if (lev == first) P[q] = 0.0;
    } else {
      P[q] = lev == first ? waves(q) : P[q] + waves(q);
    }
  }
}

// the tiles of rows[blockIdx.x] added up into its block of `out`
__global__ __launch_bounds__(FC_KB) void k_forecast_reduce(const FRow* __restrict__ rows, const double* __restrict__ ws,
                                                           double* __restrict__ out) {
  __shared__ double red[FC_KB / 64];
  const FRow& r = rows[blockIdx.x];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int PS = fc_block(r.f), tiles = r.tiles;
  const double* P = ws + opr_uniform(r.poff);
  double* O = out + opr_uniform(r.ooff);
  for (int q = 0; q < PS; ++q) {
    double s = 0.0;
    for (int t = tid; t < tiles; t += FC_KB) s += P[(long long)t * PS + q];
    s = opo_wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) O[q] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

}  // namespace mmhn
