// Seeding landscape: the four forecast scalars of EVERY genotype of a model in one backward sweep over the full lattice -
// the value functions behind metmhn_amd/model.py MetMHN.seeding_landscape (forecast.h answers the same question forwards,
// one genotype at a time, and shares no code with this file).
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
// Layout.  PLANAR: four vectors of 2^n doubles in the workspace, value k of code x at V[k * 2^n + x] - the layout of the
// entry point's `full` output, so that is one copy.
//
// Shape.  The low c = min(n, LS_TILE_BITS) bits of a code are a TILE that one workgroup finishes in LDS, the high n - c
// bits name the tile.  Tile T needs the tiles T | bit and itself: one launch of k_landscape_level per popcount of the
// high bits, descending, n - c + 1 launches, a workgroup per tile of the level through a host-built list of tile numbers
// sorted by popcount.  Stream order alone orders the levels: no cooperative launch, no flags, no atomics.  Inside a tile
//   1. the moves along the high bits, ascending: thread t owns the low offsets t, t + 256, ... and adds lambda_j(x) v(x + j)
//      for every high bit j not in T, v read from the finished tile T | j at the same offset - consecutive lanes read
//      consecutive addresses of each plane; the partial sums and the partial den go to LDS;
//   2. the backward substitution over the low bits in LDS, by popcount of the low part, descending, with orderpass.h's level
//      walk (lanes dense on a level), the low moves added in ascending bit; the tile is written out once.
// So a state's sums run over the high bits ascending, then the low bits ascending.
//
// Rates in O(1), computed once per move and shared by the four values: column j of a state (T, p) is
// HF[j] * TL[j][p & 31] * TH[j][p >> 5] - HF the factor of the tile's high bits and the diagonal, once per tile, TL / TH
// two tables over the low 5 and the next 5 bits (column n the seeding, n + 1 the clock).  TL, TH and the level walk's
// pattern table depend on the model alone: k_landscape_tables forms them once per call, a tile copies them (19 KiB, from
// L2).  As in forecast.h a product of three exponentials rounds differently from the exponential of the sum.
//
// LS_TILE_BITS = 10.  LDS of a workgroup: 5 x 8 KiB (four values and the partial den of 2^10 states) + 16.5 KiB of rate
// tables + 2 KiB of patterns + the tile's factors = 58.8 KiB, so two workgroups share a CU's 160 KiB and one streams its
// neighbour tiles while the other solves on the chip; a tile of 11 bits (105 KiB) would leave a CU one workgroup and
// nothing to overlap with, for 5 % less traffic at n = 28 (9.5 against 10 tile reads and writes per state on average).
// 256 threads, 4 states per thread in step 1: 20 accumulators (40 VGPRs); a rate lives for one move, not n of them.
// -Rpass-analysis=kernel-resource-usage (gfx950, -O3): k_landscape_level 66 VGPRs, 0 AGPRs, 56 SGPRs, scratch 0, LDS
// 60 232 B, 2 waves / SIMD (two workgroups a CU, by LDS; the registers would allow 7); k_landscape_tables 20 VGPRs,
// scratch 0, LDS 2 100 B; k_landscape_gather 18 VGPRs, scratch 0.
//
// Every shape depends on n alone: a genotype's four values do not depend on the queries, the grid or an earlier call.
// fp64 only.
#pragma once
#include "orderpass.h"

namespace mmhn {

constexpr int LS_TILE_BITS = 10;                // low bits of a code one workgroup finishes in LDS
constexpr int LS_KB = 256;                      // threads of a workgroup
constexpr int LS_SPT = (1 << LS_TILE_BITS) / LS_KB;   // states of a tile per thread in step 1
constexpr int LS_COLS = ORD_MAXN + 1;           // columns of the rate tables: n <= 31 mutations, the seeding, the clock
constexpr int LS_HALF = 5;                      // low bits of the table TL; TH takes the rest of the tile
static_assert(2 * LS_HALF >= LS_TILE_BITS, "two tables of 2^LS_HALF entries cover a tile's bits");
static_assert(LS_TILE_BITS <= 16, "the level walk's patterns are 16 bits wide");

struct LsTables {
  double TL[LS_COLS][1 << LS_HALF], TH[LS_COLS][1 << LS_HALF];
  OpoLevels L;                                  // the level walk over the c bits of a tile
};
static_assert(sizeof(LsTables) % 4 == 0, "copied word by word");

inline int ls_tile_bits(int n) { return n < LS_TILE_BITS ? n : LS_TILE_BITS; }

// what bit i adds to the exponent of column j (j < n a mutation, n the seeding, n + 1 the clock)
__device__ __forceinline__ double ls_eff(const double* __restrict__ g_lt, const double* __restrict__ g_o1, int N, int j, int i) {
  const int n = N - 1;
  if (j <= n) return i == j ? 0.0 : g_lt[j * N + i];
  return g_o1[i];
}

// the tables of a model with tiles of c bits (one workgroup)
__global__ __launch_bounds__(LS_KB) void k_landscape_tables(const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                            int N, int c, LsTables* __restrict__ out) {
  __shared__ OpoLevels L;
  const int tid = threadIdx.x, cols = N + 1;
  opo_levels_init<LS_KB>(L, opo_chunk_bits(c, LS_KB));
  for (int i = tid; i < (int)(sizeof(OpoLevels) / 4); i += LS_KB)
    reinterpret_cast<uint32_t*>(&out->L)[i] = reinterpret_cast<const uint32_t*>(&L)[i];
  for (int i = tid; i < LS_COLS << LS_HALF; i += LS_KB) {
    const int j = i >> LS_HALF, p = i & ((1 << LS_HALF) - 1);
    double sl = 0.0, sh = 0.0;
    if (j < cols)
      for (int b = 0; b < LS_HALF; ++b)
        if ((p >> b) & 1) {
          if (b < c) sl += ls_eff(g_lt, g_o1, N, j, b);
          if (b + LS_HALF < c) sh += ls_eff(g_lt, g_o1, N, j, b + LS_HALF);
        }
    out->TL[j][p] = exp(sl); out->TH[j][p] = exp(sh);
  }
}

// one level of tiles: workgroup b finishes the tile tiles[b]; every tile tiles[b] | bit is finished (earlier launches)
__global__ __launch_bounds__(LS_KB) void k_landscape_level(const LsTables* __restrict__ tabs, const uint32_t* __restrict__ tiles,
                                                           const double* __restrict__ g_lt, const double* __restrict__ g_o1,
                                                           int N, int c, int clock, double* V) {
  __shared__ LsTables S;
  __shared__ double HF[LS_COLS];                // column j: exp(diagonal + the effects of the tile's high bits)
  __shared__ double W[5][1 << LS_TILE_BITS];    // the four values of the tile's states (partial sums until a state is finished), 4: its partial den
  const int tid = threadIdx.x, n = N - 1, cols = N + 1;
  const uint32_t T = tiles[blockIdx.x];
  const uint32_t Vt = 1u << c;
  const long long plane = 1ll << n, base = (long long)T << c;
  for (int i = tid; i < (int)(sizeof(LsTables) / 4); i += LS_KB)
    reinterpret_cast<uint32_t*>(&S)[i] = reinterpret_cast<const uint32_t*>(tabs)[i];
  if (tid < cols) {
    const int j = tid;
    double v = j <= n ? g_lt[j * N + j] : 0.0;
    for (uint32_t m = T; m; m &= m - 1) v += ls_eff(g_lt, g_o1, N, j, c + __builtin_ctz(m));
    HF[j] = (j == n + 1 && !clock) ? 0.0 : exp(v);
  }
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
          const double r = hf * S.TL[j][p & 31u] * S.TH[j][p >> LS_HALF];
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
          const double r = HF[j] * S.TL[j][lo] * S.TH[j][hi];
          const uint32_t y = p | (1u << j);
          const double v0 = W[0][y];
          n0 += r * v0;
          n1 += r * W[1][y];
          n2 += r * (1.0 + W[2][y]);
          n3 += r * (v0 + W[3][y]);
          den += r;
        }
      }
      const double sig = HF[n] * S.TL[n][lo] * S.TH[n][hi];
      den += sig;
      if (clock) den += HF[n + 1] * S.TL[n + 1][lo] * S.TH[n + 1][hi];
      W[0][p] = (sig + n0) / den;
      W[1][p] = (1.0 + n1) / den;
      W[2][p] = n2 / den;
      W[3][p] = n3 / den;
    });
    __syncthreads();
  }
  for (uint32_t p = tid; p < Vt; p += LS_KB) {
    double* o = V + base + p;
    o[0] = W[0][p]; o[plane] = W[1][p]; o[2 * plane] = W[2][p]; o[3 * plane] = W[3][p];
  }
}

// the four values at the queried codes: out[i][k] = V[k][codes[i]]
__global__ __launch_bounds__(LS_KB) void k_landscape_gather(const uint32_t* __restrict__ codes, long long R,
                                                            const double* __restrict__ V, int n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * LS_KB + threadIdx.x;
  if (i >= R) return;
  const long long plane = 1ll << n, x = codes[i];
#pragma unroll
  for (int k = 0; k < 4; ++k) out[4 * i + k] = V[k * plane + x];
}

}  // namespace mmhn
