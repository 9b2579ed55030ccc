// What the sweeps over all 2^n genotypes of a model share on the device (landscape.h backwards, genodist.h and metdist.h
// forwards): the tiling, the rate tables, a tile's prologue, the column rate, the write-out of a tile and the gather of
// the queried codes.  The recursions are the sweeps' own, one level kernel each.
//
// Tiling.  x is a genotype code (bit j = mutation j held).  The low c = min(n, LS_TILE_BITS) bits of a code are a TILE
// that one workgroup finishes in LDS, the high n - c bits name the tile.  A tile needs its neighbours along the high bits
// (T | bit backwards, T - bit forwards) and itself: one launch of the sweep's level kernel per popcount of the high bits,
// n - c + 1 launches, a workgroup per tile of the level through a host-built list of tile numbers sorted by popcount.
// Stream order alone orders the levels: no cooperative launch, no flags, no atomics.  Inside a tile thread t owns the low
// offsets t, t + 256, ... for the moves along the high bits - consecutive lanes read consecutive addresses of each plane -
// and orderpass.h's level walk (lanes dense on a level) runs the substitution over the low bits in LDS; the tile is
// written out once.  The planes are PLANAR in the workspace, value k of code x at V[k * 2^n + x].
//
// Rates in O(1), computed once per move and shared by a sweep's values: column j of a state (T, p) is
// HF[j] * TL[j][p & 31] * TH[j][p >> 5] - HF the factor of the tile's high bits and the diagonal, once per tile, TL / TH
// two tables over the low 5 and the next 5 bits (column n the seeding, n + 1 the clock).  TL, TH and the level walk's
// pattern table depend on the model alone: k_landscape_tables forms them once per call, a tile copies them (19 KiB, from
// L2).  As in forecast.h a product of three exponentials rounds differently from the exponential of the sum.  Column j
// does not read bit j (ls_eff), so the column of a held mutation is the rate of the move that added it.
//
// LS_TILE_BITS = 10: 8 KiB of LDS per plane of a tile, 16.5 KiB of rate tables, 2 KiB of patterns; a tile of 11 bits
// would leave a CU one workgroup of the five-plane sweeps and nothing to overlap its neighbour reads with, for 5 % less
// traffic at n = 28 (9.5 against 10 tile reads and writes per state on average).  256 threads, 4 states per thread along
// the high bits.
// RESOURCES (gfx950, -O3, -Rpass-analysis=kernel-resource-usage): k_landscape_tables 20 VGPRs, 98 SGPRs, scratch 0, LDS
// 2 100 B; k_lattice_gather<4> / <2> / <3> 18 / 10 / 14 VGPRs, 16 / 13 / 14 SGPRs, scratch 0, no LDS, 8 waves / SIMD.
#pragma once
#include "orderpass.h"

namespace mmhn {

constexpr int LS_TILE_BITS = 10;                // low bits of a code one workgroup finishes in LDS
constexpr int LS_KB = 256;                      // threads of a workgroup
constexpr int LS_SPT = (1 << LS_TILE_BITS) / LS_KB;   // states of a tile per thread along the high bits
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

// a tile's prologue, every thread of the workgroup: the tables to the kernel's LDS copy S and HF[j] = exp(diagonal + the
// effects of the high bits of tile T) for the N + 1 columns; without `clock` the clock's column is 0.  The caller
// synchronises.
__device__ __forceinline__ void ls_tile_prologue(LsTables& S, double (&HF)[LS_COLS], const LsTables* __restrict__ tabs,
                                                 const double* __restrict__ g_lt, const double* __restrict__ g_o1, int N,
                                                 int c, uint32_t T, bool clock = true) {
  const int tid = threadIdx.x, n = N - 1, cols = N + 1;
  for (int i = tid; i < (int)(sizeof(LsTables) / 4); i += LS_KB)
    reinterpret_cast<uint32_t*>(&S)[i] = reinterpret_cast<const uint32_t*>(tabs)[i];
  if (tid < cols) {
    const int j = tid;
    double v = j <= n ? g_lt[j * N + j] : 0.0;
    for (uint32_t m = T; m; m &= m - 1) v += ls_eff(g_lt, g_o1, N, j, c + __builtin_ctz(m));
    HF[j] = (j == n + 1 && !clock) ? 0.0 : exp(v);
  }
}

// column j's rate at the state of low offsets (lo, hi) of a tile whose factor of that column is hf (= HF[j])
__device__ __forceinline__ double ls_rate(const LsTables& S, double hf, int j, uint32_t lo, uint32_t hi) {
  return hf * S.TL[j][lo] * S.TH[j][hi];
}

// the first K planes of a finished tile of Vt states from LDS to V[k * plane + base + p], thread t the offsets t, t + 256, ...
template <int K, int P>
__device__ __forceinline__ void ls_write_tile(const double (&W)[P][1 << LS_TILE_BITS], uint32_t Vt, double* V, long long base,
                                              long long plane) {
  static_assert(K <= P, "W holds the planes written");
  for (uint32_t p = threadIdx.x; p < Vt; p += LS_KB) {
    double* o = V + base + p;
#pragma unroll
    for (int k = 0; k < K; ++k) o[k * plane] = W[k][p];
  }
}

// the K values at the queried codes: out[i][k] = V[k][codes[i]]
template <int K>
__global__ __launch_bounds__(LS_KB) void k_lattice_gather(const uint32_t* __restrict__ codes, long long R,
                                                          const double* __restrict__ V, int n, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * LS_KB + threadIdx.x;
  if (i >= R) return;
  const long long plane = 1ll << n, x = codes[i];
#pragma unroll
  for (int k = 0; k < K; ++k) out[K * i + k] = V[k * plane + x];
}

}  // namespace mmhn
