// What the sweeps over all 2^n genotypes of a model share on the device (landscape.h backwards, genodist.h and metdist.h
// forwards, partner.h both ways): the tiling, the rate tables, a tile's prologue, the column rate, THE SOLVE OF A TILE
// (ls_tile_solve, the one skeleton of the level kernels but landscape.h's, which says why), a column outside the prologue (LsColumn), the block sum, the
// write-out of a tile and the gather of the queried codes.  A sweep's own are its recursion - a struct of hooks that
// ls_tile_solve calls, documented there - and its level kernel: prologue, solve, write-out.
//
// Tiling.  x is a genotype code (bit j = mutation j held).  The low c = min(n, LS_TILE_BITS) bits of a code are a TILE
// that one workgroup finishes in LDS, the high n - c bits name the tile.  A tile needs its neighbours along the high bits
// (T | bit backwards, T - bit forwards) and itself: one launch of the sweep's level kernel per popcount of the high bits,
// n - c + 1 launches, a workgroup per tile of the level through a host-built list of tile numbers sorted by popcount.
// Stream order alone orders the levels: no cooperative launch, no flags, no atomics.  Inside a tile ls_tile_solve takes
// the moves along the high bits, then the substitution over the low bits in LDS; the tile is written out once.  The
// planes are PLANAR in the workspace, value k of code x at V[k * 2^n + x].
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

// exp(theta[j][n]) per mutation j - the factor the seeding puts on rate j, mu_j = lambda_j EM[j] - or 1 where `on` is false
// (every thread; the caller synchronises; entries j >= n are 1 and no column reads them)
__device__ __forceinline__ void ls_seeded_factors(double (&EM)[ORD_MAXN + 1], const double* __restrict__ g_lt, int N, bool on) {
  const int tid = threadIdx.x, n = N - 1;
  if (tid <= ORD_MAXN) EM[tid] = (tid < n && on) ? exp(g_lt[tid * N + n]) : 1.0;
}

// One column of a set of tables for a kernel that does not take the whole prologue: its two 32-entry tables in two LDS
// arrays of the kernel, and a tile's factor of it.  factor x L[lo] x H[hi] are ls_rate's bytes for the same column, tile
// and vector
struct LsColumn {
  double (&L)[1 << LS_HALF], (&H)[1 << LS_HALF];
  // every thread; the caller synchronises
  __device__ __forceinline__ void load(const LsTables* __restrict__ tabs, int col) const {
    const int tid = threadIdx.x;
    if (tid < (1 << LS_HALF)) { L[tid] = tabs->TL[col][tid]; H[tid] = tabs->TH[col][tid]; }
  }
  // exp(v + the entries of vec at the high bits of tile T): vec a row of theta or an obs vector, v the diagonal or obs[n] or 0
  static __device__ __forceinline__ double factor(const double* __restrict__ vec, double v, int c, uint32_t T) {
    for (uint32_t m = T; m; m &= m - 1) v += vec[c + __builtin_ctz(m)];
    return exp(v);
  }
  __device__ __forceinline__ double at(double f, uint32_t lo, uint32_t hi) const { return f * L[lo] * H[hi]; }
};

// The solve of one tile, the skeleton of the level kernels: between the prologue's barrier and the write-out.
//   1. the moves along the high bits j = c .. n - 1, ascending: thread t owns the low offsets t, t + 256, ... and holds K
//      partial values and D partial dens of each in registers.  FORWARD: a bit T holds is a move pulled from the finished
//      tile T - bit at the same offset, a free one a term of den.  Backward: a held bit is skipped, a free one is a term
//      of den and, where rec.pulls(j), pulled from the finished tile T | bit.  Consecutive lanes read consecutive
//      addresses of plane k at nb + k * stride.  The partials go to W[0 .. K) and W[K .. K + D); a barrier.
//   2. the substitution over the low bits in LDS with orderpass.h's level walk, by popcount of the low part, ascending
//      when FORWARD and descending otherwise, the same rule per low bit with the neighbour read from W; lanes dense on a
//      level, ONE barrier per level.  On return W[0 .. K) holds the tile's finished values; the kernel writes them out.
// A state's sums so run over the high bits ascending, then the low bits ascending, one `a += rate * v` per move.
//
// rec is the sweep's recursion (LsRecursion has what most of them share):
//   column(j)          what rates needs of column j besides r, fetched once per column in step 1
//   rates(r, col, rt)  the D rates of a move from r = ls_rate(column j at the state): one per den, and what move scales by
//   move(f, rt, v)     adds a neighbour's K values v to the K partial values f
//   pulls(j)           backward only: whether the move along free bit j is pulled (it is a term of den either way)
//   source(p, f)       what the state of low offset p starts from, f zeroed before; whatever it loads it guards itself
//   live(p)            false: the state is outside the sweep's sub-lattice, its values are an exact 0 and nothing is read
//   finish(p, lo, hi, f, L)   the state's values from its sums f and dens L, in place in f
template <int K, int D, bool FORWARD, class Rec>
__device__ __forceinline__ void ls_tile_solve(const Rec& rec, const LsTables& S, const double (&HF)[LS_COLS],
                                              double (&W)[K + D][1 << LS_TILE_BITS], int n, int c, uint32_t T,
                                              const double* nb, long long stride) {
  const int tid = threadIdx.x;
  const uint32_t Vt = 1u << c;
  const long long base = (long long)T << c;
  {
    double f[LS_SPT][K], L[LS_SPT][D];
#pragma unroll
    for (int s = 0; s < LS_SPT; ++s) {
      const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
#pragma unroll
      for (int k = 0; k < K; ++k) f[s][k] = 0.0;
#pragma unroll
      for (int d = 0; d < D; ++d) L[s][d] = 0.0;
      if (p < Vt) rec.source(p, f[s]);
    }
    for (int j = c; j < n; ++j) {
      const bool held = (T >> (j - c)) & 1u;
      if (!FORWARD && held) continue;
      const bool pull = FORWARD ? held : rec.pulls(j);
      const double hf = HF[j];
      const auto col = rec.column(j);
      const double* q[K];                         // the neighbour tile's planes: uniform bases, a lane adds its 32-bit offset
#pragma unroll
      for (int k = 0; k < K; ++k) q[k] = (pull ? nb + base + (FORWARD ? -(1ll << j) : (1ll << j)) : nb) + k * stride;
#pragma unroll
      for (int s = 0; s < LS_SPT; ++s) {
        const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
        if (p < Vt) {
          double rt[D];
          rec.rates(ls_rate(S, hf, j, p & 31u, p >> LS_HALF), col, rt);
          if (pull) {
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = q[k][p];
            rec.move(f[s], rt, v);
          }
          if (!(FORWARD && held)) {
#pragma unroll
            for (int d = 0; d < D; ++d) L[s][d] += rt[d];
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < LS_SPT; ++s) {
      const uint32_t p = (uint32_t)tid + (uint32_t)s * LS_KB;
      if (p < Vt) {
#pragma unroll
        for (int k = 0; k < K; ++k) W[k][p] = f[s][k];
#pragma unroll
        for (int d = 0; d < D; ++d) W[K + d][p] = L[s][d];
      }
    }
  }
  __syncthreads();

  const uint32_t chunks = Vt >> S.L.c;
  for (int i = 0; i <= c; ++i) {
    opo_level<LS_KB>(S.L, 0u, chunks, FORWARD ? i : c - i, [&](uint32_t p) {
      if (!rec.live(p)) {
#pragma unroll
        for (int k = 0; k < K; ++k) W[k][p] = 0.0;
        return;
      }
      const uint32_t lo = p & 31u, hi = p >> LS_HALF;
      double f[K], L[D];
#pragma unroll
      for (int k = 0; k < K; ++k) f[k] = W[k][p];
#pragma unroll
      for (int d = 0; d < D; ++d) L[d] = W[K + d][p];
#pragma unroll
      for (int j = 0; j < LS_TILE_BITS; ++j) {
        const bool held = (p >> j) & 1u;
        if (j < c && (FORWARD || !held)) {
          double rt[D];
          rec.rates(ls_rate(S, HF[j], j, lo, hi), rec.column(j), rt);
          if (FORWARD ? held : rec.pulls(j)) {
            const uint32_t y = p ^ (1u << j);
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = W[k][y];
            rec.move(f, rt, v);
          }
          if (!(FORWARD && held)) {
#pragma unroll
            for (int d = 0; d < D; ++d) L[d] += rt[d];
          }
        }
      }
      rec.finish(p, lo, hi, f, L);
#pragma unroll
      for (int k = 0; k < K; ++k) W[k][p] = f[k];
    });
    __syncthreads();
  }
}

// the hooks most recursions share: the one rate r itself, every free bit pulled, no source, every state live, and
// `a += rate * v` per plane
struct LsRecursion {
  __device__ __forceinline__ int column(int) const { return 0; }
  __device__ __forceinline__ void rates(double r, int, double (&rt)[1]) const { rt[0] = r; }
  template <int K>
  __device__ __forceinline__ void move(double (&f)[K], const double (&rt)[1], const double (&v)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k) f[k] += rt[0] * v[k];
  }
  __device__ __forceinline__ bool pulls(int) const { return true; }
  template <int K>
  __device__ __forceinline__ void source(uint32_t, double (&)[K]) const {}
  __device__ __forceinline__ bool live(uint32_t) const { return true; }
};

// the sum of v over the workgroup's 256 threads through the caller's LDS, the same tree on every run (every thread)
__device__ __forceinline__ double ls_block_sum(double (&red)[LS_KB], double v) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int d = LS_KB / 2; d; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  return red[0];
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
