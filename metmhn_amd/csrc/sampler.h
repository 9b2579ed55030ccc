// Gillespie sampler of the joint PT/MT process (metmhn/simulations.py:8-147).
//
// One thread simulates one patient: both tumours evolve together until seeding, independently afterwards, until
// both are diagnosed or the primary is diagnosed before seeding (`stop_fun`, simulations.py:58-62).  The state is
// two bit sets (events 0..N-2 mutations, N-1 seeding, N diagnosis) and the event rates are recomputed from the
// log-parameters in LDS every step exactly as the reference does (exp of a sum of logs, `tumor_dynamics`
// :28-44); the next event is drawn by inverting the cumulative rates with one uniform per step.
// Random numbers: Philox4x32-10, key = (seed low word, seed high word), counter = (trajectory low word, trajectory
// high word, step, 0); the step's uniform is the top 27 bits of output word 0 and the top 26 of word 1 as a 53-bit
// fraction.  A trajectory depends on (seed, its index) only, not on n_sim or the launch geometry.  The stream differs
// from jax.random's threefry, the distribution does not (tests/test_montecarlo.py); tests/test_sampler_replay.py
// replays this stream and gillespie_step in NumPy (oracle/sampler_replay.py) and compares every trajectory exactly.
// k_gillespie writes every trajectory (mmhn_simulate); k_gillespie_summary draws the same ones through the same step
// function and only counts them (mmhn_simulate_summary, the layout is above the kernel); k_gillespie_pairs counts their
// pairwise co-occurrences and mutation burdens (mmhn_simulate_pairs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmhn {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr int SIM_BLOCK = 256;
constexpr int SIM_MAXN = 32;                     // events incl. seeding

// log_theta [N][N] row-major (row i: effects ON event i), pt_d / mt_d [N] -> the LDS copies every sampler kernel reads.
__device__ __forceinline__ void gillespie_load(const double* __restrict__ log_theta, const double* __restrict__ pt_d,
                                               const double* __restrict__ mt_d, int N, double* lt, double* ltp,
                                               double* dp, double* dm) {
  for (int e = threadIdx.x; e < N * N; e += SIM_BLOCK) {
    const int i = e / N, j = e % N;
    const double v = log_theta[e];
    lt[e] = v;
    ltp[e] = (j == N - 1 && i < N - 1) ? 0.0 : v;        // seeding does not act on the PT's mutations (:67-68)
  }
  for (int e = threadIdx.x; e < N; e += SIM_BLOCK) { dp[e] = pt_d[e]; dm[e] = mt_d[e]; }
}

// The trajectory has ended: both tumours diagnosed, or the PT diagnosed before seeding (`stop_fun`, :58-62).
__device__ __forceinline__ bool gillespie_done(uint32_t pt, uint32_t mt, int N) {
  const uint32_t sbit = 1u << (N - 1), dbit = 1u << N;
  return (pt & dbit) && ((mt & dbit) || !(pt & sbit));
}

// One step of trajectory `id`: the event rates from the state (`tumor_dynamics`, :28-44), the draw from Philox
// counter (id, step, 0) under `seed`, and the state update.  pt / mt: bits 0..N-1 events (N-1 = seeding), bit N =
// diagnosed; t_pt / t_mt: the step of each tumour's diagnosis.  Returns the event as simulate_orders numbers it.
__device__ __forceinline__ int gillespie_step(const double* lt, const double* ltp, const double* dp, const double* dm,
                                              int N, long long id, int step, uint64_t seed, uint32_t& pt,
                                              uint32_t& mt, int& t_pt, int& t_mt) {
  const uint32_t sbit = 1u << (N - 1), dbit = 1u << N, evmask = dbit - 1u;
  const bool pt_on = !(pt & dbit);
  const bool mt_on = (pt & sbit) && !(mt & dbit);
  // event e of tumour T: 0..N-1 mutations / seeding, N diagnosis; index in the reference's vector: e (+ N+1 for MT)
  auto rate = [&](int tum, int e) -> double {
    const uint32_t st = tum == 0 ? pt : mt;
    if (tum == 0 ? !pt_on : !mt_on) return 0.0;
    if ((st >> e) & 1u) return 0.0;
    double s = 0.0;
    if (e < N) {
      const double* row = (tum == 0 ? ltp : lt) + e * N;
      s = row[e];                                           // b_rates = diag(log_theta)
      for (uint32_t m = st & evmask; m; m &= m - 1) s += row[__ffs(m) - 1];
    } else {
      const double* dv = tum == 0 ? dp : dm;
      for (uint32_t m = st & evmask; m; m &= m - 1) s += dv[__ffs(m) - 1];
    }
    return exp(s);
  };
  double total = 0.0;
  for (int tum = 0; tum < 2; ++tum)
    for (int e = 0; e <= N; ++e) total += rate(tum, e);
  uint32_t r[4];
  philox4x32_10((uint32_t)id, (uint32_t)((uint64_t)id >> 32), (uint32_t)step, 0u, (uint32_t)seed,
                (uint32_t)(seed >> 32), r);
  const double u = ((double)(((uint64_t)(r[0] >> 5) << 26) | (uint64_t)(r[1] >> 6)) * (1.0 / 9007199254740992.0)) * total;
  int ev_t = 0, ev_e = 0;
  {
    double cum = 0.0;
    bool found = false;
    int last_t = 0, last_e = 0;
    for (int tum = 0; tum < 2 && !found; ++tum)
      for (int e = 0; e <= N; ++e) {
        const double rr = rate(tum, e);
        if (rr > 0.0) { last_t = tum; last_e = e; }
        cum += rr;
        if (cum > u) { ev_t = tum; ev_e = e; found = true; break; }   // first index with cumulative rate > u
      }
    if (!found) { ev_t = last_t; ev_e = last_e; }             // rounding at the upper end
  }
  const bool seeded = pt & sbit;
  if (ev_t == 0) {
    pt |= 1u << ev_e;
    if (!seeded) mt |= 1u << ev_e;                            // before seeding both tumours move together (:49-52)
    if (ev_e == N) { t_pt = step; if (!seeded) t_mt = step; }
  } else {
    mt |= 1u << ev_e;
    if (ev_e == N) t_mt = step;
  }
  return ev_t == 0 ? ev_e : ev_e + N + 1;
}

// dat_out  [n_sim][2(N-1)+2] = [PT_0, MT_0, ..., PT_{N-2}, MT_{N-2}, seeding, order]   (simulate_dat, :117-147)
// ord_out  [n_sim][2N+2]     event sequence padded with -99 (simulate_orders, :87-114); may be null
__global__ __launch_bounds__(SIM_BLOCK) void k_gillespie(const double* __restrict__ log_theta,
                                                         const double* __restrict__ pt_d,
                                                         const double* __restrict__ mt_d, int N, long long n_sim,
                                                         uint64_t seed, int8_t* __restrict__ dat_out,
                                                         int8_t* __restrict__ ord_out) {
  __shared__ double lt[SIM_MAXN * SIM_MAXN], ltp[SIM_MAXN * SIM_MAXN], dp[SIM_MAXN], dm[SIM_MAXN];
  gillespie_load(log_theta, pt_d, mt_d, N, lt, ltp, dp, dm);
  __syncthreads();
  const long long id = (long long)blockIdx.x * SIM_BLOCK + threadIdx.x;
  if (id >= n_sim) return;
  const uint32_t sbit = 1u << (N - 1);
  uint32_t pt = 0, mt = 0;
  int t_pt = -1, t_mt = -1;
  const int L = 2 * N + 2;
  int8_t* ord = ord_out ? ord_out + id * L : nullptr;
  if (ord) for (int e = 0; e < L; ++e) ord[e] = -99;
  for (int step = 0; step < L; ++step) {
    if (gillespie_done(pt, mt, N)) break;
    const int ev = gillespie_step(lt, ltp, dp, dm, N, id, step, seed, pt, mt, t_pt, t_mt);
    if (ord) ord[step] = (int8_t)ev;
  }
  const int n_mut = N - 1, W = 2 * n_mut + 2;
  int8_t* o = dat_out + id * W;
  for (int j = 0; j < n_mut; ++j) { o[2 * j] = (pt >> j) & 1u; o[2 * j + 1] = (mt >> j) & 1u; }
  const bool paired = pt & sbit;
  o[2 * n_mut] = paired ? 1 : 0;
  o[2 * n_mut + 1] = paired ? (t_pt < t_mt ? 1 : 2) : 0;
}

// Fused sampler that counts instead of writing (mmhn_simulate_summary): trajectory `first + i`, i in [0, n), is the one
// k_gillespie draws for sample index first + i (same Philox counter, same steps).  counts [SIM_HEAD + 5 n_mut] (int64,
// n_mut = N - 1, seeding = event N - 1) is ADDED to:
//   [0] samples  [1] seeded  [2] seeded, PT observed first  [3] seeded, MT observed first (simulate_dat's order 1 / 2)
//   then five rows of n_mut, mutation m:
//   [SIM_HEAD + 0 n_mut + m] pre     seeded, m in the PT before the seeding (the PT set at the seeding step)
//   [SIM_HEAD + 1 n_mut + m] pt      seeded, final PT bit
//   [SIM_HEAD + 2 n_mut + m] mt      seeded, final MT bit
//   [SIM_HEAD + 3 n_mut + m] shared  seeded, final PT and MT bits
//   [SIM_HEAD + 4 n_mut + m] pt_nm   unseeded, final PT bit
// Each wave counts a predicate with one ballot + popcount; lane 0 adds it to the wave's row in LDS; after the block's
// grid-stride loop the rows are summed and added to `counts` with one 64-bit global atomic per counter.  Integers
// only, so the result does not depend on the launch geometry or the order of the atomics.
constexpr int SIM_HEAD = 4;
constexpr int SIM_WAVE = 64;                     // gfx9 wavefront
constexpr int SIM_COUNTS_MAX = SIM_HEAD + 5 * (SIM_MAXN - 2);
__global__ __launch_bounds__(SIM_BLOCK) void k_gillespie_summary(const double* __restrict__ log_theta,
                                                                 const double* __restrict__ pt_d,
                                                                 const double* __restrict__ mt_d, int N,
                                                                 long long first, long long n, uint64_t seed,
                                                                 unsigned long long* __restrict__ counts) {
  __shared__ double lt[SIM_MAXN * SIM_MAXN], ltp[SIM_MAXN * SIM_MAXN], dp[SIM_MAXN], dm[SIM_MAXN];
  __shared__ unsigned long long part[SIM_BLOCK / SIM_WAVE][SIM_COUNTS_MAX];
  gillespie_load(log_theta, pt_d, mt_d, N, lt, ltp, dp, dm);
  const int n_mut = N - 1, C = SIM_HEAD + 5 * n_mut;
  for (int e = threadIdx.x; e < (SIM_BLOCK / SIM_WAVE) * SIM_COUNTS_MAX; e += SIM_BLOCK) (&part[0][0])[e] = 0ull;
  __syncthreads();
  const int wave = threadIdx.x / SIM_WAVE, lane = threadIdx.x % SIM_WAVE;
  unsigned long long* row = part[wave];
  auto count = [&](int c, bool pred) {
    const unsigned long long b = __ballot(pred);
    if (lane == 0) row[c] += (unsigned long long)__popcll(b);
  };
  const uint32_t sbit = 1u << (N - 1);
  const int L = 2 * N + 2;
  for (long long base = (long long)blockIdx.x * SIM_BLOCK; base < n; base += (long long)gridDim.x * SIM_BLOCK) {
    const long long i = base + threadIdx.x;
    const bool live = i < n;
    const long long id = first + i;
    uint32_t pt = 0, mt = 0, pre = 0;
    int t_pt = -1, t_mt = -1;
    if (live)
      for (int step = 0; step < L; ++step) {
        if (gillespie_done(pt, mt, N)) break;
        const uint32_t before = pt;
        gillespie_step(lt, ltp, dp, dm, N, id, step, seed, pt, mt, t_pt, t_mt);
        if ((pt & ~before) & sbit) pre = before;               // the seeding step: the PT set at that moment
      }
    const bool seeded = live && (pt & sbit), unseeded = live && !(pt & sbit);
    count(0, live);
    count(1, seeded);
    count(2, seeded && t_pt < t_mt);
    count(3, seeded && !(t_pt < t_mt));
    for (int m = 0; m < n_mut; ++m) {
      const bool in_pt = (pt >> m) & 1u, in_mt = (mt >> m) & 1u;
      count(SIM_HEAD + m, seeded && ((pre >> m) & 1u));
      count(SIM_HEAD + n_mut + m, seeded && in_pt);
      count(SIM_HEAD + 2 * n_mut + m, seeded && in_mt);
      count(SIM_HEAD + 3 * n_mut + m, seeded && in_pt && in_mt);
      count(SIM_HEAD + 4 * n_mut + m, unseeded && in_pt);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += SIM_BLOCK) {
    unsigned long long s = 0;
    for (int w = 0; w < SIM_BLOCK / SIM_WAVE; ++w) s += part[w][c];
    if (s) atomicAdd(counts + c, s);
  }
}

// Fused sampler that counts second-order tables (mmhn_simulate_pairs): the same trajectories `first + i` again.  With
// B = 2 n_mut genotype columns [PT_0, MT_0, PT_1, MT_1, ...] as simulate_dat orders them, P = B (B + 1) / 2 pairs (a <= b)
// numbered row by row of the upper triangle, and the class of a sample = simulate_dat's last column (0 unseeded, 1 seeded
// and PT observed first, 2 seeded and MT observed first), counts [3 + 3 P + 15 (n_mut + 1)] (int64) is ADDED to:
//   [c]                                      samples of class c
//   [3 + c P + p]                            samples of class c with both columns of pair p set (a = b: the marginal)
//   [3 + 3 P + (5 c + k)(n_mut + 1) + v]     samples of class c whose mutation count of kind k is v;
//                                            k: 0 |PT|  1 |MT|  2 |PT & MT|  3 |PT & ~MT|  4 |MT & ~PT|
// Per pass of the grid-stride loop a wave turns its 64 trajectories into B column masks and 3 class masks (one ballot
// each, dead lanes in no class) in LDS; after a barrier thread t owns the pairs t, t + 256, ... and adds
// popcount(mask_a & mask_b & class_c) of the four waves to registers of its own (SIM_PAIRS_PER_THREAD x 3, indexed at
// compile time); the burden histogram takes five LDS atomics per live trajectory.  After the loop every non-zero counter
// goes out as one 64-bit global atomic.  Integers only: no dependence on the geometry or the order of the atomics.
// A 32-bit counter receives at most SIM_BLOCK per pass; the host bounds the passes of a launch by SIM_PAIRS_MAX_PASSES.
constexpr int SIM_PAIR_COLS = 2 * (SIM_MAXN - 2);                                        // 60
constexpr int SIM_PAIRS_MAX = SIM_PAIR_COLS * (SIM_PAIR_COLS + 1) / 2;                   // 1 830
constexpr int SIM_PAIRS_PER_THREAD = (SIM_PAIRS_MAX + SIM_BLOCK - 1) / SIM_BLOCK;        // 8
constexpr int SIM_CLASSES = 3, SIM_BURDEN_KINDS = 5;
constexpr long long SIM_PAIRS_MAX_PASSES = 1ll << 23;                                    // x SIM_BLOCK = 2^31 per counter
__host__ __device__ constexpr int sim_pairs_counts(int n_mut) {
  return SIM_CLASSES + SIM_CLASSES * (n_mut * (2 * n_mut + 1)) + SIM_CLASSES * SIM_BURDEN_KINDS * (n_mut + 1);
}
__global__ __launch_bounds__(SIM_BLOCK) void k_gillespie_pairs(const double* __restrict__ log_theta,
                                                               const double* __restrict__ pt_d,
                                                               const double* __restrict__ mt_d, int N, long long first,
                                                               long long n, uint64_t seed,
                                                               unsigned long long* __restrict__ counts) {
  constexpr int WAVES = SIM_BLOCK / SIM_WAVE, HIST = SIM_CLASSES * SIM_BURDEN_KINDS * (SIM_MAXN - 1);
  __shared__ double lt[SIM_MAXN * SIM_MAXN], ltp[SIM_MAXN * SIM_MAXN], dp[SIM_MAXN], dm[SIM_MAXN];
  __shared__ unsigned long long mask[WAVES][SIM_WAVE];      // [0, B) columns, [B, B + 3) classes; B + 3 <= 63
  __shared__ uint16_t pair_ab[SIM_PAIRS_MAX];               // pair p -> a | b << 8
  __shared__ uint32_t hist[HIST + SIM_CLASSES];             // burden [c][k][v], then the class sizes
  gillespie_load(log_theta, pt_d, mt_d, N, lt, ltp, dp, dm);
  const int n_mut = N - 1, B = 2 * n_mut, P = B * (B + 1) / 2, V = n_mut + 1;
  for (int a = threadIdx.x; a < B; a += SIM_BLOCK) {        // row a of the triangle starts at a B - a (a - 1) / 2
    const int off = a * B - a * (a - 1) / 2;
    for (int b = a; b < B; ++b) pair_ab[off + b - a] = (uint16_t)(a | (b << 8));
  }
  for (int e = threadIdx.x; e < HIST + SIM_CLASSES; e += SIM_BLOCK) hist[e] = 0u;
  uint32_t acc[SIM_CLASSES][SIM_PAIRS_PER_THREAD];
#pragma unroll
  for (int c = 0; c < SIM_CLASSES; ++c)
#pragma unroll
    for (int k = 0; k < SIM_PAIRS_PER_THREAD; ++k) acc[c][k] = 0u;
  __syncthreads();
  const int wave = threadIdx.x / SIM_WAVE, lane = threadIdx.x % SIM_WAVE;
  const uint32_t sbit = 1u << (N - 1), muts = sbit - 1u;
  const int L = 2 * N + 2;
  for (long long base = (long long)blockIdx.x * SIM_BLOCK; base < n; base += (long long)gridDim.x * SIM_BLOCK) {
    const long long i = base + threadIdx.x;
    const bool live = i < n;
    const long long id = first + i;
    uint32_t pt = 0, mt = 0;
    int t_pt = -1, t_mt = -1;
    if (live)
      for (int step = 0; step < L; ++step) {
        if (gillespie_done(pt, mt, N)) break;
        gillespie_step(lt, ltp, dp, dm, N, id, step, seed, pt, mt, t_pt, t_mt);
      }
    const int cls = !(pt & sbit) ? 0 : (t_pt < t_mt ? 1 : 2);
    // lane a keeps the ballot of column a, lanes B .. B + 2 those of the classes: one LDS write per wave and pass
    unsigned long long mine = 0ull;
    for (int m = 0; m < n_mut; ++m) {
      const unsigned long long bp = __ballot(live && ((pt >> m) & 1u)), bm = __ballot(live && ((mt >> m) & 1u));
      if (lane == 2 * m) mine = bp;
      if (lane == 2 * m + 1) mine = bm;
    }
#pragma unroll
    for (int c = 0; c < SIM_CLASSES; ++c) {
      const unsigned long long bc = __ballot(live && cls == c);
      if (lane == B + c) mine = bc;
    }
    mask[wave][lane] = mine;
    if (live) {
      const uint32_t p = pt & muts, m = mt & muts;
      uint32_t* h = hist + cls * SIM_BURDEN_KINDS * V;
      atomicAdd(h + __popc(p), 1u);
      atomicAdd(h + V + __popc(m), 1u);
      atomicAdd(h + 2 * V + __popc(p & m), 1u);
      atomicAdd(h + 3 * V + __popc(p & ~m), 1u);
      atomicAdd(h + 4 * V + __popc(m & ~p), 1u);
    }
    __syncthreads();
    if (threadIdx.x < SIM_CLASSES) {
      uint32_t s = 0;
      for (int w = 0; w < WAVES; ++w) s += (uint32_t)__popcll(mask[w][B + threadIdx.x]);
      hist[HIST + threadIdx.x] += s;
    }
#pragma unroll
    for (int k = 0; k < SIM_PAIRS_PER_THREAD; ++k) {
      const int p = threadIdx.x + k * SIM_BLOCK;
      if (p < P) {
        const int a = pair_ab[p] & 0xff, b = pair_ab[p] >> 8;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
          const unsigned long long ab = mask[w][a] & mask[w][b];
#pragma unroll
          for (int c = 0; c < SIM_CLASSES; ++c) acc[c][k] += (uint32_t)__popcll(ab & mask[w][B + c]);
        }
      }
    }
    __syncthreads();                                        // the next pass overwrites the masks
  }
  for (int e = threadIdx.x; e < SIM_CLASSES; e += SIM_BLOCK)
    if (hist[HIST + e]) atomicAdd(counts + e, (unsigned long long)hist[HIST + e]);
#pragma unroll
  for (int k = 0; k < SIM_PAIRS_PER_THREAD; ++k) {
    const int p = threadIdx.x + k * SIM_BLOCK;
    if (p < P) {
#pragma unroll
      for (int c = 0; c < SIM_CLASSES; ++c)
        if (acc[c][k]) atomicAdd(counts + SIM_CLASSES + c * P + p, (unsigned long long)acc[c][k]);
    }
  }
  for (int e = threadIdx.x; e < SIM_CLASSES * SIM_BURDEN_KINDS * V; e += SIM_BLOCK)
    if (hist[e]) atomicAdd(counts + SIM_CLASSES + SIM_CLASSES * P + e, (unsigned long long)hist[e]);
}

}  // namespace mmhn
