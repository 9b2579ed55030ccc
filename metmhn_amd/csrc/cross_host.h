// Host side of the exact PT x MT co-occurrence and joint burden tables (cross.h: k_cross_seed, k_cross_founder, k_cross_back,
// k_cross_fold, k_cross_reduce): one workspace and one set-up per call - lattice_host.h's check, model upload and tile list -,
// the founder plane Z, then per block of four features one backward sweep of four planes, per pair of a PT block and an MT
// block one fold over every tile and one reduction into the device's table, and the table's way out.
//
// The planes are planned against the workspace limit.  FB = ceil(features / 4) blocks a chain, features = 2 n + 1 with the
// burden and n without.  Z and one MT block are always resident; as many PT blocks as fit are HELD, swept once and folded
// against every MT block; when not all fit, one of the slots is given to the blocks that are not held, which are swept again
// for every MT block.  All held: 1 + 4 + 4 FB planes (65 planes, 130 GiB, at n = 28 with the burden) and 2 FB sweeps; the
// minimum is 9 planes - Z, one MT block, one PT slot - and FB + FB^2 sweeps.  A plane's bytes depend on the model and its
// feature alone, so the table's bytes do not depend on the plan.
#pragma once
#include "cross.h"
#include "lattice_host.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

inline int cross_blocks(int n, bool burden) { return ((burden ? 2 * n + 1 : n) + CX_BLOCK - 1) / CX_BLOCK; }

// doubles of mmhn_cross_table's out: mass, pt [n], mt [n], cross [n][n], burden [n + 1][n + 1], gene_burden [2][n][n + 1]
inline long long cross_out_doubles(int n) { return 1 + 2ll * n + (long long)n * n + (long long)(n + 1) * (n + 1) + 2ll * n * (n + 1); }

// bytes of workspace a call with `planes` planes takes: lattice_bytes of them with both sets of tables and the tile list, the
// tiles' partial sums of one fold (CX_SUMS) and of the founder's mass, and the device's table of 4 FB x 4 FB products, the
// 2 x 4 FB marginals and the mass - FB with the burden, so that the bytes depend on n and the planes alone.
// planes = 1 + 4 + 4 x the PT blocks held, at least 9
inline long long cross_bytes(int n, int planes) {
  const long long nt = 1ll << (n - ls_tile_bits(n)), FP = (long long)CX_BLOCK * cross_blocks(n, true);
  return lattice_bytes(n, planes, 2, false) + (long long)sizeof(double) * ((CX_SUMS + 1) * nt + FP * FP + 2 * FP + 1);
}

// out: cross_out_doubles(n) doubles in the order above; without the burden the burden outputs are NaN
template <typename T>
void cross_table(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, bool burden, double* out) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the cross table kernels (n_mut <= 31)");
  static const LatticeSpec spec{"cross table", ", the rate tables, the tile list and the tiles' partial sums", "table", 2, false};
  const int n = E.n, N = E.N, c = ls_tile_bits(n), hb = n - c;
  const int F = burden ? 2 * n + 1 : n, FB = cross_blocks(n, burden), FP = CX_BLOCK * FB;
  const size_t nt = (size_t)1 << hb, plane = (size_t)1 << n;
  std::fill(out, out + cross_out_doubles(n), std::nan(""));
  const long long limit = (long long)E.cfg.plan.ws_limit;
  ls_check_workspace(spec, n, 1 + 2 * CX_BLOCK, cross_bytes(n, 1 + 2 * CX_BLOCK), limit);

  // the plan: H slots of a PT block; with all blocks held every block has its slot, otherwise the last slot is the one the
  // blocks that are not held are swept into
  const long long room = (limit - cross_bytes(n, 0)) / (long long)(sizeof(double) * plane);
  const int H = (int)std::min<long long>(FB, (room - 1 - CX_BLOCK) / CX_BLOCK);
  const int fixed = H == FB ? FB : H - 1;

  std::vector<uint32_t> tiles;
  std::vector<size_t> first;
  ls_tile_levels(hb, false, tiles, first);
  DevArr<double> par, V, part, tab;
  DevArr<LsTables> tabs;
  DevArr<uint32_t> d_tiles;
  par.alloc((size_t)N * N + 2 * N);
  V.alloc((size_t)(1 + CX_BLOCK + CX_BLOCK * H) << n);
  tabs.alloc(2);
  d_tiles.alloc(nt);
  part.alloc((size_t)(CX_SUMS + 1) * nt);
  tab.alloc((size_t)FP * FP + 2 * FP + 1);
  const double* obs[2] = {obs1, obs2};
  ls_upload_model(E.stream, N, c, 2, lt, obs, tiles, par.p, d_tiles.p, tabs.p);
  const double* d_lt = par.p;
  const PartnerChain pt{tabs.p, par.p + N * N, 0}, mt{tabs.p + 1, par.p + N * N + N, 1};
  double* Z = V.p;
  double* Bm = V.p + plane;                                  // the resident MT block
  const auto slot = [&](int s) { return V.p + (size_t)(1 + CX_BLOCK + CX_BLOCK * s) * plane; };

  // Z: G0 by levels ascending, then sigma G0 in place and the tiles' masses, added into the table
  for (int l = 0; l <= hb; ++l) {
    hipLaunchKernelGGL(k_cross_seed, dim3((unsigned)(first[l + 1] - first[l])), dim3(LS_KB), 0, E.stream, tabs.p,
                       d_tiles.p + first[l], d_lt, par.p + N * N, N, c, Z);
    HIPCHECK(hipGetLastError());
  }
  double* mass = part.p + (size_t)CX_SUMS * nt;
  hipLaunchKernelGGL(k_cross_founder, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, tabs.p, d_lt, N, c, Z, mass);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_cross_reduce, dim3(1), dim3(LS_KB), 0, E.stream, mass, (long long)nt, -1, 0, FP, tab.p);
  HIPCHECK(hipGetLastError());

  // one backward sweep: the levels of the ascending tile list from the last to the first
  const auto sweep = [&](const PartnerChain& ch, int b, double* Vb) {
    const CrossBlock blk{CX_BLOCK * b, n, F};
    for (int l = hb; l >= 0; --l) {
      hipLaunchKernelGGL(k_cross_back, dim3((unsigned)(first[l + 1] - first[l])), dim3(LS_KB), 0, E.stream, ch, blk,
                         d_tiles.p + first[l], d_lt, N, c, Vb);
      HIPCHECK(hipGetLastError());
    }
  };
  for (int i = 0; i < fixed; ++i) sweep(pt, i, slot(i));
  for (int j = 0; j < FB; ++j) {
    sweep(mt, j, Bm);
    for (int i = 0; i < FB; ++i) {
      double* A = slot(i < fixed ? i : fixed);
      if (i >= fixed) sweep(pt, i, A);
      hipLaunchKernelGGL(k_cross_fold, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, Z, A, Bm, n, c, part.p, (long long)nt);
      HIPCHECK(hipGetLastError());
      hipLaunchKernelGGL(k_cross_reduce, dim3(CX_SUMS), dim3(LS_KB), 0, E.stream, part.p, (long long)nt, CX_BLOCK * i,
                         CX_BLOCK * j, FP, tab.p);
      HIPCHECK(hipGetLastError());
    }
  }
  std::vector<double> t((size_t)FP * FP + 2 * FP + 1);
  HIPCHECK(hipMemcpyAsync(t.data(), tab.p, t.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));

  const size_t pp = (size_t)FP * FP;
  double* o = out;
  *o++ = t[pp + 2 * FP];
  for (int i = 0; i < n; ++i) *o++ = t[pp + i];
  for (int j = 0; j < n; ++j) *o++ = t[pp + FP + j];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) *o++ = t[(size_t)i * FP + j];
  if (!burden) return;
  for (int k = 0; k <= n; ++k)
    for (int l = 0; l <= n; ++l) *o++ = t[(size_t)(n + k) * FP + n + l];
  for (int i = 0; i < n; ++i)
    for (int l = 0; l <= n; ++l) *o++ = t[(size_t)i * FP + n + l];
  for (int j = 0; j < n; ++j)
    for (int k = 0; k <= n; ++k) *o++ = t[(size_t)(n + k) * FP + j];
}

}  // namespace mmhn
