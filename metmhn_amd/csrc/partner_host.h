// Host side of the genotype distribution of one tumour given the other (partner.h: k_partner_back, k_partner_seed,
// k_partner_level, k_partner_tile, k_partner_values; genodist.h's k_genodist_summary): one workspace of two planes and one
// set-up per call - lattice_host.h's checks, model upload and tile list -, then a loop over the DISTINCT valid query
// genotypes: the restricted tile list under the query's high bits (built per query, staged in two pinned buffers), the backward pass and the seeding pass over it, the
// full forward sweep, the tile kernel, the summary on request, the rows' values and, for a call of one row, the copy of the
// two planes.  Nothing a query writes is read by the next one: the outputs of a query do not depend on its neighbours.
#pragma once
#include "lattice_host.h"
#include "partner.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>)

// bytes of workspace a call takes, whatever its rows: two planes, both sets of tables, the full and the restricted tile
// list, the tiles' partial sums (formed for `mass` with or without summaries) and one query's summary.  As in lattice_sweep
// the per-row buffers - 4 B of target code and 24 B of values per valid row - fall outside the limit.
inline long long partner_bytes(int n) { return lattice_bytes(n, 2, 2, true) + (4ll << (n - ls_tile_bits(n))); }

// two pinned buffers the restricted tile lists are staged in, alternating: a query's list is built while the previous
// query's copy may still be in flight, and a buffer is written again only after the copy out of it has finished
struct PartnerStage {
  uint32_t* buf[2] = {nullptr, nullptr};
  hipEvent_t copied[2] = {nullptr, nullptr};
  explicit PartnerStage(size_t entries) {
    for (int i = 0; i < 2; ++i) {
      HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&buf[i]), entries * sizeof(uint32_t), hipHostMallocDefault));
      HIPCHECK(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
    }
  }
  ~PartnerStage() {
    for (int i = 0; i < 2; ++i) {
      if (copied[i]) (void)hipEventDestroy(copied[i]);
      if (buf[i]) (void)hipHostFree(buf[i]);
    }
  }
  PartnerStage(const PartnerStage&) = delete;
  PartnerStage& operator=(const PartnerStage&) = delete;
};

// given: 0 the primary tumour (seeded), 1 the metastasis.  gen [R][n]: 1 = held (R may be 0); target: nullptr or [R][n].
// values [R][3]: mass, W and J at the target (NaN without targets; all NaN for a row that is not valid); summaries: nullptr
// or [R][2][1 + n * n + n + 1], founder and partner; full: nullptr or [2][2^n] of the one row.
template <typename T>
void partner_distributions(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, int given,
                           const int8_t* gen, const int8_t* target, long long R, double* values, int32_t* status,
                           double* summaries, double* full) {
  REQUIRE(E.N <= ORD_MAXN, "too many events for the partner distribution kernels (n_mut <= 31)");
  REQUIRE(given == 0 || given == 1, "given must be 0 (the primary tumour) or 1 (the metastasis)");
  REQUIRE(!full || R == 1, "the full planes of a partner distribution are those of one query: full needs n_rows == 1");
  static const LatticeSpec spec{"partner distribution", ", the rate tables, the tile lists and the tiles' partial sums",
                                "distribution", 2, false};
  const int n = E.n, N = E.N, c = ls_tile_bits(n), hb = n - c;
  const size_t nt = (size_t)1 << hb, len = (size_t)gd_summary_doubles(n);
  std::fill(values, values + 3 * R, std::nan(""));
  if (summaries) std::fill(summaries, summaries + len * R, std::nan(""));
  if (full) std::fill(full, full + ((size_t)2 << n), std::nan(""));
  ls_check_workspace(spec, n, 2, partner_bytes(n), (long long)E.cfg.plan.ws_limit);

  // the valid rows, sorted by query: a query's rows are rows[at[k]] .. rows[at[k + 1] - 1]
  std::vector<uint32_t> qcode(R), tcode(R, 0u);
  {
    std::vector<uint32_t> codes;
    std::vector<long long> src;
    ls_decode_queries(gen, R, n, status, codes, src);
    for (size_t j = 0; j < src.size(); ++j) qcode[src[j]] = codes[j];
    if (target) {
      std::vector<int32_t> st(R);
      codes.clear(); src.clear();
      ls_decode_queries(target, R, n, st.data(), codes, src);
      for (size_t j = 0; j < src.size(); ++j) tcode[src[j]] = codes[j];
      for (long long i = 0; i < R; ++i)
        if (status[i] == MMHN_ORD_OK) status[i] = st[i];
    }
  }
  std::vector<long long> rows;
  for (long long i = 0; i < R; ++i)
    if (status[i] == MMHN_ORD_OK) rows.push_back(i);
  if (rows.empty()) return;
  std::stable_sort(rows.begin(), rows.end(), [&](long long a, long long b) { return qcode[a] < qcode[b]; });
  std::vector<size_t> at;
  for (size_t j = 0; j < rows.size(); ++j)
    if (j == 0 || qcode[rows[j]] != qcode[rows[j - 1]]) at.push_back(j);
  at.push_back(rows.size());
  const size_t Q = at.size() - 1;

  // the longest restricted tile list; the lists themselves are built one query at a time in the loop
  size_t most = 0;
  for (size_t k = 0; k < Q; ++k) most = std::max(most, (size_t)1 << __builtin_popcount(qcode[rows[at[k]]] >> c));
  std::vector<uint32_t> tiles, targets(rows.size()), sub;
  std::vector<size_t> first, sf;
  ls_tile_levels(hb, false, tiles, first);
  for (size_t j = 0; j < rows.size(); ++j) targets[j] = tcode[rows[j]];

  DevArr<double> par, V, part, d_sum, d_out;
  DevArr<LsTables> tabs;
  DevArr<uint32_t> d_tiles, d_sub, d_targets;
  par.alloc((size_t)N * N + 2 * N);
  V.alloc((size_t)2 << n);
  tabs.alloc(2);
  d_tiles.alloc(nt);
  d_sub.alloc(most);
  part.alloc((size_t)2 * GD_FEAT * nt);
  if (summaries) d_sum.alloc(len);
  d_out.alloc(3 * rows.size());
  if (target) {
    d_targets.alloc(rows.size());
    HIPCHECK(hipMemcpyAsync(d_targets.p, targets.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
  }
  const double* obs[2] = {obs1, obs2};
  ls_upload_model(E.stream, N, c, 2, lt, obs, tiles, par.p, d_tiles.p, tabs.p);
  const double* d_lt = par.p;
  const PartnerChain chain[2] = {{tabs.p, par.p + N * N, 0}, {tabs.p + 1, par.p + N * N + N, 1}};
  const PartnerChain back = chain[given], fwd = chain[1 - given];
  PartnerStage stage(most);

  for (size_t k = 0; k < Q; ++k) {
    const uint32_t q = qcode[rows[at[k]]];
    const int levels = __builtin_popcount(q >> c);
    ls_tile_levels_under(q >> c, sub, sf);
    if (k >= 2) HIPCHECK(hipEventSynchronize(stage.copied[k & 1]));
    std::copy(sub.begin(), sub.end(), stage.buf[k & 1]);
    HIPCHECK(hipMemcpyAsync(d_sub.p, stage.buf[k & 1], sub.size() * sizeof(uint32_t), hipMemcpyHostToDevice, E.stream));
    HIPCHECK(hipEventRecord(stage.copied[k & 1], E.stream));
    for (int l = levels; l >= 0; --l) {
      hipLaunchKernelGGL(k_partner_back, dim3((unsigned)(sf[l + 1] - sf[l])), dim3(LS_KB), 0, E.stream, back, d_sub.p + sf[l],
                         d_lt, N, c, q, V.p);
      HIPCHECK(hipGetLastError());
    }
    for (int l = 0; l <= levels; ++l) {
      hipLaunchKernelGGL(k_partner_seed, dim3((unsigned)(sf[l + 1] - sf[l])), dim3(LS_KB), 0, E.stream, tabs.p, d_sub.p + sf[l],
                         d_lt, par.p + N * N, N, c, q, V.p);
      HIPCHECK(hipGetLastError());
    }
    for (int l = 0; l <= hb; ++l) {
      hipLaunchKernelGGL(k_partner_level, dim3((unsigned)(first[l + 1] - first[l])), dim3(LS_KB), 0, E.stream, fwd,
                         d_tiles.p + first[l], d_lt, N, c, q, V.p);
      HIPCHECK(hipGetLastError());
    }
    if (full) hipLaunchKernelGGL(k_partner_tile<true>, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, fwd, N, c, q, V.p, part.p, (long long)nt);
    else hipLaunchKernelGGL(k_partner_tile<false>, dim3((unsigned)nt), dim3(LS_KB), 0, E.stream, fwd, N, c, q, V.p, part.p, (long long)nt);
    HIPCHECK(hipGetLastError());
    if (summaries) {
      hipLaunchKernelGGL(k_genodist_summary, dim3((unsigned)(2 * gd_summary_items(n))), dim3(LS_KB), 0, E.stream, part.p,
                         (long long)nt, n, c, d_sum.p);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(summaries + len * rows[at[k]], d_sum.p, sizeof(double) * len, hipMemcpyDeviceToHost, E.stream));
    }
    hipLaunchKernelGGL(k_partner_values, dim3((unsigned)(at[k + 1] - at[k])), dim3(LS_KB), 0, E.stream, part.p, (long long)nt, n,
                       q, target ? d_targets.p : (const uint32_t*)nullptr, (long long)at[k], V.p, d_out.p);
    HIPCHECK(hipGetLastError());
    if (full) HIPCHECK(hipMemcpyAsync(full, V.p, sizeof(double) * ((size_t)2 << n), hipMemcpyDeviceToHost, E.stream));
  }
  std::vector<double> out(3 * rows.size());
  HIPCHECK(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
  for (size_t k = 0; k < Q; ++k)
    for (size_t j = at[k]; j < at[k + 1]; ++j) {
      std::copy(out.begin() + 3 * j, out.begin() + 3 * j + 3, values + 3 * rows[j]);
      if (summaries && j > at[k]) std::copy(summaries + len * rows[at[k]], summaries + len * (rows[at[k]] + 1), summaries + len * rows[j]);
    }
}

}  // namespace mmhn
