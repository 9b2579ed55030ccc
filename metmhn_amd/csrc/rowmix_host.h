// Row weights (mmhn_set_row_weights) and row groups (mmhn_set_row_groups, mmhn_group_posteriors) on the host: the checks of
// what the caller hands in, the device copies, and the launches of the group kernels (rowmix.h).  The engine keeps the data
// (row_w, grp_*, gd, the counts); its evaluation only picks the reduction kernel and calls launch_mix.
// Included by engine.hip after the Engine template.
#pragma once

namespace mmhn {

// the checks that the weights of rows and of groups share: every weight finite and not negative, not all of them 0
// (fn: "mmhn_set_row_weights: ", unit: "row" / "group")
struct WeightCheck {
  std::string fn;
  const char* unit;
  bool any = false;
  void one(double w, long long i) {
    if (!std::isfinite(w) || w < 0)
      throw Fail{fn + "the weight of " + unit + " " + std::to_string(i) + (std::isfinite(w) ? " is negative" : " is not finite")};
    any = any || w != 0;
  }
  void all(long long count) const {
    REQUIRE(any, fn + "every weight is 0 (" + unit + " 0 is the first of " + std::to_string(count) + ")");
  }
};

// one weight per cohort row (nullptr: none).  Everything an evaluation needs is brought to the device here, one array per
// batch in the batch's own order of patients (PatRec::row); an evaluation then only picks k_reduce_rows_w.
template <typename T>
void set_row_weights(Engine<T>& E, const double* w, long long nw) {
  const std::string fn = "mmhn_set_row_weights: ";
  REQUIRE(!E.pending.on, fn + "an evaluation begun with mmhn_cohort_sums_begin has not been collected");
  if (!w) {
    E.row_w.clear();
    for (BatchDev& d : E.dev) d.wrow.release();
    return;
  }
  REQUIRE(!E.mixing(), fn + "the engine holds row groups (group 0 of " + std::to_string(E.grp_w.size()) +
                           "), whose weights take the role of row weights: remove them first");
  const long long n_pat = E.n_pat;
  const std::string rows = std::to_string(n_pat);
  REQUIRE(n_pat > 0 && !E.batches.empty(), fn + "the engine holds no cohort (row 0 does not exist)");
  REQUIRE(nw == n_pat, fn + std::to_string(nw) + " weights for a cohort of " + rows + " rows (" +
                           (nw < n_pat ? "row " + std::to_string(std::max<long long>(nw, 0)) + " has no weight"
                                       : "row " + rows + " does not exist") + ")");
  typename Engine<T>::Counts s;
  WeightCheck chk{fn, "row"};
  for (long long r = 0; r < n_pat; ++r) {
    chk.one(w[r], r);
    const int8_t* row = E.dat.data() + (size_t)r * E.n_cols;
    if (row[2 * E.n] == 1) s.em += w[r];
    s.pat += w[r];
    if (row[E.n_cols - 1] == 4) s.unknown += w[r];
  }
  chk.all(n_pat);
  std::vector<DevArr<double>> fresh(E.batches.size());
  std::vector<double> hw;
  for (const Batch& b : E.batches) {
    hw.resize(b.pats.size());
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = w[b.pats[i].row];
    fresh[b.id].alloc(hw.size());
    if (!hw.empty()) HIPCHECK(hipMemcpy(fresh[b.id].p, hw.data(), hw.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  for (const Batch& b : E.batches) E.dev[b.id].wrow = std::move(fresh[b.id]);
  E.row_w.assign(w, w + n_pat);
  E.weighted = s;
}

template <typename T>
void clear_row_groups(Engine<T>& E) {
  E.grp_ptr.clear(); E.grp_rows.clear(); E.grp_w.clear();
  E.gd = typename Engine<T>::GroupsDev{};
}

// mmhn_set_row_groups: group g = rows[ptr[g] .. ptr[g+1]) of the current cohort with weight w[g].  Checked in full, then
// brought to the device in full, then swapped in: a refused call leaves what was held before.
template <typename T>
void set_row_groups(Engine<T>& E, const int64_t* ptr, long long ng, const int64_t* rows, const double* w) {
  const std::string fn = "mmhn_set_row_groups: ";
  REQUIRE(!E.pending.on, fn + "an evaluation begun with mmhn_cohort_sums_begin has not been collected");
  if (ng == 0 || !ptr || !rows || !w) {
    REQUIRE(ng == 0 || (!ptr && !rows && !w), fn + "null pointer next to " + std::to_string(ng) + " groups (group 0)");
    clear_row_groups(E);
    return;
  }
  const long long n_pat = E.n_pat;
  const int n = E.n, n_cols = E.n_cols;
  const std::vector<int8_t>& dat = E.dat;
  REQUIRE(ng > 0 && ng < (1ll << 31), fn + "the number of groups must be in 0 .. 2^31 - 1 (group " + std::to_string(ng) + ")");
  REQUIRE(n_pat > 0 && !E.batches.empty(), fn + "the engine holds no cohort (row 0 of group 0 does not exist)");
  REQUIRE(E.row_w.empty(), fn + "the engine holds row weights (row 0), and group weights take their role: remove them first");
  REQUIRE(E.comm_size <= 1, fn + "the engine is rank " + std::to_string(E.comm_rank) + " of " + std::to_string(E.comm_size) +
                                ": sharding cuts through groups (group 0), so row groups need a one-rank engine");
  REQUIRE(ptr[0] == 0, fn + "ptr[0] must be 0 (group 0)");
  for (long long g = 0; g < ng; ++g) {
    const std::string at = fn + "group " + std::to_string(g);
    REQUIRE(ptr[g + 1] >= ptr[g], at + ": ptr is decreasing");
    REQUIRE(ptr[g + 1] > ptr[g], at + " is empty");
  }
  typename Engine<T>::Counts s;
  WeightCheck chk{fn, "group"};
  auto cls = [&](long long r) { const int t = dat[(size_t)r * n_cols + n_cols - 1]; return t == 0 || t == 4 ? 1 : 0; };
  auto unk = [&](long long r) { return dat[(size_t)r * n_cols + n_cols - 1] == 4; };
  auto seeded = [&](long long r) { return dat[(size_t)r * n_cols + 2 * n] == 1; };
  for (long long g = 0; g < ng; ++g) {
    const std::string at = fn + "group " + std::to_string(g);
    for (long long k = ptr[g]; k < ptr[g + 1]; ++k)
      REQUIRE(rows[k] >= 0 && rows[k] < n_pat, at + " holds row " + std::to_string(rows[k]) + ", outside the cohort of " +
                                                   std::to_string(n_pat) + " rows");
    chk.one(w[g], g);
    const long long r0 = rows[ptr[g]];
    for (long long k = ptr[g] + 1; k < ptr[g + 1]; ++k) {
      REQUIRE(cls(rows[k]) == cls(r0), at + " mixes the two blocks of the cohort sums: row " + std::to_string(r0) + " is " +
                                           (cls(r0) ? "NM / type 4" : "EM") + ", row " + std::to_string(rows[k]) + " is not");
      REQUIRE(unk(rows[k]) == unk(r0), at + " mixes rows of type 4 with others (rows " + std::to_string(r0) + " and " +
                                           std::to_string(rows[k]) + ")");
    }
    if (seeded(r0)) s.em += w[g];
    s.pat += w[g];
    if (unk(r0)) s.unknown += w[g];
  }
  chk.all(ng);
  const long long nnz = ptr[ng];
  // the transposed lists: the memberships of every cohort row, in group order
  std::vector<long long> mptr((size_t)n_pat + 1, 0);
  for (long long k = 0; k < nnz; ++k) ++mptr[(size_t)rows[k] + 1];
  for (long long r = 0; r < n_pat; ++r) mptr[(size_t)r + 1] += mptr[(size_t)r];
  std::vector<int> mgrp((size_t)nnz), hrows((size_t)nnz);
  {
    std::vector<long long> at(mptr.begin(), mptr.end() - 1);
    for (long long g = 0; g < ng; ++g)
      for (long long k = ptr[g]; k < ptr[g + 1]; ++k) { mgrp[(size_t)at[(size_t)rows[k]]++] = (int)g; hrows[(size_t)k] = (int)rows[k]; }
  }
  typename Engine<T>::GroupsDev fresh;
  auto upv = [](auto& d, const auto* src, size_t cnt) {
    d.alloc(cnt);
    if (cnt) HIPCHECK(hipMemcpy(d.p, src, cnt * sizeof(*src), hipMemcpyHostToDevice));
  };
  upv(fresh.gptr, ptr, (size_t)ng + 1);
  upv(fresh.grows, hrows.data(), (size_t)nnz);
  upv(fresh.gw, w, (size_t)ng);
  upv(fresh.mptr, mptr.data(), mptr.size());
  upv(fresh.mgrp, mgrp.data(), mgrp.size());
  fresh.lpc.alloc((size_t)n_pat); fresh.omega.alloc((size_t)n_pat); fresh.lambda.alloc((size_t)n_pat);
  fresh.lpg.alloc((size_t)ng); fresh.rho.alloc((size_t)nnz);
  E.gd = std::move(fresh);
  E.grp_ptr.assign(ptr, ptr + ng + 1);
  E.grp_rows = std::move(hrows);
  E.grp_w.assign(w, w + ng);
  E.grouped = s;
}

template <typename T>
MixDev mix_dev(const Engine<T>& E) {
  const auto& gd = E.gd;
  return MixDev{gd.gptr.p, gd.grows.p, gd.gw.p, (int)E.grp_w.size(), gd.mptr.p, gd.mgrp.p, (int)E.n_pat,
                gd.lpc.p, gd.lpg.p, gd.omega.p, gd.lambda.p};
}
// lp_g of every group, then omega / lambda of every row: after the last batch has written its rows of lpc
template <typename T>
void launch_mix(Engine<T>& E, const Lane& L) {
  const MixDev m = mix_dev(E);
  hipLaunchKernelGGL(k_group_lse, dim3((m.n_groups + MIX_WAVES - 1) / MIX_WAVES), dim3(BLOCK), 0, L.s, m, E.want_rho ? E.gd.rho.p : nullptr);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mix_weights, dim3((m.n_rows + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, L.s, m);
  HIPCHECK(hipGetLastError());
}
// score-only evaluation: lp_g [n_groups], rho [ptr[n_groups]] in the order of the group lists
template <typename T>
void group_posteriors(Engine<T>& E, const double* lt, const double* ldp, const double* ldm, double* lp_group, double* rho) {
  REQUIRE(E.mixing(), "mmhn_group_posteriors: the engine holds no row groups (mmhn_set_row_groups)");
  std::vector<double> s(2 * E.stride());
  E.want_rho = true;
  struct Unset { bool& f; ~Unset() { f = false; } } unset{E.want_rho};
  E.evaluate(lt, ldp, ldm, false, s.data(), nullptr);
  HIPCHECK(hipMemcpy(lp_group, E.gd.lpg.p, E.grp_w.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(rho, E.gd.rho.p, E.grp_rows.size() * sizeof(double), hipMemcpyDeviceToHost));
}

}  // namespace mmhn
