// Host side of the likeliest event orders of a cohort (orders.h: k_orders): row decoding, batching, launches.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"
#include "plan.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>, whose launch helpers and PList these functions use)

// ---------------------------------------------------------------- likeliest orders of a cohort (orders.h)
// Rows are decoded and checked here (model.py likeliest_order's errors -> status 2, reason in orders[i][0]), then cut
// into batches whose lattices fit the workspace limit; a row that does not fit on its own is status 3.  Every row is computed by
// one workgroup of its own, so a row's result does not depend on the batch it lands in.
struct OrdBuf {
  DevArr<ORow> rows;
  DevArr<double> tab, fvec, par;
  DevArr<uint32_t> fbp;
  DevArr<int> fcnt, status;
  DevArr<double> prob;
  DevArr<int8_t> order;
  DevArr<Desc> dd;
  DevArr<int2> map;
};
constexpr int ORD_BIG_K = 15;        // rows from this many slots up take the 1024-thread launch
static long long ord_bytes(const ORow& r, int cap) {
  const long long V = 1ll << r.k;
  return r.mode == ORD_PAIRED ? V * (5 * 8 + (long long)cap * (3 * 8 + 4) + 4) : V * (2 * 8 + 4);
}
template <typename T>
void likeliest_orders(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                      int ncols, int cap, int8_t* orders, double* prob, int32_t* status) {
  REQUIRE(ncols == 2 * E.n + 3, "dat must have 2 n_mut + 3 columns (states, diagnosis order, type)");
  REQUIRE(cap >= 0 && cap <= 65536, "front_cap must be in [0, 65536]");
  if (cap == 0) cap = MMHN_ORD_DEFAULT_FRONT_CAP;
  const int L = 2 * E.N - 1;
  std::memset(orders, -1, (size_t)npat * L);
  std::vector<ORow> todo;
  for (long long i = 0; i < npat; ++i) {
    ORow r;
    const int why = ord_decode(dat + i * ncols, ncols, E.n, r);
    prob[i] = std::nan("");
    if (why) { status[i] = 2; orders[i * L] = (int8_t)why; continue; }
    r.row = (int)i;
    if (r.k > MAXK || ord_bytes(r, cap) > (long long)E.cfg.plan.ws_limit) { status[i] = 3; continue; }
    status[i] = -1;
    todo.push_back(r);
  }
  if (todo.empty()) return;
  // the parameters: exp(log_theta) for k_diag (PS_THETA), the log-parameters themselves for k_orders
  E.build_params(lt, nullptr, nullptr);
  OrdBuf B;
  B.par.alloc((size_t)E.N * E.N + 2 * E.N);
  HIPCHECK(hipMemcpyAsync(B.par.p, lt, sizeof(double) * E.N * E.N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(B.par.p + E.N * E.N, obs1, sizeof(double) * E.N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(B.par.p + E.N * E.N + E.N, obs2, sizeof(double) * E.N, hipMemcpyHostToDevice, E.stream));
  size_t next = 0;
  while (next < todo.size()) {
    // one batch: rows in cohort order while their lattices fit; the small ones first, then the 1024-thread ones
    std::vector<ORow> small, big;
    long long used = 0;
    while (next < todo.size() && (small.empty() && big.empty() || used + ord_bytes(todo[next], cap) <= (long long)E.cfg.plan.ws_limit)) {
      used += ord_bytes(todo[next], cap);
      (todo[next].k >= ORD_BIG_K ? big : small).push_back(todo[next]);
      ++next;
    }
    std::vector<ORow> rows(small);
    rows.insert(rows.end(), big.begin(), big.end());
    long long toff = 0, foff = 0, coff = 0;
    std::vector<Desc> descs;
    std::vector<int2> map;
    std::vector<int8_t> st((size_t)(2 * E.n + 1));
    for (size_t j = 0; j < rows.size(); ++j) {
      ORow& r = rows[j];
      const long long V = 1ll << r.k;
      r.toff = toff; r.foff = foff; r.coff = coff;
      if (r.mode == ORD_PAIRED) {
        toff += 5 * V; foff += V * cap; coff += V;
        const int8_t* row = dat + (long long)r.row * ncols;
        Desc d = make_joint(row, E.n);                   // the joint diagonal of the row's state (mmhn_kron_diag's)
        d.off = r.toff;
        add_tiles(map, (int)descs.size(), d.k);
        descs.push_back(d);
      } else {
        toff += 2 * V; foff += V;
      }
      r.row = (int)j;
    }
    B.rows.alloc(rows.size());
    B.tab.alloc((size_t)std::max(toff, 1ll));
    B.fvec.alloc((size_t)std::max(3 * foff, 1ll));
    B.fbp.alloc((size_t)std::max(foff, 1ll));
    B.fcnt.alloc((size_t)std::max(coff, 1ll));
    B.status.alloc(rows.size()); B.prob.alloc(rows.size()); B.order.alloc(rows.size() * L);
    HIPCHECK(hipMemcpyAsync(B.rows.p, rows.data(), rows.size() * sizeof(ORow), hipMemcpyHostToDevice, E.stream));
    HIPCHECK(hipMemsetAsync(B.order.p, 0xFF, rows.size() * L, E.stream));
    if (!descs.empty()) {
      B.dd.alloc(descs.size()); B.map.alloc(map.size());
      HIPCHECK(hipMemcpyAsync(B.dd.p, descs.data(), descs.size() * sizeof(Desc), hipMemcpyHostToDevice, E.stream));
      HIPCHECK(hipMemcpyAsync(B.map.p, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
      E.launch_diag(E.main, B.dd.p, B.map.p, (int)map.size(), nullptr, B.tab.p, nullptr, KD_DQ);
    }
    const double* g_lt = B.par.p;
#define ORD_ARGS E.stream, B.rows.p + off, g_lt, g_lt + E.N * E.N, g_lt + E.N * E.N + E.N, E.N, cap, B.tab.p, B.fvec.p, B.fbp.p, \
               B.fcnt.p, B.order.p, B.prob.p, B.status.p, L
    if (!small.empty()) {
      const size_t off = 0;
      hipLaunchKernelGGL((k_orders<256>), dim3(small.size()), dim3(256), 0, ORD_ARGS);
      HIPCHECK(hipGetLastError());
    }
    if (!big.empty()) {
      const size_t off = small.size();
      hipLaunchKernelGGL((k_orders<1024>), dim3(big.size()), dim3(1024), 0, ORD_ARGS);
      HIPCHECK(hipGetLastError());
    }
#undef ORD_ARGS
    std::vector<int> bst(rows.size());
    std::vector<double> bpr(rows.size());
    std::vector<int8_t> bor(rows.size() * L);
    HIPCHECK(hipMemcpyAsync(bst.data(), B.status.p, rows.size() * sizeof(int), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipMemcpyAsync(bpr.data(), B.prob.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipMemcpyAsync(bor.data(), B.order.p, rows.size() * L, hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipStreamSynchronize(E.stream));
    for (size_t j = 0; j < rows.size(); ++j) {
      const long long i = (j < small.size() ? small[j] : big[j - small.size()]).row;
      status[i] = bst[j];
      prob[i] = bst[j] == 0 ? bpr[j] : std::nan("");
      std::memcpy(orders + i * L, bor.data() + j * L, (size_t)L);
      if (bst[j] != 0) std::memset(orders + i * L, -1, (size_t)L);
    }
  }
}

}  // namespace mmhn
