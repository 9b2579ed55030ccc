// Host side of the pairwise precedence posteriors of a cohort (orderprec.h: k_order_prec): row decoding (orders.h:
// ord_decode, the one mmhn_likeliest_orders uses), batching, launches, the scatter of a row's compact slot matrix to the
// event codes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "host.h"
#include "orderprec.h"
#include "plan.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T> and orders_host.h, whose ORD_BIG_K it shares)

static long long oprec_bytes(const ORow& r) {
  return oprec_doubles(r, r.k >= ORD_BIG_K ? 1024 : 256) * (long long)sizeof(double);
}

// k_order_prec / k_order_pos (orderpos.h): both write log_ev and a compact k x k block per row
using OprKernel = void (*)(const ORow*, const double*, const double*, const double*, int, double*, double*, double*);

// Rows are decoded and checked (status MMHN_ORD_INVALID with the reason in the high half), then cut into batches whose
// lattices fit the workspace limit; a row that does not fit on its own is MMHN_ORD_TOO_LARGE.  The workspace is
// allocated once, for the largest batch.  One workgroup per row (k256 below ORD_BIG_K slots, k1024 from there on), so a
// row's result does not depend on the batch it lands in.  scatter(row, cohort row, block) takes a finished row's k x k
// block to the caller's arrays, which the caller has filled with NaN.
template <typename T, class Scatter>
void opr_rows(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
              int ncols, double* log_ev, int32_t* status, OprKernel k256, OprKernel k1024, Scatter scatter) {
  REQUIRE(ncols == 2 * E.n + 3, "dat must have 2 n_mut + 3 columns (states, diagnosis order, type)");
  REQUIRE(E.N <= ORD_MAXN, "too many events for the order kernels (n_mut <= 31)");
  const int n = E.n, N = E.N;
  std::fill(log_ev, log_ev + npat, std::nan(""));
  const long long limit = (long long)E.cfg.plan.ws_limit;
  std::vector<ORow> todo;
  for (long long i = 0; i < npat; ++i) {
    ORow r;
    const int why = ord_decode(dat + i * ncols, ncols, n, r);
    if (why) { status[i] = MMHN_ORD_INVALID | (why << 16); continue; }
    r.row = (int)i;
    // (more than OPO_CB joint events, 23 slots or more: the unseeded states would not fit the kernels' LDS)
    if (r.k > MAXK || __builtin_popcount(r.joint) > OPO_CB || oprec_bytes(r) > limit) { status[i] = MMHN_ORD_TOO_LARGE; continue; }
    status[i] = MMHN_ORD_OK;
    todo.push_back(r);
  }
  if (todo.empty()) return;
  // batches [first, last) of todo, rows in cohort order while their lattices fit
  std::vector<size_t> cut{0};
  long long used = 0, most = 0;
  for (size_t j = 0; j < todo.size(); ++j) {
    const long long b = oprec_bytes(todo[j]);
    if (j > cut.back() && used + b > limit) { cut.push_back(j); used = 0; }
    used += b;
    most = std::max(most, used);
  }
  cut.push_back(todo.size());
  // the parameters: exp(log_theta) for k_diag (PS_THETA), the log-parameters themselves for the order kernel
  E.build_params(lt, nullptr, nullptr);
  DevArr<double> par, tab, d_le, d_prec;
  DevArr<ORow> d_rows;
  DevArr<Desc> dd;
  DevArr<int2> dmap;
  par.alloc((size_t)N * N + 2 * N);
  HIPCHECK(hipMemcpyAsync(par.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N, obs1, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N + N, obs2, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  tab.alloc((size_t)(most / (long long)sizeof(double)));
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    // the small rows first, then the 1024-thread ones
    std::vector<ORow> small, big;
    for (size_t j = cut[c]; j < cut[c + 1]; ++j) (todo[j].k >= ORD_BIG_K ? big : small).push_back(todo[j]);
    std::vector<ORow> rows(small);
    rows.insert(rows.end(), big.begin(), big.end());
    std::vector<long long> src(rows.size());
    long long toff = 0, poff = 0;
    std::vector<Desc> descs;
    std::vector<int2> map;
    for (size_t j = 0; j < rows.size(); ++j) {
      ORow& r = rows[j];
      src[j] = r.row;
      r.toff = toff;
      r.coff = toff + opost_doubles(r);
      r.foff = poff;
      toff += oprec_bytes(r) / (long long)sizeof(double);
      poff += (long long)r.k * r.k;
      if (r.mode == ORD_PAIRED) {
        Desc d = make_joint(dat + (long long)r.row * ncols, n);       // the joint diagonal of the row's state (mmhn_kron_diag's)
        d.off = r.toff;
        add_tiles(map, (int)descs.size(), d.k);
        descs.push_back(d);
      }
      r.row = (int)j;
    }
    REQUIRE((size_t)toff <= tab.n, "order kernels: batch larger than its workspace");
    const size_t R = rows.size();
    d_rows.alloc(R); d_le.alloc(R); d_prec.alloc((size_t)poff + 1);
    HIPCHECK(hipMemcpyAsync(d_rows.p, rows.data(), R * sizeof(ORow), hipMemcpyHostToDevice, E.stream));
    if (!descs.empty()) {
      dd.alloc(descs.size()); dmap.alloc(map.size());
      HIPCHECK(hipMemcpyAsync(dd.p, descs.data(), descs.size() * sizeof(Desc), hipMemcpyHostToDevice, E.stream));
      HIPCHECK(hipMemcpyAsync(dmap.p, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
      E.launch_diag(dd.p, dmap.p, (int)map.size(), nullptr, tab.p, nullptr, KD_DQ);
    }
#define OPR_ARGS E.stream, d_rows.p + off, par.p, par.p + N * N, par.p + N * N + N, N, tab.p, d_le.p, d_prec.p
    if (!small.empty()) {
      const size_t off = 0;
      hipLaunchKernelGGL(k256, dim3(small.size()), dim3(256), 0, OPR_ARGS);
      HIPCHECK(hipGetLastError());
    }
    if (!big.empty()) {
      const size_t off = small.size();
      hipLaunchKernelGGL(k1024, dim3(big.size()), dim3(1024), 0, OPR_ARGS);
      HIPCHECK(hipGetLastError());
    }
#undef OPR_ARGS
    std::vector<double> b_le(R), b_prec((size_t)poff + 1);
    HIPCHECK(hipMemcpyAsync(b_le.data(), d_le.p, R * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipMemcpyAsync(b_prec.data(), d_prec.p, (size_t)poff * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipStreamSynchronize(E.stream));
    for (size_t j = 0; j < R; ++j) {
      log_ev[src[j]] = b_le[j];
      scatter(rows[j], src[j], b_prec.data() + rows[j].foff);
    }
  }
}

// prec [npat][2n+1][2n+1] over the event codes: NaN where a code is not in the row.
template <typename T>
void order_precedences(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                       int ncols, double* log_ev, double* prec, int32_t* status) {
  const long long L = 2 * E.n + 1;
  std::fill(prec, prec + npat * L * L, std::nan(""));
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, k_order_prec<256>, k_order_prec<1024>,
           [&](const ORow& r, long long i, const double* in) {
             double* out = prec + i * L * L;
             for (int a = 0; a < r.k; ++a)
               for (int b = 0; b < r.k; ++b) out[r.code[a] * L + r.code[b]] = in[a * r.k + b];
           });
}

}  // namespace mmhn
