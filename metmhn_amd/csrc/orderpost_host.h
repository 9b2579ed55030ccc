// Host side of the order-posterior entry points of a cohort: row decoding (orders.h: ord_decode, the one
// mmhn_likeliest_orders uses), limits, batching, launches and the copy back, in one place (opr_rows) - orderprec_host.h,
// orderpos_host.h and ordersample_host.h call it too -, and the pre-seeding posteriors themselves (orderpost.h: k_order_post).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "host.h"
#include "orderpost.h"
#include "plan.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T> and orders_host.h, whose ORD_BIG_K it shares)

// k_order_post / k_order_prec (orderprec.h) / k_order_pos (orderpos.h): each writes log_ev and one block of doubles per row
using OprKernel = void (*)(const ORow*, const double*, const double*, const double*, int, double*, double*, double*);

// the launch of these three kernels as opr_rows takes it
inline auto opr_launch(OprKernel k256, OprKernel k1024) {
  return [=](bool big, size_t grid, hipStream_t stream, const ORow* rows, const double* par, int N, double* tab, double* le,
             double* out, int8_t*) {
    hipLaunchKernelGGL(big ? k1024 : k256, dim3(grid), dim3(big ? 1024 : 256), 0, stream, rows, par, par + N * N,
                       par + N * N + N, N, tab, le, out);
  };
}

// Rows are decoded and checked (status MMHN_ORD_INVALID with the reason in the high half), then cut into batches whose
// lattices fit the workspace limit; a row that does not fit on its own is MMHN_ORD_TOO_LARGE.  The workspace is
// allocated once, for the largest batch.  One workgroup per row (256 threads below ORD_BIG_K slots, 1024 from there on), so
// a row's result does not depend on the batch it lands in.  Per entry point: launch(big, rows of the launch, stream, their
// ORow, parameters lt / obs1 / obs2 one behind the other, N, workspace, log_ev, the batch's block of doubles, its block of
// bytes) starts the kernel (opr_launch for those that write doubles only), doubles(row) the row's workspace in doubles,
// block(row) the doubles of its output block, obytes(row) the bytes of its int8 output block, count_out: the output blocks
// count in the batch cut beside the workspace, fits(row) what else the kernel asks of a row, scatter(row, cohort row, block
// of doubles, block of bytes) takes a finished row's blocks to the caller's arrays; the caller fills (NaN, -1) what no
// finished row writes.
// A kernel finds its blocks by ORow::foff, the row's offset in the block of doubles - a kernel with an int8 block writes
// the same number of entries per double to it -, and the cohort row in ORow::pad_.
template <typename T, class Launch, class Doubles, class Block, class Bytes, class Fits, class Scatter>
void opr_rows(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
              int ncols, double* log_ev, int32_t* status, Launch launch, Doubles doubles, Block block, Bytes obytes,
              bool count_out, Fits fits, Scatter scatter) {
  REQUIRE(ncols == 2 * E.n + 3, "dat must have 2 n_mut + 3 columns (states, diagnosis order, type)");
  REQUIRE(E.N <= ORD_MAXN, "too many events for the order kernels (n_mut <= 31)");
  const int n = E.n, N = E.N;
  std::fill(log_ev, log_ev + npat, std::nan(""));
  const long long limit = (long long)E.cfg.plan.ws_limit;
  const auto bytes = [&](const ORow& r) {
    const long long out = count_out ? (long long)block(r) * (long long)sizeof(double) + (long long)obytes(r) : 0;
    return (long long)doubles(r) * (long long)sizeof(double) + out;
  };
  std::vector<ORow> todo;
  for (long long i = 0; i < npat; ++i) {
    ORow r;
    const int why = ord_decode(dat + i * ncols, ncols, n, r);
    if (why) { status[i] = MMHN_ORD_INVALID | (why << 16); continue; }
    r.row = (int)i;
    if (r.k > MAXK || !fits(r) || bytes(r) > limit) { status[i] = MMHN_ORD_TOO_LARGE; continue; }
    status[i] = MMHN_ORD_OK;
    todo.push_back(r);
  }
  if (todo.empty()) return;
  // batches [first, last) of todo, rows in cohort order while their lattices fit
  std::vector<size_t> cut{0};
  long long used = 0, ws = 0, most = 0;                  // most: doubles of the largest batch's workspace
  for (size_t j = 0; j < todo.size(); ++j) {
    const long long b = bytes(todo[j]);
    if (j > cut.back() && used + b > limit) { cut.push_back(j); used = 0; ws = 0; }
    used += b;
    ws += doubles(todo[j]);
    most = std::max(most, ws);
  }
  cut.push_back(todo.size());
  // the parameters: exp(log_theta) for k_diag (PS_THETA), the log-parameters themselves for the order kernel
  E.build_params(lt, nullptr, nullptr);
  DevArr<double> par, tab, d_le, d_out;
  DevArr<int8_t> d_bytes;
  DevArr<ORow> d_rows;
  DevArr<Desc> dd;
  DevArr<int2> dmap;
  par.alloc((size_t)N * N + 2 * N);
  HIPCHECK(hipMemcpyAsync(par.p, lt, sizeof(double) * N * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N, obs1, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(par.p + N * N + N, obs2, sizeof(double) * N, hipMemcpyHostToDevice, E.stream));
  tab.alloc((size_t)most);
  for (size_t c = 0; c + 1 < cut.size(); ++c) {
    // the small rows first, then the 1024-thread ones
    std::vector<ORow> small, big;
    for (size_t j = cut[c]; j < cut[c + 1]; ++j) (todo[j].k >= ORD_BIG_K ? big : small).push_back(todo[j]);
    std::vector<ORow> rows(small);
    rows.insert(rows.end(), big.begin(), big.end());
    std::vector<long long> src(rows.size()), boffs(rows.size());
    long long toff = 0, poff = 0, boff = 0;
    std::vector<Desc> descs;
    std::vector<int2> map;
    for (size_t j = 0; j < rows.size(); ++j) {
      ORow& r = rows[j];
      src[j] = r.row;
      r.toff = toff;
      r.coff = toff + opost_doubles(r);                               // the move-mass kernels' partials; k_order_post has none there
      r.foff = poff;
      r.pad_ = r.row;                                                 // the cohort row (the sample kernel's random stream)
      boffs[j] = boff;
      toff += doubles(r);
      poff += block(r);
      boff += obytes(r);
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
    d_rows.alloc(R); d_le.alloc(R); d_out.alloc((size_t)poff + 1);
    HIPCHECK(hipMemcpyAsync(d_rows.p, rows.data(), R * sizeof(ORow), hipMemcpyHostToDevice, E.stream));
    if (!descs.empty()) {
      dd.alloc(descs.size()); dmap.alloc(map.size());
      HIPCHECK(hipMemcpyAsync(dd.p, descs.data(), descs.size() * sizeof(Desc), hipMemcpyHostToDevice, E.stream));
      HIPCHECK(hipMemcpyAsync(dmap.p, map.data(), map.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
      E.launch_diag(E.main, dd.p, dmap.p, (int)map.size(), nullptr, tab.p, nullptr, KD_DQ);
    }
    if (boff) d_bytes.alloc((size_t)boff);
    if (!small.empty()) {
      launch(false, small.size(), E.stream, d_rows.p, par.p, N, tab.p, d_le.p, d_out.p, d_bytes.p);
      HIPCHECK(hipGetLastError());
    }
    if (!big.empty()) {
      launch(true, big.size(), E.stream, d_rows.p + small.size(), par.p, N, tab.p, d_le.p, d_out.p, d_bytes.p);
      HIPCHECK(hipGetLastError());
    }
    std::vector<double> b_le(R), b_out((size_t)poff + 1);
    std::unique_ptr<int8_t[]> b_bytes(new int8_t[(size_t)boff + 1]);      // (not zeroed: it can be the largest array of the call)
    if (boff) HIPCHECK(hipMemcpyAsync(b_bytes.get(), d_bytes.p, (size_t)boff, hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipMemcpyAsync(b_le.data(), d_le.p, R * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipMemcpyAsync(b_out.data(), d_out.p, (size_t)poff * sizeof(double), hipMemcpyDeviceToHost, E.stream));
    HIPCHECK(hipStreamSynchronize(E.stream));
    for (size_t j = 0; j < R; ++j) {
      log_ev[src[j]] = b_le[j];
      scatter(rows[j], src[j], b_out.data() + rows[j].foff, b_bytes.get() + boffs[j]);
    }
  }
}

// pre [npat][n], seed_pos [npat][n+1]: NaN in the "absent" rows, which have no seeding to place.  With 76 B per sub-state a
// cohort is normally one batch.
template <typename T>
void order_posteriors(Engine<T>& E, const double* lt, const double* obs1, const double* obs2, const int8_t* dat, long long npat,
                      int ncols, double* log_ev, double* pre, double* seed_pos, int32_t* status) {
  const int n = E.n, N = E.N;
  std::fill(pre, pre + npat * n, std::nan(""));
  std::fill(seed_pos, seed_pos + npat * N, std::nan(""));
  opr_rows(E, lt, obs1, obs2, dat, npat, ncols, log_ev, status, opr_launch(k_order_post<256>, k_order_post<1024>),
           [](const ORow& r) { return opost_doubles(r); }, [&](const ORow&) { return (long long)n + N; },
           [](const ORow&) { return 0ll; }, false, [](const ORow&) { return true; },
           [&](const ORow&, long long i, const double* in, const int8_t*) {
             if (dat[i * ncols + ncols - 1] == 0) return;                  // "absent": no seeding in the observation, NaN
             std::memcpy(pre + i * n, in, sizeof(double) * n);
             std::memcpy(seed_pos + i * N, in + n, sizeof(double) * N);
           });
}

}  // namespace mmhn
