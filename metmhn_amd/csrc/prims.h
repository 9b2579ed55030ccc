// Single-problem primitives of the C ABI (capi.h: mmhn_kronvec, mmhn_resolvent, mmhn_x_partial_Q_y, ... and the mmhn_v_* ones):
// one restricted space per call, set up from scratch, run through the engine's launch helpers and copied back.  These are
// the paths of the API and the tests; the cohort evaluation (engine.hip) does not come through here.
#pragma once
#include <vector>

#include "host.h"
#include "plan.h"

namespace mmhn {

// (engine.hip includes this file behind the definition of Engine<T>, whose launch helpers and PList these functions use)

// ---------------------------------------------------------------- single-problem primitives (API / tests)
template <typename T>
struct Mini {
  Desc d;
  DevArr<Desc> dd;
  DevArr<int2> map, lmap;
  std::vector<int> lof;
  int ntiles = 0;
  DevArr<T> a, b, c, e, tab;
  PList<T> plist(long long vec) const { return PList<T>{dd.p, map.p, ntiles, d.k, vec, lmap.p, &lof, tab.p}; }
};
template <typename T>
void mini_setup(Engine<T>& E, Mini<T>& m, const Desc& d) {
  m.d = d;
  m.d.off = 0; m.d.aoff = 0; m.d.toff = 0;
  REQUIRE(d.k <= MAXK, "too many active events");
  std::vector<int2> mp;
  add_tiles(mp, 0, d.k);
  m.ntiles = (int)mp.size();
  std::vector<int2> lm;
  build_levels(mp, nullptr, false, lm, m.lof);
  m.lmap.alloc(lm.size());
  HIPCHECK(hipMemcpyAsync(m.lmap.p, lm.data(), lm.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
  m.dd.alloc(1); m.map.alloc(mp.size());
  HIPCHECK(hipMemcpyAsync(m.dd.p, &m.d, sizeof(Desc), hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(m.map.p, mp.data(), mp.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
  m.tab.alloc((size_t)std::max<long long>(table_size(m.d), 1));
  E.prep(E.main, m.dd.p, 1, m.tab.p);
  HIPCHECK(hipStreamSynchronize(E.stream));
}
template <typename T>
void up(Engine<T>& E, DevArr<T>& dst, const double* src, size_t count) {
  dst.alloc(count);
  std::vector<T> tmp(src, src + count);
  HIPCHECK(hipMemcpyAsync(dst.p, tmp.data(), count * sizeof(T), hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
}
template <typename T>
void down(Engine<T>& E, double* dst, const T* src, size_t count) {
  std::vector<T> tmp(count);
  HIPCHECK(hipMemcpyAsync(tmp.data(), src, count * sizeof(T), hipMemcpyDeviceToHost, E.stream));
  HIPCHECK(hipStreamSynchronize(E.stream));
  for (size_t i = 0; i < count; ++i) dst[i] = (double)tmp[i];
}

template <typename T>
void api_kronvec(Engine<T>& E, const Desc& d, const double* p, double* y, bool diag, bool tr) {
  Mini<T> m; mini_setup(E, m, d);
  const size_t V = (size_t)1 << d.k;
  up(E, m.a, p, V);
  m.b.alloc(V);
  E.poison_fill(E.main, m.b.p, (long long)V);
  if (d.k > TB) {
    std::vector<int2> live;
    for (int tl = 0; tl < m.ntiles; ++tl) if (!dead_tile(m.d, (uint32_t)tl)) live.push_back(make_int2(0, tl));
    DevArr<int2> dlive;
    DevArr<T> hxt;
    dlive.alloc(live.size());
    hxt.alloc(live.size() * (size_t)d.k);
    HIPCHECK(hipMemcpyAsync(dlive.p, live.data(), live.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
    HIPCHECK(hipMemsetAsync(m.b.p, 0, V * sizeof(T), E.stream));      // structurally zero tiles are not launched
    hipLaunchKernelGGL((k_hx<T>), dim3((unsigned)live.size()), dim3(64), 0, E.stream, m.dd.p, dlive.p, m.tab.p, hxt.p, d.k);
    HIPCHECK(hipGetLastError());
    E.launch_kv(E.main, tr, m.dd.p, dlive.p, (int)live.size(), d.k, m.a.p, m.b.p, m.tab.p, hxt.p);
    HIPCHECK(hipStreamSynchronize(E.stream));
  } else {
    E.launch_sweep(E.main, tr, m.dd.p, m.map.p, m.ntiles, d.k, m.a.p, m.b.p, nullptr, nullptr, 0, nullptr, 0, m.tab.p);
  }
  if (diag) E.launch_diag(E.main, m.dd.p, m.map.p, m.ntiles, m.a.p, m.b.p, nullptr, KD_ADDQP);
  down(E, y, m.b.p, V);
}
// ---- batched product (kronvec.py:499-539 applied to `batch` vectors of one restricted space): ONE launch over every
// tile of every vector.  Nothing is cleared beforehand: tiles where Q_off has no entries are zeroed by the kernel
// itself (k_kv's kind 1), so y may be any buffer - this is the launch sequence mmhn_bench_kronvec times.
template <typename T>
struct KvBatch {
  Desc d;
  long long batch = 0, V = 0;
  int ntiles = 0, nlive = 0;                    // tiles of the batch; those of them where Q_off has entries
  bool use_kv = false;
  DevArr<Desc> dd;
  DevArr<int2> map, live;                       // every tile; the tiles with entries (what the plain product launches)
  DevArr<int> zmap;                             // per live tile: the structurally zero tile its workgroup clears, -1: none
  DevArr<T> tab, hxl;                           // hxl: tile-bit factors of the live tiles
};
template <typename T>
void kv_setup(Engine<T>& E, KvBatch<T>& kb, const Desc& d0, long long batch) {
  REQUIRE(batch >= 1, "batch must be positive");
  REQUIRE(d0.k <= MAXK, "too many active events");
  kb.d = d0; kb.batch = batch; kb.V = 1ll << d0.k;
  std::vector<Desc> ds((size_t)batch, d0);
  std::vector<int2> mp;
  for (long long i = 0; i < batch; ++i) { ds[i].off = i * kb.V; ds[i].aoff = 0; ds[i].toff = 0; add_tiles(mp, (int)i, d0.k); }
  kb.ntiles = (int)mp.size();
  std::vector<int2> lv;
  std::vector<int> zm;
  for (const int2& m : mp) {
    if (dead_tile(ds[m.x], (uint32_t)m.y)) continue;
    lv.push_back(m);
    // a seeded tile clears its seed = 0 counterpart when Q_off has no entries there (dead tiles only exist with the
    // seeding bit above the tile bits, and the counterpart of a dead tile is always live)
    int z = -1;
    if (d0.mode == JOINT && d0.seedbit >= TB) {
      const uint32_t sb = 1u << (d0.seedbit - TB);
      if (((uint32_t)m.y & sb) && dead_tile(ds[m.x], (uint32_t)m.y & ~sb)) z = (int)((uint32_t)m.y & ~sb);
    }
    zm.push_back(z);
  }
  kb.nlive = (int)lv.size();
  {
    size_t cleared = 0;
    for (int z : zm) cleared += z >= 0;
    REQUIRE(cleared + lv.size() == mp.size(), "kronvec: a structurally zero tile has no live counterpart");
  }
  kb.live.alloc(lv.size()); kb.zmap.alloc(zm.size());
  HIPCHECK(hipMemcpyAsync(kb.live.p, lv.data(), lv.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(kb.zmap.p, zm.data(), zm.size() * sizeof(int), hipMemcpyHostToDevice, E.stream));
  kb.dd.alloc(ds.size()); kb.map.alloc(mp.size());
  HIPCHECK(hipMemcpyAsync(kb.dd.p, ds.data(), ds.size() * sizeof(Desc), hipMemcpyHostToDevice, E.stream));
  HIPCHECK(hipMemcpyAsync(kb.map.p, mp.data(), mp.size() * sizeof(int2), hipMemcpyHostToDevice, E.stream));
  kb.tab.alloc((size_t)std::max<long long>(table_size(d0), 1));
  E.prep(E.main, kb.dd.p, 1, kb.tab.p);                    // one table: every vector lives in the same space
  kb.use_kv = d0.k > TB;
  if (kb.use_kv) {
    kb.hxl.alloc(lv.size() * (size_t)d0.k);
    hipLaunchKernelGGL((k_hx<T>), dim3((unsigned)kb.nlive), dim3(64), 0, E.stream, kb.dd.p, kb.live.p, kb.tab.p, kb.hxl.p, d0.k);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipStreamSynchronize(E.stream));
}
// the live tiles, each seeded one also filling its counterpart without entries of Q_off (zeros; lidg * rhs in the
// fused Jacobi step): all of y is written by one launch
template <typename T>
void kv_launch(Engine<T>& E, const KvBatch<T>& kb, bool tr, const T* p, T* y, const T* lidg = nullptr, const T* rhs = nullptr) {
  if (kb.use_kv) E.launch_kv(E.main, tr, kb.dd.p, kb.live.p, kb.nlive, kb.d.k, p, y, kb.tab.p, kb.hxl.p, kb.zmap.p, lidg, rhs);
  else E.launch_sweep(E.main, tr, kb.dd.p, kb.map.p, kb.ntiles, kb.d.k, p, y, lidg, rhs, 0, nullptr, 0, kb.tab.p);
}
template <typename T>
void api_kronvec_batched(Engine<T>& E, const Desc& d, long long batch, const double* p, double* y, bool diag, bool tr) {
  KvBatch<T> kb; kv_setup(E, kb, d, batch);
  const size_t tot = (size_t)(batch * kb.V);
  DevArr<T> a, b;
  up(E, a, p, tot);
  b.alloc(tot);
  HIPCHECK(hipMemsetAsync(b.p, 0xFF, tot * sizeof(T), E.stream));   // NaN pattern: every element must be written by the launch
  kv_launch(E, kb, tr, a.p, b.p);
  if (diag) E.launch_diag(E.main, kb.dd.p, kb.map.p, kb.ntiles, a.p, b.p, nullptr, KD_ADDQP);
  down(E, y, b.p, tot);
}
// one fused Jacobi step of R_i_inv_vec (likelihood.py:253-255) for `batch` vectors of one space:
// y = lidg * (Q_off p + rhs) (transposed: Q_off^T), lidg = 1 / (D_p + D_m - diag Q) - the launch mmhn_bench_kronvec
// times with jacobi != 0
template <typename T>
void api_jacobi_step_batched(Engine<T>& E, const Desc& d, long long batch, const double* p, const double* rhs, double* y, bool tr) {
  KvBatch<T> kb; kv_setup(E, kb, d, batch);
  const size_t tot = (size_t)(batch * kb.V);
  DevArr<T> a, b, c, r;
  up(E, a, p, tot);
  up(E, r, rhs, tot);
  b.alloc(tot); c.alloc(tot);
  E.poison_fill(E.main, c.p, (long long)tot);
  E.launch_diag(E.main, kb.dd.p, kb.map.p, kb.ntiles, nullptr, c.p, nullptr, KD_LIDG);
  HIPCHECK(hipMemsetAsync(b.p, 0xFF, tot * sizeof(T), E.stream));
  kv_launch(E, kb, tr, a.p, b.p, c.p, r.p);
  down(E, y, b.p, tot);
}
template <typename T>
void api_diag(Engine<T>& E, const Desc& d, const double* p, double* outp, int what, int pbit = -1) {
  Mini<T> m; mini_setup(E, m, d);
  const size_t V = (size_t)1 << d.k;
  if (p) up(E, m.a, p, V);
  m.b.alloc(V);
  E.poison_fill(E.main, m.b.p, (long long)V);
  E.launch_diag(E.main, m.dd.p, m.map.p, m.ntiles, m.a.p, m.b.p, nullptr, what, pbit);
  down(E, outp, m.b.p, V);
}
// vanilla.x_partial_D_y (vanilla.py:190-203): weighted bit marginals of x * y under the two parts of scal_d_pt
template <typename T>
void api_xDy_single(Engine<T>& E, const Desc& d0, const double* x, const double* y, double* ddp, double* ddm) {
  Mini<T> m; mini_setup(E, m, d0);
  const size_t V = (size_t)1 << d0.k;
  up(E, m.a, y, V);
  up(E, m.b, x, V);
  m.e.alloc(64);
  E.poison_fill(E.main, m.e.p, 64);
  E.zero(E.main, m.e.p, 64);
  hipLaunchKernelGGL((k_bit_marg<T>), dim3(m.ntiles), dim3(BLOCK), 0, E.stream, m.dd.p, m.map.p, E.d_par.p, m.a.p,
                     m.b.p, m.e.p);
  HIPCHECK(hipGetLastError());
  double bm[64];
  down(E, bm, m.e.p, 64);
  for (int i = 0; i < E.N; ++i) {
    const int b = d0.bitP[i];
    ddp[i] = b >= 0 ? bm[b] : 0.0;
    ddm[i] = b >= 0 ? bm[32 + b] : 0.0;
  }
}
template <typename T>
void api_resolvent(Engine<T>& E, Desc d, const double* dvec, const double* x, double* y, bool tr) {
  if (dvec) d.obs = OBS_VEC;
  Mini<T> m; mini_setup(E, m, d);
  const size_t V = (size_t)1 << d.k;
  up(E, m.a, x, V);
  if (dvec) up(E, m.e, dvec, V);
  m.b.alloc(V); m.c.alloc(V);
  E.poison_fill(E.main, m.b.p, (long long)V);
  E.poison_fill(E.main, m.c.p, (long long)V);
  E.launch_diag(E.main, m.dd.p, m.map.p, m.ntiles, nullptr, m.c.p, m.e.p, KD_LIDG);
  E.solve(E.main, tr, m.plist((long long)V), m.b.p, m.c.p, m.a.p, 0, nullptr);
  down(E, y, m.b.p, V);
}
template <typename T>
void api_xQy_joint(Engine<T>& E, const Desc& d0, const double* x, const double* y, double* G) {
  Mini<T> m; mini_setup(E, m, d0);
  const size_t V = (size_t)1 << d0.k;
  up(E, m.a, y, V);   // p (right vector)
  up(E, m.b, x, V);   // q (left vector)
  m.c.alloc((size_t)a_size(m.d));
  m.e.alloc((size_t)3 * E.N * E.N);
  E.poison_fill(E.main, m.c.p, a_size(m.d));
  E.poison_fill(E.main, m.e.p, 3ll * E.N * E.N);
  E.zero(E.main, m.e.p, 3ll * E.N * E.N);
  E.zero(E.main, m.c.p, a_size(m.d));
  hipLaunchKernelGGL((k_class_marg<T>), dim3(m.ntiles), dim3(CMB), 2 * sizeof(T) << TB, E.stream, m.dd.p, m.map.p,
                     m.a.p, m.b.p, m.c.p);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL((k_eq_flows<T>), dim3(1), dim3(BLOCK), 0, E.stream, m.dd.p, static_cast<const WDesc*>(nullptr), m.a.p, m.b.p, m.c.p);
  HIPCHECK(hipGetLastError());
  for (int kd = 0; kd < 3; ++kd) {
    std::vector<int2> gc = grad_chunks(std::vector<Desc>{m.d}, kd);
    DevArr<int2> dgc; dgc.alloc(gc.size());
    HIPCHECK(hipMemcpy(dgc.p, gc.data(), gc.size() * sizeof(int2), hipMemcpyHostToDevice));
    E.launch_grad_rows(E.main, m.dd.p, 1, d0.k, m.c.p, nullptr, nullptr, m.e.p + kd * E.N * E.N, kd, dgc);
    HIPCHECK(hipStreamSynchronize(E.stream));
  }
  std::vector<double> g(3 * E.N * E.N);
  down(E, g.data(), m.e.p, g.size());
  for (int e = 0; e < E.N * E.N; ++e) G[e] = g[e] + g[E.N * E.N + e] + g[2 * E.N * E.N + e];
}
template <typename T>
void api_xQy_single(Engine<T>& E, const Desc& d0, const double* x, const double* y, double* G, double* ddiag) {
  Mini<T> m; mini_setup(E, m, d0);
  const size_t V = (size_t)1 << d0.k;
  up(E, m.a, y, V);
  up(E, m.b, x, V);
  m.e.alloc((size_t)E.N * E.N);
  E.poison_fill(E.main, m.e.p, (long long)E.N * E.N);
  E.zero(E.main, m.e.p, (long long)E.N * E.N);
  {
    std::vector<int2> gc = grad_chunks(std::vector<Desc>{m.d}, GK_S);
    DevArr<int2> dgc; dgc.alloc(gc.size());
    HIPCHECK(hipMemcpy(dgc.p, gc.data(), gc.size() * sizeof(int2), hipMemcpyHostToDevice));
    E.launch_grad_rows(E.main, m.dd.p, 1, d0.k, nullptr, m.a.p, m.b.p, m.e.p, GK_S, dgc);
    HIPCHECK(hipStreamSynchronize(E.stream));
  }
  down(E, G, m.e.p, (size_t)E.N * E.N);
  if (ddiag)
    for (int j = 0; j < E.N; ++j) {
      double s = 0;
      for (int i = 0; i < E.N; ++i) if (i != j) s -= G[i * E.N + j];
      ddiag[j] = s;
    }
}
template <typename T>
void api_xDy_joint(Engine<T>& E, const Desc& d0, const double* x, const double* y, double* ddp, double* ddm) {
  Mini<T> m; mini_setup(E, m, d0);
  const size_t V = (size_t)1 << d0.k;
  up(E, m.a, y, V);
  up(E, m.b, x, V);
  m.e.alloc(64);
  E.poison_fill(E.main, m.e.p, 64);
  E.zero(E.main, m.e.p, 64);
  hipLaunchKernelGGL((k_bit_marg<T>), dim3(m.ntiles), dim3(BLOCK), 0, E.stream, m.dd.p, m.map.p, E.d_par.p, m.a.p,
                     m.b.p, m.e.p);
  HIPCHECK(hipGetLastError());
  double bm[64];
  down(E, bm, m.e.p, 64);
  for (int i = 0; i < E.N; ++i) {
    const int bp = i == E.n ? d0.seedbit : d0.bitP[i];
    const int bq = i == E.n ? d0.seedbit : d0.bitM[i];
    ddp[i] = bp >= 0 ? bm[bp] : 0.0;
    ddm[i] = bq >= 0 ? bm[32 + bq] : 0.0;
  }
}

// compatible indices (obs_states + jnp.where(size=)): integer host arithmetic, bit-exact
static void obs_indices(const Desc& d, bool pt_first, int64_t* idx, int64_t* count) {
  REQUIRE(d.seedbit >= 0, "obs_states needs an active seeding slot");
  const uint32_t fixed = (pt_first ? d.maskP : d.maskM) | (1u << d.seedbit);
  const uint32_t free_ = pt_first ? d.maskM : d.maskP;
  const int64_t cntv = (int64_t)1 << popc(free_);
  for (int64_t e = 0; e < cntv; ++e) {
    uint32_t v = (uint32_t)e, m = free_, o = 0;
    while (m) { const uint32_t low = m & (0u - m); if (v & 1u) o |= low; v >>= 1; m ^= low; }
    idx[e] = (int64_t)(o | fixed);
  }
  *count = cntv;
}

}  // namespace mmhn
