// Likeliest event orders of a cohort: the device form of metmhn_amd/model.py MetMHN.likeliest_order.
//
// One workgroup per row walks the row's lattice of 2^k sub-states level by level (level = popcount); the whole lattice
// lives in the batch workspace, so a level reads the levels below it after a barrier and nothing else synchronises.
//   ORD_PT / ORD_MT  max-product Viterbi over a one-tumour chain (model.py _single_tables / _single_viterbi):
//                    best[x] = max_b best[x - b] num_b[x] / den[x], one back-pointer (the slot) per state.
//   ORD_PAIRED       the Pareto-front DP of model.py _likeliest_order_paired: per sub-state, every candidate vector
//                    (a, b_P, b_M) no other candidate dominates once "the first observation happens here" is folded in
//                    (_settle); candidates are stored unsettled with one back-pointer each (predecessor candidate, slot,
//                    joint flag).  Before the seeding only joint events (slots b, b+1) move and a state keeps the
//                    candidate with the largest a; a joint move spans two levels, which the stored lattice covers.
// Per-row tables (den, o1, o2, den_mt, den_pt) are computed once at the start of the launch; the numerators num_b[y]
// (k x 2^k values) are formed on the fly.  The diagonal of the restricted joint rate matrix is k_diag's (diag.h),
// launched before this kernel into the row's den table.  Sums and products are formed in the host code's order
// (ascending bit, exp of the summed logs), so the probabilities agree with it to a few ulp.
// A front that would exceed its capacity sets the row's overflow flag: the row is finished with truncated fronts and
// reported as status 1, never as a result.  fp64 only.
#pragma once
#include <cstring>
#include "common.h"
#include "../../include/metmhn_amd.h"

namespace mmhn {

enum { ORD_PT = 0, ORD_MT = 1, ORD_PAIRED = 2 };
enum { ORD_K_PT = 0, ORD_K_MT = 1, ORD_K_SEED = 2 };     // slot kinds of a paired row (model.py _paired_tables: kind)
constexpr int ORD_MAXN = 32;

struct ORow {
  int k;               // occupied slots (index bits of the lattice)
  int mode;            // ORD_PT / ORD_MT / ORD_PAIRED
  int pt_first, mt_first;
  int row;             // row of the output arrays
  int pad_;            // the cohort row (opr_rows sets it; `row` is the row of the batch there)
  long long toff;      // tables: paired den, o1, o2, den_mt, den_pt (5 x 2^k); one tumour den, best (2 x 2^k)
  long long foff;      // front slots (paired: 2^k x cap) / back-pointers of the Viterbi (2^k)
  long long coff;      // front sizes (paired: 2^k)
  uint32_t joint;      // paired: PT slots b whose slot b+1 is the same event in the metastasis
  uint32_t pt_mask, mt_mask;
  int seeded_top;      // one tumour: the seeding is the top slot
  int8_t ev[32];       // event of slot b (seeding: n)
  int8_t kind[32];     // ORD_K_* of slot b (paired)
  int8_t code[32];     // event code written to the order for slot b
};

// decode row `row` of dat (post_training_analyses.ipynb: type column -1, diagnosis order -2); 0 or MMHN_ORD_* reason
inline int ord_decode(const int8_t* row, int ncols, int n, ORow& r) {
  std::memset(&r, 0, sizeof(r));
  const int type = row[ncols - 1], first = row[ncols - 2];
  const bool seed = row[2 * n] != 0;
  auto pt = [&](int e) { return row[2 * e] != 0; };
  auto mt = [&](int e) { return row[2 * e + 1] != 0; };
  bool any_pt = false, any_mt = false, same = true;
  for (int e = 0; e < n; ++e) { any_pt |= pt(e); any_mt |= mt(e); same &= pt(e) == mt(e); }
  int k = 0;
  // slot k of the row; a row of more than MAXK slots only counts them (the caller turns it away as too large)
  auto put = [&](int e, int code, int kd) {
    if (k < MAXK) {
      r.ev[k] = (int8_t)e; r.code[k] = (int8_t)code; r.kind[k] = (int8_t)kd;
      if (kd == ORD_K_PT) r.pt_mask |= 1u << k;
      if (kd == ORD_K_MT) r.mt_mask |= 1u << k;
    }
    ++k;
  };
  if (type == 0 || type == 1) {                          // "absent" / "present": the primary tumour's chain
    if (type == 0 && (seed || any_mt)) return MMHN_ORD_ABSENT_MET;
    if (type == 1 && (!seed || any_mt)) return MMHN_ORD_PRESENT_MET;
    r.mode = ORD_PT;
    for (int e = 0; e < n; ++e) if (pt(e)) put(e, 2 * e, ORD_K_PT);
    if (seed) put(n, 2 * n, ORD_K_SEED);
    r.seeded_top = seed;
  } else if (type == 2) {                                // "isMetastasis": the metastasis' chain after the seeding
    if (any_pt) return MMHN_ORD_MT_PT_PART;
    if (!seed) return MMHN_ORD_MT_NO_SEEDING;
    r.mode = ORD_MT;
    for (int e = 0; e < n; ++e) if (mt(e)) put(e, 2 * e + 1, ORD_K_MT);
    put(n, 2 * n, ORD_K_SEED);
    r.seeded_top = 1;
  } else if (type == 3) {     // "isPaired": diag_order 0 "unknown", 1 "PT", any other "Met" (as the objective reads it)
    if (!seed && !same) return MMHN_ORD_UNREACHABLE;
    if (!seed) return MMHN_ORD_NO_SEEDING;
    r.mode = ORD_PAIRED;
    r.pt_first = first == 0 || first == 1;
    r.mt_first = first != 1;
    for (int s = 0; s <= 2 * n; ++s)
      if (row[s]) put(s == 2 * n ? n : s / 2, s, s == 2 * n ? ORD_K_SEED : (s & 1));
    for (int b = 0; b + 1 < k && b + 1 < MAXK; ++b)
      if (r.kind[b] == ORD_K_PT && r.kind[b + 1] == ORD_K_MT && r.ev[b] == r.ev[b + 1]) r.joint |= 1u << b;
  } else {
    return MMHN_ORD_BAD_STATUS;
  }
  r.k = k;
  return 0;
}

// back-pointer word: predecessor candidate (16 bits) | slot (8 bits) | joint flag
__device__ __forceinline__ uint32_t ord_bp(int pc, int b, bool jnt) { return (uint32_t)pc | ((uint32_t)b << 16) | (jnt ? 1u << 24 : 0u); }

struct OrdTab {
  const double* o1;
  const double* o2;
  const double* dmt;
  const double* dpt;
};

// _settle: fold "the first observation happens at y" into the b's
__device__ __forceinline__ void ord_settle(const ORow& r, const OrdTab& t, uint32_t y, double& a, double& bp, double& bm) {
  if ((y >> (r.k - 1)) & 1u) {
    if (r.pt_first && (y & r.pt_mask) == r.pt_mask) bp = bp + a * t.o1[y] / t.dmt[y];
    if (r.mt_first && (y & r.mt_mask) == r.mt_mask) bm = bm + a * t.o2[y] / t.dpt[y];
  }
}

// exp(sum over the set bits j of y in `flags`, ascending, of lt[e][ev_j]) - model.py's exp(_subset_sums(...)[y]);
// pt: the primary tumour does not feel the seeding (theta[i, n] = 0 for i < n)
__device__ __forceinline__ double ord_num(const double* lt, int N, const ORow& r, int e, uint32_t y, bool pt) {
  const int n = N - 1;
  double s = 0.0;
  for (uint32_t m = y; m; m &= m - 1) {
    const int j = __builtin_ctz(m), f = r.ev[j];
    if (!(pt && f == n && e < n)) s += lt[e * N + f];
  }
  return exp(s);
}

// model.py _single_diag over the events `n_events` with the slots in `sel` as the event list: minus the summed rates of
// every event not yet present at y
__device__ __forceinline__ double ord_single_diag(const double* lt, int N, const ORow& r, uint32_t sel, uint32_t y,
                                                  int n_events, bool pt) {
  const int n = N - 1;
  double dg = 0.0;
  for (int i = 0; i < n_events; ++i) {
    double s = 0.0;
    bool present = false;
    for (uint32_t m = y & sel; m; m &= m - 1) {
      const int j = __builtin_ctz(m), f = r.ev[j];
      if (f == i) present = true;
      if (!(pt && f == n && i < n)) s += lt[i * N + f];
    }
    const double rate = exp(lt[i * N + i] + s);
    dg -= present ? 0.0 : rate;
  }
  return dg;
}

__device__ __forceinline__ double ord_obs_sum(const double* w, const ORow& r, uint32_t y) {
  double s = 0.0;
  for (uint32_t m = y; m; m &= m - 1) s += w[r.ev[__builtin_ctz(m)]];
  return s;
}

// rows[blockIdx.x]; lt [N][N], obs1 / obs2 [N]; diagJ already in tab[toff ..] of the paired rows (k_diag, KD_DQ).
// out_order [row][L], out_prob [row], out_status [row] (0 ok, 1 front overflow)
template <int KB>
__global__ __launch_bounds__(KB) void k_orders(const ORow* __restrict__ rows, const double* __restrict__ g_lt,
                                               const double* __restrict__ g_o1, const double* __restrict__ g_o2, int N,
                                               int cap, double* tab, double* fvec, uint32_t* fbp, int* fcnt,
                                               int8_t* out_order, double* out_prob, int* out_status, int L) {
  __shared__ double lt[ORD_MAXN * ORD_MAXN];
  __shared__ double o1w[ORD_MAXN], o2w[ORD_MAXN];
  __shared__ ORow r;
  __shared__ int overflow;
  const int tid = threadIdx.x;
  for (int i = tid; i < N * N; i += KB) lt[i] = g_lt[i];
  for (int i = tid; i < N; i += KB) { o1w[i] = g_o1[i]; o2w[i] = g_o2[i]; }
  if (tid == 0) { r = rows[blockIdx.x]; overflow = 0; }
  __syncthreads();
  const int n = N - 1, k = r.k;
  const uint32_t V = 1u << k, full = V - 1u;
  double* den = tab + r.toff;

  if (r.mode != ORD_PAIRED) {
    // ---------------------------------------------------------------- one tumour: _single_tables + _single_viterbi
    const bool pt = r.mode == ORD_PT;
    const double* after = pt ? o1w : o2w;
    double* best = den + V;
    uint32_t* last = fbp + r.foff;
    for (uint32_t x = tid; x < V; x += KB) {
      const bool sd = r.seeded_top && ((x >> (k - 1)) & 1u);
      const double ob = exp(sd ? ord_obs_sum(after, r, x) : ord_obs_sum(o1w, r, x));
      den[x] = ob - ord_single_diag(lt, N, r, full, x, N, pt);
    }
    __syncthreads();
    if (tid == 0) best[0] = 1.0 / den[0];
    __syncthreads();
    for (int lev = 1; lev <= k; ++lev) {
      for (uint32_t x = tid; x < V; x += KB) {
        if (__builtin_popcount(x) != lev) continue;
        double top = -1.0;
        int arg = -1;
        for (uint32_t m = x; m; m &= m - 1) {
          const int b = __builtin_ctz(m);
          const double c = best[x ^ (1u << b)] * ord_num(lt, N, r, r.ev[b], x, pt);
          if (c > top) { top = c; arg = b; }
        }
        best[x] = top / den[x];
        last[x] = (uint32_t)arg;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const bool sd = r.seeded_top && k > 0;
      const double fin = exp(sd ? ord_obs_sum(after, r, full) : ord_obs_sum(o1w, r, full));
      int8_t* o = out_order + (long long)r.row * L;
      uint32_t x = full;
      for (int i = k - 1; i >= 0; --i) {
        const int b = (int)last[x];
        o[i] = r.code[b];
        x ^= 1u << b;
      }
      out_prob[r.row] = best[full] * fin;
      out_status[r.row] = 0;
    }
    return;
  }

  // ---------------------------------------------------------------- both tumours: _paired_tables
  double* o1 = den + V;
  double* o2 = o1 + V;
  double* dmt = o2 + V;
  double* dpt = dmt + V;
  const uint32_t seedm = 1u << (k - 1);
  const uint32_t in_mt = r.mt_mask | seedm;
  for (uint32_t x = tid; x < V; x += KB) {
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t m = x; m; m &= m - 1) {
      const int j = __builtin_ctz(m);
      if (r.kind[j] != ORD_K_MT) s1 += o1w[r.ev[j]];
      if (r.kind[j] != ORD_K_PT) s2 += o2w[r.ev[j]];
    }
    const double e1 = exp(s1), e2 = exp(s2);
    o1[x] = e1; o2[x] = e2;
    den[x] = (e1 + ((x & seedm) ? e2 : 0.0)) - den[x];
    // the tumour left after the first observation runs on alone: the metastasis with the seeding's effects under obs2,
    // the primary tumour without them under obs1
    if (r.pt_first) dmt[x] = e2 - ord_single_diag(lt, N, r, in_mt, x, N, false);
    if (r.mt_first) dpt[x] = e1 - ord_single_diag(lt, N, r, r.pt_mask, x, n, false);
  }
  const OrdTab t{o1, o2, dmt, dpt};
  double* fv = fvec + 3 * r.foff;
  uint32_t* fb = fbp + r.foff;
  int* cnt = fcnt + r.coff;
  if (tid == 0) {
    fv[0] = 1.0 / den[0]; fv[1] = 0.0; fv[2] = 0.0;       // reads den[0], written by thread 0 above
    fb[0] = 0u;
    cnt[0] = 1;
  }
  __syncthreads();

  for (int lev = 1; lev <= k; ++lev) {
    for (uint32_t y = tid; y < V; y += KB) {
      if (__builtin_popcount(y) != lev) continue;
      const long long ys = (long long)y * cap;
      if (!(y & seedm)) {
        // before the seeding: both tumours carry the same events, joint moves only, the largest a is kept
        const uint32_t lo = y & r.joint;
        if (y != (lo | lo << 1)) { cnt[y] = 0; continue; }
        double top = -1.0;
        int arg = -1;
        for (uint32_t m = lo; m; m &= m - 1) {
          const int b = __builtin_ctz(m);
          const uint32_t x = y ^ (3u << b);
          const double a = fv[3 * (long long)x * cap] * ord_num(lt, N, r, r.ev[b], y & r.pt_mask, false) / den[y];
          if (a > top) { top = a; arg = b; }
        }
        fv[3 * ys] = top; fv[3 * ys + 1] = 0.0; fv[3 * ys + 2] = 0.0;
        fb[ys] = ord_bp(0, arg, true);
        cnt[y] = 1;
        continue;
      }
      // seeded: every move; the front is kept as the candidates no other one dominates (model.py _pareto: the first
      // of equal vectors wins; candidates in ascending slot, then in the predecessor's front order)
      int nk = 0;
      for (uint32_t m = y; m; m &= m - 1) {
        const int b = __builtin_ctz(m);
        const uint32_t x = y ^ (1u << b);
        const int nx = cnt[x];
        if (nx == 0) continue;
        const bool pt_ev = r.kind[b] == ORD_K_PT;
        const double num = ord_num(lt, N, r, r.ev[b], y & (pt_ev ? r.pt_mask : in_mt), false);
        for (int c = 0; c < nx; ++c) {
          const long long xs = ((long long)x * cap + c) * 3;
          double a = fv[xs], bp = fv[xs + 1], bm = fv[xs + 2];
          ord_settle(r, t, x, a, bp, bm);                                // _advance
          bp = (r.pt_first && r.kind[b] == ORD_K_MT) ? bp * num / dmt[y] : 0.0;
          bm = (r.mt_first && pt_ev) ? bm * num / dpt[y] : 0.0;
          a = a * num / den[y];
          double sa = a, sp = bp, sm = bm;
          ord_settle(r, t, y, sa, sp, sm);
          bool dominated = false;
          for (int i = 0; i < nk && !dominated; ++i) {
            const long long ws = (ys + i) * 3;
            double wa = fv[ws], wp = fv[ws + 1], wm = fv[ws + 2];
            ord_settle(r, t, y, wa, wp, wm);
            dominated = wa >= sa && wp >= sp && wm >= sm;
          }
          if (dominated) continue;
          int j = 0;
          for (int i = 0; i < nk; ++i) {
            const long long ws = (ys + i) * 3;
            const double ua = fv[ws], up = fv[ws + 1], um = fv[ws + 2];
            double wa = ua, wp = up, wm = um;
            ord_settle(r, t, y, wa, wp, wm);
            if (sa >= wa && sp >= wp && sm >= wm && (sa > wa || sp > wp || sm > wm)) continue;
            if (j != i) {
              const long long ds = (ys + j) * 3;
              fv[ds] = ua; fv[ds + 1] = up; fv[ds + 2] = um;
              fb[ys + j] = fb[ys + i];
            }
            ++j;
          }
          nk = j;
          if (nk == cap) { atomicOr(&overflow, 1); continue; }
          const long long ds = (ys + nk) * 3;
          fv[ds] = a; fv[ds + 1] = bp; fv[ds + 2] = bm;
          fb[ys + nk] = ord_bp(c, b, false);
          ++nk;
        }
      }
      cnt[y] = nk;
    }
    __syncthreads();
    const int ov = overflow;             // every wave reads it before any wave can set it again
    __syncthreads();
    if (ov) break;
  }

  if (tid == 0) {
    if (overflow) {
      out_status[r.row] = 1;
      out_prob[r.row] = 0.0;
      return;
    }
    // _total over the full state's front, the first maximum; then the back-pointers down to the empty state
    int bc = 0;
    double bt = -1.0;
    for (int c = 0; c < cnt[full]; ++c) {
      const long long s = ((long long)full * cap + c) * 3;
      double a = fv[s], bp = fv[s + 1], bm = fv[s + 2];
      ord_settle(r, t, full, a, bp, bm);
      const double tot = bp * o2[full] + bm * o1[full];
      if (tot > bt) { bt = tot; bc = c; }
    }
    int8_t* o = out_order + (long long)r.row * L;
    int i = k;
    uint32_t y = full;
    int c = bc;
    while (y && i > 0) {
      const uint32_t w = fb[(long long)y * cap + c];
      const int b = (int)((w >> 16) & 0xFFu);
      if ((w >> 24) && i >= 2) {
        o[--i] = r.code[b + 1];
        o[--i] = r.code[b];
        y ^= 3u << b;
      } else {
        o[--i] = r.code[b];
        y ^= 1u << b;
      }
      c = (int)(w & 0xFFFFu);
    }
    out_prob[r.row] = bt;
    out_status[r.row] = 0;
  }
}

}  // namespace mmhn
