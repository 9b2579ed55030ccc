// The cohort planner: how a cohort is cut into batches, which route every joint problem takes, and every work list,
// offset and layout the kernels of one evaluation read.  Pure host arithmetic on Desc records - nothing in this file
// talks to the GPU runtime; the engine uploads a finished plan (engine.hip: upload) and sizes its workspace from it.
// The order of every list fixes the floating-point summation order of an evaluation.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "host.h"
#include "kernels.h"
#include "tsolve.h"
#include "small.h"
#include "wsolve.h"
#include "wclass.h"

namespace mmhn {

// the knobs the planner reads (engine.hip: Config names the MMHN_* variable behind each)
struct PlanCfg {
  size_t ws_limit = 0;          // bytes one batch may occupy (mmhn_set_workspace_limit; default: 70 % of the free memory)
  int n_cu = 256;               // compute units of the GPU
  bool use_jacobi = false;      // MMHN_SOLVER=jacobi: the reference's k+1 sweeps instead of substitution
  int wsolve_mode = 1;          // joint solves of per-patient batches in the window layout (wsolve.h); MMHN_WSOLVE=0: the tile
                                // kernels (k_psolve2) for every problem, 2: window solves converted back to index order
  int wsolve_min = 128;         // window-shaped joint problems in a batch from which they take the window route (MMHN_WSOLVE_MIN;
                                // follows MMHN_PSOLVE_MIN when only that one is set)
  int psolve_min = 384;         // multi-tile joint problems (outside the window route) in a batch from which they take one workgroup
                                // per patient (k_psolve2) instead of the cooperative tile launch (MMHN_PSOLVE_MIN)
  int wsolve_wgs = 0;           // MMHN_WSOLVE_WGS: workgroups of the window solve (default: one per CU)
  int prep_split_max = 2048;    // MMHN_PREP_SPLIT: problems up to which k_prep / k_pclass run a workgroup per table / class pass
  int pcl_per = 16;             // MMHN_PCL_PER: tiles of a class pass per work item of k_pclass
  bool small_path = true;       // MMHN_SMALL=0: keep the staged kernels for single-tumour spaces that fit one tile
};

// work list of one cooperative solve launch (tsolve.h: k_csolve)
struct CList {
  std::vector<CItem> items;
  std::vector<int> deps;         // never empty next to items: a list without dependencies holds one placeholder entry
  int maxk = 0;
  int nlevels = 0;               // levels of the deepest problem (1: no tile waits for another one)
  void clear() { items.clear(); deps.clear(); maxk = 0; nlevels = 0; }
};
enum Route : uint8_t { RT_W = 0, RT_P = 1, RT_T = 2 };

// the lists of the staged single-tumour kernels for one group of patients of a batch
struct Staged {
  std::vector<int> pats, paired, probs;      // patients; those of them with a joint problem; their single-tumour problems
  std::vector<int2> map, lmap;               // tiles of the problems (map order / by level)
  std::vector<int> lof;
  std::vector<int2> grc;                     // k_grad_rows work list (GK_S)
  CList cl[2];                               // cooperative work lists, forward / transposed
  int maxk = 0;
  bool kind2 = false;                        // a patient of the group is an MT-only row
  bool empty() const { return pats.empty(); }
};

// static (per cohort) description of one batch of patients
struct Batch {
  std::vector<PatRec> pats;
  std::vector<Desc> dJ, dS;
  std::vector<int2> mapJ, mapS;
  long long vecJ = 0, vecS = 0, asize = 0, tabJ = 0, tabS = 0;
  long long aclr = 0;            // class-marginal arrays cleared per evaluation: [0, aclr); the rest is written whole (k_wclass, eq flows)
  int id = 0;
  int maxkJ = 0;
  int maxkcJ = 0;                // most bits of one class (PT / MT) over the joint problems
  // joint tiles sorted by level = popcount(tile index) for the substitution solver; lofJ = level offsets
  std::vector<int2> lmapJ;
  std::vector<int> lofJ;
  // tiles of the joint problems with more than PCA + PCH bits in one class: k_pclass skips them, k_class_marg
  // takes them
  std::vector<int2> mapX;
  std::vector<int2> grcJ;        // k_grad_rows work list of the joint problems: the three kinds (GK_P, GK_M, GK_E) in one list
                                 // (kind in bits 24+ of .y): one launch
  // small-space path (small.h): patients whose single-tumour spaces all fit a tile, by size class of the largest one
  // [0]: patients that are their own problem (dat types 0-2: nothing of the joint path feeds them), [1]: paired rows (their
  // single-tumour problems are marginals of the joint forward solution), [2]: the paired rows with both marginal problems
  // whose class has a side-by-side kernel (small.h PAIR) - taken out of [1]
  std::vector<int> sp_list[3][SP_NCLASS];
  bool has_small = false;        // some patient takes the small-space path
  int mk1p = 9;                  // bits the 256-thread class of the paired rows is sized for (spatient_class_maxk(1) or up to 10)
  // ... the other patients (a single-tumour space of more than a tile; MMHN_SMALL=0 / the Jacobi solver: every patient)
  // take the staged kernels over these lists
  // [0]: patients that are their own problem (nothing of the joint path feeds them: a side stream), [1]: paired rows
  Staged stg[2];
  std::vector<int> paired;       // patients with a joint problem
  // ---- per-problem dispatch of the joint solves (round 5).  Every joint problem takes ONE of three routes:
  //   RT_W  window layout, a chain of patients per workgroup (wsolve.h) - when the batch has enough window-shaped problems
  //   RT_P  one workgroup per patient walking its tiles (k_psolve2)   - multi-tile problems, when there are enough of them
  //   RT_T  the tiles of all remaining problems in ONE cooperative launch (tsolve.h: k_csolve) - several workgroups per patient
  std::vector<uint8_t> route;
  std::vector<int> olist;        // the RT_P problems
  bool wpath = false;            // the batch has RT_W problems
  bool wdirect = false;          // the consumers read the window layout in place (no conversion to index order)
  std::vector<WDesc> wd;         // sorted by shape; the state vectors of consecutive entries lie back to back
  int wnx = -1;                  // external bits of every window problem of the batch, -1: they differ
  std::vector<WChain> wchains;   // runs of same-shape entries, one workgroup each (wsolve.h)
  long long offT = 0;            // the RT_T problems' vectors start here (the tile solver skips their dead tiles: kept zero)
  CList clJ[2];                  // cooperative work lists of the RT_T tiles, forward / transposed
  std::vector<int2> lmapT;       // the RT_T tiles by level (MMHN_COOP=0: one launch per level)
  std::vector<int> lofT;
  int maxkT = 0, maxkP = 0;      // largest RT_T / RT_P problem
  int max_dl = 0;                // largest (2^#P bits in a tile + 2^#M bits in a tile) over the RT_P problems
  std::vector<int> ptoff;        // live (seeded) tiles of the RT_P problems in index order (k_psolve2)
  std::vector<uint32_t> ptiles;
  // class marginals of the problems in index order: work items of k_pclass (problem, class pass or eq block, range of its
  // outer loop) - a large problem is several workgroups
  std::vector<int4> pcl;
};

inline long long up4(long long v) { return (v + 3) / 4 * 4; }

// A seed = 0 tile of a joint space is dead when none of its states has PT == MT: with a right-hand
// side supported on e_0 / the seed = 1 half the solution is identically zero there, so the engine
// never launches it (the buffers are zeroed once; API calls with arbitrary vectors keep every tile).
static bool dead_tile(const Desc& d, uint32_t H) {
  if (d.mode != JOINT || d.seedbit < TB) return false;
  const uint32_t xhi = H << TB, hmask = ~((1u << TB) - 1u);
  if (xhi & (1u << d.seedbit)) return false;
  if (xhi & d.lone & hmask) return true;
  const uint32_t pp = d.pairP & hmask & ~(1u << 31);           // pairs whose P bit is a tile bit
  const uint32_t pm = (pp << 1);
  if (((xhi & pp) << 1) != (xhi & pm)) return true;
  // pair straddling the tile boundary (P bit TB-1, M bit TB): M set needs P set - possible inside the tile
  return false;
}

// sort a tile list by level (stable) and record the level offsets; prune drops dead tiles
static void build_levels(const std::vector<int2>& map, const std::vector<Desc>* descs, bool prune,
                         std::vector<int2>& lmap, std::vector<int>& lof) {
  int maxl = 0;
  std::vector<int2> keep;
  keep.reserve(map.size());
  for (const int2& m : map) {
    if (prune && descs && dead_tile((*descs)[m.x], (uint32_t)m.y)) continue;
    keep.push_back(m);
    maxl = std::max(maxl, popc((uint32_t)m.y));
  }
  lof.assign(maxl + 2, 0);
  for (const int2& m : keep) lof[popc((uint32_t)m.y) + 1]++;
  for (int l = 0; l <= maxl; ++l) lof[l + 1] += lof[l];
  lmap.resize(keep.size());
  std::vector<int> cur(lof.begin(), lof.end() - 1);
  for (const int2& m : keep) lmap[cur[popc((uint32_t)m.y)]++] = m;
}

static inline long long a_size(const Desc& d) {
  const int kP = popc(d.maskP), kM = popc(d.maskM), kE = popc(d.pairP);
  return ((long long)(kP + 1) << kP) + ((long long)(kM + 1) << kM) + ((long long)(kE + 2) << kE);
}

static void add_tiles(std::vector<int2>& map, int prob, int k) {
  const int tiles = k > TB ? 1 << (k - TB) : 1;
  for (int t = 0; t < tiles; ++t) map.push_back(make_int2(prob, t));
}

// the tiles a tile's step A reads (tsolve.h: tsolve_tile, same conditions): moves whose bits reach beyond the tile
static void tile_deps(const Desc& d, uint32_t H, bool tr, std::vector<uint32_t>& out) {
  out.clear();
  const int k = d.k, t = k < TB ? k : TB;
  const bool joint = d.mode == JOINT;
  for (int b = (t > 0 ? t - 1 : 0); b < k; ++b) {
    const bool is_pair = joint && ((d.pairP >> b) & 1u);
    for (int kind = 0; kind < 2; ++kind) {
      if (kind == 1 && !is_pair) continue;
      const uint32_t mv = kind == 0 ? (1u << b) : (3u << b);
      const uint32_t mh = mv >> t;
      if (mh == 0) continue;
      if (tr ? (H & mh) != 0 : (H & mh) != mh) continue;
      const uint32_t Hn = H ^ mh;
      if (std::find(out.begin(), out.end(), Hn) == out.end()) out.push_back(Hn);
    }
  }
}

// Work list of a cooperative solve over the tiles `map` (dead tiles of joint spaces dropped when `prune`): a topological
// order of the (transposed) system in which the deepest problems start first - key = levels a tile still has in front of
// it, counted from the END of its problem, so that every problem finishes in the last rounds (longest remaining path first).
static void build_clist(const std::vector<int2>& map, const std::vector<Desc>& descs, bool prune, bool tr, CList& cl) {
  cl.clear();
  struct Ent { int prob; uint32_t H; int key; int k; };
  std::vector<Ent> ents;
  ents.reserve(map.size());
  std::vector<int> maxlev(descs.size(), 0);
  for (const int2& m : map) {
    if (prune && dead_tile(descs[m.x], (uint32_t)m.y)) continue;
    maxlev[m.x] = std::max(maxlev[m.x], popc((uint32_t)m.y));
    ents.push_back(Ent{m.x, (uint32_t)m.y, 0, descs[m.x].k});
  }
  if (ents.empty()) return;
  for (Ent& e : ents) {
    const int lev = popc(e.H);
    e.key = tr ? -lev : lev - maxlev[e.prob];
    cl.maxk = std::max(cl.maxk, e.k);
    cl.nlevels = std::max(cl.nlevels, maxlev[e.prob] + 1);
  }
  std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.key != b.key ? a.key < b.key : a.k > b.k; });
  // position of every live tile in the list
  std::vector<long long> toff(descs.size() + 1, 0);
  std::vector<char> used(descs.size(), 0);
  for (const Ent& e : ents) used[e.prob] = 1;
  for (size_t p = 0; p < descs.size(); ++p) toff[p + 1] = toff[p] + (used[p] ? (descs[p].k > TB ? 1ll << (descs[p].k - TB) : 1) : 0);
  std::vector<int> pos((size_t)toff.back(), -1);
  for (size_t i = 0; i < ents.size(); ++i) pos[(size_t)(toff[ents[i].prob] + ents[i].H)] = (int)i;
  cl.items.resize(ents.size());
  std::vector<uint32_t> nb;
  for (size_t i = 0; i < ents.size(); ++i) {
    const Ent& e = ents[i];
    tile_deps(descs[e.prob], e.H, tr, nb);
    CItem it{e.prob, e.H, (int)cl.deps.size(), 0};
    for (uint32_t Hn : nb) {
      const int j = pos[(size_t)(toff[e.prob] + Hn)];
      if (j < 0) continue;                                   // a dead tile: zeros, written by nobody
      if (j >= (int)i) throw Fail{"cooperative solve: the work list is not a topological order"};
      cl.deps.push_back(j);
      ++it.ndep;
    }
    if (it.ndep > 63) throw Fail{"cooperative solve: more than 63 dependencies of one tile"};
    cl.items[i] = it;
  }
  if (cl.deps.empty()) cl.deps.push_back(0);
}

// work list of k_grad_rows: one entry per (problem, chunk of 2^GR_CHUNK subsets of the kind's lattice)
static std::vector<int2> grad_chunks(const std::vector<Desc>& ds, int kind) {
  std::vector<int2> out;
  for (size_t i = 0; i < ds.size(); ++i) {
    const Desc& d = ds[i];
    const int kc = kind == GK_P ? popc(d.maskP) : kind == GK_M ? popc(d.maskM) : kind == GK_E ? popc(d.pairP) : d.k;
    const int nch = 1 << std::max(0, kc - GR_CHUNK);
    for (int c = 0; c < nch; ++c) out.push_back(int2{(int)i, c});
  }
  return out;
}

// ---------------------------------------------------------------- cutting the cohort into batches
// A cohort that does not fit the workspace is cut into batches of about equal size (not: full ones and a small
// remainder - every batch should be large enough for the per-patient kernels): soft target per batch in bytes, or
// a number of paired rows per batch (0: not used)
struct CutTargets {
  double soft = 0;
  long long pats = 0;
};
template <typename T>
static CutTargets batch_targets(const PlanCfg& c, const int8_t* dat, long long np, int nc, int n) {
  CutTargets t;
  double total = 0;
  long long npJ = 0;
  for (long long r = 0; r < np; ++r) {
    const int8_t* row = dat + r * nc;
    int kp = 0, km = 0, ke = 0;
    for (int j = 0; j < n; ++j) { kp += row[2 * j] != 0; km += row[2 * j + 1] != 0; ke += row[2 * j] && row[2 * j + 1]; }
    const int type = row[nc - 1];
    double el = 0;
    if (type == 3) {
      ++npJ;
      el = (c.use_jacobi || c.wsolve_mode == 2 ? 4.0 : 2.0) * std::ldexp(1.0, kp + km + 1) + 4.0 * (std::ldexp(1.0, km + 1) + std::ldexp(1.0, kp + 1)) +
           (kp + 1) * std::ldexp(1.0, kp) + (km + 1) * std::ldexp(1.0, km) + (ke + 2) * std::ldexp(1.0, ke);
    } else if (type == 4) {
      el = 4.0 * (std::ldexp(1.0, kp) + std::ldexp(1.0, kp + 1));      // both parts of an unknown-status row
    } else {
      el = 4.0 * std::ldexp(1.0, (type == 2 ? km : kp) + 1);
    }
    total += el * sizeof(T);
  }
  const double nb = std::ceil(total / (double)std::max<size_t>(c.ws_limit, 1));
  t.soft = nb > 1 ? total / nb * 1.02 : 0;
  // the per-patient kernels take one patient per CU at a time: a batch of 400 costs two rounds of 256.  Batches of a cut
  // cohort hold a multiple of the CU count (rounded down: more, fuller rounds)
  if (nb > 1 && npJ > 0) {
    const double per_batch = (double)c.ws_limit / (total / (double)npJ);     // paired rows (they are what occupies a CU)
    if (per_batch >= (double)c.n_cu) {
      t.pats = (long long)(per_batch / c.n_cu) * c.n_cu;
      // a remainder too small for the window / per-patient routes would be a batch on the tile route alone: spread the
      // rows evenly over the same number of batches instead
      const long long nbt = (npJ + t.pats - 1) / t.pats, rem = npJ - (nbt - 1) * t.pats;
      if (nbt > 1 && rem < std::max(c.psolve_min, c.wsolve_min)) t.pats = (npJ + nbt - 1) / nbt;
    }
  }
  return t;
}

// the problems of one cohort row: a joint one and / or up to two single-tumour ones (pr.j / pr.s[] are set when the
// row joins a batch)
struct RowProblems {
  PatRec pr{};
  Desc dj{}, ds[2]{};
  bool hasJ = false, has[2] = {false, false};
};
static RowProblems decode_row(const int8_t* row, long long r, int n, int nc) {
  const int type = row[nc - 1];
  const int order = row[nc - 2];
  const std::string at = " (row " + std::to_string(r) + ")";
  REQUIRE(type >= 0 && type <= 4, "dat: type column must be 0..4" + at);
  for (int c = 0; c < 2 * n + 1; ++c) REQUIRE(row[c] == 0 || row[c] == 1, "dat: event columns must be 0/1");
  if (type == 4) {
    // a primary tumour of unknown metastatic status: nothing but PT events may be set
    for (int j = 0; j < n; ++j) REQUIRE(row[2 * j + 1] == 0, "dat: rows of unknown status (type 4) must have no MT event" + at);
    REQUIRE(row[2 * n] == 0, "dat: rows of unknown status (type 4) must have seeding = 0" + at);
  }
  RowProblems p;
  PatRec& pr = p.pr;
  pr.kind = type; pr.order = (order == 0 || order == 1) ? order : 2; pr.j = -1; pr.s[0] = pr.s[1] = -1;
  pr.row = (int)r;
  // active slots of every problem of the row, counted before any Desc is built: a restricted space - joint or
  // single-tumour - holds at most MAXK index bits (the marginal problems of a paired row are smaller than its joint one)
  int npt = 0, nmt = 0;
  for (int j = 0; j < n; ++j) { npt += row[2 * j]; nmt += row[2 * j + 1]; }
  const int kmax = type == 4 ? npt + 1 : type == 3 ? npt + nmt + 1 : type == 2 ? nmt + 1 : npt + row[2 * n];
  const bool unseeded_pair = type == 3 && row[2 * n] != 1;   // refused below with its own message
  REQUIRE(unseeded_pair || kmax <= MAXK, type == 4 ? "too many active events for one patient" + at : std::string("too many active events for one patient"));
  std::vector<int8_t> st(2 * n + 2);
  if (type == 4) {
    // the PT genotype without the seeding (what a type-0 row scores) and with it (a type-1 row with seeding = 1): two problems of
    // the patient's own, their final entries are added.  An empty genotype has no part 0: its share is the closed form of kind 4
    pr.kind = 5;
    for (int j = 0; j < n; ++j) st[j] = row[2 * j];
    st[n] = 0;
    if (npt > 0) { p.ds[0] = make_single(st.data(), n, PS_PRIM, OBS_ONE); p.has[0] = true; }
    st[n] = 1;
    p.ds[1] = make_single(st.data(), n, PS_PRIM, OBS_ONE);
    p.has[1] = true;
  } else if (type == 0 || type == 1) {
    for (int j = 0; j <= n; ++j) st[j] = row[2 * j];          // PT slots + seeding (regularized_optimization.py:189)
    int np_ = 0;
    for (int j = 0; j <= n; ++j) np_ += st[j];
    if (type == 0 && np_ == 0) pr.kind = 4;
    else { p.ds[0] = make_single(st.data(), n, PS_PRIM, OBS_ONE); p.has[0] = true; }
  } else if (type == 2) {
    for (int j = 0; j < n; ++j) st[j] = row[2 * j + 1];       // MT slots, seeding = 1 (:216-219)
    st[n] = 1;
    p.ds[0] = make_single(st.data(), n, PS_THETA, OBS_MET);
    p.has[0] = true;
  } else {
    REQUIRE(row[2 * n] == 1, "dat: paired rows (type 3) must have seeding = 1");
    p.dj = make_joint(row, n);
    p.hasJ = true;
    if (pr.order == 0 || pr.order == 1) {                     // PT observed first -> MT marginal
      for (int j = 0; j < n; ++j) st[j] = row[2 * j + 1];
      st[n] = 1;
      p.ds[0] = make_single(st.data(), n, PS_MET, OBS_ONE);
      p.has[0] = true;
    }
    if (pr.order != 1) {                                      // MT observed first -> PT marginal
      for (int j = 0; j <= n; ++j) st[j] = row[2 * j];
      p.ds[1] = make_single(st.data(), n, PS_PRIM, OBS_ONE);
      p.has[1] = true;
    }
  }
  return p;
}

// bytes a batch of these sizes occupies: state vectors, class-marginal arrays, the per-evaluation tables and the
// per-problem / per-patient result buffers
template <typename T>
static size_t footprint(const PlanCfg& c, int N, long long vJ, long long vS, long long as, long long tabs, size_t nJp, size_t nSp,
                        size_t npat) {
  const size_t stride = 1 + (size_t)N * N + 2 * (size_t)N;
  const size_t small = (nSp * (size_t)(N * N + 64 + 1) + nJp * (size_t)(3 * N * N + 3 * N + 64)) * sizeof(T) +
                       nJp * sizeof(JLink<T>) + npat * (stride + 1) * sizeof(double) + npat * 2 * sizeof(T);
  return (size_t)((c.use_jacobi || c.wsolve_mode == 2 ? 4 : 2) * vJ + 4 * vS + as + tabs) * sizeof(T) + small;
}

// the row's problems become the next ones of the batch (index-order offsets; layout_joint_vectors and
// layout_class_arrays move the joint ones later)
static void append_row(Batch& cur, RowProblems& p) {
  if (p.hasJ) {
    Desc& dj = p.dj;
    dj.off = cur.vecJ; dj.aoff = cur.asize; dj.toff = cur.tabJ; cur.tabJ += table_size(dj);
    cur.vecJ += 1ll << dj.k; cur.asize += a_size(dj);
    p.pr.j = (int)cur.dJ.size();
    add_tiles(cur.mapJ, p.pr.j, dj.k);
    cur.maxkJ = std::max(cur.maxkJ, dj.k);
    cur.maxkcJ = std::max(cur.maxkcJ, std::max(popc(dj.maskP), popc(dj.maskM)));
    cur.dJ.push_back(dj);
  }
  for (int part = 0; part < 2; ++part) {
    if (!p.has[part]) continue;
    Desc& ds = p.ds[part];
    ds.off = cur.vecS; cur.vecS += 1ll << ds.k; ds.toff = cur.tabS; cur.tabS += table_size(ds);
    p.pr.s[part] = (int)cur.dS.size();
    add_tiles(cur.mapS, p.pr.s[part], ds.k);
    cur.dS.push_back(ds);
  }
  cur.pats.push_back(p.pr);
}

// rows in cohort order; a batch is closed when the next row would overflow the workspace or the batch has reached
// its target.  n_em: rows with the seeding event
template <typename T>
static std::vector<Batch> split_into_batches(const PlanCfg& c, const int8_t* dat, long long np, int nc, int n, double& n_em) {
  const int N = n + 1;
  const CutTargets tg = batch_targets<T>(c, dat, np, nc, n);
  std::vector<Batch> batches;
  Batch cur;
  auto flush = [&]() {
    if (cur.pats.empty()) return;
    batches.push_back(std::move(cur));
    cur = Batch();
  };
  n_em = 0;
  for (long long r = 0; r < np; ++r) {
    const int8_t* row = dat + r * nc;
    RowProblems p = decode_row(row, r, n, nc);
    n_em += row[2 * n];
    // would the batch overflow the workspace?  (incl. the incoming problems' tables)
    const long long nvJ = p.hasJ ? (1ll << p.dj.k) : 0, nvS = (p.has[0] ? (1ll << p.ds[0].k) : 0) + (p.has[1] ? (1ll << p.ds[1].k) : 0);
    const long long ntab = (p.hasJ ? table_size(p.dj) : 0) + (p.has[0] ? table_size(p.ds[0]) : 0) + (p.has[1] ? table_size(p.ds[1]) : 0);
    const size_t need = footprint<T>(c, N, cur.vecJ + nvJ, cur.vecS + nvS, cur.asize + (p.hasJ ? a_size(p.dj) : 0), cur.tabJ + cur.tabS + ntab,
                                     cur.dJ.size() + (p.hasJ ? 1 : 0), cur.dS.size() + (p.has[0] ? 1 : 0) + (p.has[1] ? 1 : 0), cur.pats.size() + 1);
    const size_t have = footprint<T>(c, N, cur.vecJ, cur.vecS, cur.asize, cur.tabJ + cur.tabS, cur.dJ.size(), cur.dS.size(), cur.pats.size());
    if (!cur.pats.empty() && (need > c.ws_limit || (tg.pats > 0 ? (p.hasJ && (long long)cur.dJ.size() >= tg.pats)
                                                                 : (tg.soft > 0 && (double)have >= tg.soft)))) flush();
    append_row(cur, p);
  }
  flush();
  int bid = 0;
  for (Batch& b : batches) b.id = bid++;
  return batches;
}

// ---------------------------------------------------------------- the joint problems of a batch
// routes of the joint problems (Batch::route)
template <typename T>
static void route_joint_problems(const PlanCfg& c, Batch& b) {
  const int nJ = (int)b.dJ.size();
  auto is_multi = [](const Desc& dj) { return dj.seedbit >= TB && popc(dj.pairP) <= TB; };   // what k_psolve2 takes
  b.route.assign((size_t)nJ, RT_T);
  b.olist.clear(); b.wd.clear(); b.wchains.clear();
  b.wpath = false;
  if (c.use_jacobi || nJ == 0) return;
  int nW = 0, nP = 0;
  if (c.wsolve_mode != 0) for (const Desc& dj : b.dJ) nW += window_ok<T>(dj) ? 1 : 0;
  b.wpath = nW > 0 && nW >= c.wsolve_min;
  for (int pj = 0; pj < nJ; ++pj) {
    if (b.wpath && window_ok<T>(b.dJ[pj])) b.route[pj] = RT_W;
    else if (is_multi(b.dJ[pj])) ++nP;
  }
  if (nP > 0 && nP >= c.psolve_min)
    for (int pj = 0; pj < nJ; ++pj) if (b.route[pj] != RT_W && is_multi(b.dJ[pj])) b.route[pj] = RT_P;
  for (int pj = 0; pj < nJ; ++pj) {
    if (b.route[pj] == RT_W) b.wd.push_back(make_wdesc<T>(b.dJ[pj], pj));
    else if (b.route[pj] == RT_P) b.olist.push_back(pj);
  }
}

// layout of the joint vectors (the offsets are the engine's own business: every kernel goes through Desc::off):
// the window problems sorted by shape - a chain of same-shape patients is one contiguous buffer -, then the
// per-patient problems, then the tile route's, whose dead tiles must stay zero
static void layout_joint_vectors(Batch& b) {
  const int nJ = (int)b.dJ.size();
  std::stable_sort(b.wd.begin(), b.wd.end(), [](const WDesc& x, const WDesc& y) { return x.kR != y.kR ? x.kR < y.kR : x.kC < y.kC; });
  long long off = 0;
  for (const WDesc& w : b.wd) { b.dJ[w.prob].off = off; off += 1ll << b.dJ[w.prob].k; }
  for (int pj : b.olist) { b.dJ[pj].off = off; off += 1ll << b.dJ[pj].k; }
  b.offT = off;
  for (int pj = 0; pj < nJ; ++pj) if (b.route[pj] == RT_T) { b.dJ[pj].off = off; off += 1ll << b.dJ[pj].k; }
  REQUIRE(off == b.vecJ, "offsets of the joint problems do not add up");
}

// chains (wsolve.h): about one run of same-shape problems per workgroup
template <typename T>
static void build_window_chains(const PlanCfg& c, Batch& b) {
  if (!b.wpath) return;
  const int nW = (int)b.wd.size();
  b.wnx = b.wd[0].nXc + b.wd[0].nXr;
  for (const WDesc& w : b.wd) if (w.nXc + w.nXr != b.wnx) b.wnx = -1;
  const int groups = std::max(1, c.wsolve_wgs > 0 ? c.wsolve_wgs : c.n_cu);
  const int per = (nW + groups - 1) / groups;
  for (int i0 = 0; i0 < nW;) {
    const WDesc& w = b.wd[i0];
    const int k = b.dJ[w.prob].k;
    // a chain keeps two patients' tables alive at once: it needs 2^nX > 6 passes per patient; its span must stay
    // below 2 GB (32-bit buffer offsets)
    const int maxlen = w.nXc + w.nXr >= 3 ? (int)std::min<long long>(per, (1ll << 31) / ((long long)sizeof(T) << k) - 1) : 1;
    int len = 1;
    while (len < maxlen && i0 + len < nW && b.wd[i0 + len].kR == w.kR && b.wd[i0 + len].kC == w.kC && (i0 + len) % per != 0) ++len;
    b.wchains.push_back(WChain{i0, len});
    i0 += len;
  }
  if ((int)b.wchains.size() <= groups) return;
  // more chains than workgroups (shape changes cut chains short): workgroup g takes the entries g, g + groups, ... -
  // deal the chains longest first to the least loaded workgroup, empty entries fill the rounds
  std::vector<WChain> srt = b.wchains;
  std::stable_sort(srt.begin(), srt.end(), [](const WChain& x, const WChain& y) { return x.count > y.count; });
  std::vector<std::vector<WChain>> mine((size_t)groups);
  std::vector<int> load((size_t)groups, 0);
  for (const WChain& ch : srt) {
    const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    mine[g].push_back(ch);
    load[g] += ch.count;
  }
  size_t rounds = 0;
  for (const auto& m : mine) rounds = std::max(rounds, m.size());
  b.wchains.assign(rounds * (size_t)groups, WChain{0, 0});
  for (int g = 0; g < groups; ++g)
    for (size_t r = 0; r < mine[g].size(); ++r) b.wchains[r * (size_t)groups + g] = mine[g][r];
}

// the tile route: every tile of its problems in one cooperative launch (or level by level)
static void build_tile_route(const PlanCfg& c, Batch& b) {
  b.lmapT.clear(); b.lofT.clear(); b.maxkT = 0;
  b.clJ[0].clear(); b.clJ[1].clear();
  if (c.use_jacobi) return;
  std::vector<int2> mt;
  for (const int2& m : b.mapJ) if (b.route[m.x] == RT_T) { mt.push_back(m); b.maxkT = std::max(b.maxkT, b.dJ[m.x].k); }
  if (mt.empty()) return;
  build_levels(mt, &b.dJ, true, b.lmapT, b.lofT);
  if (b.lofT.size() > 2) { build_clist(mt, b.dJ, true, false, b.clJ[0]); build_clist(mt, b.dJ, true, true, b.clJ[1]); }
}

// k_psolve2 solves the seed = 0 part of a multi-tile space (only its PT == MT states carry values) as a small
// lattice over the paired events, so only the seeded tiles of its problems are listed
static void build_psolve_tiles(Batch& b) {
  const int nJ = (int)b.dJ.size();
  b.ptoff.assign(1, 0);
  b.ptiles.clear();
  b.maxkP = 0; b.max_dl = 0;
  for (int pj = 0; pj < nJ; ++pj) {
    const Desc& dj = b.dJ[pj];
    if (b.route[pj] == RT_P) {
      const uint32_t nt = 1u << (dj.k - TB);
      for (uint32_t Ht = 0; Ht < nt; ++Ht) if (((Ht << TB) >> dj.seedbit) & 1u) b.ptiles.push_back(Ht);
      b.maxkP = std::max(b.maxkP, dj.k);
      b.max_dl = std::max(b.max_dl, (1 << popc(dj.maskP & ((1u << TB) - 1u))) + (1 << popc(dj.maskM & ((1u << TB) - 1u))));
    }
    b.ptoff.push_back((int)b.ptiles.size());
  }
}

// class marginals of the problems in index order as work items (short launches; a large problem is several
// workgroups): per problem its eq block, per class pass the outer loop cut into ranges
static void build_pclass_items(const PlanCfg& c, Batch& b) {
  const int nJ = (int)b.dJ.size();
  b.pcl.clear();
  if (c.use_jacobi || nJ > c.prep_split_max) return;
  for (int pj = 0; pj < nJ; ++pj) {
    const Desc& dj = b.dJ[pj];
    b.pcl.push_back(int4{pj, 2, 0, 0});
    const int kP = popc(dj.maskP), kM = popc(dj.maskM);
    if (b.route[pj] == RT_W && c.wsolve_mode != 2) continue;             // (k_wclass)
    if (kP > PCA + PCH || kM > PCA + PCH) continue;                     // (k_class_marg)
    for (int cl = 0; cl < 2; ++cl) {
      const int kc = cl == 0 ? kP : kM, kf = cl == 0 ? kM : kP;
      const int no = pclass_outer_bits(kc, kf), nh = kc > PCA ? kc - PCA : 0;
      const int per = std::max(1, c.pcl_per >> nh);                     // tiles per item: (2^nh class blocks) x (per settings)
      for (int o0 = 0; o0 < (1 << no); o0 += per) b.pcl.push_back(int4{pj, cl, o0, std::min(o0 + per, 1 << no)});
    }
  }
  // longest items first (tiles of the item = range x class blocks above the tile): the launch ends with the short ones
  auto item_tiles = [&](const int4& it) -> long long {
    if (it.y == 2) return 0;
    const Desc& dj = b.dJ[it.x];
    const int kc = popc(it.y == 0 ? dj.maskP : dj.maskM);
    return (long long)(it.w - it.z) << (kc > PCA ? kc - PCA : 0);
  };
  std::stable_sort(b.pcl.begin(), b.pcl.end(), [&](const int4& x, const int4& y) { return item_tiles(x) > item_tiles(y); });
}

// lists in index order that need no decision: every joint tile by level (the Jacobi solver's list), the tiles
// k_class_marg takes, the patients with a joint problem
static void build_index_lists(const PlanCfg& c, Batch& b) {
  build_levels(b.mapJ, &b.dJ, !c.use_jacobi, b.lmapJ, b.lofJ);
  b.mapX.clear();
  for (const int2& m : b.mapJ) {
    const Desc& dj = b.dJ[m.x];
    if (popc(dj.maskP) > PCA + PCH || popc(dj.maskM) > PCA + PCH) b.mapX.push_back(m);
  }
  b.paired.clear();
  for (size_t pi_ = 0; pi_ < b.pats.size(); ++pi_) if (b.pats[pi_].j >= 0) b.paired.push_back((int)pi_);
}

// ---------------------------------------------------------------- the single-tumour problems of a batch
// small-space path for the patients whose spaces all fit a tile (by size class), staged kernels for the rest
template <typename T>
static void assign_small_classes(const PlanCfg& c, int N, Batch& b) {
  for (int w = 0; w < 3; ++w) for (int cl = 0; cl < SP_NCLASS; ++cl) b.sp_list[w][cl].clear();
  for (int w = 0; w < 2; ++w) { Staged& g = b.stg[w]; g.pats.clear(); g.paired.clear(); g.probs.clear(); g.kind2 = false; }
  bool class_fits[SP_NCLASS];
  for (int cl = 0; cl < SP_NCLASS; ++cl)
    class_fits[cl] = (spatient_lds<T>(N, spatient_class_maxk(cl)) + 15) / 16 * 16 * (size_t)(cl == 0 ? SP_PPB0 : cl == 1 ? 2 : 1) + 64 <= (size_t)160 * 1024;
  const bool all_staged = !c.small_path || c.use_jacobi;
  for (size_t pi_ = 0; pi_ < b.pats.size(); ++pi_) {
    const PatRec& pr = b.pats[pi_];
    int ks = -1;
    for (int part = 0; part < 2; ++part) if (pr.s[part] >= 0) ks = std::max(ks, b.dS[pr.s[part]].k);
    if (ks < 0) continue;
    int cl = 0;
    while (cl < SP_NCLASS - 1 && ks > spatient_class_maxk(cl)) ++cl;
    if (all_staged || ks > TB || !class_fits[cl]) {
      // (MMHN_SMALL=0 / Jacobi: one group on the main stream - its solver clears and sweeps whole buffers)
      Staged& g = b.stg[all_staged || pr.j >= 0 ? 1 : 0];
      g.pats.push_back((int)pi_);
      if (pr.j >= 0) g.paired.push_back((int)pi_);
      for (int part = 0; part < 2; ++part) if (pr.s[part] >= 0) g.probs.push_back(pr.s[part]);
      if (pr.kind == 2) g.kind2 = true;
      continue;
    }
    const bool side_by_side = pr.j >= 0 && pr.s[0] >= 0 && pr.s[1] >= 0 && cl < 2;
    b.sp_list[side_by_side ? 2 : pr.j >= 0 ? 1 : 0][cl].push_back((int)pi_);
  }
  // paired rows of the 1024-thread class: when they are few and of at most 10 bits they ride in the merged 256-thread
  // launch (its LDS sized for them) - on a small cohort their own launch is a side stream, a fork and a join
  // (~20 us of queue latency) for a handful of patients
  b.mk1p = spatient_class_maxk(1);
  if (!b.sp_list[1][2].empty() && b.sp_list[1][2].size() <= 16) {
    int mk = 0;
    for (int pi_ : b.sp_list[1][2])
      for (int part = 0; part < 2; ++part) if (b.pats[pi_].s[part] >= 0) mk = std::max(mk, b.dS[b.pats[pi_].s[part]].k);
    if (mk <= 10 && (spatient_lds<T>(N, mk) + 15) / 16 * 16 * 2 + 64 <= (size_t)160 * 1024) {
      for (int pi_ : b.sp_list[1][2]) b.sp_list[b.pats[pi_].s[0] >= 0 && b.pats[pi_].s[1] >= 0 ? 2 : 1][1].push_back(pi_);
      b.sp_list[1][2].clear();
      b.mk1p = mk;
    }
  }
  // largest spaces first: the waves of one workgroup (class 0: one patient each) then finish together and the
  // long patients do not form the tail of the launch
  auto ksize = [&](int pi_) {
    const PatRec& pr = b.pats[pi_];
    int ks = 0;
    for (int part = 0; part < 2; ++part) if (pr.s[part] >= 0) ks = std::max(ks, 64 * b.dS[pr.s[part]].k + (pr.s[0] >= 0 && pr.s[1] >= 0 ? 32 : 0) + pr.kind);
    return ks;
  };
  b.has_small = false;
  for (int w = 0; w < 3; ++w)
    for (int cl = 0; cl < SP_NCLASS; ++cl) {
      std::stable_sort(b.sp_list[w][cl].begin(), b.sp_list[w][cl].end(), [&](int x, int y) { return ksize(x) > ksize(y); });
      if (!b.sp_list[w][cl].empty()) b.has_small = true;
    }
}

// lists of the staged kernels for the two groups assign_small_classes filled
static void build_staged_groups(const PlanCfg& c, Batch& b) {
  const std::vector<int2> chunks = grad_chunks(b.dS, GK_S);
  for (int w = 0; w < 2; ++w) {
    Staged& g = b.stg[w];
    std::vector<char> isg(b.dS.size(), 0);
    for (int sp : g.probs) isg[sp] = 1;
    g.map.clear(); g.maxk = 0;
    for (const int2& m : b.mapS) if (isg[m.x]) { g.map.push_back(m); g.maxk = std::max(g.maxk, b.dS[m.x].k); }
    build_levels(g.map, nullptr, false, g.lmap, g.lof);
    g.cl[0].clear(); g.cl[1].clear();
    if (!c.use_jacobi && g.lof.size() > 2) { build_clist(g.map, b.dS, false, false, g.cl[0]); build_clist(g.map, b.dS, false, true, g.cl[1]); }
    g.grc.clear();
    for (const int2& e : chunks) if (isg[e.x]) g.grc.push_back(e);
  }
}

// ---------------------------------------------------------------- gradient work arrays of a batch
// class-marginal arrays: the problems whose tables are added into first, then the window-layout ones.
// The window layout stays in place: every consumer of the joint vectors reads it there (k_gather_marg / the small-space
// kernels, k_eq_flows, k_wclass); MMHN_WSOLVE=2 converts to index order after each solve instead (k_wconvert)
static void layout_class_arrays(const PlanCfg& c, Batch& b) {
  const int nJ = (int)b.dJ.size();
  b.wdirect = b.wpath && c.wsolve_mode != 2;
  long long ao = 0;
  for (int pj = 0; pj < nJ; ++pj) if (!(b.wdirect && b.route[pj] == RT_W)) { b.dJ[pj].aoff = ao; ao += a_size(b.dJ[pj]); }
  b.aclr = up4(ao);
  ao = b.aclr;
  for (int pj = 0; pj < nJ; ++pj) if (b.wdirect && b.route[pj] == RT_W) { b.dJ[pj].aoff = ao; ao += a_size(b.dJ[pj]); }
  b.asize = ao;
  for (Desc& dj : b.dJ) dj.wl = -1;
  if (b.wdirect) for (size_t i = 0; i < b.wd.size(); ++i) b.dJ[b.wd[i].prob].wl = (int)i;
}

static void build_grad_chunks(Batch& b) {
  b.grcJ.clear();
  for (int kd = 0; kd < 3; ++kd)
    for (const int2& e : grad_chunks(b.dJ, kd)) b.grcJ.push_back(int2{e.x, e.y | (kd << 24)});
}

// the plan of a cohort: dat[np][nc] (nc = 2 n + 3: checked by the caller) under configuration c
template <typename T>
static std::vector<Batch> plan_cohort(const PlanCfg& c, const int8_t* dat, long long np, int nc, int n, double& n_em) {
  const int N = n + 1;
  std::vector<Batch> batches = split_into_batches<T>(c, dat, np, nc, n, n_em);
  for (Batch& b : batches) {
    route_joint_problems<T>(c, b);
    layout_joint_vectors(b);
    build_window_chains<T>(c, b);
    build_tile_route(c, b);
    build_psolve_tiles(b);
    build_pclass_items(c, b);
    build_index_lists(c, b);
    assign_small_classes<T>(c, N, b);
    build_staged_groups(c, b);
    layout_class_arrays(c, b);
    build_grad_chunks(b);
  }
  return batches;
}

}  // namespace mmhn
