// Stand-alone check of the cohort planner (metmhn_amd/csrc/plan.h) against brute force on the host.
//
// The program builds plans for generated cohorts under a sweep of PlanCfg and checks every list of every batch.  The
// reference is the model itself, written out below: the bit roles of a row are decoded here from the raw row, a tile's
// states are enumerated, and the moves of the model decide which tiles are dead and which tiles feed which.  Nothing on
// the reference side calls dead_tile, tile_deps, build_levels or a_size.  No GPU runtime call is made: the program runs
// on any host, and is meant to be built with the host sanitizers.
//
//   plan_check                         the whole sweep; one line of counts per check, exit status 1 on the first violation
//   plan_check --cohort FILE NP N      the int8 cohort FILE[NP][2 N + 3] under the window route with three workgroups
//                                      (wsolve_min = 1, wsolve_wgs = 3) and under the default configuration
#include <cstdarg>
#include <cstdio>
#include <map>
#include <set>
#include <string>

#include "plan.h"

using namespace mmhn;

// ------------------------------------------------------------------------------------ reporting
static std::string g_ctx;          // cohort / config / batch the checks are looking at
struct Count { long long plans = 0, problems = 0, tiles = 0; };
static std::map<std::string, Count> g_cnt;
static std::map<std::string, long long> g_shape;   // targeted shapes and other counts that are printed only

[[noreturn]] static void fail(const char* family, const char* fmt, ...) {
  std::printf("VIOLATION [%s] %s: ", family, g_ctx.c_str());
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
  std::fflush(stdout);
  std::exit(1);
}
#define CHECK(cond, family, ...) do { if (!(cond)) fail(family, __VA_ARGS__); } while (0)

struct Lcg {
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 2654435761u + 12345u) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int m) { return (int)(next() % (uint32_t)m); }
  double unit() { return next() / 2147483648.0; }
};

// ------------------------------------------------------------------------------------ the model
// bit roles of one restricted space, decoded from the raw row (not from a Desc)
struct Space {
  int k = 0, seed = -1;
  bool joint = false;
  uint32_t maskP = 0, maskM = 0, pairP = 0, lone = 0;
};
static Space joint_space(const int8_t* row, int n) {
  Space s;
  s.joint = true;
  for (int j = 0; j < n; ++j) {
    const bool p = row[2 * j] != 0, m = row[2 * j + 1] != 0;
    if (p) { s.maskP |= 1u << s.k; if (m) s.pairP |= 1u << s.k; else s.lone |= 1u << s.k; ++s.k; }
    if (m) { s.maskM |= 1u << s.k; if (!p) s.lone |= 1u << s.k; ++s.k; }
  }
  if (row[2 * n]) s.seed = s.k++;
  return s;
}
static Space single_space(int nbits, int seed) {
  Space s;
  s.k = nbits; s.seed = seed;
  s.maskP = nbits >= 32 ? ~0u : (1u << nbits) - 1u;
  return s;
}
// PT == MT without the seeding bit: no lone bit set, the two bits of every pair equal
static bool pt_eq_mt(const Space& s, uint32_t x) {
  if (x & s.lone) return false;
  for (int b = 0; b < s.k; ++b)
    if ((s.pairP >> b) & 1u) if (((x >> b) & 1u) != ((x >> (b + 1)) & 1u)) return false;
  return true;
}
// the states a state's value is computed from (tr: the transposed system)
template <typename F>
static void sources(const Space& s, uint32_t x, bool tr, F&& emit) {
  if (!s.joint) {
    for (int b = 0; b < s.k; ++b) if ((((x >> b) & 1u) != 0) != tr) emit(x ^ (1u << b));
    return;
  }
  const uint32_t sm = 1u << s.seed;
  if (x & sm) {
    // seeded: the two tumours move one event at a time; the seeding itself enters from a PT == MT state
    for (int b = 0; b < s.k; ++b) if (b != s.seed && ((((x >> b) & 1u) != 0) != tr)) emit(x ^ (1u << b));
    if (!tr && pt_eq_mt(s, x & ~sm)) emit(x ^ sm);
  } else if (pt_eq_mt(s, x)) {
    // not seeded: only PT == MT states carry values, an event sets both bits of its pair
    for (int b = 0; b < s.k; ++b)
      if ((s.pairP >> b) & 1u) if ((((x >> b) & 1u) != 0) != tr) emit(x ^ (3u << b));
    if (tr) emit(x | sm);
  }
}

struct TileModel {
  int t = 0;
  uint32_t ntiles = 1;
  std::vector<char> dead;
  std::vector<std::vector<uint32_t>> src[2];   // source tiles other than the tile itself, forward / transposed
};
static TileModel enumerate_tiles(const Space& s) {
  TileModel m;
  m.t = s.k < TB ? s.k : TB;
  m.ntiles = 1u << (s.k - m.t);
  m.dead.assign(m.ntiles, 0);
  std::vector<uint32_t> stamp(m.ntiles, 0);
  uint32_t cur = 0;
  for (int tr = 0; tr < 2; ++tr) {
    m.src[tr].assign(m.ntiles, {});
    for (uint32_t H = 0; H < m.ntiles; ++H) {
      ++cur;
      bool any_eq = false;
      std::vector<uint32_t>& out = m.src[tr][H];
      for (uint32_t xl = 0; xl < (1u << m.t); ++xl) {
        const uint32_t x = (H << m.t) | xl;
        if (tr == 0 && s.joint && !any_eq && !((x >> s.seed) & 1u) && pt_eq_mt(s, x)) any_eq = true;
        sources(s, x, tr != 0, [&](uint32_t y) {
          const uint32_t Hy = y >> m.t;
          if (Hy != H && stamp[Hy] != cur) { stamp[Hy] = cur; out.push_back(Hy); }
        });
      }
      if (tr == 0) m.dead[H] = s.joint && s.seed >= TB && !(((H << m.t) >> s.seed) & 1u) && !any_eq;
    }
  }
  return m;
}

// ------------------------------------------------------------------------------------ cohorts
struct Cohort {
  std::string name;
  int n = 0;
  std::vector<int8_t> dat;
  long long np() const { return (long long)dat.size() / (2 * n + 3); }
  const int8_t* row(long long r) const { return dat.data() + r * (2 * n + 3); }
  // per-row models, built on demand (the same row is planned under many configurations)
  mutable std::map<std::pair<long long, int>, TileModel> models;
  mutable int multi_models = 0;
};
// events as a string: J = both tumours, P = PT only, M = MT only, - = neither
static bool add_pattern(Cohort& c, const std::string& ev, int seed, int order, int type) {
  if ((int)ev.size() > c.n) return false;
  std::vector<int8_t> r(2 * c.n + 3, 0);
  for (size_t j = 0; j < ev.size(); ++j) {
    r[2 * j] = ev[j] == 'J' || ev[j] == 'P';
    r[2 * j + 1] = ev[j] == 'J' || ev[j] == 'M';
  }
  r[2 * c.n] = (int8_t)seed; r[2 * c.n + 1] = (int8_t)order; r[2 * c.n + 2] = (int8_t)type;
  c.dat.insert(c.dat.end(), r.begin(), r.end());
  return true;
}
static const int ORDERS[4] = {0, 1, 2, -99};
constexpr int KCAP = 18;            // bits of the largest generated joint space (its 2^k states are enumerated)

static void add_random_rows(Cohort& c, Lcg& g, int count) {
  const double dens[5] = {0.15, 0.3, 0.5, 0.8, 1.0};
  for (int i = 0; i < count; ++i) {
    const double d = dens[g.below(5)];
    const int type = g.below(4);
    std::string ev(c.n, '-');
    int bits = 0;
    for (int j = 0; j < c.n; ++j) {
      const bool p = g.unit() < d, m = g.unit() < d;
      char ch = type <= 1 ? (p ? 'P' : '-') : type == 2 ? (m ? 'M' : '-') : (p && m ? 'J' : p ? 'P' : m ? 'M' : '-');
      const int w = ch == 'J' ? 2 : ch == '-' ? 0 : 1;
      if (bits + w + 1 > KCAP) ch = '-';
      else bits += w;
      ev[j] = ch;
    }
    add_pattern(c, ev, type == 0 ? 0 : 1, type == 3 ? ORDERS[g.below(4)] : -99, type);
  }
}
static std::string rep(char ch, int m) { return std::string((size_t)std::max(m, 0), ch); }
// the shapes the planner's special cases are about, at every order
static void add_targeted_rows(Cohort& c) {
  const std::string pats[] = {
      "JJJJJPJ",                    // pair on bits 11 / 12, seeding on 13: k = 14
      "JJJJJMJ", "PJJJJJJ",         // the same pair behind an MT-only event; with a second pair above the tile
      "JJJJJPJP", "JJJJJPJM", "JJJJJPJJ",
      "JJJJJP",                     // seeding on bit 11: k = 12
      "JJJJJJ", "PPPPPPMMMMMM", "JJJJJPM",      // seeding on bit 12: k = 13
      "JJJJJJP", "JJJJJJM", "JJJPPPPMMM" "P",   // seeding on bit 13: k = 14
      "JJJJJJJ", "JJJJJJJJ", "PPPPPPPPPPPPJ", "MMMMMMMMMMMMMJ",   // pairs above the tile
      "JJJJPPPPP", "JJJPPPMMMMM", "JPPPPPPMMMMMM",   // lone-heavy, k > 12
      "JJJJJJJJJ", "JJJJJJJJP",                      // pair-heavy
      rep('P', 12), rep('P', 13), rep('P', 16), rep('P', 14) + "M",     // PT only (a class of 16 bits: k_class_marg)
      rep('M', 12), rep('M', 13), rep('M', 16), "P" + rep('M', 14),     // MT only
      rep('P', 12) + "JJ", rep('M', 13) + "J",                           // single-tumour spaces of more than a tile
      rep('P', 10) + "MMMMM", rep('P', 11) + "MMMM", "MMMM" + rep('P', 11), rep('P', 12) + "MMMM", rep('P', 10) + "JMMMM",   // window shapes
  };
  for (const std::string& p : pats)
    for (int o = 0; o < 4; ++o) add_pattern(c, p, 1, ORDERS[o], 3);
  // unpaired rows beyond a tile
  for (int kk : {12, 13, 15}) {
    add_pattern(c, rep('P', kk), 1, -99, 1);
    add_pattern(c, rep('P', kk), 0, -99, 0);
    add_pattern(c, rep('M', kk), 1, -99, 2);
  }
}
static Cohort random_cohort(const char* name, int n, int count, uint64_t seed, bool targeted) {
  Cohort c;
  c.name = name; c.n = n;
  Lcg g(seed);
  add_random_rows(c, g, count / 2);
  if (targeted) add_targeted_rows(c);
  add_random_rows(c, g, count - count / 2);
  return c;
}
// paired rows of the 1 024-thread small class (largest single-tumour space of 10 .. 12 bits) between small ones
static Cohort small_class_cohort(const char* name, int n, int count, int bits) {
  Cohort c;
  c.name = name; c.n = n;
  Lcg g(77 + count);
  for (int i = 0; i < count; ++i) {
    add_random_rows(c, g, 2);
    const int other = g.below(3);
    const std::string ev = i % 2 ? rep('P', bits - 1) + rep('M', other) : rep('M', bits - 1) + rep('P', other);
    add_pattern(c, ev.substr(0, (size_t)n), 1, ORDERS[i % 4], 3);
  }
  return c;
}

// many window-shaped rows of few shapes: chains of several rows, cut at the shape changes and at the workgroup shares
static Cohort window_cohort(const char* name, int n) {
  Cohort c;
  c.name = name; c.n = n;
  Lcg g(5);
  const std::string pats[] = {"JJJJJPPPPPPP", "JJJJPPPPPPPPM", "JJJJJJPPPPPP", "JJJMMMMMMMMMP", "JJJPPPPPPPMM", "JJJJPPPPPPPP"};
  const int count[] = {14, 11, 11, 7, 3, 2};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < count[i]; ++j) { add_pattern(c, pats[i], 1, ORDERS[g.below(4)], 3); if (g.below(3) == 0) add_random_rows(c, g, 1); }
  return c;
}

// n = 31, the largest event count: rows over the events 26 .. 30 and the seeding (event index 31, column 62) at every type
// and order, and a few paired rows over the events 24 .. 30 that pass the tile bits (k = 13, 14)
static Cohort top_event_cohort(const char* name, int count, uint64_t seed) {
  Cohort c;
  c.name = name; c.n = 31;
  Lcg g(seed);
  const double dens[4] = {0.3, 0.5, 0.8, 1.0};
  for (int i = 0; i < count; ++i) {
    const double d = dens[g.below(4)];
    const int type = g.below(4);
    std::string ev(26, '-');
    for (int j = 26; j < 31; ++j) {
      const bool p = g.unit() < d, m = g.unit() < d;
      ev += type <= 1 ? (p ? 'P' : '-') : type == 2 ? (m ? 'M' : '-') : (p && m ? 'J' : p ? 'P' : m ? 'M' : '-');
    }
    add_pattern(c, ev, type == 0 ? 0 : 1, type == 3 ? ORDERS[g.below(4)] : -99, type);
  }
  for (const char* tail : {"JJJJJJ-", "JJJJJPJ", "JJJJJMJ", "PJJJJJJ", "JJJJJJP", "JJJJJJM", "PPMMJJJ"})
    for (int o = 0; o < 4; ++o) add_pattern(c, rep('-', 24) + tail, 1, ORDERS[o], 3);
  add_pattern(c, rep('-', 30) + "P", 0, -99, 0);
  add_pattern(c, rep('-', 30) + "P", 1, -99, 1);
  add_pattern(c, rep('-', 30) + "M", 1, -99, 2);
  add_pattern(c, "", 0, -99, 0);
  for (int type = 1; type <= 3; ++type) add_pattern(c, "", 1, type == 3 ? 0 : -99, type);
  return c;
}

// ------------------------------------------------------------------------------------ configurations
struct NamedCfg { PlanCfg c; std::string name; };
static std::string cfg_name(const PlanCfg& c) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "ws=%zuMiB wmin=%d pmin=%d wgs=%d cu=%d wmode=%d jac=%d small=%d split=%d per=%d", c.ws_limit >> 20,
                c.wsolve_min, c.psolve_min, c.wsolve_wgs, c.n_cu, c.wsolve_mode, (int)c.use_jacobi, (int)c.small_path, c.prep_split_max, c.pcl_per);
  return buf;
}
static std::vector<PlanCfg> config_sweep() {
  std::vector<PlanCfg> out;
  PlanCfg base;
  base.ws_limit = (size_t)8 << 30;
  auto add = [&](auto&& edit) { PlanCfg c = base; edit(c); out.push_back(c); };
  add([](PlanCfg&) {});
  add([](PlanCfg& c) { c.psolve_min = 1; c.wsolve_min = 1; });
  add([](PlanCfg& c) { c.psolve_min = 1000000; c.wsolve_min = 1; c.wsolve_wgs = 3; });
  add([](PlanCfg& c) { c.psolve_min = 1; c.wsolve_min = 1; c.wsolve_wgs = 1; });
  add([](PlanCfg& c) { c.psolve_min = 1; c.wsolve_min = 1; c.wsolve_wgs = 7; c.wsolve_mode = 2; });
  add([](PlanCfg& c) { c.psolve_min = 1; c.wsolve_min = 1; c.wsolve_mode = 0; });
  add([](PlanCfg& c) { c.psolve_min = 1000000; c.wsolve_min = 128; c.n_cu = 4; });
  add([](PlanCfg& c) { c.use_jacobi = true; });
  add([](PlanCfg& c) { c.use_jacobi = true; c.psolve_min = 1; c.wsolve_min = 1; c.ws_limit = (size_t)4 << 20; });
  add([](PlanCfg& c) { c.small_path = false; });
  add([](PlanCfg& c) { c.prep_split_max = 0; });
  add([](PlanCfg& c) { c.pcl_per = 1; c.psolve_min = 1; });
  add([](PlanCfg& c) { c.ws_limit = (size_t)1 << 20; c.psolve_min = 1; c.wsolve_min = 1; c.n_cu = 4; });
  add([](PlanCfg& c) { c.ws_limit = (size_t)8 << 20; c.n_cu = 4; c.psolve_min = 1; c.wsolve_min = 1; c.wsolve_wgs = 3; });
  add([](PlanCfg& c) { c.ws_limit = (size_t)32 << 20; c.n_cu = 4; c.wsolve_min = 128; c.psolve_min = 1000000; });
  add([](PlanCfg& c) { c.ws_limit = (size_t)32 << 20; c.n_cu = 4; c.wsolve_min = 1; c.psolve_min = 1; c.prep_split_max = 0; });
  Lcg g(2024);
  const size_t wss[5] = {(size_t)1 << 20, (size_t)4 << 20, (size_t)32 << 20, (size_t)256 << 20, (size_t)8 << 30};
  const int wgs[4] = {0, 1, 3, 7};
  for (int i = 0; i < 12; ++i) {
    PlanCfg c;
    c.ws_limit = wss[g.below(5)];
    c.wsolve_min = g.below(2) ? 1 : 128;
    c.psolve_min = g.below(2) ? 1 : 1000000;
    c.wsolve_wgs = wgs[g.below(4)];
    c.n_cu = g.below(2) ? 4 : 256;
    c.wsolve_mode = g.below(3);
    c.use_jacobi = g.below(6) == 0;
    c.small_path = g.below(4) != 0;
    c.prep_split_max = g.below(3) == 0 ? 0 : 2048;
    c.pcl_per = g.below(2) ? 1 : 16;
    out.push_back(c);
  }
  return out;
}

// ------------------------------------------------------------------------------------ the checks of one plan
static long long class_array_size(const Space& s) {
  const int kP = popc(s.maskP), kM = popc(s.maskM), kE = popc(s.pairP);
  return (long long)(kP + 1) * (1ll << kP) + (long long)(kM + 1) * (1ll << kM) + (long long)(kE + 2) * (1ll << kE);
}
static uint32_t tiles_of(int k) { return k > TB ? 1u << (k - TB) : 1u; }
static void bump(const char* name, long long problems, long long tiles) {
  Count& c = g_cnt[name];
  c.problems += problems; c.tiles += tiles;
}

// what the program knows about the problems of one batch, from the raw rows alone
struct BatchModel {
  std::vector<Space> sJ, sS;
  std::vector<const TileModel*> mJ, mS;       // nullptr: beyond the cap of enumerated problems
  std::vector<char> straddle;                 // a pair on bits TB - 1 / TB of a multi-tile joint space
};
constexpr int MODEL_CAP = 400;                // multi-tile problems enumerated per cohort

static const TileModel* model_of(const Cohort& co, long long row, int part, const Space& s) {
  auto key = std::make_pair(row, part);
  auto it = co.models.find(key);
  if (it != co.models.end()) return &it->second;
  if (s.k > TB) {
    if (co.multi_models >= MODEL_CAP) return nullptr;
    ++co.multi_models;
  }
  return &(co.models[key] = enumerate_tiles(s));
}

static void check_level_list(const char* what, const std::vector<int2>& lmap, const std::vector<int>& lof,
                             const std::set<std::pair<int, uint32_t>>& want) {
  CHECK(lmap.size() == want.size(), "levels", "%s: %zu tiles listed, %zu expected", what, lmap.size(), want.size());
  if (lmap.empty()) { CHECK(lof.empty() || lof.back() == 0, "levels", "%s: offsets of an empty list", what); return; }
  std::set<std::pair<int, uint32_t>> seen;
  int maxl = 0;
  for (const int2& m : lmap) {
    CHECK(want.count({m.x, (uint32_t)m.y}), "levels", "%s: problem %d tile %d is not a tile of the list", what, m.x, m.y);
    CHECK(seen.insert({m.x, (uint32_t)m.y}).second, "levels", "%s: problem %d tile %d listed twice", what, m.x, m.y);
    maxl = std::max(maxl, popc((uint32_t)m.y));
  }
  CHECK((int)lof.size() == maxl + 2 && lof[0] == 0 && lof.back() == (int)lmap.size(), "levels", "%s: %zu level offsets for %d levels", what, lof.size(), maxl + 1);
  for (int l = 0; l <= maxl; ++l) {
    CHECK(lof[l] <= lof[l + 1], "levels", "%s: offsets decrease at level %d", what, l);
    for (int i = lof[l]; i < lof[l + 1]; ++i)
      CHECK(popc((uint32_t)lmap[i].y) == l, "levels", "%s: problem %d tile %d sits in level %d", what, lmap[i].x, lmap[i].y, l);
  }
}

// a cooperative list over `tiles` (problem, H) of the problems `spaces` / `models`; `live(p, H)` says which are listed
static void check_clist(const char* what, const CList& cl, bool tr, const std::set<std::pair<int, uint32_t>>& live,
                        const std::vector<Space>& spaces, const std::vector<const TileModel*>& models, bool expected) {
  if (!expected) {
    CHECK(cl.items.empty() && cl.deps.empty(), "clist", "%s: a list where none is expected", what);
    return;
  }
  CHECK(cl.items.size() == live.size(), "clist", "%s: %zu items, %zu live tiles", what, cl.items.size(), live.size());
  CHECK(!cl.deps.empty(), "clist", "%s: deps is empty next to items", what);
  std::map<std::pair<int, uint32_t>, int> pos;
  int maxk = 0, nlev = 0;
  std::map<int, int> maxlev;
  long long dep_total = 0;
  for (size_t i = 0; i < cl.items.size(); ++i) {
    const CItem& it = cl.items[i];
    CHECK(live.count({it.prob, it.H}), "clist", "%s: item %zu (problem %d tile %u) is not a live tile of the list", what, i, it.prob, it.H);
    CHECK(pos.emplace(std::make_pair(it.prob, it.H), (int)i).second, "clist", "%s: problem %d tile %u listed twice", what, it.prob, it.H);
    CHECK(it.ndep >= 0 && it.ndep <= 63, "clist", "%s: problem %d tile %u has %d dependencies", what, it.prob, it.H, it.ndep);
    CHECK(it.dep0 == dep_total && (size_t)(it.dep0 + it.ndep) <= cl.deps.size(), "clist", "%s: item %zu: dependency range [%d, +%d)", what, i, it.dep0, it.ndep);
    dep_total += it.ndep;
    maxk = std::max(maxk, spaces[it.prob].k);
    int& ml = maxlev[it.prob];
    ml = std::max(ml, popc(it.H));
  }
  CHECK(cl.deps.size() == (size_t)std::max(dep_total, 1ll), "clist", "%s: %zu dependency entries, %lld used", what, cl.deps.size(), dep_total);
  for (auto& kv : maxlev) nlev = std::max(nlev, kv.second + 1);
  CHECK(cl.maxk == maxk, "clist", "%s: maxk %d, expected %d", what, cl.maxk, maxk);
  CHECK(cl.nlevels == nlev, "clist", "%s: nlevels %d, expected %d", what, cl.nlevels, nlev);
  long long checked = 0, surplus = 0, needed = 0;
  for (size_t i = 0; i < cl.items.size(); ++i) {
    const CItem& it = cl.items[i];
    std::set<uint32_t> have;
    for (int j = 0; j < it.ndep; ++j) {
      const int dj = cl.deps[(size_t)it.dep0 + j];
      CHECK(dj >= 0 && dj < (int)i, "clist", "%s: problem %d tile %u: dependency %d is not an earlier item (item %zu)", what, it.prob, it.H, dj, i);
      CHECK(cl.items[dj].prob == it.prob, "clist", "%s: problem %d tile %u depends on a tile of problem %d", what, it.prob, it.H, cl.items[dj].prob);
      have.insert(cl.items[dj].H);
    }
    const TileModel* m = models[it.prob];
    if (!m) continue;
    ++checked;
    std::set<uint32_t> need;
    for (uint32_t Hs : m->src[tr ? 1 : 0][it.H]) if (live.count({it.prob, Hs})) need.insert(Hs);
    for (uint32_t Hs : need)
      CHECK(have.count(Hs), "clist-missing-dependency", "%s (%s): problem %d (k = %d) tile %u reads tile %u, which is not among its dependencies",
            what, tr ? "transposed" : "forward", it.prob, spaces[it.prob].k, it.H, Hs);
    needed += (long long)need.size();
    surplus += (long long)have.size() - (long long)need.size();
  }
  bump("cooperative lists", 0, checked);
  g_shape["cooperative dependencies required by the model"] += needed;
  g_shape["cooperative dependencies surplus (harmless, not asserted)"] += surplus;
}

template <typename T>
static void check_batch(const PlanCfg& c, const Cohort& co, const Batch& b, bool is_last, long long& next_row) {
  const int n = co.n, N = n + 1;
  const int nJ = (int)b.dJ.size(), nS = (int)b.dS.size();
  BatchModel bm;
  bm.sJ.resize(nJ); bm.mJ.assign(nJ, nullptr); bm.straddle.assign(nJ, 0);
  bm.sS.resize(nS); bm.mS.assign(nS, nullptr);

  // ---- batches: rows in cohort order, PatRec indices valid and of the right kind
  CHECK(!b.pats.empty(), "batches", "an empty batch");
  int cntJ = 0, cntS = 0;
  std::vector<int> paired;
  for (size_t pi = 0; pi < b.pats.size(); ++pi) {
    const PatRec& pr = b.pats[pi];
    CHECK(pr.row == next_row, "batches", "patient %zu is row %d, expected row %lld", pi, pr.row, next_row);
    ++next_row;
    const int8_t* row = co.row(pr.row);
    const int type = row[2 * n + 2], order = row[2 * n + 1];
    const int ord = order == 0 || order == 1 ? order : 2;
    int npt = 0, nmt = 0;
    for (int j = 0; j < n; ++j) { npt += row[2 * j] != 0; nmt += row[2 * j + 1] != 0; }
    const int sd = row[2 * n] != 0;
    const bool allzero = type == 0 && npt + sd == 0;
    CHECK(pr.kind == (allzero ? 4 : type) && pr.order == ord, "batches", "row %d: kind %d order %d", pr.row, pr.kind, pr.order);
    int ks[2] = {-1, -1}, seed[2] = {-1, -1}, pset[2] = {0, 0}, obs[2] = {OBS_ONE, OBS_ONE};
    if (type <= 1) { if (!allzero) { ks[0] = npt + sd; seed[0] = sd ? npt : -1; pset[0] = PS_PRIM; } }
    else if (type == 2) { ks[0] = nmt + 1; seed[0] = nmt; pset[0] = PS_THETA; obs[0] = OBS_MET; }
    else {
      if (ord != 2) { ks[0] = nmt + 1; seed[0] = nmt; pset[0] = PS_MET; }
      if (ord != 1) { ks[1] = npt + 1; seed[1] = npt; pset[1] = PS_PRIM; }
    }
    if (type == 3) {
      CHECK(pr.j == cntJ, "batches", "row %d: joint problem %d, expected %d", pr.row, pr.j, cntJ);
      const Space s = joint_space(row, n);
      const Desc& d = b.dJ[pr.j];
      CHECK(d.mode == JOINT && d.k == s.k && d.seedbit == s.seed && d.maskP == s.maskP && d.maskM == s.maskM && d.pairP == s.pairP && d.lone == s.lone && d.N == N,
            "batches", "row %d: the joint descriptor does not describe the row", pr.row);
      bm.sJ[cntJ] = s;
      bm.mJ[cntJ] = model_of(co, pr.row, 2, s);
      bm.straddle[cntJ] = s.k > TB && ((s.pairP >> (TB - 1)) & 1u);
      paired.push_back((int)pi);
      ++cntJ;
    } else CHECK(pr.j == -1, "batches", "row %d of type %d has a joint problem", pr.row, type);
    for (int part = 0; part < 2; ++part) {
      if (ks[part] < 0) { CHECK(pr.s[part] == -1, "batches", "row %d: unexpected single-tumour problem %d", pr.row, part); continue; }
      CHECK(pr.s[part] == cntS, "batches", "row %d: single-tumour problem %d, expected %d", pr.row, pr.s[part], cntS);
      const Desc& d = b.dS[cntS];
      CHECK(d.mode == SINGLE && d.k == ks[part] && d.seedbit == seed[part] && d.pset == pset[part] && d.obs == obs[part] && d.N == N &&
                d.maskP == single_space(ks[part], seed[part]).maskP,
            "batches", "row %d: single-tumour descriptor %d does not describe the row", pr.row, part);
      bm.sS[cntS] = single_space(ks[part], seed[part]);
      bm.mS[cntS] = model_of(co, pr.row, part, bm.sS[cntS]);
      ++cntS;
    }
  }
  CHECK(cntJ == nJ && cntS == nS, "batches", "%d joint / %d single problems without a patient", nJ - cntJ, nS - cntS);
  CHECK(b.paired == paired, "paired", "the list of patients with a joint problem is not exact");
  g_cnt["batches"].problems += nJ + nS;
  g_cnt["paired"].problems += nJ;

  // ---- index-order tile maps
  {
    size_t i = 0;
    int maxk = 0, maxkc = 0;
    for (int p = 0; p < nJ; ++p) {
      maxk = std::max(maxk, bm.sJ[p].k);
      maxkc = std::max(maxkc, std::max(popc(bm.sJ[p].maskP), popc(bm.sJ[p].maskM)));
      for (uint32_t H = 0; H < tiles_of(bm.sJ[p].k); ++H, ++i)
        CHECK(i < b.mapJ.size() && b.mapJ[i].x == p && (uint32_t)b.mapJ[i].y == H, "layouts", "mapJ entry %zu", i);
    }
    CHECK(i == b.mapJ.size() && b.maxkJ == maxk && b.maxkcJ == maxkc, "layouts", "mapJ / maxkJ / maxkcJ");
    i = 0;
    for (int p = 0; p < nS; ++p)
      for (uint32_t H = 0; H < tiles_of(bm.sS[p].k); ++H, ++i)
        CHECK(i < b.mapS.size() && b.mapS[i].x == p && (uint32_t)b.mapS[i].y == H, "layouts", "mapS entry %zu", i);
    CHECK(i == b.mapS.size(), "layouts", "mapS has %zu entries", b.mapS.size());
  }

  // ---- dead tiles: the planner's rule against enumeration, both ways
  std::set<std::pair<int, uint32_t>> liveJ, allJ;
  for (int p = 0; p < nJ; ++p) {
    const TileModel* m = bm.mJ[p];
    for (uint32_t H = 0; H < tiles_of(bm.sJ[p].k); ++H) {
      const bool dead = dead_tile(b.dJ[p], H);
      allJ.insert({p, H});
      if (!dead) liveJ.insert({p, H});
      if (!m) continue;
      CHECK(dead == (m->dead[H] != 0), "dead-tiles", "problem %d (row %d, k = %d, pairs %#x, lone %#x) tile %u: the planner says %s, enumeration says %s", p,
            b.pats[b.paired[p]].row, bm.sJ[p].k, bm.sJ[p].pairP, bm.sJ[p].lone, H, dead ? "dead" : "live", m->dead[H] ? "dead" : "live");
      if (bm.sJ[p].k > TB) {
        bump("dead tiles", 0, 1);
        if (m->dead[H]) ++g_shape["dead tiles"];
        if (bm.straddle[p]) { ++g_shape["straddling tiles"]; if (!m->dead[H] && !(((H << TB) >> bm.sJ[p].seed) & 1u)) ++g_shape["straddling tiles live without seeding"]; }
      }
    }
    if (m && bm.sJ[p].k > TB) bump("dead tiles", 1, 0);
    // forward sources lie in strictly lower levels
    if (m) for (uint32_t H = 0; H < m->ntiles; ++H) for (uint32_t Hs : m->src[0][H])
      CHECK(popc(Hs) < popc(H), "levels", "problem %d tile %u reads tile %u of no lower level", p, H, Hs);
  }

  // ---- routes
  auto is_multi = [](const Space& s) { return s.seed >= TB && popc(s.pairP) <= TB; };
  int nW = 0, nP = 0;
  std::vector<char> wok(nJ, 0);
  for (int p = 0; p < nJ; ++p) { wok[p] = !c.use_jacobi && c.wsolve_mode != 0 && window_ok<T>(b.dJ[p]); nW += wok[p]; }
  const bool wpath = nW > 0 && nW >= c.wsolve_min;
  for (int p = 0; p < nJ; ++p) if (!(wpath && wok[p]) && is_multi(bm.sJ[p])) ++nP;
  const bool ppath = !c.use_jacobi && nP > 0 && nP >= c.psolve_min;
  CHECK((int)b.route.size() == nJ && b.wpath == wpath, "routes", "wpath %d with %d window-shaped problems", (int)b.wpath, nW);
  std::vector<int> olist;
  std::set<int> wset;
  for (int p = 0; p < nJ; ++p) {
    const int want = wpath && wok[p] ? RT_W : ppath && is_multi(bm.sJ[p]) ? RT_P : RT_T;
    CHECK(b.route[p] == want, "routes", "problem %d (k = %d) takes route %d, expected %d", p, bm.sJ[p].k, b.route[p], want);
    if (want == RT_P) olist.push_back(p);
    if (want == RT_W) wset.insert(p);
    ++g_shape[want == RT_W ? "problems on the window route" : want == RT_P ? "problems on the per-patient route" : "problems on the tile route"];
  }
  CHECK(b.olist == olist, "routes", "olist is not the per-patient problems in index order");
  CHECK(b.wd.size() == wset.size(), "routes", "%zu window descriptors for %zu window problems", b.wd.size(), wset.size());
  for (const WDesc& w : b.wd) CHECK(wset.count(w.prob), "routes", "window descriptor of problem %d", w.prob);
  g_cnt["routes"].problems += nJ;
  {  // per-patient tiles
    CHECK((int)b.ptoff.size() == nJ + 1 && b.ptoff[0] == 0, "ptiles", "ptoff has %zu entries", b.ptoff.size());
    int maxkP = 0, max_dl = 0;
    for (int p = 0; p < nJ; ++p) {
      std::vector<uint32_t> want;
      if (b.route[p] == RT_P) {
        const Space& s = bm.sJ[p];
        for (uint32_t H = 0; H < tiles_of(s.k); ++H) if (((uint64_t)H << TB) >> s.seed & 1u) want.push_back(H);
        maxkP = std::max(maxkP, s.k);
        const uint32_t tm = (1u << TB) - 1u;
        max_dl = std::max(max_dl, (1 << popc(s.maskP & tm)) + (1 << popc(s.maskM & tm)));
        bump("ptiles", 1, (long long)want.size());
      }
      CHECK(b.ptoff[p] <= b.ptoff[p + 1] && (size_t)b.ptoff[p + 1] <= b.ptiles.size(), "ptiles", "ptoff of problem %d", p);
      const std::vector<uint32_t> got(b.ptiles.begin() + b.ptoff[p], b.ptiles.begin() + b.ptoff[p + 1]);
      CHECK(got == want, "ptiles", "problem %d (k = %d, seeding on bit %d): %zu tiles listed, %zu seeded tiles", p, bm.sJ[p].k, bm.sJ[p].seed, got.size(), want.size());
    }
    CHECK((size_t)b.ptoff[nJ] == b.ptiles.size() && b.maxkP == maxkP && b.max_dl == max_dl, "ptiles", "maxkP %d (%d), max_dl %d (%d)", b.maxkP, maxkP, b.max_dl, max_dl);
  }

  // ---- layouts
  {
    CHECK(std::is_sorted(b.wd.begin(), b.wd.end(), [](const WDesc& x, const WDesc& y) { return x.kR != y.kR ? x.kR < y.kR : x.kC < y.kC; }),
          "layouts", "the window descriptors are not sorted by shape");
    long long off = 0;
    for (const WDesc& w : b.wd) { CHECK(b.dJ[w.prob].off == off, "layouts", "vector offset of window problem %d", w.prob); off += 1ll << bm.sJ[w.prob].k; }
    for (int p : b.olist) { CHECK(b.dJ[p].off == off, "layouts", "vector offset of per-patient problem %d", p); off += 1ll << bm.sJ[p].k; }
    CHECK(b.offT == off, "layouts", "offT %lld, expected %lld", b.offT, off);
    for (int p = 0; p < nJ; ++p) if (b.route[p] == RT_T) { CHECK(b.dJ[p].off == off, "layouts", "vector offset of tile-route problem %d", p); off += 1ll << bm.sJ[p].k; }
    CHECK(off == b.vecJ, "layouts", "the joint vectors cover %lld of %lld elements", off, b.vecJ);
    const bool wdirect = wpath && c.wsolve_mode != 2;
    CHECK(b.wdirect == wdirect, "layouts", "wdirect %d", (int)b.wdirect);
    std::vector<std::pair<long long, long long>> rng;
    long long tab = 0;
    for (int p = 0; p < nJ; ++p) {
      const long long sz = class_array_size(bm.sJ[p]), ao = b.dJ[p].aoff;
      const bool wd_ = wdirect && b.route[p] == RT_W;
      CHECK(ao >= 0 && ao + sz <= b.asize, "layouts", "class arrays of problem %d: [%lld, +%lld) outside [0, %lld)", p, ao, sz, b.asize);
      CHECK(wd_ ? ao >= b.aclr : ao + sz <= b.aclr, "layouts", "class arrays of problem %d at %lld (+%lld) on the wrong side of aclr = %lld", p, ao, sz, b.aclr);
      rng.push_back({ao, ao + sz});
      CHECK(b.dJ[p].toff == tab, "layouts", "table offset of joint problem %d", p);
      tab += table_size(b.dJ[p]);
      if (!wd_) CHECK(b.dJ[p].wl == -1, "layouts", "wl of problem %d outside the window layout", p);
    }
    CHECK(tab == b.tabJ, "layouts", "tabJ");
    std::sort(rng.begin(), rng.end());
    for (size_t i = 1; i < rng.size(); ++i) CHECK(rng[i - 1].second <= rng[i].first, "layouts", "class arrays overlap at %lld", rng[i].first);
    CHECK(b.aclr % 4 == 0 && b.aclr <= b.asize, "layouts", "aclr = %lld is not a multiple of 4 (asize %lld)", b.aclr, b.asize);
    if (wdirect) for (size_t i = 0; i < b.wd.size(); ++i) CHECK(b.dJ[b.wd[i].prob].wl == (int)i, "layouts", "wl of window problem %d", b.wd[i].prob);
    long long so = 0, st = 0;
    for (int p = 0; p < nS; ++p) {
      CHECK(b.dS[p].off == so && b.dS[p].toff == st, "layouts", "offsets of single-tumour problem %d", p);
      so += 1ll << bm.sS[p].k; st += table_size(b.dS[p]);
    }
    CHECK(so == b.vecS && st == b.tabS, "layouts", "vecS / tabS");
    g_cnt["layouts"].problems += nJ + nS;
  }

  // ---- window chains
  if (wpath) {
    const int nWd = (int)b.wd.size();
    const int groups = std::max(1, c.wsolve_wgs > 0 ? c.wsolve_wgs : c.n_cu), per = (nWd + groups - 1) / groups;
    std::vector<int> hit((size_t)nWd, 0);
    size_t nonempty = 0;
    int prev_start = -1;
    bool ordered = true;
    for (const WChain& ch : b.wchains) {
      CHECK(ch.count >= 0 && ch.start >= 0 && ch.start + ch.count <= nWd, "chains", "chain [%d, +%d) outside the %d window problems", ch.start, ch.count, nWd);
      if (ch.count == 0) continue;
      ++nonempty;
      if (ch.start < prev_start) ordered = false;
      prev_start = ch.start;
      const WDesc& w0 = b.wd[ch.start];
      long long bytes = 0;
      for (int i = ch.start; i < ch.start + ch.count; ++i) {
        ++hit[i];
        CHECK(b.wd[i].kR == w0.kR && b.wd[i].kC == w0.kC, "chains", "chain at %d holds two shapes", ch.start);
        CHECK(i == ch.start || i % per != 0, "chains", "chain [%d, +%d) runs across entry %d, a multiple of the %d entries per workgroup", ch.start, ch.count, i, per);
        bytes += (long long)sizeof(T) << bm.sJ[b.wd[i].prob].k;
      }
      CHECK(ch.count == 1 || w0.nXc + w0.nXr >= 3, "chains", "chain at %d of length %d with %d external bits", ch.start, ch.count, w0.nXc + w0.nXr);
      CHECK(ch.count <= per, "chains", "chain at %d of length %d, %d entries per workgroup", ch.start, ch.count, per);
      CHECK(bytes < (1ll << 31), "chains", "chain at %d spans %lld bytes", ch.start, bytes);
    }
    for (int i = 0; i < nWd; ++i) CHECK(hit[i] == 1, "chains", "window problem %d lies in %d chains", i, hit[i]);
    if (nonempty > (size_t)groups) {
      CHECK(b.wchains.size() % (size_t)groups == 0, "chains", "%zu entries dealt to %d workgroups", b.wchains.size(), groups);
      ++g_shape["batches with dealt chains"];
      g_shape["dealt chain entries left empty"] += (long long)(b.wchains.size() - nonempty);
    } else {
      CHECK(b.wchains.size() == nonempty && ordered, "chains", "empty or unordered entries without dealing");
    }
    int wnx = b.wd[0].nXc + b.wd[0].nXr;
    for (const WDesc& w : b.wd) {
      CHECK(w.kR - WTB == w.nXr && w.nXc == w.kC - WCfg<T>::RB - WCfg<T>::HB, "chains", "external bits of window problem %d", w.prob);
      if (w.nXc + w.nXr != wnx) wnx = -1;
    }
    CHECK(b.wnx == wnx, "chains", "wnx %d, expected %d", b.wnx, wnx);
    bump("window chains", nWd, 0);
    g_shape["window chains"] += (long long)nonempty;
    for (const WChain& ch : b.wchains) if (ch.count > 1) ++g_shape["window chains of several rows"];
  } else CHECK(b.wchains.empty() && b.wd.empty(), "chains", "chains without a window route");

  // ---- level lists and cooperative lists of the joint problems
  check_level_list("lmapJ", b.lmapJ, b.lofJ, c.use_jacobi ? allJ : liveJ);
  std::set<std::pair<int, uint32_t>> liveT;
  int maxkT = 0, maxlevT = 0;
  for (auto& e : liveJ) if (b.route[e.first] == RT_T && !c.use_jacobi) { liveT.insert(e); maxlevT = std::max(maxlevT, popc(e.second)); }
  for (int p = 0; p < nJ; ++p) if (b.route[p] == RT_T && !c.use_jacobi) maxkT = std::max(maxkT, bm.sJ[p].k);
  check_level_list("lmapT", b.lmapT, b.lofT, liveT);
  CHECK(b.maxkT == maxkT, "levels", "maxkT %d, expected %d", b.maxkT, maxkT);
  check_clist("clJ[0]", b.clJ[0], false, liveT, bm.sJ, bm.mJ, maxlevT > 0);
  check_clist("clJ[1]", b.clJ[1], true, liveT, bm.sJ, bm.mJ, maxlevT > 0);
  bump("level lists", nJ, (long long)b.lmapJ.size() + (long long)b.lmapT.size());
  g_cnt["cooperative lists"].problems += nJ;

  // ---- pcl
  {
    const bool none = c.use_jacobi || nJ > c.prep_split_max;
    if (none) {
      CHECK(b.pcl.empty(), "pcl", "%zu items where none are expected", b.pcl.size());
      if (!c.use_jacobi && nJ > 0) ++g_shape["batches with an empty pcl (nJ > prep_split_max)"];
    } else {
      std::vector<int> eq(nJ, 0);
      std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> rg;
      long long prev = -1;
      for (const int4& it : b.pcl) {
        CHECK(it.x >= 0 && it.x < nJ && it.y >= 0 && it.y <= 2, "pcl", "item of problem %d, pass %d", it.x, it.y);
        long long len = 0;
        if (it.y == 2) ++eq[it.x];
        else {
          CHECK(it.z < it.w, "pcl", "empty range of problem %d", it.x);
          rg[{it.x, it.y}].push_back({it.z, it.w});
          const int kc = popc(it.y == 0 ? bm.sJ[it.x].maskP : bm.sJ[it.x].maskM);
          len = (long long)(it.w - it.z) << (kc > PCA ? kc - PCA : 0);
        }
        CHECK(prev < 0 || len <= prev, "pcl", "the items are not sorted longest first");
        prev = len;
      }
      for (int p = 0; p < nJ; ++p) {
        CHECK(eq[p] == 1, "pcl", "%d eq items of problem %d", eq[p], p);
        const int kP = popc(bm.sJ[p].maskP), kM = popc(bm.sJ[p].maskM);
        const bool taken = (b.route[p] == RT_W && c.wsolve_mode != 2) || kP > PCA + PCH || kM > PCA + PCH;
        for (int cl = 0; cl < 2; ++cl) {
          auto it = rg.find({p, cl});
          if (taken) { CHECK(it == rg.end(), "pcl", "class items of problem %d, which another kernel takes", p); continue; }
          CHECK(it != rg.end(), "pcl", "no class %d items of problem %d", cl, p);
          const int kc = cl == 0 ? kP : kM, kf = cl == 0 ? kM : kP;
          const int no = pclass_outer_bits(kc, kf), per = std::max(1, c.pcl_per >> (kc > PCA ? kc - PCA : 0));
          std::sort(it->second.begin(), it->second.end());
          int at = 0;
          for (auto& r : it->second) {
            CHECK(r.first == at && r.second - r.first <= per, "pcl", "problem %d class %d: range [%d, %d) after %d, %d per item", p, cl, r.first, r.second, at, per);
            at = r.second;
          }
          CHECK(at == 1 << no, "pcl", "problem %d class %d: ranges end at %d of %d", p, cl, at, 1 << no);
        }
      }
      g_cnt["pcl"].problems += nJ;
      g_shape["pcl items"] += (long long)b.pcl.size();
    }
  }

  // ---- mapX
  {
    std::vector<std::pair<int, uint32_t>> want, got;
    for (int p = 0; p < nJ; ++p)
      if (popc(bm.sJ[p].maskP) > PCA + PCH || popc(bm.sJ[p].maskM) > PCA + PCH)
        for (uint32_t H = 0; H < tiles_of(bm.sJ[p].k); ++H) want.push_back({p, H});
    for (const int2& m : b.mapX) got.push_back({m.x, (uint32_t)m.y});
    CHECK(want == got, "mapX", "%zu tiles listed, %zu expected", got.size(), want.size());
    bump("mapX", nJ, (long long)want.size());
  }

  // ---- small-space classes and staged groups
  {
    const bool all_staged = !c.small_path || c.use_jacobi;
    std::vector<int> where(b.pats.size(), 0);
    auto largest = [&](int pi) { int ks = -1; for (int part = 0; part < 2; ++part) if (b.pats[pi].s[part] >= 0) ks = std::max(ks, bm.sS[b.pats[pi].s[part]].k); return ks; };
    auto both = [&](int pi) { return b.pats[pi].s[0] >= 0 && b.pats[pi].s[1] >= 0; };
    // the rows whose natural class is the 1 024-thread one
    std::vector<int> big;
    int mk = 0;
    for (size_t pi = 0; pi < b.pats.size(); ++pi) {
      const int ks = largest((int)pi);
      if (!all_staged && b.pats[pi].j >= 0 && ks > spatient_class_maxk(1) && ks <= TB) { big.push_back((int)pi); mk = std::max(mk, ks); }
    }
    const bool merge = !big.empty() && big.size() <= 16 && mk <= 10 && (spatient_lds<T>(N, mk) + 15) / 16 * 16 * 2 + 64 <= (size_t)160 * 1024;
    CHECK(b.mk1p == (merge ? mk : spatient_class_maxk(1)), "small", "mk1p %d with %zu rows of the large class (largest %d bits)", b.mk1p, big.size(), mk);
    if (merge) { g_shape["rows merged into the 256-thread launch"] += (long long)big.size(); ++g_shape["batches with a merge"]; }
    else if (!big.empty()) ++g_shape["batches with a launch of the 1024-thread class"];
    bool has_small = false;
    for (int w = 0; w < 3; ++w)
      for (int cl = 0; cl < SP_NCLASS; ++cl) {
        int prevk = 1 << 30;
        for (int pi : b.sp_list[w][cl]) {
          CHECK(pi >= 0 && pi < (int)b.pats.size(), "small", "patient %d", pi);
          has_small = true;
          ++where[pi];
          const PatRec& pr = b.pats[pi];
          const int ks = largest(pi);
          CHECK(ks >= 0 && !all_staged && ks <= TB, "small", "patient %d (largest space %d bits) on the small-space path", pi, ks);
          CHECK(ks <= (cl == 1 && w >= 1 ? b.mk1p : spatient_class_maxk(cl)), "small", "patient %d: %d bits in class %d", pi, ks, cl);
          int nat = 0;
          while (nat < SP_NCLASS - 1 && ks > spatient_class_maxk(nat)) ++nat;
          CHECK(cl == (nat == 2 && merge && pr.j >= 0 ? 1 : nat), "small", "patient %d (%d bits) in class %d, expected %d%s", pi, ks, cl, nat, merge ? " (merged)" : "");
          CHECK(w == (pr.j < 0 ? 0 : both(pi) && cl < 2 ? 2 : 1), "small", "patient %d in list %d of class %d", pi, w, cl);
          const int key = 64 * ks + (both(pi) ? 32 : 0) + pr.kind;
          CHECK(key <= prevk, "small", "class list [%d][%d] is not sorted largest first", w, cl);
          prevk = key;
        }
      }
    CHECK(b.has_small == has_small, "small", "has_small");
    const std::vector<int2> none;
    for (int w = 0; w < 2; ++w) {
      const Staged& g = b.stg[w];
      std::vector<int> paired_, probs;
      bool kind2 = false;
      int prev = -1;
      for (int pi : g.pats) {
        CHECK(pi > prev && pi < (int)b.pats.size(), "staged", "patients of group %d are not ascending", w);
        prev = pi;
        ++where[pi];
        const PatRec& pr = b.pats[pi];
        const int ks = largest(pi);
        CHECK(ks >= 0 && (all_staged || ks > TB), "staged", "patient %d (largest space %d bits) in a staged group", pi, ks);
        CHECK(w == (all_staged || pr.j >= 0 ? 1 : 0), "staged", "patient %d in group %d", pi, w);
        if (pr.j >= 0) paired_.push_back(pi);
        for (int part = 0; part < 2; ++part) if (pr.s[part] >= 0) probs.push_back(pr.s[part]);
        kind2 = kind2 || pr.kind == 2;
        if (ks > TB) ++g_shape["patients with a single-tumour space beyond a tile"];
      }
      CHECK(g.paired == paired_ && g.probs == probs && g.kind2 == kind2, "staged", "paired / probs / kind2 of group %d", w);
      std::set<int> ps(probs.begin(), probs.end());
      std::set<std::pair<int, uint32_t>> tiles;
      std::vector<std::pair<int, int>> map, grc, gmap, ggrc;
      int maxk = 0, maxlev = 0;
      for (int p : ps) {
        maxk = std::max(maxk, bm.sS[p].k);
        for (uint32_t H = 0; H < tiles_of(bm.sS[p].k); ++H) { map.push_back({p, (int)H}); tiles.insert({p, H}); maxlev = std::max(maxlev, popc(H)); }
        for (int ch = 0; ch < 1 << std::max(0, bm.sS[p].k - GR_CHUNK); ++ch) grc.push_back({p, ch});
        const TileModel* m = bm.mS[p];
        if (m) for (uint32_t H = 0; H < m->ntiles; ++H) for (uint32_t Hs : m->src[0][H])
          CHECK(popc(Hs) < popc(H), "levels", "single-tumour problem %d tile %u reads tile %u of no lower level", p, H, Hs);
      }
      for (const int2& m : g.map) gmap.push_back({m.x, m.y});
      for (const int2& m : g.grc) ggrc.push_back({m.x, m.y});
      CHECK(gmap == map && ggrc == grc && g.maxk == maxk, "staged", "map / grc / maxk of group %d", w);
      check_level_list(w ? "stg[1].lmap" : "stg[0].lmap", g.lmap, g.lof, tiles);
      const bool expect = !c.use_jacobi && maxlev > 0;
      check_clist(w ? "stg[1].cl[0]" : "stg[0].cl[0]", g.cl[0], false, tiles, bm.sS, bm.mS, expect);
      check_clist(w ? "stg[1].cl[1]" : "stg[0].cl[1]", g.cl[1], true, tiles, bm.sS, bm.mS, expect);
      bump("staged groups", (long long)ps.size(), (long long)tiles.size());
    }
    for (size_t pi = 0; pi < b.pats.size(); ++pi)
      CHECK(where[pi] == (largest((int)pi) >= 0 ? 1 : 0), "small", "patient %zu lies in %d lists", pi, where[pi]);
    g_cnt["small-space classes"].problems += (long long)b.pats.size();
  }

  // ---- gradient chunks
  {
    std::vector<std::pair<int, int>> want, got;
    for (int kd = 0; kd < 3; ++kd)
      for (int p = 0; p < nJ; ++p) {
        const int kc = popc(kd == 0 ? bm.sJ[p].maskP : kd == 1 ? bm.sJ[p].maskM : bm.sJ[p].pairP);
        for (int ch = 0; ch < 1 << std::max(0, kc - GR_CHUNK); ++ch) want.push_back({p, ch | (kd << 24)});
      }
    for (const int2& e : b.grcJ) got.push_back({e.x, e.y});
    CHECK(want == got, "grad-chunks", "%zu entries, %zu expected", got.size(), want.size());
    bump("gradient chunks", nJ, (long long)want.size());
  }

  // ---- footprint
  {
    long long as = 0;
    for (int p = 0; p < nJ; ++p) as += class_array_size(bm.sJ[p]);
    const size_t fp = footprint<T>(c, N, b.vecJ, b.vecS, as, b.tabJ + b.tabS, (size_t)nJ, (size_t)nS, b.pats.size());
    CHECK(fp <= c.ws_limit || b.pats.size() == 1, "batches", "a batch of %zu rows occupies %zu bytes of %zu", b.pats.size(), fp, c.ws_limit);
    CHECK(b.asize >= as && b.asize <= as + 3, "layouts", "asize %lld for %lld elements of class arrays", b.asize, as);
  }
  (void)is_last;
}

template <typename T>
static void check_plan(const PlanCfg& c, const Cohort& co, const char* tname) {
  g_ctx = "cohort " + co.name + " (n = " + std::to_string(co.n) + ", " + tname + "), config {" + cfg_name(c) + "}";
  const int n = co.n, nc = 2 * n + 3;
  double n_em = -1;
  std::vector<Batch> plan;
  try {
    plan = plan_cohort<T>(c, co.dat.data(), co.np(), nc, n, n_em);
  } catch (const Fail& f) {
    fail("plan", "the planner refused the cohort: %s", f.msg.c_str());
  }
  const std::string base = g_ctx;
  long long next_row = 0, em = 0, npJ = 0;
  for (long long r = 0; r < co.np(); ++r) { em += co.row(r)[2 * n]; npJ += co.row(r)[2 * n + 2] == 3; }
  CHECK(n_em == (double)em, "batches", "n_em %g, %lld rows with the seeding", n_em, em);
  for (size_t i = 0; i < plan.size(); ++i) {
    g_ctx = base + ", batch " + std::to_string(i) + " of " + std::to_string(plan.size());
    CHECK(plan[i].id == (int)i, "batches", "batch id %d", plan[i].id);
    check_batch<T>(c, co, plan[i], i + 1 == plan.size(), next_row);
  }
  g_ctx = base;
  CHECK(next_row == co.np(), "batches", "%lld of %lld rows are in a batch", next_row, co.np());
  // a cut cohort with a target of paired rows per batch: every batch but the last holds the target, unless the next
  // paired row would not have fitted (necessity); without such a batch the last one holds the remainder, which an even
  // spread keeps within one row per batch of the target
  const CutTargets tg = batch_targets<T>(c, co.dat.data(), co.np(), nc, n);
  if (plan.size() > 1) ++g_shape["plans with a cut cohort"];
  if (tg.pats > 0 && plan.size() > 1) {
    bool forced = false;
    for (size_t i = 0; i + 1 < plan.size(); ++i) {
      const long long have = (long long)plan[i].dJ.size();
      CHECK(have <= tg.pats, "batches", "batch %zu holds %lld paired rows, target %lld", i, have, tg.pats);
      if (have < tg.pats) forced = true;
    }
    if (!forced) {
      const long long nb = (npJ + tg.pats - 1) / tg.pats, last = npJ - (nb - 1) * tg.pats;
      CHECK((long long)plan.size() == nb && (long long)plan.back().dJ.size() == last, "batches", "%zu batches of %lld paired rows at %lld per batch", plan.size(), npJ, tg.pats);
      if (tg.pats % c.n_cu != 0) {   // the target is no multiple of the CU count: the rows were spread evenly
        CHECK(last >= tg.pats - (nb - 1), "batches", "the last batch holds %lld paired rows against %lld in the others", last, tg.pats);
        ++g_shape["cohorts with an evenly spread target"];
      }
      ++g_shape["cohorts cut by a paired-row target"];
    }
  }
  for (auto* name : {"batches", "paired", "dead tiles", "cooperative lists", "level lists", "routes", "ptiles", "layouts", "window chains", "pcl", "mapX",
                     "small-space classes", "staged groups", "gradient chunks"})
    ++g_cnt[name].plans;
}

// ------------------------------------------------------------------------------------ rejections
static const char* TOO_MANY = "too many active events for one patient";
static void check_rejections() {
  g_ctx = "rejections";
  PlanCfg c;
  c.ws_limit = (size_t)1 << 30;
  // the planner's message, "" when the cohort is accepted
  auto refusal = [&](const Cohort& co) -> std::string {
    double n_em;
    try { plan_cohort<double>(c, co.dat.data(), co.np(), 2 * co.n + 3, co.n, n_em); } catch (const Fail& f) { return f.msg.empty() ? "?" : f.msg; }
    return "";
  };
  auto throws = [&](const Cohort& co) { return !refusal(co).empty(); };
  Cohort a; a.n = 4; add_pattern(a, "JP", 1, 0, 4);
  Cohort a2; a2.n = 4; add_pattern(a2, "JP", 1, 0, -1);
  Cohort b; b.n = 4; add_pattern(b, "JP", 1, 0, 3); b.dat[1] = 2;
  Cohort b2; b2.n = 4; add_pattern(b2, "JP", 1, 0, 3); b2.dat[2 * 4] = 2;
  Cohort s; s.n = 4; add_pattern(s, "JP", 0, 0, 3);
  Cohort k; k.n = 16; add_pattern(k, rep('J', 15), 1, 0, 3);            // 31 bits
  Cohort ok; ok.n = 16; add_pattern(ok, rep('J', 8), 1, 0, 3);
  CHECK(throws(a) && throws(a2), "rejections", "a type outside 0 .. 3 is accepted");
  CHECK(throws(b) && throws(b2), "rejections", "an event column other than 0 / 1 is accepted");
  CHECK(throws(s), "rejections", "a paired row without seeding is accepted");
  CHECK(refusal(k) == TOO_MANY, "rejections", "a row of more than MAXK active events is accepted");
  CHECK(!throws(ok), "rejections", "a valid row is refused");
  g_cnt["rejections"].plans += 7;
  // single-tumour spaces of more than MAXK bits: unpaired rows, alone, behind a valid row (the last row of the cohort) and
  // between two valid rows.  Every cohort is planned before the first verdict, so that a run on a planner that accepts
  // them still shows what the sanitizers say about the 32-bit row
  struct Wide { const char* what; int n, type, seed; char ch; int events; };
  const Wide wide[] = {{"type 0, n = 31, 31 PT events (k = 31)", 31, 0, 0, 'P', 31},
                       {"type 1, n = 31, 31 PT events and the seeding (k = 32)", 31, 1, 1, 'P', 31},
                       {"type 2, n = 30, 30 MT events and the seeding (k = 31)", 30, 2, 1, 'M', 30},
                       {"type 3, n = 31, 31 joint events and the seeding (k = 63)", 31, 3, 1, 'J', 31}};
  std::vector<std::pair<std::string, std::string>> got;
  for (const Wide& w : wide)
    for (int place = 0; place < 3; ++place) {
      Cohort co; co.n = w.n;
      if (place >= 1) add_pattern(co, "JP", 1, 0, 3);
      add_pattern(co, rep(w.ch, w.events), w.seed, w.type == 3 ? 0 : -99, w.type);
      if (place == 2) add_pattern(co, "P", 1, -99, 1);
      got.push_back({std::string(w.what) + (place == 0 ? ", alone" : place == 1 ? ", last behind a valid row" : ", between valid rows"), refusal(co)});
    }
  for (auto& e : got) std::printf("refusal of %s: \"%s\"\n", e.first.c_str(), e.second.c_str());
  for (auto& e : got) CHECK(e.second == TOO_MANY, "rejections", "%s: %s", e.first.c_str(), e.second.empty() ? "accepted" : e.second.c_str());
  // a paired row without seeding keeps its own message whatever its size
  Cohort s31; s31.n = 31; add_pattern(s31, rep('J', 31), 0, 0, 3);
  CHECK(refusal(s31) == "dat: paired rows (type 3) must have seeding = 1", "rejections", "a wide paired row without seeding: \"%s\"", refusal(s31).c_str());
  g_cnt["rejections"].plans += (long long)got.size() + 1;
}

// ------------------------------------------------------------------------------------ the size limits
// Spaces of exactly MAXK = 30 bits at n = 31 are planned; their 2^30 states are not enumerated - sizes only
template <typename T>
static void check_limit_sizes(const char* tname) {
  PlanCfg c;
  c.ws_limit = (size_t)64 << 30;
  const int n = 31, nc = 2 * n + 3, N = n + 1;
  struct Case { const char* name; std::string ev; int order, type; };
  const Case cases[] = {{"type 1, 29 PT events and the seeding", rep('P', 29), -99, 1},
                        {"paired, 15 PT and 14 MT events and the seeding", rep('P', 15) + rep('M', 14), 0, 3},
                        {"paired, 10 joint, 5 PT and 4 MT events and the seeding", rep('J', 10) + rep('P', 5) + rep('M', 4), 2, 3}};
  for (const Case& cs : cases) {
    g_ctx = std::string("limit sizes (") + tname + "): " + cs.name;
    Cohort co; co.n = n;
    add_pattern(co, "JP", 1, 1, 3);                       // a small row (k = 4) in front: the offsets of the large one are not 0
    add_pattern(co, cs.ev, 1, cs.order, cs.type);
    double n_em = -1;
    std::vector<Batch> plan;
    try { plan = plan_cohort<T>(c, co.dat.data(), co.np(), nc, n, n_em); } catch (const Fail& f) { fail("limits", "refused: %s", f.msg.c_str()); }
    CHECK(plan.size() == 1 && plan[0].pats.size() == 2 && n_em == 2.0, "limits", "%zu batches", plan.size());
    const Batch& b = plan[0];
    const long long big = 1ll << MAXK;
    long long prev = -1, as = 0, tabs = 0;
    if (cs.type == 3) {
      CHECK(b.dJ.size() == 2 && b.dJ[1].k == MAXK && b.vecJ == big + 16 && b.maxkJ == MAXK, "limits", "vecJ %lld", b.vecJ);
      CHECK(b.mapJ.size() == (size_t)(1 << (MAXK - TB)) + 1, "limits", "%zu joint tiles", b.mapJ.size());
      CHECK(b.mapJ.back().x == 1 && b.mapJ.back().y == (1 << (MAXK - TB)) - 1, "limits", "last joint tile %d", b.mapJ.back().y);
      CHECK(b.dS.size() == (cs.order == 0 ? 3u : 2u), "limits", "%zu single-tumour problems", b.dS.size());
      std::vector<long long> offs;
      for (const Desc& d : b.dJ) offs.push_back(d.off);
      std::sort(offs.begin(), offs.end());
      CHECK(offs[0] == 0 && (offs[1] == 16 || offs[1] == big), "limits", "joint offsets %lld, %lld", offs[0], offs[1]);
    } else {
      CHECK(b.dJ.size() == 1 && b.dS.size() == 2 && b.dS[1].k == MAXK && b.dS[1].seedbit == MAXK - 1, "limits", "single-tumour problems");
      CHECK(b.vecS == big + 4 && b.dS[1].off == 4, "limits", "vecS %lld", b.vecS);
      CHECK(b.mapS.size() == (size_t)(1 << (MAXK - TB)) + 1 && b.mapS.back().y == (1 << (MAXK - TB)) - 1, "limits", "%zu single-tumour tiles", b.mapS.size());
      CHECK(b.stg[0].map.size() == (size_t)1 << (MAXK - TB) && b.stg[0].maxk == MAXK && b.stg[0].lmap.size() == b.stg[0].map.size(),
            "limits", "%zu staged tiles", b.stg[0].map.size());
      CHECK(b.stg[0].cl[0].items.size() == b.stg[0].map.size() && b.stg[0].cl[1].items.size() == b.stg[0].map.size(), "limits", "cooperative lists");
      CHECK(b.stg[0].grc.size() == (size_t)1 << (MAXK - GR_CHUNK), "limits", "%zu gradient chunks", b.stg[0].grc.size());
    }
    for (const Desc& d : b.dS) {
      CHECK(d.off > prev && d.off >= 0 && d.toff >= 0 && d.off + (1ll << d.k) <= b.vecS, "limits", "single-tumour offset %lld after %lld", d.off, prev);
      prev = d.off;
      tabs += table_size(d);
    }
    for (const Desc& d : b.dJ) {
      CHECK(d.off >= 0 && d.off + (1ll << d.k) <= b.vecJ && d.aoff >= 0 && d.toff >= 0, "limits", "joint offsets %lld / %lld / %lld", d.off, d.aoff, d.toff);
      as += a_size(d); tabs += table_size(d);
    }
    CHECK(b.tabJ + b.tabS == tabs && b.asize >= as && b.asize <= as + 3, "limits", "tables %lld + %lld, class arrays %lld", b.tabJ, b.tabS, b.asize);
    // the footprint in 64-bit size_t against the sum of its large terms in long double: not wrapped, within the workspace
    const size_t fp = footprint<T>(c, N, b.vecJ, b.vecS, b.asize, tabs, b.dJ.size(), b.dS.size(), b.pats.size());
    const long double lower = ((long double)2 * b.vecJ + (long double)4 * b.vecS + (long double)b.asize + (long double)tabs) * sizeof(T);
    CHECK((long double)fp >= lower && (long double)fp <= lower + (long double)(1 << 20) && fp <= c.ws_limit, "limits", "footprint %zu for %.0Lf bytes of vectors", fp, lower);
    ++g_shape["plans with a space of MAXK bits"];
  }
}

static void print_counts() {
  for (auto& kv : g_cnt)
    std::printf("check %-22s plans %6lld  problems %9lld  tiles %10lld\n", kv.first.c_str(), kv.second.plans, kv.second.problems, kv.second.tiles);
  for (auto& kv : g_shape) std::printf("count %s: %lld\n", kv.first.c_str(), kv.second);
}

template <typename T>
static void sweep(const Cohort& co, const std::vector<PlanCfg>& cfgs, const char* tname) {
  for (const PlanCfg& c : cfgs) check_plan<T>(c, co, tname);
}

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "--cohort") {
    Cohort co;
    co.name = argv[2];
    const long long np = std::atoll(argv[3]);
    co.n = std::atoi(argv[4]);
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[2]); return 2; }
    co.dat.resize((size_t)np * (2 * co.n + 3));
    const size_t got = std::fread(co.dat.data(), 1, co.dat.size(), f);
    std::fclose(f);
    if (got != co.dat.size()) { std::printf("%s is shorter than %lld rows\n", argv[2], np); return 2; }
    PlanCfg c;
    c.ws_limit = (size_t)8 << 30;
    check_plan<double>(c, co, "double");
    c.psolve_min = 1;
    check_plan<double>(c, co, "double");
    c = PlanCfg();
    c.ws_limit = (size_t)8 << 30; c.wsolve_min = 1;
    check_plan<double>(c, co, "double");
    c.wsolve_wgs = 3;
    check_plan<double>(c, co, "double");
    c = PlanCfg();
    c.ws_limit = (size_t)8 << 30; c.prep_split_max = 0;
    check_plan<double>(c, co, "double");
    c.prep_split_max = 2048; c.pcl_per = 1;
    check_plan<double>(c, co, "double");
    print_counts();
    std::printf("plan_check: cohort ok\n");
    return 0;
  }
  const std::vector<PlanCfg> cfgs = config_sweep();
  std::vector<Cohort> cohorts;
  cohorts.push_back(random_cohort("random-3", 3, 200, 3, false));
  cohorts.push_back(random_cohort("random-9", 9, 300, 9, true));
  cohorts.push_back(random_cohort("random-13", 13, 160, 13, true));
  cohorts.push_back(random_cohort("random-16", 16, 120, 16, true));
  cohorts.push_back(window_cohort("window-13", 13));
  cohorts.push_back(small_class_cohort("small-16x10", 9, 16, 10));
  cohorts.push_back(small_class_cohort("small-17x10", 9, 17, 10));
  cohorts.push_back(small_class_cohort("small-16x11", 13, 16, 11));
  cohorts.push_back(small_class_cohort("small-3x10", 16, 3, 10));
  for (const Cohort& co : cohorts) {
    sweep<double>(co, cfgs, "double");
    sweep<float>(co, cfgs, "float");
  }
  // the largest event count: the seeding is event 31, dat has 65 columns
  const Cohort top = top_event_cohort("top-events-31", 120, 31);
  sweep<double>(top, cfgs, "double");
  sweep<float>(top, cfgs, "float");
  g_shape["rows planned at n = 31"] += top.np();
  check_rejections();
  check_limit_sizes<double>("double");
  check_limit_sizes<float>("float");
  print_counts();
  const char* must[] = {"rows planned at n = 31", "plans with a space of MAXK bits", "straddling tiles", "straddling tiles live without seeding", "dead tiles", "batches with dealt chains", "window chains of several rows", "rows merged into the 256-thread launch",
                        "batches with a launch of the 1024-thread class", "batches with an empty pcl (nJ > prep_split_max)", "plans with a cut cohort",
                        "patients with a single-tumour space beyond a tile", "problems on the window route", "problems on the per-patient route",
                        "problems on the tile route", "cooperative dependencies required by the model"};
  g_ctx = "sweep";
  for (const char* m : must) CHECK(g_shape[m] > 0, "coverage", "the sweep reached no case of: %s", m);
  std::printf("plan_check: ok\n");
  return 0;
}
