// Stand-alone check of the storage-row permutation of the window layout (metmhn_amd/csrc/wlayout.h: wrho, wrho_inv).
//
// No GPU runtime call is made: the program runs on any host, and is meant to be built with the host sanitizers.
//   * wrho is a bijection of 16 waves x 64 lanes onto the 1024 storage rows of a block, and wrho_inv inverts it;
//   * the rows of every (w, m) group - wave w, lanes of lane-level m = popcount of l - are one contiguous run, in lane order
//     (what a wave instruction of k_wsolve requests);
//   * the all-ones row wpos_marg addresses is wrho(15, 63), and both branches of wpos_marg agree with wpos_nat;
//   * the line model: a step of the solve requests the rows of one CLASS (m, lam), lam = popcount of w, together, so a
//     line (of 4 rows: 128 bytes, or of 2 rows: 64 bytes) counts once per class that has a row in it.  A block is 256
//     lines; the order "lane-level, then wave" the layout had before requests 304 lines and 544 half-lines (recomputed
//     here from that order, which pins the model), and the shipped order must stay strictly below both.
// Prints "lines128 N" and "lines64 N"; exit status 1 on the first violation.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "wlayout.h"

using namespace mmhn;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("VIOLATION: " __VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// the order before: rows sorted by lane-level, then wave, then rank of the lane in its level
static uint32_t rho_by_level_then_wave(uint32_t w, uint32_t l) {
  static const int binom[7] = {1, 6, 15, 20, 15, 6, 1};
  const int m = popc(l);
  int before = 0, rank = 0;
  for (int j = 0; j < m; ++j) before += binom[j];
  for (uint32_t j = 0; j < l; ++j) rank += popc(j) == m;
  return 16u * (uint32_t)before + w * (uint32_t)binom[m] + (uint32_t)rank;
}

// lines of `rows_per_line` storage rows requested per block, a line shared only inside a class (m, lam)
template <typename F>
static int lines_requested(F rho, int rows_per_line) {
  std::set<std::pair<int, uint32_t>> touched;                  // (class, line)
  for (uint32_t w = 0; w < 16; ++w)
    for (uint32_t l = 0; l < 64; ++l) touched.insert({popc(l) * 8 + popc(w), rho(w, l) / (uint32_t)rows_per_line});
  return (int)touched.size();
}

template <typename T>
static long long check_marg(int kR, int kC, bool majP) {
  // the two classes interleaved over the k - 1 natural bits below the seeding bit, the row class on the even bits first
  WDesc wd{};
  const int k = kR + kC + 1;
  int nr = 0, nc = 0;
  for (int b = 0; b < k - 1; ++b) {
    const bool row = (b % 2 == 0 && nr < kR) || nc == kC;
    if (row) { wd.rowmask |= 1u << b; wd.rb[nr++] = (int8_t)b; } else { wd.colmask |= 1u << b; wd.cb[nc++] = (int8_t)b; }
  }
  CHECK(nr == kR && nc == kC, "bit deal kR %d kC %d", kR, kC);
  wd.kR = kR; wd.kC = kC; wd.majP = majP;
  wd.nXc = kC - WCfg<T>::RB - WCfg<T>::HB; wd.nXr = kR - WTB;
  const long long half = 1ll << (k - 1);
  long long n = 0;
  std::set<long long> seen;
  for (uint32_t f = 0; f < (1u << kR); ++f, ++n) {
    const long long a = wpos_marg<T>(wd, k, true, f), b = half + wpos_nat<T>(wd, pdep32(f, wd.rowmask) | wd.colmask);
    CHECK(a == b, "wpos_marg (free rows) f %u: %lld, wpos_nat %lld", f, a, b);
    CHECK(a >= half && a < 2 * half && seen.insert(a).second, "wpos_marg (free rows) f %u out of the half or met twice", f);
  }
  seen.clear();
  for (uint32_t f = 0; f < (1u << kC); ++f, ++n) {
    const long long a = wpos_marg<T>(wd, k, false, f), b = half + wpos_nat<T>(wd, pdep32(f, wd.colmask) | wd.rowmask);
    CHECK(a == b, "wpos_marg (free columns) f %u: %lld, wpos_nat %lld", f, a, b);
    CHECK(a >= half && a < 2 * half && seen.insert(a).second, "wpos_marg (free columns) f %u out of the half or met twice", f);
    const uint32_t Sigma = (f >> (WCfg<T>::RB + WCfg<T>::HB)) | (((1u << wd.nXr) - 1u) << wd.nXc);
    const long long c = half + wpos<T>(Sigma, (f >> WCfg<T>::RB) & ((1u << WCfg<T>::HB) - 1u), wrho(15, 63), f & ((1u << WCfg<T>::RB) - 1u));
    CHECK(a == c, "wpos_marg (free columns) f %u: %lld, through wrho(15, 63) %lld", f, a, c);
  }
  return n;
}

int main() {
  // bijection and inverse
  std::vector<int> owner(WROWS, -1);
  for (uint32_t w = 0; w < 16; ++w)
    for (uint32_t l = 0; l < 64; ++l) {
      const uint32_t r = wrho(w, l);
      CHECK(r < (uint32_t)WROWS, "wrho(%u, %u) = %u is no row of a block", w, l, r);
      CHECK(owner[r] < 0, "wrho(%u, %u) = %u is also the row of thread %d", w, l, r, owner[r]);
      owner[r] = (int)(w << 6 | l);
      CHECK(wrho_inv(r) == (w << 6 | l), "wrho_inv(%u) = %u, wrho(%u, %u) = %u", r, wrho_inv(r), w, l, r);
    }
  for (uint32_t r = 0; r < (uint32_t)WROWS; ++r) {
    const uint32_t t = wrho_inv(r);
    CHECK(t < (uint32_t)WROWS && wrho(t >> 6, t & 63u) == r, "wrho(wrho_inv(%u)) = %u", r, wrho(t >> 6, t & 63u));
  }
  // every (w, m) group is one contiguous run, its lanes in ascending order
  int groups = 0;
  for (uint32_t w = 0; w < 16; ++w)
    for (int m = 0; m <= 6; ++m, ++groups) {
      uint32_t next = 0;
      bool first = true;
      for (uint32_t l = 0; l < 64; ++l) {
        if (popc(l) != m) continue;
        const uint32_t r = wrho(w, l);
        CHECK(first || r == next, "group (w %u, m %d): lane %u at row %u, expected %u", w, m, l, r, next);
        first = false;
        next = r + 1;
      }
    }
  // every class (m, lam) is one contiguous run as well (its groups are requested in one step)
  for (int lam = 0; lam <= 4; ++lam)
    for (int m = 0; m <= 6; ++m) {
      uint32_t lo = WROWS, hi = 0, cnt = 0;
      for (uint32_t w = 0; w < 16; ++w)
        for (uint32_t l = 0; l < 64; ++l)
          if (popc(w) == lam && popc(l) == m) { const uint32_t r = wrho(w, l); lo = r < lo ? r : lo; hi = r > hi ? r : hi; ++cnt; }
      CHECK(hi - lo + 1 == cnt, "class (m %d, lam %d): %u rows in the run %u .. %u", m, lam, cnt, lo, hi);
    }
  // wpos_marg against wpos_nat: fp64 and fp32 shapes with and without external bits of either kind
  long long states = 0;
  states += check_marg<double>(10, 4, true);
  states += check_marg<double>(12, 6, false);
  states += check_marg<double>(11, 8, true);
  states += check_marg<float>(10, 5, false);
  states += check_marg<float>(12, 7, true);
  // the line model
  const int old128 = lines_requested(rho_by_level_then_wave, 4), old64 = lines_requested(rho_by_level_then_wave, 2);
  CHECK(old128 == 304 && old64 == 544, "the model gives %d lines / %d half-lines for the order (m, w), not 304 / 544", old128, old64);
  const int l128 = lines_requested(wrho, 4), l64 = lines_requested(wrho, 2);
  std::printf("groups %d\nmarginal states %lld\nlines128 %d\nlines64 %d\n", groups, states, l128, l64);
  CHECK(l128 >= 256 && l64 >= 512, "fewer lines than a block has: %d / %d", l128, l64);
  CHECK(l128 < 304, "%d lines of 128 bytes per block, not below 304", l128);
  CHECK(l64 < 544, "%d lines of 64 bytes per block, not below 544", l64);
  return 0;
}
