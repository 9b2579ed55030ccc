// Class marginals of p (x) q for joint problems stored in the window layout (wlayout.h) - what k_pclass / k_class_marg
// compute for index-order vectors (kernels.h; reference: the reductions of x_partial_Q_y, likelihood.py:25-201, in the
// class-marginal form of DESIGN.md 3.2):
//   slot 0      W[S]   = - sum_T p[S,T] q[S,T]
//   slot 1 + l  V_l[S] =   sum_T p[S,T] q[S | bit_l, T]      (bit_l not in S)
// for both classes.  The seeded half is a matrix rows x columns (row class = the class with more bits); the layout
// keeps 1024 rows x NC columns ("a block") and, across blocks, RCH storage rows x every column contiguous in runs of
// RCH * 32 bytes.  One 1024-thread workgroup per patient, two phases, each reads p and q once:
//   phase R (row class):    thread = row.  Per block the rows' q values go through LDS (every thread-bit neighbour of a
//                           row is another row of the same block), the sums over the columns stay in registers for the
//                           whole patient and every table entry is written once - no atomics, no cross-lane reduction.
//                           Neighbours along the external row bits that phase C does not cover are other blocks:
//                           one extra read of q each.
//   phase C (column class): thread = 16-byte piece of columns x some rows of a chunk of RCH storage rows x the 2^m
//                           settings of the lowest m external row bits x all columns staged in LDS (every column
//                           neighbour and every neighbour along those m row bits is in the chunk); column sums over the
//                           rows in registers, one small reduction over the threads that share a piece at the end; the
//                           sums along the m external row bits are reduced per row over the threads that share it
//                           (DPP segment sums, across waves through LDS) and written once each.
//   m is the most of the external row bits for which a chunk still reads runs of at least one 128-byte line (fp64 at
//   k = 20: every external row bit of every shape).
#pragma once
#include "kernels.h"

namespace mmhn {

template <typename T>
struct WClass {
  static constexpr int CHE = 32768 / (int)sizeof(T);          // elements of one staged array (a block, or a chunk of rows)
  static constexpr int LGCHE = sizeof(T) == 8 ? 12 : 13;
  static constexpr int LGMINR = 2;                             // a run of a chunk: at least 4 storage rows (128 bytes)
  // most external row bits phase C covers (its chunks hold 2^(kC + m) <= CHE / 4 elements per storage row, kC >= RB + HB)
  static constexpr int MX = WCfg<T>::KR - WTB < LGCHE - LGMINR - WCfg<T>::RB - WCfg<T>::HB ? WCfg<T>::KR - WTB
                                                                                           : LGCHE - LGMINR - WCfg<T>::RB - WCfg<T>::HB;
  // partial sums of those: m * (CHE >> kC) rows x max(1, 2^kC / QE / 64) waves, at most MX * (CHE >> (RB + HB))
  static constexpr int XP = MX * (CHE >> (WCfg<T>::RB + WCfg<T>::HB));
  static constexpr size_t lds = (4 * (size_t)CHE + 2 * (size_t)XP) * sizeof(T) + WROWS * sizeof(uint16_t) + 64;
  static_assert((1 << LGCHE) == CHE, "");
};
// external row bits whose neighbours phase C of k_wclass sums (the rest: phase R's extra reads of q)
template <typename T>
__host__ __device__ inline int wclass_mbits(int kC, int nXr) {
  const int m = WClass<T>::LGCHE - WClass<T>::LGMINR - kC;
  return m < 0 ? 0 : m < nXr ? m : nXr;
}
// sum over aligned groups of 2^lg lanes (lg <= 6, wave-uniform): the total lands in the last lane of each group
template <typename T>
__device__ __forceinline__ T seg_sum(T v, int lg) {
  if (lg > 0) v = dpp_stage<0>(v);
  if (lg > 1) v = dpp_stage<1>(v);
  if (lg > 2) v = dpp_stage<2>(v);
  if (lg > 3) v = dpp_stage<3>(v);
  if (lg > 4) v = dpp_stage<4>(v);
  if (lg > 5) v = dpp_stage<5>(v);
  return v;
}
template <typename T>
constexpr size_t wclass_lds() { return WClass<T>::lds; }

template <typename T>
__global__ __launch_bounds__(WROWS) void k_wclass(const Desc* __restrict__ descs, const WDesc* __restrict__ wds, int nw,
                                                  const T* __restrict__ p, const T* __restrict__ q, T* A) {
  using C = WCfg<T>;
  constexpr int RB = C::RB, HB = C::HB, NC = 1 << RB, H = 1 << HB, KC = C::KC, WNXR = C::KR - WTB;
  constexpr int QE = 16 / (int)sizeof(T), LGQ = QE == 2 ? 1 : 2, NQ = NC / QE;
  constexpr int CHE = WClass<T>::CHE;
  typedef T VecT __attribute__((ext_vector_type(NC)));
  typedef T QT __attribute__((ext_vector_type(QE)));
  static_assert(NQ == 2 && CHE == WROWS * NC, "a block row is two 16-byte pieces; a block fills one staged array");
  extern __shared__ __align__(16) unsigned char smem[];
  T* const lds = reinterpret_cast<T*>(smem);                 // four staged arrays of CHE elements
  const int tid = threadIdx.x;
  const uint32_t rho = wrho((uint32_t)tid >> 6, (uint32_t)tid & 63u);
  // row index of storage row rho (wrho_inv, a chain of dependent table reads, out of the hot loop; read after the first
  // barrier of the problem loop)
  uint16_t* const rinv = reinterpret_cast<uint16_t*>(lds + 4 * (size_t)CHE + 2 * (size_t)WClass<T>::XP);
  rinv[rho] = (uint16_t)tid;
  for (int it = blockIdx.x; it < nw; it += gridDim.x) {
    const WDesc& wd = wds[it];
    const Desc& d = descs[wd.prob];
    const int k = d.k, kR = wd.kR, kC = wd.kC, nXc = wd.nXc, nXr = wd.nXr;
    const bool majP = wd.majP != 0;
    const long long half = 1ll << (k - 1);
    const T* ps = p + d.off + half;
    const T* qs = q + d.off + half;
    const int kP = __popc(d.maskP);
    T* outR = A + d.aoff + (majP ? 0 : class_block_size(kP));
    T* outC = A + d.aoff + (majP ? class_block_size(kP) : 0);
    const int NBc = (1 << nXc) << HB;                         // blocks of one external row setting
    const int mX = wclass_mbits<T>(kC, nXr);                  // external row bits of phase C
    auto ldv = [&](const T* src, uint32_t Sigma, uint32_t beta, uint32_t row) -> VecT {
      const QT* a = reinterpret_cast<const QT*>(src + wpos<T>(Sigma, beta, row, 0));
      const QT lo = a[0], hi = a[1];
      VecT v;
#pragma unroll
      for (int e = 0; e < QE; ++e) { v[e] = lo[e]; v[QE + e] = hi[e]; }
      return v;
    };
    auto dot = [&](const VecT& a, const VecT& b) -> T {
      T s = a[0] * b[0];
#pragma unroll
      for (int c = 1; c < NC; ++c) s += a[c] * b[c];
      return s;
    };
    // =============================== phase R: thread = row
    __syncthreads();                                           // the previous problem is done with the staged arrays
    for (uint32_t Sx = 0; Sx < (1u << nXr); ++Sx) {
      T acc[1 + WTB + WNXR];
#pragma unroll
      for (int s = 0; s < 1 + WTB + WNXR; ++s) acc[s] = T(0);
      VecT pn = ldv(ps, Sx << nXc, 0, rho), qn = ldv(qs, Sx << nXc, 0, rho);
      for (int B = 0; B < NBc; ++B) {
        const uint32_t Sigma = ((uint32_t)B >> HB) | (Sx << nXc), beta = (uint32_t)B & (uint32_t)(H - 1);
        const VecT pv = pn, qv = qn;
        if (B + 1 < NBc) {
          const uint32_t Sg2 = ((uint32_t)(B + 1) >> HB) | (Sx << nXc), b2 = (uint32_t)(B + 1) & (uint32_t)(H - 1);
          pn = ldv(ps, Sg2, b2, rho); qn = ldv(qs, Sg2, b2, rho);
        }
        T* qb = lds + (B & 1) * CHE;                          // [piece][row]: conflict-free 16-byte accesses
        {
          QT lo, hi;
#pragma unroll
          for (int e = 0; e < QE; ++e) { lo[e] = qv[e]; hi[e] = qv[QE + e]; }
          *reinterpret_cast<QT*>(qb + (size_t)tid * QE) = lo;
          *reinterpret_cast<QT*>(qb + (size_t)(WROWS + tid) * QE) = hi;
        }
        __syncthreads();
        acc[0] -= dot(pv, qv);
#pragma unroll
        for (int i = 0; i < WTB; ++i) {
          const uint32_t nb = (uint32_t)tid | (1u << i);
          const QT lo = *reinterpret_cast<const QT*>(qb + (size_t)nb * QE);
          const QT hi = *reinterpret_cast<const QT*>(qb + (size_t)(WROWS + nb) * QE);
          T s = T(0);
#pragma unroll
          for (int e = 0; e < QE; ++e) s += pv[e] * lo[e] + pv[QE + e] * hi[e];
          acc[1 + i] += s;                                     // (a row that has bit i never writes this slot: no select)
        }
#pragma unroll
        for (int i = 0; i < WNXR; ++i) {
          if (i >= mX && i < nXr && !((Sx >> i) & 1u)) {      // (uniform)
            const VecT qx = ldv(qs, Sigma | (1u << (nXc + i)), beta, rho);
            acc[1 + WTB + i] += dot(pv, qx);
          }
        }
      }
      const long long S = (long long)tid | ((long long)Sx << WTB);
      outR[S] = acc[0];
#pragma unroll
      for (int i = 0; i < WTB; ++i)
        if (!((tid >> i) & 1)) outR[((long long)(1 + i) << kR) + S] = acc[1 + i];
#pragma unroll
      for (int i = 0; i < WNXR; ++i)
        if (i >= mX && i < nXr && !((Sx >> i) & 1u)) outR[((long long)(1 + WTB + i) << kR) + S] = acc[1 + WTB + i];
    }
    // =============================== phase C: thread = piece of QE columns, rows of a chunk dealt over the threads
    {
      // a chunk: storage rows ch * RCH .. + RCH of the 2^mX row settings Sx = sxl | sxh << mX, every column; in LDS row
      // (sxl << lgR | r) x column T
      constexpr int XP = WClass<T>::XP, JU = sizeof(T) == 8 ? 2 : 1;
      static_assert(CHE == 2 * WROWS * QE, "a thread takes two rows of a chunk");
      const int lgR = WClass<T>::LGCHE - kC - mX;              // log2 of the storage rows of a chunk
      const int RCH = 1 << lgR, RCX = RCH << mX;               // storage rows, rows in LDS (= CHE >> kC)
      const int lgnch = WTB - lgR, nch = 1 << lgnch;
      const int lgP = kC - LGQ, NPc = 1 << lgP;                // pieces of a row (NPc divides 1024)
      const int cp = tid & (NPc - 1);
      const int r0 = tid >> lgP, rstep = WROWS >> lgP;         // rows r0, r0 + rstep of a chunk
      const int lgRX = lgR + mX, nW = lgP > 6 ? 1 << (lgP - 6) : 1;   // a row's sums: nW partials (one per wave)
      T* const xpart = lds + 4 * (size_t)CHE;                  // [2][XP]: [bit][row][wave] partials of the external row sums
      T ac[QE][1 + KC];
#pragma unroll
      for (int e = 0; e < QE; ++e)
#pragma unroll
        for (int s = 0; s <= KC; ++s) ac[e][s] = T(0);
      // piece g of a chunk (both arrays): run = block (sxl, Tx, beta), inside the run row-major
      const int lgrl = lgR + 1;                                // log2 of the pieces of a run (RCH rows x NQ pieces)
      auto piece_src = [&](int g, uint32_t sxh, int ch) -> long long {
        const int run = g >> lgrl, rr = g & ((1 << lgrl) - 1);
        const uint32_t Sigma = ((uint32_t)run >> HB) | (sxh << (nXc + mX)), beta = (uint32_t)run & (uint32_t)(H - 1);
        return wpos<T>(Sigma, beta, (uint32_t)(ch * RCH + (rr >> 1)), (uint32_t)((rr & 1) * QE));
      };
      auto piece_dst = [&](int g) -> int {
        const int run = g >> lgrl, rr = g & ((1 << lgrl) - 1);
        const int sxl = run >> (kC - RB), cb = run & ((1 << (kC - RB)) - 1);
        return (((sxl << lgR) | (rr >> 1)) << kC) + (cb << RB) + (rr & 1) * QE;
      };
      // table index of LDS row r of chunk cidx (without the slot)
      auto row_S = [&](int cidx, int r) -> long long {
        const uint32_t Sx = (uint32_t)(r >> lgR) | ((uint32_t)(cidx >> lgnch) << mX);
        return (long long)rinv[((cidx & (nch - 1)) << lgR) | (r & (RCH - 1))] | ((long long)Sx << WTB);
      };
      // the external row sums of chunk cidx: add the partials of a row in a fixed order, write the tables
      auto xfinish = [&](int cidx) {
        const T* xp = xpart + (cidx & 1) * XP;
        for (int i = tid; i < (mX << lgRX); i += WROWS) {
          const int l = i >> lgRX, r = i & (RCX - 1);
          if (!((r >> (lgR + l)) & 1)) {
            T v = xp[(size_t)i * nW];
            for (int w = 1; w < nW; ++w) v += xp[(size_t)i * nW + w];
            outR[((long long)(1 + WTB + l) << kR) + row_S(cidx, r)] = v;
          }
        }
      };
      const int ntot = nch << (nXr - mX);                      // chunks of the patient
      QT rp[2], rq[2];
      auto fetch = [&](int cidx) {
        const uint32_t sxh = (uint32_t)(cidx >> lgnch);
        const int ch = cidx & (nch - 1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const long long src = piece_src(tid + WROWS * j, sxh, ch);
          rp[j] = *reinterpret_cast<const QT*>(ps + src);
          rq[j] = *reinterpret_cast<const QT*>(qs + src);
        }
      };
      __syncthreads();                                         // phase R is done with the staged arrays
      fetch(0);
      for (int cidx = 0; cidx < ntot; ++cidx) {
        T* pc = lds + (size_t)(2 * (cidx & 1)) * CHE;
        T* qc = pc + CHE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int dst = piece_dst(tid + WROWS * j);
          *reinterpret_cast<QT*>(pc + dst) = rp[j];
          *reinterpret_cast<QT*>(qc + dst) = rq[j];
        }
        if (cidx + 1 < ntot) fetch(cidx + 1);
        __syncthreads();
        if (mX > 0 && cidx > 0) xfinish(cidx - 1);             // (its partials were written before this barrier)
#pragma unroll JU
        for (int j = 0; j < 2; ++j) {                          // (fp32 rolled: unrolled, it spills)
          const int r = r0 + j * rstep;
          const T* prow = pc + ((size_t)r << kC);
          const T* qrow = qc + ((size_t)r << kC);
          const QT pv = *reinterpret_cast<const QT*>(prow + cp * QE);
          const QT qv = *reinterpret_cast<const QT*>(qrow + cp * QE);
#pragma unroll
          for (int e = 0; e < QE; ++e) ac[e][0] -= pv[e] * qv[e];
#pragma unroll
          for (int b = 0; b < LGQ; ++b)
#pragma unroll
            for (int e = 0; e < QE; ++e)
              if (!((e >> b) & 1)) ac[e][1 + b] += pv[e] * qv[e | (1 << b)];
#pragma unroll
          for (int b = LGQ; b < KC; ++b) {
            if (b < kC) {
              // (a column that has bit b never writes this slot: the sum it collects here is dropped, no select)
              const QT nq = *reinterpret_cast<const QT*>(qrow + (cp | (1 << (b - LGQ))) * QE);
#pragma unroll
              for (int e = 0; e < QE; ++e) ac[e][1 + b] += pv[e] * nq[e];
            }
          }
          // external row bits l < mX: the row's neighbour S | l is LDS row r | RCH << l (a row that has bit l computes a
          // sum that is dropped); every lane takes part in the segment sums
#pragma unroll 1
          for (int l = 0; l < mX; ++l) {                       // (uniform; rolled: the accumulators above fill the registers)
            const QT nq = *reinterpret_cast<const QT*>(qc + ((size_t)(r | (RCH << l)) << kC) + cp * QE);
            T s = pv[0] * nq[0];
#pragma unroll
            for (int e = 1; e < QE; ++e) s += pv[e] * nq[e];
            s = seg_sum(s, lgP < 6 ? lgP : 6);                 // (the last lane of a row's segment holds its sum)
            if ((cp & 63) == ((NPc - 1) & 63))
              xpart[(cidx & 1) * XP + (size_t)((l << lgRX) + r) * nW + (cp >> 6)] = s;
          }
        }
      }
      // ---- sum over the threads that share a piece, write the tables
      __syncthreads();
      if (mX > 0) xfinish(ntot - 1);
      T* red = lds;
#pragma unroll
      for (int s = 0; s <= KC; ++s) {
#pragma unroll
        for (int e = 0; e < QE; ++e) {
          if (s <= kC) {                                       // (uniform; no early exit: the accumulators keep static indices)
            red[tid] = ac[e][s];
            __syncthreads();
            if (tid < NPc) {
              T v = T(0);
              for (int g = 0; g < rstep; ++g) v += red[tid + g * NPc];
              const uint32_t Tc = (uint32_t)(tid * QE + e);
              if (s == 0 || !((Tc >> (s - 1)) & 1u)) outC[((long long)s << kC) + Tc] = v;
            }
            __syncthreads();
          }
        }
      }
    }
  }
}

}  // namespace mmhn
