// Per-patient assembly, the deterministic cohort reduction, and the small kernels at the two ends of an evaluation
// (parameter upload, packing of the cohort sums).  Reference: likelihood.py:441-512, 623-731;
// regularized_optimization.py:256-266.
#pragma once
#include "common.h"
#include "gradrows.h"

namespace mmhn {

// ------------------------------------------------------------------------------------
// per-patient assembly (likelihood.py:441-512, :623-731) and cohort reduction
// out[pat] = [ lp, G[N][N], d_dp[N], d_dm[N] ]
// ------------------------------------------------------------------------------------
template <typename T>
struct AsmArgs {
  const PatRec* pats; const Desc* dJ; const Desc* dS; const Params<T>* par;
  const T* GS; const T* GJ; long long gj_stride; const T* dots; const T* DJ; long long dj_stride; const T* bmS;
  const double* lp; int N; int with_grad;
};

// element e of patient `pat`'s row
template <typename T>
__device__ __forceinline__ double assemble_elem(const AsmArgs<T>& a, const PatRec& pr, int pat, int e) {
  const int N = a.N, n = N - 1;
  if (pr.kind == 4) {                              // _grad_prim_obs_az, likelihood.py:464-478
    const Params<T>& P0 = a.par[PS_THETA];
    const int q = e - 1;
    const bool diag = a.with_grad && q >= 0 && q < N * N && q / N == q % N;
    if (e != 0 && !diag) return 0.0;
    double s = 0;
    for (int i = 0; i < N; ++i) s += (double)P0.th[i][i];
    return e == 0 ? -log1p(s) : -(double)P0.th[q / N][q / N] / (1.0 + s);
  }
  if (e == 0) return a.lp[pat];
  if (!a.with_grad) return 0.0;
  if (e < 1 + N * N) {                             // theta gradient
    const int q = e - 1, i = q / N, j = q % N;
    double g = 0;
    if (pr.kind == 5 && pr.s[0] < 0 && i == j) {   // empty genotype of unknown status: r0 * (the row of kind 4); the solved
      const Params<T>& P0 = a.par[PS_THETA];       // part's row below carries r1 already (its adjoint seed is 1 / (p0 + p1))
      double s = 0;
      for (int t = 0; t < N; ++t) s += (double)P0.th[t][t];
      g = -exp(-log1p(s) - a.lp[pat]) * (double)P0.th[i][i] / (1.0 + s);
    }
    for (int part = 0; part < 2; ++part)
      if (pr.s[part] >= 0) {
        const bool prim_space = a.dS[pr.s[part]].pset == PS_PRIM;
        if (!(prim_space && j == n && i < n)) g += (double)a.GS[(long long)pr.s[part] * N * N + q];
      }
    if (pr.j >= 0)
      for (int kd = 0; kd < 3; ++kd) g += (double)a.GJ[kd * a.gj_stride + (long long)pr.j * N * N + q];
    return g;
  }
  // observation-rate gradients
  const int r0 = e - 1 - N * N, i = r0 % N;
  double gp = 0, gm = 0;
  for (int part = 0; part < 2; ++part) {
    if (pr.s[part] < 0) continue;
    const Desc& ds = a.dS[pr.s[part]];
    const T* g = a.GS + (long long)pr.s[part] * N * N;
    double dd = (double)g[i * N + i];              // d_diag[i] = -sum_{r != i} val[r, i], vanilla.py:392
#pragma unroll 7
    for (int r = 0; r < N; ++r) dd -= (double)g[r * N + i];
    if (pr.kind == 3) {
      const Desc& dj = a.dJ[pr.j];
      const double dot = (double)a.dots[2 * pat + part];
      if (part == 0) { gm += dd; if (i == n || dj.bitP[i] >= 0) gp += dot; }
      else           { gp += dd; if (i == n || dj.bitM[i] >= 0) gm += dot; }
    } else if (pr.kind == 2) {                     // _grad_met_obs, likelihood.py:481-512
      const T* bm = a.bmS + (long long)pr.s[0] * 64;
      const int b = ds.bitP[i];
      if (b >= 0) {
        if (b != ds.seedbit) gp -= (double)bm[b];
        gm += 1.0 - (double)bm[32 + b];
      }
    } else {
      gp += dd;                                    // _grad_prim_obs, likelihood.py:441-461
    }
  }
  if (pr.kind == 3) {                              // minus x_partial_D_y(q_J, pi), likelihood.py:536,694-695
    const long long o = (long long)pr.j * N + i;
    gp -= (double)a.DJ[GK_P * a.dj_stride + o] + (double)a.DJ[GK_E * a.dj_stride + o];
    gm -= (double)a.DJ[GK_M * a.dj_stride + o];
  }
  return r0 < N ? gp : gm;
}

// rows of all patients (mmhn_patient_grads)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_finalize(AsmArgs<T> a, double* out) {
  const PatRec pr = a.pats[blockIdx.x];
  const int stride = 1 + a.N * a.N + 2 * a.N;
  double* o = out + (long long)blockIdx.x * stride;
  for (int e = threadIdx.x; e < (a.with_grad ? stride : 1); e += BLOCK) o[e] = assemble_elem(a, pr, (int)blockIdx.x, e);
}

// cohort sums, stage 1: thread = element e (coalesced over the rows), workgroup (blockIdx.y) = a chunk of `per`
// consecutive patients added in index order; part[chunk][cls][e], cls 0: type != 0 (EM), 1: type 0 (NM)
constexpr int RED_MAX_CHUNKS = 128;
__host__ __device__ inline int red_per(int npat) { return max(32, (npat + RED_MAX_CHUNKS - 1) / RED_MAX_CHUNKS); }
__global__ __launch_bounds__(BLOCK) void k_reduce_rows(const PatRec* __restrict__ pats, int npat, int per,
                                                       const double* __restrict__ out, int stride, int nelem,
                                                       double* __restrict__ part) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= nelem) return;
  const int i0 = blockIdx.y * per, i1 = min(npat, i0 + per);
  double acc0 = 0, acc1 = 0;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) {
    const int kd = pats[i].kind;
    const double v = out[(long long)i * stride + e];
    if (kd == 0 || kd >= 4) acc1 += v; else acc0 += v;    // (4, 5: the closed-form row and the rows of unknown status)
  }
  part[((long long)blockIdx.y * 2 + 0) * stride + e] = acc0;
  part[((long long)blockIdx.y * 2 + 1) * stride + e] = acc1;
}

// k_reduce_rows with one weight per patient of the batch (mmhn_set_row_weights; wrow in BATCH order, as pats): the same rows
// in the same order, chunks and part[] layout, every addend w * v.  A row of weight 0 is selected out, not multiplied (its
// values may be anything, inf and NaN included: the row is absent).  The weight is uniform over the workgroup: a scalar load.
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_w(const PatRec* __restrict__ pats, int npat, int per,
                                                         const double* __restrict__ out, int stride, int nelem,
                                                         const double* __restrict__ wrow, double* __restrict__ part) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e >= nelem) return;
  const int i0 = blockIdx.y * per, i1 = min(npat, i0 + per);
  double acc0 = 0, acc1 = 0;
#pragma unroll 8
  for (int i = i0; i < i1; ++i) {
    const int kd = pats[i].kind;
    const double w = wrow[i];
    const double v = out[(long long)i * stride + e];
    const double a = w == 0.0 ? 0.0 : w * v;
    if (kd == 0 || kd >= 4) acc1 += a; else acc0 += a;
  }
  part[((long long)blockIdx.y * 2 + 0) * stride + e] = acc0;
  part[((long long)blockIdx.y * 2 + 1) * stride + e] = acc1;
}

// sums[cls][e] += the chunk sums in chunk order
__global__ __launch_bounds__(BLOCK) void k_reduce_parts(const double* __restrict__ part, int stride, int nelem, int nchunk,
                                                        double* sums) {
  const int e = blockIdx.x * BLOCK + threadIdx.x, cls = blockIdx.y;
  if (e >= nelem) return;
  double acc = 0;
#pragma unroll 8
  for (int c = 0; c < nchunk; ++c) acc += part[((long long)c * 2 + cls) * stride + e];
  sums[cls * stride + e] += acc;
}

// sums[2][stride] (EM, NM rows of k_reduce_parts) -> the buffer layout of mmhn_cohort_sums (include/metmhn_amd.h)
__global__ void k_pack_sums(const double* __restrict__ sums, int N, double n_em, double n_pat, double* __restrict__ o) {
  const int st = 1 + N * N + 2 * N, NN = N * N;
  const double* em = sums;
  const double* nm = sums + st;
  const int total = 4 + 2 * NN + 3 * N;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    double v;
    if (e == 0) v = em[0];
    else if (e == 1) v = nm[0];
    else if (e == 2) v = n_em;
    else if (e == 3) v = n_pat;
    else {
      int q = e - 4;
      if (q < NN) v = em[1 + q];
      else if ((q -= NN) < NN) v = nm[1 + q];
      else if ((q -= NN) < N) v = em[1 + NN + q];
      else if ((q -= N) < N) v = nm[1 + NN + q];
      else v = em[1 + NN + N + (q - N)];
    }
    o[e] = v;
  }
}

// sums[2][stride] -> the pre-combined buffer of mmhn_cohort_wsums: [w s_EM + s_NM, w G_EM + G_NM, w p_EM + p_NM, w m_EM]
// (regularized_optimization.py:256-266 without the division by n_full): 1 + N^2 + 2 N doubles, the all-reduce
// payload of SURVEY 8e - the weight w only needs the GLOBAL counts, which every rank knows when the cohort is set
__global__ void k_pack_wsums(const double* __restrict__ sums, int N, double w, double* __restrict__ o, double flag) {
  const int st = 1 + N * N + 2 * N, NN = N * N;
  if (blockIdx.x == 0 && threadIdx.x == 0) o[st] = flag;              // (mmhn_set_reduce_flag: rides in the same all-reduce)
  const double* em = sums;
  const double* nm = sums + st;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < st; e += gridDim.x * blockDim.x)
    o[e] = e < 1 + NN + N ? w * em[e] + nm[e] : w * em[e];          // (d_d_m has no NM part, :266)
}

// host <-> device traffic of an evaluation without the copy engine: the parameters are read from, and the result is
// written to, pinned host memory by kernels of the evaluation's own queue.  (A hipMemcpyAsync in front of the first
// launch costs the hand-over between the copy engine and the compute queue - on a 0.4 ms evaluation of a small cohort
// ~60 us passed between the 27 KB upload and the first kernel - and the download the same at the other end.)
__global__ void k_copy_words(const uint4* __restrict__ src, uint4* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// ... and the head of an evaluation in ONE launch: the parameter upload, the cleared cohort sums and the cleared gradient
// work arrays of the first batch (three launches otherwise, each a few us of queue latency on a short evaluation)
__global__ void k_begin_eval(const uint4* __restrict__ src, uint4* __restrict__ dst, int n, double* __restrict__ sums, int nsums,
                             uint4* __restrict__ z, long long nz) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  if (i0 < n) dst[i0] = src[i0];
  if (i0 < nsums) sums[i0] = 0.0;
  for (long long i = i0; i < nz; i += step) z[i] = uint4{0u, 0u, 0u, 0u};
}

// k_reduce_parts of the LAST batch and the packing in one launch: thread e adds the chunk sums of both classes in chunk
// order (as k_reduce_parts does), keeps sums[] current and writes its entries of the packed buffer
// (mode 1: k_pack_sums layout, a = n_em, b = n_pat; mode 2: k_pack_wsums, a = w)
__global__ __launch_bounds__(BLOCK) void k_reduce_parts_pack(const double* __restrict__ part, int stride, int nelem, int nchunk,
                                                             double* sums, int mode, int N, double a, double b,
                                                             double* __restrict__ o) {
  const int e = blockIdx.x * BLOCK + threadIdx.x;
  if (e == 0 && mode == 2) o[stride] = b;                             // (mode 2: b = the reduce flag, behind the buffer)
  if (e >= stride) return;
  double em = sums[e], nm = sums[stride + e];
  if (e < nelem) {
    double acc0 = 0, acc1 = 0;
#pragma unroll 8
    for (int c = 0; c < nchunk; ++c) {
      acc0 += part[((long long)c * 2 + 0) * stride + e];
      acc1 += part[((long long)c * 2 + 1) * stride + e];
    }
    em += acc0; nm += acc1;
    sums[e] = em; sums[stride + e] = nm;
  }
  const int NN = N * N;
  if (mode == 2) { o[e] = e < 1 + NN + N ? a * em + nm : a * em; return; }
  if (e == 0) { o[0] = em; o[1] = nm; o[2] = a; o[3] = b; }
  else if (e < 1 + NN) { o[4 + (e - 1)] = em; o[4 + NN + (e - 1)] = nm; }
  else if (e < 1 + NN + N) { o[4 + 2 * NN + (e - 1 - NN)] = em; o[4 + 2 * NN + N + (e - 1 - NN)] = nm; }
  else o[4 + 2 * NN + 2 * N + (e - 1 - NN - N)] = em;
}

}  // namespace mmhn
