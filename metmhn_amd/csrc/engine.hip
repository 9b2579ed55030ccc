// Host side of the metMHN engine: the engine's state, its kernel launches and the cohort evaluation.
// One engine = one GPU; one main lane (host.h: Lane - a HIP stream with its cooperative flag
// set and its fork / join events) and three side lanes that an evaluation forks off it.
// The rest of the host side lives in headers of this one translation unit: plan.h (the cohort planner, host-only:
// batches, routes, work lists, offsets), host.h (errors, device arrays, lanes, the kernel timer, MMHN_* knob readers), comm.h (RCCL),
// tsolve_host.h (the book-keeping of the cooperative launches), capi.h (the C ABI of include/metmhn_amd.h, included last),
// rowmix_host.h (row weights and row groups: their checks, device copies and the launches of the group kernels),
// prims.h / orders_host.h / orderpost_host.h (the batching of the order-posterior entry points, opr_rows) /
// orderprec_host.h / orderpos_host.h / ordertime_host.h / ordersnap_host.h / ordersample_host.h / forecast_host.h / lattice_host.h / landscape_host.h / genodist_host.h / metdist_host.h / partner_host.h / cross_host.h / sampler_host.h / bench.h (what is not the cohort evaluation).
//
// Pipeline of one evaluation (reference call graph: regularized_optimization.py:163-267 ->
// likelihood.py:_g_coupled_*, _grad_prim_obs, _grad_met_obs), run batch by batch with every
// patient of the batch in flight at once:
//   1  lidg_J = 1/(D_p + D_m - diag Q)                       k_diag(KD_LIDG)
//   2  pi    = (D - Q)^-1 e_0          k+1 fused Jacobi sweeps  k_sweep<false>
//   3  v     = D_obs * pi[compatible]  -> marginal right-hand sides  k_gather_marg
//   4  single-tumour spaces (marginals of paired patients and the unpaired patients):
//      lidg_S, forward solve, scores -> adjoint seeds 1/score, adjoint solve,
//      flow gradient                  k_diag, k_sweep, k_seeds, k_sweep<true>, k_grad_rows
//   5  rhs_J = D_obs * scatter(q_S), q_J = (D - Q)^-T rhs_J  k_scatter_marg, k_sweep<true>
//   6  joint gradient: class marginals, eq block, flow rows, observation-rate marginals
//                                      k_class_marg, k_eq_flows, k_grad_rows, k_bit_marg
//   7  per-patient assembly and deterministic cohort reduction  k_finalize, k_reduce_rows (k_reduce_rows_w with row weights;
//      with row groups k_mix_gather, k_group_lse, k_mix_weights, k_reduce_rows_mix - rowmix.h), k_reduce_parts
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/metmhn_amd.h"
#include "host.h"
#include "comm.h"
#include "plan.h"
#include "tsolve_host.h"
#include "sampler.h"
#include "rowmix.h"

namespace mmhn {

static thread_local std::string g_err;

// ---- device copies of a batch's plan (plan.h): one array per non-empty host list of the same name, filled by
// Engine::upload.  An empty host list leaves its array null.
struct CListDev {
  DevArr<CItem> items;
  DevArr<int> deps;
};
struct StagedDev {
  DevArr<int> pats, paired, probs;
  DevArr<int2> map, lmap, grc;
  CListDev cl[2];
};
struct BatchDev {
  DevArr<PatRec> pats;
  DevArr<Desc> dJ, dS;
  DevArr<int2> mapJ, mapS, lmapJ, mapX, grcJ, lmapT;
  DevArr<int> sp_list[3][SP_NCLASS], paired, olist, ptoff;
  DevArr<uint32_t> ptiles;
  DevArr<WDesc> wd;
  DevArr<WChain> wchains;
  DevArr<int4> pcl;
  DevArr<double> wrow;          // mmhn_set_row_weights: the weight of every patient of the batch, in batch order (null: no weights)
  CListDev clJ[2];
  StagedDev stg[2];
};

// every MMHN_* environment knob, read once when an engine is created (the planner's are PlanCfg's: plan.h)
struct Config {
  PlanCfg plan;
  bool zero_copy = true;        // MMHN_ZEROCOPY=0: hipMemcpyAsync up and down instead
  bool poison = false;          // MMHN_POISON=1: NaN-fill the solution buffers of per-patient batches before each evaluation
                                // and the result buffers of every api_* path (poison_fill)
  bool force_timing = false;    // MMHN_TIME_KERNELS=1: HIP events around the solve / class-marginal launches of every batch (bench
                                // breakdowns of small cohorts; an event pair costs the host ~10 us)
  bool coop_fault = false;      // MMHN_COOP_FAULT=1 (tests): the first tile of every cooperative launch never raises its flag
  int coop_wgs = 0;             // MMHN_COOP_WGS: workgroups of a cooperative launch (default: one per CU - with two the launch holds every
                                // wave slot of the chip and the side streams' kernels wait for its end: 1.65 against 1.47 ms on the 28-event LUAD cohort)
  bool coop = true;             // MMHN_COOP=0: tile solves as one launch per level (k_tsolve) instead of one cooperative launch
  long long sim_chunk = 1ll << 26;   // MMHN_SIM_CHUNK: samples per launch of mmhn_simulate_summary / mmhn_simulate_pairs
  int stream_blocks = 256 * 8;  // MMHN_STREAM_BLOCKS: workgroups of mmhn_bench_stream's kernel
  bool trace_host = false;      // MMHN_TRACE_HOST: print the host time to issue an evaluation against its total (diagnostic)
  Config() {
    plan.use_jacobi = env_is("MMHN_SOLVER", "jacobi");
    plan.psolve_min = (int)env_int("MMHN_PSOLVE_MIN", plan.psolve_min);
    plan.wsolve_min = (int)env_int("MMHN_WSOLVE_MIN", env_set("MMHN_PSOLVE_MIN") ? plan.psolve_min : plan.wsolve_min);
    plan.wsolve_mode = (int)env_int("MMHN_WSOLVE", plan.wsolve_mode);
    plan.wsolve_wgs = (int)env_int("MMHN_WSOLVE_WGS", plan.wsolve_wgs);
    plan.prep_split_max = (int)env_int("MMHN_PREP_SPLIT", plan.prep_split_max);
    plan.pcl_per = std::max(1, (int)env_int("MMHN_PCL_PER", plan.pcl_per));
    plan.small_path = env_flag("MMHN_SMALL", plan.small_path);
    zero_copy = env_flag("MMHN_ZEROCOPY", zero_copy);
    poison = env_flag("MMHN_POISON", poison);
    force_timing = env_flag("MMHN_TIME_KERNELS", force_timing);
    coop_fault = env_flag("MMHN_COOP_FAULT", coop_fault);
    coop_wgs = (int)env_int("MMHN_COOP_WGS", coop_wgs);
    coop = env_flag("MMHN_COOP", coop);
    sim_chunk = std::max(1ll, env_int("MMHN_SIM_CHUNK", sim_chunk));
    stream_blocks = (int)env_int("MMHN_STREAM_BLOCKS", stream_blocks);
    trace_host = env_set("MMHN_TRACE_HOST");
  }
};

// what of an engine does not depend on its dtype: the ABI reads it without a dispatch (capi.h)
struct EngineBase {
  virtual ~EngineBase() = default;
  int dtype = 0;
  int device = 0;
  hipStream_t stream = nullptr;       // the main lane's (Engine::main.s): set when the engine is created, never reassigned
  Config cfg;
  int n = 0, N = 0;
  // ---- cohort: its shape
  long long n_pat = 0;
  int n_cols = 0;
  long long n_unknown = 0;            // rows of dat type 4
  // the three counts of the objective: sum of w [seeding = 1], sum of w, sum of w [type 4], taken on the host in row order -
  // plain: w = 1 (the integer counts), weighted: the row weights, grouped: the weights of the row groups
  struct Counts { double em = 0, pat = 0, unknown = 0; } plain, weighted, grouped;
  // ---- row weights (mmhn_set_row_weights, rowmix_host.h): by cohort row, empty = none
  std::vector<double> row_w;
  // ---- row groups (mmhn_set_row_groups, rowmix.h, rowmix_host.h): the group lists and weights as given (grp_ptr empty = none)
  std::vector<long long> grp_ptr;
  std::vector<int> grp_rows;
  std::vector<double> grp_w;
  double reduce_flag = 0.0, reduce_flag_sum = 0.0;            // mmhn_set_reduce_flag / mmhn_get_reduce_flag
  // ---- communicator: patient shards on several GPUs, one communicator per engine, the all-reduce runs on the engine's stream
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  mmhn_counters cnt{};                // mmhn_get_counters

  int stride() const { return 1 + N * N + 2 * N; }
  int full_len() const { return 4 + 2 * N * N + 3 * N; }     // doubles of mmhn_cohort_sums
  bool mixing() const { return !grp_ptr.empty(); }
  // the counts of the objective that hold for the next evaluation (with row groups: the group-weighted ones)
  const Counts& counts() const { return mixing() ? grouped : row_w.empty() ? plain : weighted; }
  void row_weight_sums(double* out3) const { out3[0] = counts().em; out3[1] = counts().pat; out3[2] = counts().unknown; }
  void reset_counters() {                              // (what RCCL said about the communicator stays)
    const int r = cnt.comm_ranks, k = cnt.comm_rank;
    cnt = mmhn_counters{};
    cnt.comm_ranks = r; cnt.comm_rank = k;
  }
  void comm_init(const ncclUniqueId& id, int rank, int nranks) {
    REQUIRE(nranks >= 1 && rank >= 0 && rank < nranks, "comm_init: rank / n_ranks out of range");
    REQUIRE(nranks == 1 || !mixing(), "comm_init: the engine holds row groups, which need a one-rank engine (remove them first)");
    comm_destroy();
    RCCLCHECK(rccl().CommInitRank(&comm, nranks, id, rank));
    comm_rank = rank; comm_size = nranks;
    // what RCCL itself says about the communicator (mmhn_get_counters: the bench line's proof that it spans the ranks)
    int cnt_ = 0, rk_ = -1;
    RCCLCHECK(rccl().CommCount(comm, &cnt_));
    RCCLCHECK(rccl().CommUserRank(comm, &rk_));
    if (cnt_ != nranks || rk_ != rank) {
      comm_destroy();
      throw Fail{"comm_init: RCCL reports " + std::to_string(cnt_) + " ranks / rank " + std::to_string(rk_) + ", asked for " +
                 std::to_string(nranks) + " / " + std::to_string(rank)};
    }
    cnt.comm_ranks = cnt_; cnt.comm_rank = rk_;
  }
  void comm_destroy() {
    if (comm) { (void)rccl().CommDestroy(comm); comm = nullptr; }
    comm_rank = 0; comm_size = 1;
    cnt.comm_ranks = 0; cnt.comm_rank = -1;
  }
};

template <typename T> struct Engine;
// rowmix_host.h: what the engine itself calls of it
template <typename T> void clear_row_groups(Engine<T>& E);
template <typename T> void launch_mix(Engine<T>& E, const Lane& L);

// one list of problems with its tile maps (cl / dcl: its cooperative work lists, forward / transposed, or nullptr)
template <typename T>
struct PList {
  const Desc* d; const int2* map; int ntiles; int maxk; long long vec;
  const int2* lmap; const std::vector<int>* lof; const T* tab;
  const CList* cl = nullptr;
  const CListDev* dcl = nullptr;
  int kslot = MMHN_K_OTHER_SOLVE;    // counter class of its launches
};

// kernels may need more than the default dynamic LDS window
template <typename... K>
static void raise_lds(size_t bytes, K... kernels) {
  for (const void* k : {reinterpret_cast<const void*>(kernels)...})
    HIPCHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

template <typename T>
struct Engine : EngineBase {
  using PList = mmhn::PList<T>;
  // ---- parameters
  DevArr<Params<T>> d_par;
  Params<T>* h_par = nullptr;         // pinned: the per-evaluation upload is a true async copy
  void* h_par_dev = nullptr;          // device view of it
  // popcount-ordered state permutations of every tile size (k_tsolve step B)
  DevArr<uint16_t> d_perm;
  DevArr<int> d_lvl;
  // ---- cohort: the rows, their plan (plan.h) and its device copy, one entry per batch
  std::vector<int8_t> dat;
  std::vector<Batch> batches;
  std::vector<BatchDev> dev;
  // ---- workspace (sized for the largest batch)
  DevArr<T> pi, lidgJ, qJ, rhsJ, rhsS, pS, lidgS, qS, seedS, GS, dots, bmJ, bmS, tabJ, tabS;
  DevArr<T> piM, qM;            // matrix / window path: solutions in their own layout
  // accumulators of the joint gradient that must be zero on entry - rows of the three G matrices, observation-rate rows,
  // class marginals - share one allocation, laid out per batch and cleared by ONE memset at the start of the batch.  The
  // arrays of the window-layout problems lie at the end of it, outside that memset: k_wclass writes every entry of their
  // class tables that a consumer reads, the eq-block flows every entry of their eq blocks.
  DevArr<T> zarena;
  struct View { T* p = nullptr; } GJ, DJ, Abuf;
  int pi_owner = -1, qJ_owner = -1;   // batch whose (pruned) layout the zero-initialised buffers hold
  DevArr<double> lp, out, sums, redbuf;
  DevArr<double> resp;                // [n_pat] by cohort row: P(seeded | genotype) of the rows of unknown status (dat type 4), written
                                      // where their score is formed; NaN everywhere else (filled once, when the cohort is set)
  // ---- row groups on the device (the lists and weights as given: EngineBase): the group lists, the transposed lists and the
  // per-evaluation arrays
  struct GroupsDev {
    DevArr<long long> gptr, mptr;
    DevArr<int> grows, mgrp;
    DevArr<double> gw, lpc, lpg, omega, lambda, rho;
  } gd;
  bool want_rho = false;              // mmhn_group_posteriors: k_group_lse also writes rho
  DevArr<JLink<T>> links;
  // ---- lanes (host.h): main carries the joint path; side[0], side[1] the small-space launches (small_classes), side[2] the
  // staged own-problem patients, whose cooperative launches use the second flag set
  Lane main, side[3];
  // ---- cooperative launches (tsolve_host.h)
  CoopState coop;
  bool coop_alone = false;          // set per batch: no side stream carries whole-CU work next to the joint solves (tsolve.h: WPE)
  // ---- set by cohort_sums_begin around evaluate(): the last batch's reduction also packs (k_reduce_parts_pack; done: it did)
  struct Pack { int mode = 0; double a = 0, b = 0; double* dst = nullptr; bool done = false; } pack;
  // ---- pending evaluation (cohort_sums_begin ... cohort_sums_end)
  struct Pending {
    bool on = false;
    std::chrono::steady_clock::time_point t0, issued;
    int len = 0;                        // doubles of the pending result
    bool flag = false;                  // the reduce flag rides behind them
    DevArr<double> abi_sums;            // the buffer that is all-reduced
    double* h_abi = nullptr;            // pinned landing buffer of the result download
    double* h_abi_dev = nullptr;        // device view of it
  } pending;
  // ---- timed launches (host.h), set per batch
  KernelTimer timer;

  static long long zarena_elems(long long nJ, long long asize, int N) { return up4(3 * nJ * N * N) + up4(3 * nJ * N) + up4(asize); }
  // elements of a batch's zarena that the memset clears
  static long long zclear_elems(const Batch& b, int N) { return zarena_elems((long long)b.dJ.size(), b.aclr, N); }

  Engine(int dev_id, int n_mut) {
    dtype = std::is_same<T, double>::value ? MMHN_F64 : MMHN_F32;
    device = dev_id;
    n = n_mut; N = n_mut + 1;
    cnt.comm_rank = -1;
    REQUIRE(n_mut >= 1 && n_mut < MAXN, "n_mut must be in [1, 31]");
    DevGuard guard(device);
    HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    main.s = stream;
    main.flags = 0;
    d_par.alloc(NPSET);
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&h_par), NPSET * sizeof(Params<T>), hipHostMallocDefault));
    HIPCHECK(hipHostGetDevicePointer(&h_par_dev, h_par, 0));
    static_assert(sizeof(Params<T>) % sizeof(uint4) == 0, "parameter block: whole 16-byte words");
    sums.alloc(2 * stride());
    size_t free_b = 0, total_b = 0;
    HIPCHECK(hipMemGetInfo(&free_b, &total_b));
    cfg.plan.ws_limit = (size_t)(0.7 * (double)free_b);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, device));
    cfg.plan.n_cu = std::max(1, prop.multiProcessorCount);
    {
      std::vector<uint16_t> perm((size_t)(TB + 1) << TB, 0);
      std::vector<int> lvl((size_t)(TB + 1) * (TB + 2), 0);
      for (int t = 0; t <= TB; ++t) {
        int pos = 0;
        for (int l = 0; l <= t; ++l) {
          lvl[(size_t)t * (TB + 2) + l] = pos;
          for (uint32_t x = 0; x < (1u << t); ++x)
            if (popc(x) == l) perm[((size_t)t << TB) + pos++] = (uint16_t)x;
        }
        lvl[(size_t)t * (TB + 2) + t + 1] = pos;
      }
      d_perm.alloc(perm.size());
      d_lvl.alloc(lvl.size());
      HIPCHECK(hipMemcpy(d_perm.p, perm.data(), perm.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      HIPCHECK(hipMemcpy(d_lvl.p, lvl.data(), lvl.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    raise_lds(wsolve_lds<T>(), &k_wsolve<T, false>, &k_wsolve<T, true>, &k_wsolve<T, false, WCfg<T>::NXT>, &k_wsolve<T, true, WCfg<T>::NXT>);
    raise_lds(wclass_lds<T>(), &k_wclass<T>);
    raise_lds(160 * 1024, &k_spatient2<T>, &k_spatient<T, 1024, 1>);
    raise_lds(150 * 1024,
              &k_csolve<T, false, false>, &k_csolve<T, true, false>, &k_csolve<T, false, true>, &k_csolve<T, true, true>,
              &k_csolve<T, false, false, 4>, &k_csolve<T, true, false, 4>,
              &k_psolve2<T, false, true>, &k_psolve2<T, true, true>, &k_psolve2<T, false, false>, &k_psolve2<T, true, false>,
              &k_tsolve<T, false, false>, &k_tsolve<T, true, false>, &k_tsolve<T, false, true>, &k_tsolve<T, true, true>,
              &k_kv<T, false, 1, false>, &k_kv<T, true, 1, false>, &k_kv<T, false, 1, true>, &k_kv<T, true, 1, true>,
              &k_sweep<T, false>, &k_sweep<T, true>, &k_diag<T>, &k_diag<T, 1024>,
              &k_prep<T, false>, &k_prep<T, true>, &k_prep<T, false, 1024>, &k_grad_rows<T, 1>, &k_grad_rows<T>,
              &k_pclass<T, false>, &k_pclass<T, true>, &k_class_marg<T>);
    coop.init();
    for (Lane& l : side) {
      HIPCHECK(hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking));
      HIPCHECK(hipEventCreateWithFlags(&l.ev_fork, hipEventDisableTiming));
      HIPCHECK(hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming));
    }
    side[2].flags = 1;
  }
  // runs under the DevGuard of mmhn_destroy.  The order of the releases is written out here (communicator, timing events,
  // side lanes, pinned buffers, main stream); device arrays go with their DevArr afterwards.
  ~Engine() override {
    comm_destroy();
    timer.release();
    for (Lane& l : side) {
      if (l.ev_join) (void)hipEventDestroy(l.ev_join);
      if (l.ev_fork) (void)hipEventDestroy(l.ev_fork);
      if (l.s) (void)hipStreamDestroy(l.s);
    }
    if (h_par) (void)hipHostFree(h_par);
    if (pending.h_abi) (void)hipHostFree(pending.h_abi);
    coop.release();
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }

  // ---------------------------------------------------------------- parameters
  // lt == nullptr: a zero log-theta (exp(0.0) is exactly 1.0)
  void build_params(const double* lt, const double* ldp, const double* ldm, bool upload = true) {
    REQUIRE(!pending.on, "an evaluation begun with mmhn_cohort_sums_begin has not been collected (its parameter upload may still be in flight)");
    // exp(theta_ij - d_j) = exp(theta_ij) * exp(-d_j): N^2 + 2N exponentials per evaluation instead of 3 N^2 (this runs
    // on the host before the first launch of every evaluation - 26 us of a 400 us LUAD evaluation as three full passes)
    std::vector<double> eth((size_t)N * N), enp(N, 1.0), enm(N, 1.0);
    for (int e = 0; e < N * N; ++e) eth[e] = lt ? std::exp(lt[e]) : 1.0;
    if (ldp) for (int j = 0; j < N; ++j) enp[j] = std::exp(-ldp[j]);
    if (ldm) for (int j = 0; j < N; ++j) enm[j] = std::exp(-ldm[j]);
    for (int s = 0; s < NPSET; ++s) {
      Params<T>& P = h_par[s];
      std::memset(&P, 0, sizeof(P));
      for (int i = 0; i < N; ++i) {
        for (int j = 0; j < N; ++j) {
          double v = eth[i * N + j];
          if (s == PS_PRIM && j == n && i < n) v = 1.0;             // likelihood.py:313
          if (s == PS_MET && i != j) v *= enm[j];                   // kronvec.py:18
          if (s == PS_PRIM && i != j) v *= enp[j];
          P.th[i][j] = (T)v;
        }
        P.baseP[i] = (T)eth[i * N + i];
        P.baseM[i] = i < n ? (T)(eth[i * N + i] * eth[i * N + n]) : (T)0;
        P.dp[i] = (T)(ldp ? std::exp(ldp[i]) : 1.0);
        P.dm[i] = (T)(ldm ? std::exp(ldm[i]) : 1.0);
      }
    }
    if (!upload) return;                                   // (the caller's first launch carries it: k_begin_eval)
    if (cfg.zero_copy) {
      const int nw = (int)(NPSET * sizeof(Params<T>) / sizeof(uint4));
      hipLaunchKernelGGL(k_copy_words, dim3((nw + 255) / 256), dim3(256), 0, stream, static_cast<const uint4*>(h_par_dev),
                         reinterpret_cast<uint4*>(d_par.p), nw);
      HIPCHECK(hipGetLastError());
    } else {
      HIPCHECK(hipMemcpyAsync(d_par.p, h_par, NPSET * sizeof(Params<T>), hipMemcpyHostToDevice, stream));
    }
  }

  // ---------------------------------------------------------------- launches
  size_t sweep_lds(int maxk) const { return DESC_PAD + ((size_t)(1 << TB) + 2 * (size_t)std::max(maxk, 1) * 64) * sizeof(T); }
  // joint: a workgroup per table of a problem (three class tables + the rate tables, k_prep) when the launch is short
  // enough for its length to be one workgroup's chain; large cohorts keep one workgroup per problem
  // (tables of more than 2^13 entries - k = 25 - are also cut into parts of 2^13: grid.y = 4 * parts)
  // plist (optional): the problems to prepare, nprob of them (k_prep)
  void prep(const Lane& L, const Desc* descs, int nprob, T* tab, bool joint = false, int maxkc = 0, const int* plist = nullptr) {
    if (nprob == 0) return;
    // SPLIT: a table of more than 2^9 entries is dealt over several workgroups (the launch is the head of every evaluation
    // of a short cohort; at most 32 parts: the workgroups of the shorter tables of the launch exit at once, but they are launched)
    const int parts = maxkc > 9 ? 1 << std::min(maxkc - 9, 5) : 1;
    if (joint && nprob <= cfg.plan.prep_split_max) hipLaunchKernelGGL((k_prep<T, true>), dim3(nprob, 4 * parts), dim3(BLOCK), prep_lds<T>(N), L.s, descs, d_par.p, tab, plist);
    else if (nprob >= 256) hipLaunchKernelGGL((k_prep<T, false, 1024>), dim3(nprob), dim3(1024), prep_lds<T>(N), L.s, descs, d_par.p, tab, plist);
    else hipLaunchKernelGGL((k_prep<T, false>), dim3(nprob), dim3(BLOCK), prep_lds<T>(N), L.s, descs, d_par.p, tab, plist);
    HIPCHECK(hipGetLastError());
  }

  void launch_sweep(const Lane& L, bool tr, const Desc* descs, const int2* map, int ntiles, int maxk, const T* p, T* y,
                    const T* lidg, const T* rhs, int rhs_mode, const T* scal, double alg_bytes, const T* tab) {
    if (ntiles == 0) return;
    const size_t lds = sweep_lds(maxk);
    auto launch = [&]() {
      with_flags([&](auto tr_) {
        hipLaunchKernelGGL((k_sweep<T, tr_()>), dim3(ntiles), dim3(KSB), lds, L.s, descs, map, d_par.p, p, y,
                           lidg, rhs, rhs_mode, scal, std::max(maxk, 1), tab);
      }, tr);
    };
    if (alg_bytes > 0) { timer.timed(L, MMHN_K_OTHER_SOLVE, alg_bytes, launch); return; }   // (a launch without algorithmic bytes is never timed)
    launch();
    HIPCHECK(hipGetLastError());
  }
  // plain product on full tiles of multi-tile spaces (k_kv); hxt from k_hx for the same map
  // zmap: see k_kv; lidg / rhs: fused Jacobi step y = lidg * (Q_off p + rhs) over the same tile list
  void launch_kv(const Lane& L, bool tr, const Desc* descs, const int2* map, int ntiles, int maxk, const T* p, T* y, const T* tab, const T* hxt,
                 const int* zmap = nullptr, const T* lidg = nullptr, const T* rhs = nullptr) {
    if (ntiles == 0) return;
    const size_t lds = DESC_PAD + ((size_t)(1 << TB) + 2 * (size_t)maxk * 64 + 32) * sizeof(T);
    with_flags([&](auto tr_, auto jac) {
      hipLaunchKernelGGL((k_kv<T, tr_(), 1, jac()>), dim3(ntiles), dim3(KSB), lds, L.s, descs, map, ntiles, p, y, tab, hxt, maxk, zmap, lidg, rhs);
    }, tr, lidg != nullptr);
    HIPCHECK(hipGetLastError());
  }

  void launch_diag(const Lane& L, const Desc* descs, const int2* map, int ntiles, const T* p, T* outp, const T* dvec, int what,
                   int pbit = -1) {
    if (ntiles == 0) return;
    const size_t lds = DESC_PAD + ((size_t)4 * N * 64 + 256) * sizeof(T);
    if (ntiles >= 256)
      hipLaunchKernelGGL((k_diag<T, 1024>), dim3(ntiles), dim3(1024), lds, L.s, descs, map, d_par.p, p, outp, dvec, what, N, pbit);
    else
      hipLaunchKernelGGL((k_diag<T>), dim3(ntiles), dim3(BLOCK), lds, L.s, descs, map, d_par.p, p, outp, dvec,
                         what, N, pbit);
    HIPCHECK(hipGetLastError());
  }
  // dj != nullptr (joint kinds): one extra row per problem with the observation-rate gradient
  // partial rows of the subset chunks are added up: G (and dj) must be zero on entry
  // kind < 0: the work list holds the three joint kinds (kind in bits 24+ of the chunk field), G matrices gstride apart
  void launch_grad_rows(const Lane& L, const Desc* descs, int nprob, int maxk, const T* A, const T* p, const T* q, T* G, int kind,
                        const DevArr<int2>& chunks, T* dj = nullptr, long long gstride = 0) {
    if (nprob == 0 || chunks.n == 0) return;
    (void)maxk;
    const int rows = N + (dj ? 1 : 0);
    if (chunks.n >= 1024) {
      // long launches: one row (wave) per workgroup - no barrier, nothing shared but the class-bit list (measured on the bench cohort,
      // rows per workgroup 1 / 2 / 4 / 8 / 12: the step minus its big kernels 4.08 / 4.12 / 4.16 / 4.45 / 4.62 ms)
      const size_t lds1 = ((size_t)192 + 32) * sizeof(T);
      hipLaunchKernelGGL((k_grad_rows<T, 1>), dim3((unsigned)chunks.n, rows), dim3(64), lds1, L.s,
                         descs, d_par.p, A, p, q, G, kind, dj, chunks.p, nprob, gstride);
      HIPCHECK(hipGetLastError());
      return;
    }
    const size_t lds = ((size_t)WAVES * 192 + WAVES * 32) * sizeof(T);
    hipLaunchKernelGGL((k_grad_rows<T>), dim3((unsigned)chunks.n, (rows + WAVES - 1) / WAVES), dim3(BLOCK), lds, L.s,
                       descs, d_par.p, A, p, q, G, kind, dj, chunks.p, nprob, gstride);
    HIPCHECK(hipGetLastError());
  }
  void zero(const Lane& L, T* p, long long count) {
    if (count > 0) HIPCHECK(hipMemsetAsync(p, 0, (size_t)count * sizeof(T), L.s));
  }
  // MMHN_POISON=1 (tests): the result buffers of the api_* paths start as NaNs, filled as soon as they are allocated and
  // before the path's own clearing, so an element that no launch (or memset) writes shows in the output
  void poison_fill(const Lane& L, T* p, long long count) {
    if (cfg.poison && count > 0) HIPCHECK(hipMemsetAsync(p, 0xFF, (size_t)count * sizeof(T), L.s));
  }

  // k_psolve2 (one workgroup per patient, all-seeded-tile launches)
  size_t psolve2_lds(int maxk) const {
    return DESC_PAD + ((size_t)(1 << TB) + (size_t)((1 << TB) / TSB) + 3 * (size_t)maxk * 64 + (size_t)maxk * maxk + maxk) * sizeof(T) + 400 * sizeof(uint32_t) + (size_t)TSB * sizeof(uint16_t);
  }
  // the joint solves of a batch, every problem on its route (Batch::route)
  void psolve(const Lane& L, bool tr, const Batch& b, T* y, int rhs_mode) {
    const int nJ = (int)b.dJ.size();
    if (nJ == 0) return;
    const BatchDev& db = dev[b.id];
    if (b.wpath) {
      // window route: the solution is written once (seeded half)
      const int nW = (int)b.wd.size();
      double bytes = 0;
      for (const WDesc& w : b.wd) bytes += 0.5 * (double)(1ll << b.dJ[w.prob].k) * sizeof(T);
      T* yw = b.wdirect ? y : (tr ? qM.p : piM.p);
      timer.timed(L, tr ? MMHN_K_PSOLVE_ADJ : MMHN_K_PSOLVE_FWD, bytes, [&]() {
        const int nch = (int)b.wchains.size();
        const dim3 g((unsigned)std::min(nch, cfg.plan.wsolve_wgs > 0 ? cfg.plan.wsolve_wgs : cfg.plan.n_cu)), bk(WROWS);
        const size_t lds = wsolve_lds<T>();
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, g, bk, lds, L.s, db.dJ.p, db.wd.p, db.wchains.p, nch, yw, tabJ.p, links.p, qS.p); };
        // (a batch whose chains all have the same number of external bits - every k = 20 cohort: 5, k = 25: 9 - runs the instantiation
        // that knows it at compile time)
        if (b.wnx == WCfg<T>::NXT) { if (tr) go(&k_wsolve<T, true, WCfg<T>::NXT>); else go(&k_wsolve<T, false, WCfg<T>::NXT>); }
        else if (tr) go(&k_wsolve<T, true>);
        else go(&k_wsolve<T, false>);
      });
      if (!b.wdirect) {
        hipLaunchKernelGGL((k_wconvert<T>), dim3(nW, 32), dim3(WROWS), 0, L.s, db.dJ.p, db.wd.p, yw, y);
        HIPCHECK(hipGetLastError());
      }
    }
    if (!b.olist.empty()) {
      // one workgroup per patient (multi-tile problems, many of them)
      const int mk = std::max(b.maxkP, 1);
      const long long spare = (80 * 1024 - 64) - (long long)psolve2_lds(mk);
      const int dl_cap = (int)std::max<long long>(0, std::min<long long>(PS_DL2, spare / (long long)sizeof(T)));
      const size_t lds = psolve2_lds(mk) + (size_t)dl_cap * sizeof(T);
      const double bytes = (double)b.ptiles.size() * (double)(1 << TB) * sizeof(T);
      const bool dlok = b.max_dl <= dl_cap;       // every patient's dP / dM tile slices fit the dl area: branch-free instantiation
      const int nold = (int)b.olist.size();
      timer.timed(L, tr ? MMHN_K_PSOLVE_ADJ : MMHN_K_PSOLVE_FWD, bytes, [&]() {
        with_flags([&](auto tr_, auto dl) {
          hipLaunchKernelGGL((k_psolve2<T, tr_(), dl()>), dim3(nold), dim3(TSB), lds, L.s, db.dJ.p, db.ptoff.p, db.ptiles.p, d_par.p, y, rhs_mode,
                             d_perm.p, mk, tabJ.p, links.p, qS.p, dl_cap, db.olist.p);
        }, tr, dlok);
      });
    }
    if (!b.lmapT.empty()) {
      // everything else: all tiles in one cooperative launch (several workgroups per patient)
      const PList LT{db.dJ.p, nullptr, (int)b.lmapT.size(), b.maxkT, 0, db.lmapT.p, &b.lofT, tabJ.p, b.clJ, db.clJ,
                     tr ? MMHN_K_CSOLVE_ADJ : MMHN_K_CSOLVE_FWD};
      solve(L, tr, LT, y, nullptr, nullptr, rhs_mode, nullptr);
    }
  }

  // (D - Q)^-1 rhs (tr: transposed) on every problem of a list.
  //   default: tile-level substitution, ONE cooperative launch over the list's work list (k_csolve); a list of one level,
  //   lists without a work list (API calls) and MMHN_COOP=0: one launch per level of tile-index popcount (k_tsolve);
  //   MMHN_SOLVER=jacobi: k+1 in-place fused Jacobi sweeps from zero (the reference's iteration).
  void solve(const Lane& L, bool tr, const PList& P, T* y, const T* lidg, const T* rhs, int rhs_mode, const T* scal) {
    if (P.ntiles == 0) return;
    if (cfg.plan.use_jacobi) {
      zero(L, y, P.vec);
      const double bytes = 4.0 * (double)P.vec * sizeof(T);   // read y, lidg, rhs; write y (B_js)
      for (int s = 0; s <= P.maxk; ++s)
        launch_sweep(L, tr, P.d, P.map, P.ntiles, P.maxk, y, y, lidg, rhs, rhs_mode, scal, bytes, P.tab);
      return;
    }
    const int nlev = (int)P.lof->size() - 1;
    const size_t lds = sweep_lds(P.maxk);
    const int mk = std::max(P.maxk, 1);
    // compulsory traffic of a tile: write y (+ read dense rhs, + read the lidg vector when there is one)
    const double per_tile = (double)((rhs_mode == 0 ? 2 : 1) + (lidg ? 1 : 0)) * (double)(1 << std::min(P.maxk, TB)) * sizeof(T);   // modes 1-3: rhs is not a 2^k vector
    if (cfg.coop && P.cl && nlev > 1) {
      const CList& cl = P.cl[tr ? 1 : 0];
      const CListDev& dcl = P.dcl[tr ? 1 : 0];
      const int nitems = (int)cl.items.size();
      REQUIRE(nitems == P.ntiles, "cooperative solve: work list and tile list differ");
      REQUIRE(L.flags >= 0, "cooperative solve: issued on a lane without a flag set");
      const CoopState::Launch cl_ = coop.begin_launch(L, nitems);
      timer.timed(L, P.kslot, per_tile * nitems, [&]() {
        const dim3 g((unsigned)std::min(nitems, cfg.coop_wgs > 0 ? cfg.coop_wgs : cfg.plan.n_cu)), bk(TSB);
        auto go = [&](auto kern) {
          hipLaunchKernelGGL(kern, g, bk, lds, L.s, P.d, dcl.items.p, dcl.deps.p, nitems, cl_.flags, cl_.epoch, coop.ctl.p, cl_.slot, coop.h_abort_dev,
                             cfg.coop_fault ? 1 : 0, y, lidg, rhs, rhs_mode, scal, d_perm.p, mk, P.tab, links.p, qS.p);
        };
        // (three of the four (lidg, coop_alone) variants exist: a list with a lidg vector never runs the 4-wave one)
        with_flags([&](auto tr_) {
          if (lidg) go(&k_csolve<T, tr_(), true>);
          else if (coop_alone) go(&k_csolve<T, tr_(), false, 4>);   // (nothing runs beside the joint solves of this batch: 93 registers)
          else go(&k_csolve<T, tr_(), false>);
        }, tr);
      });
      return;
    }
    for (int s = 0; s < nlev; ++s) {
      const int lev = tr ? nlev - 1 - s : s;
      const int beg = (*P.lof)[lev], cntl = (*P.lof)[lev + 1] - beg;
      if (cntl == 0) continue;
      timer.timed(L, P.kslot, per_tile * cntl, [&]() {
        with_flags([&](auto tr_, auto jac) {
          hipLaunchKernelGGL((k_tsolve<T, tr_(), jac()>), dim3(cntl), dim3(TSB), lds, L.s, P.d, P.lmap + beg, d_par.p, y, lidg, rhs, rhs_mode, scal,
                             d_perm.p, d_lvl.p, mk, P.tab, links.p, qS.p);
        }, tr, lidg != nullptr);
      });
    }
  }

  // ---------------------------------------------------------------- cohort
  // device copy of a batch's plan: every non-empty host list (a null array otherwise - kernels receive those pointers)
  void upload(const Batch& b, BatchDev& d) {
    auto up = [](auto& to, const auto& host) {
      if (host.empty()) return;
      to.alloc(host.size());
      HIPCHECK(hipMemcpy(to.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice));
    };
    auto up_clist = [&](CListDev& to, const CList& cl) { up(to.items, cl.items); up(to.deps, cl.deps); };
    up(d.pats, b.pats); up(d.dJ, b.dJ); up(d.dS, b.dS);
    up(d.mapJ, b.mapJ); up(d.mapS, b.mapS); up(d.lmapJ, b.lmapJ); up(d.mapX, b.mapX); up(d.grcJ, b.grcJ);
    up(d.wd, b.wd); up(d.wchains, b.wchains); up(d.olist, b.olist); up(d.ptoff, b.ptoff); up(d.ptiles, b.ptiles);
    up(d.lmapT, b.lmapT); up_clist(d.clJ[0], b.clJ[0]); up_clist(d.clJ[1], b.clJ[1]);
    up(d.pcl, b.pcl); up(d.paired, b.paired);
    for (int w = 0; w < 3; ++w) for (int c = 0; c < SP_NCLASS; ++c) up(d.sp_list[w][c], b.sp_list[w][c]);
    for (int w = 0; w < 2; ++w) {
      const Staged& g = b.stg[w];
      StagedDev& dg = d.stg[w];
      up(dg.pats, g.pats); up(dg.paired, g.paired); up(dg.probs, g.probs);
      up(dg.map, g.map); up(dg.lmap, g.lmap); up(dg.grc, g.grc);
      up_clist(dg.cl[0], g.cl[0]); up_clist(dg.cl[1], g.cl[1]);
    }
  }
  void set_cohort(const int8_t* d_, long long np, int nc) {
    REQUIRE(nc == 2 * n + 3, "dat must have 2*n_mut+3 columns");
    REQUIRE(np >= 0, "negative patient count");
    REQUIRE(!pending.on, "mmhn_set_cohort: an evaluation begun with mmhn_cohort_sums_begin has not been collected");
    dat.assign(d_, d_ + np * nc);
    n_pat = np;
    n_cols = nc;
    batches.clear();
    dev.clear();
    row_w.clear();                                          // (the weights belong to the rows they were set for)
    clear_row_groups(*this);                                // (and so do the groups)
    n_unknown = 0;
    plain = Counts{0, (double)np, 0};
    // a cohort that is refused, or whose plan cannot be brought to the device, leaves the engine without one (no patient
    // count next to an empty or half-uploaded plan)
    try {
      batches = plan_cohort<T>(cfg.plan, dat.data(), np, nc, n, plain.em);
      for (long long r = 0; r < np; ++r) n_unknown += dat[(size_t)r * nc + nc - 1] == 4;
      plain.unknown = (double)n_unknown;
      place_cohort();
    } catch (...) {
      dat.clear(); batches.clear(); dev.clear();
      n_pat = 0; n_unknown = 0;
      plain = Counts{};
      throw;
    }
  }
  // device copies of the plan and the workspace
  void place_cohort() {
    dev.resize(batches.size());
    // the workspace: sized for the largest batch
    long long mvJ = 0, mvS = 0, mtJ = 0, mtS = 0, mvM = 0;
    size_t mZ = 0, mnJ = 0, mnS = 0, mp = 0;
    for (const Batch& b : batches) {
      upload(b, dev[b.id]);
      mvJ = std::max(mvJ, b.vecJ); mvS = std::max(mvS, b.vecS);
      mZ = std::max<size_t>(mZ, (size_t)zarena_elems((long long)b.dJ.size(), b.asize, N));
      mtJ = std::max(mtJ, b.tabJ); mtS = std::max(mtS, b.tabS);
      if (b.wpath && !b.wdirect) mvM = std::max(mvM, b.vecJ);
      mnJ = std::max(mnJ, b.dJ.size()); mnS = std::max(mnS, b.dS.size()); mp = std::max(mp, b.pats.size());
    }
    pi.alloc(mvJ); qJ.alloc(mvJ);
    piM.alloc(mvM); qM.alloc(mvM);
    if (cfg.plan.use_jacobi) { lidgJ.alloc(mvJ); rhsJ.alloc(mvJ); }
    links.alloc(std::max<size_t>(mnJ, 1));
    tabJ.alloc(mtJ); tabS.alloc(mtS);
    pi_owner = qJ_owner = -1;
    rhsS.alloc(mvS); pS.alloc(mvS); lidgS.alloc(mvS); qS.alloc(mvS);
    seedS.alloc(mnS);
    GS.alloc(mnS * N * N); zarena.alloc(mZ);
    dots.alloc(2 * mp); bmJ.alloc(mnJ * 64); bmS.alloc(mnS * 64);
    resp.alloc((size_t)std::max<long long>(n_pat, 1));
    {
      const std::vector<double> nans(resp.n, std::nan(""));
      HIPCHECK(hipMemcpy(resp.p, nans.data(), resp.n * sizeof(double), hipMemcpyHostToDevice));
    }
    lp.alloc(mp); out.alloc(mp * stride()); redbuf.alloc(((mp + red_per((int)mp) - 1) / red_per((int)mp)) * 2 * (size_t)stride());
  }

  // ---------------------------------------------------------------- one evaluation
  // small-space path (small.h): every single-tumour space of the batch fits one tile -> one launch per size class does
  // stage 4, the adjoint seeds, the single-tumour gradients and the <q, rhs> dots, one workgroup (or wave) per patient.
  // which = 0: the patients that are their own problem (launched first: nothing of the joint path feeds them), 1: the
  // paired ones (after k_gather_marg).  The size classes are independent of each other.
  // Lanes: the own-problem launches go to side[0], next to the joint path on the main lane, and are joined before the
  // assembly; of the paired launches the 1024-thread class goes to side[1], the merged one stays on the main lane.
  // The point of the main lane that the side launches of which = 0 wait for is recorded ahead of time (Lane::record_fork: the
  // launches of the critical chain are issued first).  The caller joins (Lane::join).
  void small_classes(const Batch& b, int which, bool grad) {
    const BatchDev& db = dev[b.id];
    const int n0 = (int)b.sp_list[which][0].size(), n1 = (int)b.sp_list[which][1].size(), n2 = (int)b.sp_list[which][2].size();
    const int np0 = which ? (int)b.sp_list[2][0].size() : 0, np1 = which ? (int)b.sp_list[2][1].size() : 0;
    const int mk0 = spatient_class_maxk(0), mk1 = which ? b.mk1p : spatient_class_maxk(1), mk2 = spatient_class_maxk(2);
    const bool on_side = which == 0 ? (n0 + n1 + n2 > 0) : n2 > 0;
    Lane& sd = side[which];
    if (on_side) sd.begin(main);
    else sd.reset();                                          // (a fork recorded ahead of time goes unused)
#define SP_TAIL db.pats.p, db.dS.p, d_par.p, d_perm.p, d_lvl.p, db.dJ.p, db.wd.p, pi.p, links.p, pS.p, qS.p, GS.p, bmS.p, dots.p, lp.p, resp.p
    if (n2) {
      const size_t lds = (spatient_lds<T>(N, mk2) + 15) / 16 * 16;
      hipLaunchKernelGGL((k_spatient<T, 1024, 1>), dim3(n2), dim3(1024), lds, sd.s, db.sp_list[which][2].p, n2, SP_TAIL, mk2, N, grad ? 1 : 0);
      HIPCHECK(hipGetLastError());
    }
    if (n0 + n1 + np0 + np1) {
      const size_t s0 = (spatient_lds<T>(N, mk0) + 15) / 16 * 16, s1 = (spatient_lds<T>(N, mk1) + 15) / 16 * 16;
      const size_t lds = std::max(s0 * SP_PPB0, n1 + np1 ? s1 * (np1 ? 2 : 1) : 0) + 64;
      const int nblk = (n0 + SP_PPB0 - 1) / SP_PPB0 + n1 + (np0 + SP_PPB0 / 2 - 1) / (SP_PPB0 / 2) + np1;
      hipLaunchKernelGGL((k_spatient2<T>), dim3(nblk), dim3(256), lds, which == 0 ? sd.s : main.s,
                         db.sp_list[which][0].p, n0, mk0, db.sp_list[which][1].p, n1, mk1,
                         db.sp_list[2][0].p, np0, db.sp_list[2][1].p, np1, SP_TAIL, N, grad ? 1 : 0);
      HIPCHECK(hipGetLastError());
    }
#undef SP_TAIL
    if (on_side) sd.end();
  }

  // ---- the stages of an evaluation, in the order evaluate() issues them
  // The head: parameters up, cohort sums and - when it fits the same launch - the first batch's gradient work arrays
  // cleared.  Returns whether that clear was done.
  bool eval_head(const double* lt, const double* ldp, const double* ldm, bool grad) {
    const int st = stride();
    bool head_done = false;
    if (cfg.zero_copy && !batches.empty()) {
      build_params(lt, ldp, ldm, false);
      const Batch& b0 = batches.front();
      // (a large batch clears its ~GB of work arrays with the runtime's fill, which is faster at that size: +1.0 ms
      // per evaluation on the 5 000-patient bench cohort when this kernel did it)
      long long nz = grad && !b0.dJ.empty() ? zclear_elems(b0, N) * (long long)sizeof(T) / 16 : 0;
      const bool fill_here = nz <= (32ll << 20) / 16;
      if (!fill_here) nz = 0;
      const int nw = (int)(NPSET * sizeof(Params<T>) / sizeof(uint4));
      const long long need = std::max<long long>(std::max<long long>(nw, 2 * st), nz);
      const int nblk = (int)std::min<long long>((need + 255) / 256, 4096);
      hipLaunchKernelGGL(k_begin_eval, dim3(nblk), dim3(256), 0, main.s, static_cast<const uint4*>(h_par_dev),
                         reinterpret_cast<uint4*>(d_par.p), nw, sums.p, 2 * st, reinterpret_cast<uint4*>(zarena.p), nz);
      HIPCHECK(hipGetLastError());
      head_done = fill_here;
    } else {
      build_params(lt, ldp, ldm);
      HIPCHECK(hipMemsetAsync(sums.p, 0, 2 * st * sizeof(double), main.s));
    }
    if (mixing() && cfg.poison) HIPCHECK(hipMemsetAsync(gd.lpc.p, 0xFF, (size_t)n_pat * sizeof(double), main.s));
    return head_done;
  }
  // What a batch decides for all its launches, the views into zarena, and the clear of its accumulators (cleared: the
  // head of the evaluation did it)
  void batch_prepare(const Batch& b, bool grad, bool cleared) {
    const int nJ = (int)b.dJ.size();
    coop_alone = b.stg[0].empty();                          // (no second cooperative launch on a side stream next to the joint solves)
    timer.on = cfg.force_timing || b.vecJ + b.vecS >= (1ll << 26);
    GJ.p = zarena.p;
    DJ.p = GJ.p + up4(3ll * nJ * N * N);
    Abuf.p = DJ.p + up4(3ll * nJ * N);
    if (grad && nJ && !cleared) zero(main, zarena.p, zclear_elems(b, N));
    // (MMHN_POISON=1, tests: the arrays outside the memset start as NaNs - an entry that a consumer reads and no launch
    // wrote shows in the gradient)
    if (grad && nJ && cfg.poison) poison_fill(main, Abuf.p + b.aclr, b.asize - b.aclr);
  }
  // The tile solver skips dead tiles and its consumers read them: those parts of pi / q_J must hold zeros - the vectors
  // of the tile route lie behind offT and are cleared once per batch.  The window and per-patient kernels never let a
  // value of a dead tile into arithmetic (they are only ever loaded behind a per-state select): no clearing, which
  // matters when a cohort takes several batches per evaluation; MMHN_POISON=1 (tests) NaN-fills their part.
  void clear_dead_tiles(const Batch& b, bool grad) {
    if (cfg.plan.use_jacobi || b.dJ.empty()) return;
    if (pi_owner != b.id) { zero(main, pi.p + b.offT, b.vecJ - b.offT); pi_owner = b.id; }
    if (grad && qJ_owner != b.id) { zero(main, qJ.p + b.offT, b.vecJ - b.offT); qJ_owner = b.id; }
    if (cfg.poison && b.offT > 0) {
      HIPCHECK(hipMemsetAsync(pi.p, 0xFF, (size_t)b.offT * sizeof(T), main.s));
      if (grad) HIPCHECK(hipMemsetAsync(qJ.p, 0xFF, (size_t)b.offT * sizeof(T), main.s));
    }
  }
  // every joint problem of a batch as one list (Jacobi solver only)
  PList joint_list(const Batch& b) const {
    const BatchDev& db = dev[b.id];
    return PList{db.dJ.p, db.mapJ.p, (int)b.mapJ.size(), b.maxkJ, b.vecJ, db.lmapJ.p, &b.lofJ, tabJ.p};
  }
  // 1-2 joint forward
  void joint_forward(const Batch& b) {
    const BatchDev& db = dev[b.id];
    if (cfg.plan.use_jacobi) {
      launch_diag(main, db.dJ.p, db.mapJ.p, (int)b.mapJ.size(), nullptr, lidgJ.p, nullptr, KD_LIDG);
      solve(main, false, joint_list(b), pi.p, lidgJ.p, nullptr, 2, nullptr);
    } else {
      psolve(main, false, b, pi.p, 2);
    }
  }
  // 3-4 the staged kernels of one group of patients (Batch::stg[w]; 0: own-problem patients, 1: paired rows): forward part
  // (tables, right-hand sides, 1/diag, forward solve, scores and adjoint seeds) and gradient part (adjoint solve, gradient
  // rows, observation-rate marginals)
  // (Jacobi / MMHN_SMALL=0: the group is every single-tumour problem, so that vec = every single-tumour vector)
  PList staged_list(const Batch& b, int w) const {
    const Staged& g = b.stg[w];
    const StagedDev& dg = dev[b.id].stg[w];
    return PList{dev[b.id].dS.p, dg.map.p, (int)g.map.size(), g.maxk, b.vecS, dg.lmap.p, &g.lof, tabS.p, g.cl, dg.cl};
  }
  void staged_fwd(const Lane& L, const Batch& b, int w, bool grad) {
    const BatchDev& db = dev[b.id];
    const Staged& g = b.stg[w];
    const StagedDev& dg = db.stg[w];
    if (g.empty()) return;
    const int nG = (int)g.pats.size(), tG = (int)g.map.size();
    // (the group's accumulators cleared, the e_0 right-hand sides written: before anything of the group runs)
    hipLaunchKernelGGL((k_staged_init<T>), dim3(nG), dim3(BLOCK), 0, L.s, db.pats.p, db.dS.p, rhsS.p, GS.p, bmS.p, N, grad ? 1 : 0, dg.pats.p);
    HIPCHECK(hipGetLastError());
    prep(L, db.dS.p, (int)g.probs.size(), tabS.p, false, 0, dg.probs.p);
    // marginal right-hand sides (the small-space kernels read pi themselves and write the links)
    if (!g.paired.empty()) {
      hipLaunchKernelGGL((k_gather_marg<T>), dim3((unsigned)g.paired.size(), 2, g.maxk > 10 ? 8 : 1), dim3(BLOCK), 0, L.s,
                         db.pats.p, db.dJ.p, db.dS.p, d_par.p, pi.p, rhsS.p, links.p, dg.paired.p, db.wd.p);
      HIPCHECK(hipGetLastError());
    }
    launch_diag(L, db.dS.p, dg.map.p, tG, nullptr, lidgS.p, nullptr, KD_LIDG);
    solve(L, false, staged_list(b, w), pS.p, lidgS.p, rhsS.p, 0, nullptr);
    hipLaunchKernelGGL((k_seeds<T>), dim3((nG + 255) / 256), dim3(256), 0, L.s, db.pats.p, nG, db.dS.p,
                       d_par.p, pS.p, seedS.p, lp.p, resp.p, N, dg.pats.p);
    HIPCHECK(hipGetLastError());
  }
  void staged_adj(const Lane& L, const Batch& b, int w) {
    const BatchDev& db = dev[b.id];
    const Staged& g = b.stg[w];
    const StagedDev& dg = db.stg[w];
    if (g.empty()) return;
    solve(L, true, staged_list(b, w), qS.p, lidgS.p, nullptr, 1, seedS.p);
    launch_grad_rows(L, db.dS.p, (int)g.probs.size(), g.maxk, nullptr, pS.p, qS.p, GS.p, GK_S, dg.grc);
    if (g.kind2) {
      hipLaunchKernelGGL((k_bit_marg<T>), dim3((unsigned)g.map.size()), dim3(BLOCK), 0, L.s, db.dS.p, dg.map.p, d_par.p, pS.p, qS.p, bmS.p);
      HIPCHECK(hipGetLastError());
    }
  }
  // 5 joint adjoint: right-hand side D_obs * scatter(q_S) formed on the fly inside the solve
  void joint_adjoint(const Batch& b) {
    const BatchDev& db = dev[b.id];
    if (cfg.plan.use_jacobi) zero(main, rhsJ.p, b.vecJ);
    for (int part = 0; part < 2 && !b.stg[1].paired.empty(); ++part) {
      if (b.stg[1].paired.size() >= 256)
        hipLaunchKernelGGL((k_scatter_marg<T, 1024>), dim3((unsigned)b.stg[1].paired.size()), dim3(1024), 0, main.s, db.pats.p, db.dJ.p,
                           db.dS.p, d_par.p, qS.p, rhsS.p, cfg.plan.use_jacobi ? rhsJ.p : nullptr, dots.p, part, db.stg[1].paired.p);
      else
        hipLaunchKernelGGL((k_scatter_marg<T>), dim3((unsigned)b.stg[1].paired.size()), dim3(BLOCK), 0, main.s, db.pats.p, db.dJ.p,
                           db.dS.p, d_par.p, qS.p, rhsS.p, cfg.plan.use_jacobi ? rhsJ.p : nullptr, dots.p, part, db.stg[1].paired.p);
      HIPCHECK(hipGetLastError());
    }
    if (cfg.plan.use_jacobi) solve(main, true, joint_list(b), qJ.p, lidgJ.p, rhsJ.p, 0, nullptr);
    else psolve(main, true, b, qJ.p, 3);
  }
  // 6 joint gradient (accumulators cleared at the start of the batch)
  void joint_gradient(const Batch& b) {
    const BatchDev& db = dev[b.id];
    const int nJ = (int)b.dJ.size();
    if (!cfg.plan.use_jacobi) {
      // algorithmic bytes: the seeded halves of pi and q_J read once
      const double mbytes = (double)b.vecJ * sizeof(T);
      timer.timed(main, MMHN_K_PCLASS, mbytes, [&]() {
        if (b.wdirect) {                                                  // window-layout problems: both classes, two reads
          const int nW = (int)b.wd.size();
          hipLaunchKernelGGL((k_wclass<T>), dim3((unsigned)std::min(nW, cfg.plan.n_cu)), dim3(WROWS), wclass_lds<T>(), main.s, db.dJ.p, db.wd.p, nW, pi.p, qJ.p, Abuf.p);
        }
        // the problems in index order: work items (class passes of a problem cut into ranges + its eq block's flows)
        // on short launches, one workgroup per problem on long ones
        if (!b.pcl.empty())
          hipLaunchKernelGGL((k_pclass<T, true>), dim3((unsigned)b.pcl.size()), dim3(CMB), PC_LDS_ELEMS * sizeof(T), main.s, db.dJ.p, db.wd.p, pi.p, qJ.p, Abuf.p, db.pcl.p);
        else if ((int)b.wd.size() < nJ || !b.wdirect)
          hipLaunchKernelGGL((k_pclass<T, false>), dim3(nJ), dim3(CMB), PC_LDS_ELEMS * sizeof(T), main.s, db.dJ.p, db.wd.p, pi.p, qJ.p, Abuf.p);
      });
      if (!b.mapX.empty())
        hipLaunchKernelGGL((k_class_marg<T>), dim3((unsigned)b.mapX.size()), dim3(CMB), 2 * sizeof(T) << TB, main.s,
                           db.dJ.p, db.mapX.p, pi.p, qJ.p, Abuf.p);
    } else {
      hipLaunchKernelGGL((k_class_marg<T>), dim3((unsigned)b.mapJ.size()), dim3(CMB), 2 * sizeof(T) << TB, main.s, db.dJ.p,
                         db.mapJ.p, pi.p, qJ.p, Abuf.p);
    }
    HIPCHECK(hipGetLastError());
    // (its own launch: folded into the workgroups of k_pclass it cost more than the launch - k_pclass 20.5 -> 21.9 ms
    // on the bench cohort, the LUAD evaluation +25 us; short launches run it as work items of k_pclass)
    if (b.pcl.empty()) {
      hipLaunchKernelGGL((k_eq_flows<T>), dim3(nJ), dim3(BLOCK), 0, main.s, db.dJ.p, db.wd.p, pi.p, qJ.p, Abuf.p);
      HIPCHECK(hipGetLastError());
    }
    launch_grad_rows(main, db.dJ.p, nJ, b.maxkcJ, Abuf.p, nullptr, nullptr, GJ.p, -1, db.grcJ, DJ.p, (long long)nJ * N * N);
  }
  // 7 per-patient assembly; gather: the rows' lp into lpc for the row groups (first sweep)
  void finalize_batch(const Batch& b, bool grad, bool gather) {
    const BatchDev& db = dev[b.id];
    const int npat = (int)b.pats.size(), nJ = (int)b.dJ.size();
    const AsmArgs<T> aa{db.pats.p, db.dJ.p, db.dS.p, d_par.p, GS.p, GJ.p, (long long)nJ * N * N, dots.p, DJ.p, (long long)nJ * N, bmS.p, lp.p, N,
                        grad ? 1 : 0};
    hipLaunchKernelGGL((k_finalize<T>), dim3(npat), dim3(BLOCK), 0, main.s, aa, out.p);
    HIPCHECK(hipGetLastError());
    if (gather) {
      hipLaunchKernelGGL(k_mix_gather, dim3((npat + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, main.s, db.pats.p, npat, out.p, stride(), gd.lpc.p);
      HIPCHECK(hipGetLastError());
      if (batches.size() == 1) launch_mix(*this, main);
    }
  }
  // cohort reduction of one batch (nelem elements of its rows) into sums; the last batch's also packs
  void reduce_batch(const Batch& b, int nelem) {
    const BatchDev& db = dev[b.id];
    const int st = stride(), npat = (int)b.pats.size();
    const int per = red_per(npat), nchunk = (npat + per - 1) / per;
    const dim3 cols((nelem + BLOCK - 1) / BLOCK);
    if (mixing())
      hipLaunchKernelGGL(k_reduce_rows_mix, dim3(cols.x, nchunk), dim3(BLOCK), 0, main.s, db.pats.p, npat, per, out.p, st, nelem,
                         gd.omega.p, gd.lambda.p, redbuf.p);
    else if (row_w.empty())
      hipLaunchKernelGGL(k_reduce_rows, dim3(cols.x, nchunk), dim3(BLOCK), 0, main.s, db.pats.p, npat, per, out.p, st, nelem, redbuf.p);
    else
      hipLaunchKernelGGL(k_reduce_rows_w, dim3(cols.x, nchunk), dim3(BLOCK), 0, main.s, db.pats.p, npat, per, out.p, st, nelem,
                         db.wrow.p, redbuf.p);
    HIPCHECK(hipGetLastError());
    if (pack.mode && &b == &batches.back()) {
      hipLaunchKernelGGL(k_reduce_parts_pack, dim3((st + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, main.s, redbuf.p, st, nelem, nchunk,
                         sums.p, pack.mode, N, pack.a, pack.b, pack.dst);
      pack.done = true;
    } else {
      hipLaunchKernelGGL(k_reduce_parts, dim3(cols.x, 2), dim3(BLOCK), 0, main.s, redbuf.p, st, nelem, nchunk, sums.p);
    }
    HIPCHECK(hipGetLastError());
  }
  // the per-patient rows of a batch to their cohort rows of host_out (waits for the batch)
  void download_rows(const Batch& b, double* host_out) {
    const int st = stride(), npat = (int)b.pats.size();
    std::vector<double> tmp((size_t)npat * st);
    HIPCHECK(hipMemcpyAsync(tmp.data(), out.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, main.s));
    HIPCHECK(hipStreamSynchronize(main.s));
    coop.check_abort();
    for (int i = 0; i < npat; ++i)
      std::memcpy(host_out + (size_t)b.pats[i].row * st, tmp.data() + (size_t)i * st, st * sizeof(double));
  }
  void download_sums(double* host_sums) {
    std::vector<double> hs(2 * stride());
    HIPCHECK(hipMemcpyAsync(hs.data(), sums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, main.s));
    HIPCHECK(hipStreamSynchronize(main.s));
    coop.check_abort();
    std::memcpy(host_sums, hs.data(), hs.size() * sizeof(double));
  }

  // host_out (optional): per-patient rows [n_pat][stride]; host_sums: [2][stride] (EM, NM)
  // With row groups (rowmix.h) the reduction needs lp of EVERY cohort row before the first row is added: one batch, or a
  // score-only evaluation, is one sweep (the reductions of a score-only evaluation of several batches read no per-batch
  // buffer and run behind the last batch); several batches with a gradient are a score-only sweep that fills lpc, then
  // the sweep with gradient.
  void evaluate(const double* lt, const double* ldp, const double* ldm, bool want_grad, double* host_sums,
                double* host_out) {
    REQUIRE(!pending.on, "an evaluation begun with mmhn_cohort_sums_begin has not been collected");
    const bool mix = mixing();
    const int nsweep = mix && want_grad && batches.size() > 1 ? 2 : 1;
    const bool reduce_behind = mix && !want_grad && batches.size() > 1;
    auto t0 = std::chrono::steady_clock::now();
    for (Lane& l : side) l.reset();
    bool head_done = eval_head(lt, ldp, ldm, want_grad && nsweep == 1);   // (the gradient of the first sweep: what the head clears for)
    for (int sweep = 0; sweep < nsweep; ++sweep) {
      const bool last_sweep = sweep == nsweep - 1;
      const bool grad = want_grad && last_sweep;
      if (sweep > 0) { launch_mix(*this, main); head_done = false; }     // (lpc is whole; the head cleared nothing for a gradient)
      for (const Batch& b : batches) {
        const BatchDev& db = dev[b.id];
        const int nJ = (int)b.dJ.size();
        batch_prepare(b, grad, head_done && &b == &batches.front());
        prep(main, db.dJ.p, nJ, tabJ.p, true, b.maxkcJ);              // (first: the head of the critical chain)
        // staged patients that are their own problem: a side lane of their own from here to the assembly, with its own
        // flag set for their cooperative launches (a timed batch keeps them on the main lane, where its events are recorded)
        Lane& own = timer.on ? main : side[2];
        const bool own_apart = &own != &main && !b.stg[0].empty();
        if (own_apart) {
          own.begin(main);
          staged_fwd(own, b, 0, grad);
          if (grad) staged_adj(own, b, 0);
          own.end();
        }
        // patients that are their own single-tumour problem need nothing of the joint path: their small-space kernels
        // run on a side lane from here on, next to the joint forward solve (whose launch is issued first - it is the
        // critical chain); the assembly waits for them
        if (b.has_small) side[0].record_fork(main);
        clear_dead_tiles(b, grad);
        joint_forward(b);
        if (b.has_small) { small_classes(b, 0, grad); small_classes(b, 1, grad); }
        // 3-4 the staged single-tumour problems (the paired rows' after the joint forward solve)
        if (!own_apart) staged_fwd(main, b, 0, grad);
        staged_fwd(main, b, 1, grad);
        if (grad) {
          if (!own_apart) staged_adj(main, b, 0);
          staged_adj(main, b, 1);
          // (the 1024-thread class of the paired small-space launches ran on its side lane next to the staged kernels above:
          // the joint adjoint is the first consumer of what it wrote)
          side[1].join(main);
          if (nJ) { joint_adjoint(b); joint_gradient(b); }
        }
        for (Lane& l : side) l.join(main);
        finalize_batch(b, grad, mix && sweep == 0);
        if (last_sweep && !reduce_behind) reduce_batch(b, grad ? stride() : 1);
        if (host_out && last_sweep) download_rows(b, host_out);
      }
    }
    if (reduce_behind) {
      launch_mix(*this, main);
      for (const Batch& b : batches) reduce_batch(b, 1);
    }
    timer.on = true;
    if (host_sums) {
      download_sums(host_sums);
      finish_eval(t0);
    }
  }
  // score-only evaluation: lp of every row, P(seeded | genotype) of the rows of unknown status (NaN for the others)
  void patient_status(const double* lt, const double* ldp, const double* ldm, double* lp_out, double* p_seeded) {
    const int st = stride();
    std::vector<double> rows((size_t)n_pat * st), s(2 * st);
    evaluate(lt, ldp, ldm, false, s.data(), rows.data());
    for (long long i = 0; i < n_pat; ++i) lp_out[i] = rows[(size_t)i * st];
    if (n_pat > 0) HIPCHECK(hipMemcpy(p_seeded, resp.p, (size_t)n_pat * sizeof(double), hipMemcpyDeviceToHost));
  }
  void finish_eval(std::chrono::steady_clock::time_point t0) {
    timer.collect(cnt);
    cnt.eval_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    cnt.evals += 1;
  }

  // sums layout of the C ABI (include/metmhn_amd.h): packed on the device, summed over the ranks of the
  // communicator (one RCCL all-reduce on this stream, regularized_optimization.py:256-266 needs nothing else),
  // then one download and one synchronisation per evaluation
  // begin: everything is issued (evaluation, packing, the all-reduce, the download into pinned memory), nothing is
  // waited for - the caller's host work (the reference computes its penalty terms on the host after the score,
  // regularized_optimization.py:296) runs next to the GPU; end: wait and copy out.
  // w_combined (optional): pack w * EM + NM on the device (k_pack_wsums) - 1 + N^2 + 2N doubles travel instead of
  // 4 + 2 N^2 + 3 N
  void cohort_sums_begin(const double* lt, const double* ldp, const double* ldm, bool grad, const double* w_combined = nullptr) {
    Pending& pd = pending;
    REQUIRE(!pd.on, "mmhn_cohort_sums_begin: the previous evaluation has not been collected");
    pd.t0 = std::chrono::steady_clock::now();
    const int total = w_combined ? stride() : full_len();
    pd.abi_sums.alloc(full_len());
    if (!pd.h_abi) {
      HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&pd.h_abi), (size_t)full_len() * sizeof(double), hipHostMallocDefault));
      HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&pd.h_abi_dev), pd.h_abi, 0));
    }
    // without a communicator the packing kernel writes the result straight into the pinned buffer; with one the
    // all-reduce works on device memory and the copy engine brings its result down
    double* packed = (cfg.zero_copy && !comm) ? pd.h_abi_dev : pd.abi_sums.p;
    // the reduce flag belongs to the weighted evaluation alone: a plain one in between leaves it for the next weighted one.
    // Taken out of the member before anything is issued, so that an evaluation that throws cannot leave it to a later one.
    double flag = 0.0;
    if (w_combined) { flag = reduce_flag; reduce_flag = 0.0; }
    pack = Pack{w_combined ? 2 : 1, w_combined ? *w_combined : counts().em, w_combined ? flag : counts().pat, packed, false};
    struct Unset { int& m; ~Unset() { m = 0; } } unset{pack.mode};
    evaluate(lt, ldp, ldm, grad, nullptr, nullptr);
    if (!pack.done) {                                      // (no batch: an empty cohort)
      if (w_combined) hipLaunchKernelGGL(k_pack_wsums, dim3(2), dim3(256), 0, stream, sums.p, N, *w_combined, packed, flag);
      else hipLaunchKernelGGL(k_pack_sums, dim3(2), dim3(256), 0, stream, sums.p, N, counts().em, counts().pat, packed);
      HIPCHECK(hipGetLastError());
    }
    const int moved = total + (w_combined ? 1 : 0);            // (the reduce flag rides behind the pre-combined buffer)
    if (comm) RCCLCHECK(rccl().AllReduce(pd.abi_sums.p, pd.abi_sums.p, (size_t)moved, ncclFloat64, ncclSum, comm, stream));
    if (packed == pd.abi_sums.p) HIPCHECK(hipMemcpyAsync(pd.h_abi, pd.abi_sums.p, moved * sizeof(double), hipMemcpyDeviceToHost, stream));
    pd.flag = w_combined != nullptr;
    pd.issued = std::chrono::steady_clock::now();
    pd.on = true;
    pd.len = total;
  }
  void cohort_sums_end(double* o, int expect_len) {
    Pending& pd = pending;
    REQUIRE(pd.on, "mmhn_cohort_sums_end without mmhn_cohort_sums_begin");
    REQUIRE(expect_len == pd.len, "mmhn_cohort_sums_end / mmhn_cohort_wsums_end does not match the _begin call");
    pd.on = false;
    HIPCHECK(hipStreamSynchronize(stream));
    coop.check_abort();
    std::memcpy(o, pd.h_abi, (size_t)pd.len * sizeof(double));
    reduce_flag_sum = pd.flag ? pd.h_abi[pd.len] : 0.0;
    if (cfg.trace_host)
      std::fprintf(stderr, "[mmhn] evaluation issued after %.1f us, complete after %.1f us\n",
                   std::chrono::duration<double, std::micro>(pd.issued - pd.t0).count(),
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - pd.t0).count());
    finish_eval(pd.t0);
  }
  // (A hipGraph replay of the evaluation was measured on the LUAD-reduced cohort, ROCm 7.0.2: the host is free after
  // 75 us instead of 535 us, but the graph takes 660 us to execute against 550 us for the eager launches - dropped.)
  void cohort_sums(const double* lt, const double* ldp, const double* ldm, bool grad, double* o) {
    cohort_sums_begin(lt, ldp, ldm, grad);
    cohort_sums_end(o, full_len());
  }
};

}  // namespace mmhn

// what is not the cohort evaluation: free functions over an engine's launch helpers
#include "rowmix_host.h"
#include "prims.h"
#include "orders_host.h"
#include "orderpost_host.h"
#include "orderprec_host.h"
#include "orderpos_host.h"
#include "ordertime_host.h"
#include "ordersnap_host.h"
#include "ordersample_host.h"
#include "forecast_host.h"
#include "landscape_host.h"
#include "genodist_host.h"
#include "metdist_host.h"
#include "partner_host.h"
#include "cross_host.h"
#include "sampler_host.h"
#include "bench.h"
#include "capi.h"
