// Host side of the metMHN engine: the engine's state, its kernel launches, the cohort evaluation and the
// C ABI of include/metmhn_amd.h.  One engine = one GPU; one main lane (host.h: Lane - a HIP stream with its cooperative flag
// set and its fork / join events) and three side lanes that an evaluation forks off it.
// The rest of the host side lives in headers of this one translation unit: plan.h (the cohort planner, host-only:
// batches, routes, work lists, offsets), host.h (errors, device arrays, lanes, MMHN_* knob readers), comm.h (RCCL),
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

struct EngineBase {
  virtual ~EngineBase() = default;
  int dtype = 0;
  int device = 0;
  hipStream_t stream = nullptr;       // the main lane's (Engine::main.s): set when the engine is created, never reassigned
  Config cfg;
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
  int n = 0, N = 0;
  // ---- parameters
  DevArr<Params<T>> d_par;
  Params<T>* h_par = nullptr;         // pinned: the per-evaluation upload is a true async copy
  void* h_par_dev = nullptr;          // device view of it
  // popcount-ordered state permutations of every tile size (k_tsolve step B)
  DevArr<uint16_t> d_perm;
  DevArr<int> d_lvl;
  // ---- cohort: the rows, their plan (plan.h) and its device copy, one entry per batch
  std::vector<int8_t> dat;
  long long n_pat = 0;
  int n_cols = 0;
  // the three counts of the objective: sum of w [seeding = 1], sum of w, sum of w [type 4], taken on the host in row order -
  // plain: w = 1 (the integer counts), weighted: the row weights, grouped: the weights of the row groups
  struct Counts { double em = 0, pat = 0, unknown = 0; } plain, weighted, grouped;
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
  DevArr<double> lp, out, sums, abi_sums, redbuf;
  DevArr<double> resp;                // [n_pat] by cohort row: P(seeded | genotype) of the rows of unknown status (dat type 4), written
                                      // where their score is formed; NaN everywhere else (filled once, when the cohort is set)
  long long n_unknown = 0;            // rows of dat type 4
  // ---- row weights (mmhn_set_row_weights, rowmix_host.h): by cohort row, empty = none
  std::vector<double> row_w;
  // ---- row groups (mmhn_set_row_groups, rowmix.h, rowmix_host.h): the group lists and weights as given (grp_ptr empty =
  // none), the transposed lists and the per-evaluation arrays on the device
  std::vector<long long> grp_ptr;
  std::vector<int> grp_rows;
  std::vector<double> grp_w;
  struct GroupsDev {
    DevArr<long long> gptr, mptr;
    DevArr<int> grows, mgrp;
    DevArr<double> gw, lpc, lpg, omega, lambda, rho;
  } gd;
  bool want_rho = false;              // mmhn_group_posteriors: k_group_lse also writes rho
  DevArr<JLink<T>> links;
  double* h_abi = nullptr;            // pinned landing buffer of the result download
  double* h_abi_dev = nullptr;        // device view of it
  // ---- lanes (host.h): main carries the joint path; side[0], side[1] the small-space launches (small_classes), side[2] the
  // staged own-problem patients, whose cooperative launches use the second flag set
  Lane main, side[3];
  // ---- cooperative launches (tsolve.h): queue heads + abort word, the flags of the tiles (value = epoch of the launch that
  // finished the tile), the pinned host copy of the abort word
  DevArr<CoopCtl> coop_ctl;
  DevArr<unsigned> coop_flags[2];   // one set per lane that issues such launches (Lane::flags): two may be in flight together
  unsigned coop_epoch = 0;
  int coop_slot = 0;
  unsigned* h_abort = nullptr;
  unsigned* h_abort_dev = nullptr;
  bool coop_used = false;           // an evaluation issued a cooperative launch since the last check_abort
  bool coop_alone = false;          // set per batch: no side stream carries whole-CU work next to the joint solves (tsolve.h: WPE)
  // ---- pending evaluation (cohort_sums_begin ... cohort_sums_end)
  bool sums_pending = false;
  std::chrono::steady_clock::time_point sums_t0, sums_issued;
  int sums_len = 0;                                           // doubles of the pending result
  // set by cohort_sums_begin around evaluate(): the last batch's reduction also packs (k_reduce_parts_pack)
  int pack_mode = 0;
  double pack_a = 0, pack_b = 0;
  double* pack_dst = nullptr;
  bool packed_in_eval = false;
  double reduce_flag = 0.0, reduce_flag_sum = 0.0;            // mmhn_set_reduce_flag / mmhn_get_reduce_flag
  bool flag_pending = false;
  // ---- communicator: patient shards on several GPUs, one communicator per engine, the all-reduce runs on the engine's stream
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_size = 1;
  // ---- counters (mmhn_get_counters).  HIP events around the dominant kernels: an event record costs ~5 us of host time,
  // which a short evaluation cannot afford (it is bound by the host's issue rate) - only batches of at least 2^26 states
  // are timed (set per batch; MMHN_TIME_KERNELS=1: every batch)
  bool time_kernels = true;
  mmhn_counters cnt{};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::vector<double> ev_bytes;
  std::vector<int> ev_slot;           // MMHN_K_* class of the timed launch

  static long long zarena_elems(long long nJ, long long asize, int N) { return up4(3 * nJ * N * N) + up4(3 * nJ * N) + up4(asize); }
  // elements of a batch's zarena that the memset clears
  static long long zclear_elems(const Batch& b, int N) { return zarena_elems((long long)b.dJ.size(), b.aclr, N); }

  Engine(int dev_id, int n_mut) : n(n_mut), N(n_mut + 1) {
    device = dev_id;
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
    coop_ctl.alloc(1);
    HIPCHECK(hipMemset(coop_ctl.p, 0, sizeof(CoopCtl)));
    HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&h_abort), 64, hipHostMallocDefault));
    HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_abort_dev), h_abort, 0));
    *h_abort = 0u;
    for (Lane& l : side) {
      HIPCHECK(hipStreamCreateWithFlags(&l.s, hipStreamNonBlocking));
      HIPCHECK(hipEventCreateWithFlags(&l.ev_fork, hipEventDisableTiming));
      HIPCHECK(hipEventCreateWithFlags(&l.ev_join, hipEventDisableTiming));
    }
    side[2].flags = 1;
  }
  ~Engine() override {                       // runs under the DevGuard of mmhn_destroy
    comm_destroy();
    for (auto& e : ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (Lane& l : side) {
      if (l.ev_join) (void)hipEventDestroy(l.ev_join);
      if (l.ev_fork) (void)hipEventDestroy(l.ev_fork);
      if (l.s) (void)hipStreamDestroy(l.s);
    }
    if (h_par) (void)hipHostFree(h_par);
    if (h_abi) (void)hipHostFree(h_abi);
    if (h_abort) (void)hipHostFree(h_abort);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }
  int stride() const { return 1 + N * N + 2 * N; }

  // ---------------------------------------------------------------- parameters
  void build_params(const double* lt, const double* ldp, const double* ldm, bool upload = true) {
    REQUIRE(!sums_pending, "an evaluation begun with mmhn_cohort_sums_begin has not been collected (its parameter upload may still be in flight)");
    // exp(theta_ij - d_j) = exp(theta_ij) * exp(-d_j): N^2 + 2N exponentials per evaluation instead of 3 N^2 (this runs
    // on the host before the first launch of every evaluation - 26 us of a 400 us LUAD evaluation as three full passes)
    std::vector<double> eth((size_t)N * N), enp(N, 1.0), enm(N, 1.0);
    for (int e = 0; e < N * N; ++e) eth[e] = std::exp(lt[e]);
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
    if (alg_bytes > 0) { timed(L, MMHN_K_OTHER_SOLVE, alg_bytes, launch); return; }   // (a launch without algorithmic bytes is never timed)
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
  void collect_events() {
    for (size_t i = 0; i < ev_used; ++i) {
      float ms = 0;
      HIPCHECK(hipEventElapsedTime(&ms, ev_pool[i].first, ev_pool[i].second));
      mmhn_kernel_counter& c = cnt.kernel[ev_slot[i]];
      c.ms += ms;
      c.launches += 1;
      c.alg_bytes += ev_bytes[i];
    }
    ev_used = 0;
    ev_bytes.clear();
    ev_slot.clear();
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
  // timed launch helper shared by the two solvers: the events are recorded on the lane of the launch (they are not
  // created with hipEventDisableTiming - evaluate() keeps a timed batch on the main lane)
  template <typename F>
  void timed(const Lane& L, int slot, double alg_bytes, F&& launch) {
    if (!time_kernels) {
      launch();
      HIPCHECK(hipGetLastError());
      return;
    }
    if (ev_used == ev_pool.size()) {
      hipEvent_t a, b;
      HIPCHECK(hipEventCreate(&a));
      HIPCHECK(hipEventCreate(&b));
      ev_pool.push_back({a, b});
    }
    hipEvent_t e0 = ev_pool[ev_used].first, e1 = ev_pool[ev_used].second;
    ++ev_used;
    ev_bytes.push_back(alg_bytes);
    ev_slot.push_back(slot);
    HIPCHECK(hipEventRecord(e0, L.s));
    launch();
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(e1, L.s));
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
      timed(L, tr ? MMHN_K_PSOLVE_ADJ : MMHN_K_PSOLVE_FWD, bytes, [&]() {
        const int nch = (int)b.wchains.size();
        const dim3 g((unsigned)std::min(nch, cfg.plan.wsolve_wgs > 0 ? cfg.plan.wsolve_wgs : cfg.plan.n_cu)), bk(WROWS);
        const size_t lds = wsolve_lds<T>();
#define WS_ARGS g, bk, lds, L.s, db.dJ.p, db.wd.p, db.wchains.p, nch, yw, tabJ.p, links.p, qS.p
        // (a batch whose chains all have the same number of external bits - every k = 20 cohort: 5, k = 25: 9 - runs the instantiation
        // that knows it at compile time)
        if (b.wnx == WCfg<T>::NXT) { if (tr) hipLaunchKernelGGL((k_wsolve<T, true, WCfg<T>::NXT>), WS_ARGS); else hipLaunchKernelGGL((k_wsolve<T, false, WCfg<T>::NXT>), WS_ARGS); }
        else if (tr) hipLaunchKernelGGL((k_wsolve<T, true>), WS_ARGS);
        else hipLaunchKernelGGL((k_wsolve<T, false>), WS_ARGS);
#undef WS_ARGS
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
      timed(L, tr ? MMHN_K_PSOLVE_ADJ : MMHN_K_PSOLVE_FWD, bytes, [&]() {
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
      DevArr<unsigned>& flags = coop_flags[L.flags];
      if (flags.n < (size_t)nitems) {
        HIPCHECK(hipStreamSynchronize(L.s));                // (a launch of this lane may still poll the old array)
        flags.alloc((size_t)nitems + 1024);
        HIPCHECK(hipMemsetAsync(flags.p, 0, flags.n * sizeof(unsigned), L.s));
      }
      if (++coop_epoch == 0u) {                                // (wrapped: no stale flag may equal a future epoch)
        HIPCHECK(hipDeviceSynchronize());
        for (auto& f : coop_flags) if (f.p) HIPCHECK(hipMemset(f.p, 0, f.n * sizeof(unsigned)));
        coop_epoch = 1u;
      }
      coop_slot = (coop_slot + 1) & 3;
      const int slot = L.flags * 4 + coop_slot;
      coop_used = true;
      timed(L, P.kslot, per_tile * nitems, [&]() {
        const dim3 g((unsigned)std::min(nitems, cfg.coop_wgs > 0 ? cfg.coop_wgs : cfg.plan.n_cu)), bk(TSB);
#define CS_ARGS g, bk, lds, L.s, P.d, dcl.items.p, dcl.deps.p, nitems, flags.p, coop_epoch, coop_ctl.p, slot, h_abort_dev, cfg.coop_fault ? 1 : 0, \
                y, lidg, rhs, rhs_mode, scal, d_perm.p, mk, P.tab, links.p, qS.p
        // (three of the four (lidg, coop_alone) variants exist: a list with a lidg vector never runs the 4-wave one)
        with_flags([&](auto tr_) {
          if (lidg) hipLaunchKernelGGL((k_csolve<T, tr_(), true>), CS_ARGS);
          else if (coop_alone) hipLaunchKernelGGL((k_csolve<T, tr_(), false, 4>), CS_ARGS);   // (nothing runs beside the joint solves of this batch: 93 registers)
          else hipLaunchKernelGGL((k_csolve<T, tr_(), false>), CS_ARGS);
        }, tr);
#undef CS_ARGS
      });
      return;
    }
    for (int s = 0; s < nlev; ++s) {
      const int lev = tr ? nlev - 1 - s : s;
      const int beg = (*P.lof)[lev], cntl = (*P.lof)[lev + 1] - beg;
      if (cntl == 0) continue;
      timed(L, P.kslot, per_tile * cntl, [&]() {
        with_flags([&](auto tr_, auto jac) {
          hipLaunchKernelGGL((k_tsolve<T, tr_(), jac()>), dim3(cntl), dim3(TSB), lds, L.s, P.d, P.lmap + beg, d_par.p, y, lidg, rhs, rhs_mode, scal,
                             d_perm.p, d_lvl.p, mk, P.tab, links.p, qS.p);
        }, tr, lidg != nullptr);
      });
    }
  }
  // a spin of a cooperative launch timed out (tsolve.h): the results of the evaluation are garbage - fail the call, and put
  // the words back so that the engine stays usable.  Call after the stream has been synchronised.
  void check_abort() {
    if (!coop_used) return;
    coop_used = false;
    if (*h_abort == 0u) return;
    *h_abort = 0u;
    (void)hipMemset(coop_ctl.p, 0, sizeof(CoopCtl));
    throw Fail{"cooperative tile solve: a wait for another workgroup's tile timed out (results discarded)"};
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
    REQUIRE(!sums_pending, "mmhn_set_cohort: an evaluation begun with mmhn_cohort_sums_begin has not been collected");
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
  bool mixing() const { return !grp_ptr.empty(); }
  // the counts of the objective that hold for the next evaluation (with row groups: the group-weighted ones)
  const Counts& counts() const { return mixing() ? grouped : row_w.empty() ? plain : weighted; }
  void row_weight_sums(double* out3) const { out3[0] = counts().em; out3[1] = counts().pat; out3[2] = counts().unknown; }
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
    time_kernels = cfg.force_timing || b.vecJ + b.vecS >= (1ll << 26);
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
      timed(main, MMHN_K_PCLASS, mbytes, [&]() {
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
    if (pack_mode && &b == &batches.back()) {
      hipLaunchKernelGGL(k_reduce_parts_pack, dim3((st + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, main.s, redbuf.p, st, nelem, nchunk,
                         sums.p, pack_mode, N, pack_a, pack_b, pack_dst);
      packed_in_eval = true;
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
    check_abort();
    for (int i = 0; i < npat; ++i)
      std::memcpy(host_out + (size_t)b.pats[i].row * st, tmp.data() + (size_t)i * st, st * sizeof(double));
  }
  void download_sums(double* host_sums) {
    std::vector<double> hs(2 * stride());
    HIPCHECK(hipMemcpyAsync(hs.data(), sums.p, hs.size() * sizeof(double), hipMemcpyDeviceToHost, main.s));
    HIPCHECK(hipStreamSynchronize(main.s));
    check_abort();
    std::memcpy(host_sums, hs.data(), hs.size() * sizeof(double));
  }

  // host_out (optional): per-patient rows [n_pat][stride]; host_sums: [2][stride] (EM, NM)
  // With row groups (rowmix.h) the reduction needs lp of EVERY cohort row before the first row is added: one batch, or a
  // score-only evaluation, is one sweep (the reductions of a score-only evaluation of several batches read no per-batch
  // buffer and run behind the last batch); several batches with a gradient are a score-only sweep that fills lpc, then
  // the sweep with gradient.
  void evaluate(const double* lt, const double* ldp, const double* ldm, bool want_grad, double* host_sums,
                double* host_out) {
    REQUIRE(!sums_pending, "an evaluation begun with mmhn_cohort_sums_begin has not been collected");
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
        Lane& own = time_kernels ? main : side[2];
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
    time_kernels = true;
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
  void reset_counters() {                              // (what RCCL said about the communicator stays)
    const int r = cnt.comm_ranks, k = cnt.comm_rank;
    cnt = mmhn_counters{};
    cnt.comm_ranks = r; cnt.comm_rank = k;
  }
  void finish_eval(std::chrono::steady_clock::time_point t0) {
    collect_events();
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
    REQUIRE(!sums_pending, "mmhn_cohort_sums_begin: the previous evaluation has not been collected");
    sums_t0 = std::chrono::steady_clock::now();
    const int full = 4 + 2 * N * N + 3 * N;
    const int total = w_combined ? stride() : full;
    abi_sums.alloc(full);
    if (!h_abi) {
      HIPCHECK(hipHostMalloc(reinterpret_cast<void**>(&h_abi), (size_t)full * sizeof(double), hipHostMallocDefault));
      HIPCHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_abi_dev), h_abi, 0));
    }
    // without a communicator the packing kernel writes the result straight into the pinned buffer; with one the
    // all-reduce works on device memory and the copy engine brings its result down
    double* packed = (cfg.zero_copy && !comm) ? h_abi_dev : abi_sums.p;
    // the reduce flag belongs to the weighted evaluation alone: a plain one in between leaves it for the next weighted one.
    // Taken out of the member before anything is issued, so that an evaluation that throws cannot leave it to a later one.
    double flag = 0.0;
    if (w_combined) { flag = reduce_flag; reduce_flag = 0.0; }
    pack_mode = w_combined ? 2 : 1;
    pack_a = w_combined ? *w_combined : counts().em; pack_b = w_combined ? flag : counts().pat; pack_dst = packed;
    packed_in_eval = false;
    struct Unset { int& m; ~Unset() { m = 0; } } unset{pack_mode};
    evaluate(lt, ldp, ldm, grad, nullptr, nullptr);
    if (!packed_in_eval) {                                 // (no batch: an empty cohort)
      if (w_combined) hipLaunchKernelGGL(k_pack_wsums, dim3(2), dim3(256), 0, stream, sums.p, N, *w_combined, packed, flag);
      else hipLaunchKernelGGL(k_pack_sums, dim3(2), dim3(256), 0, stream, sums.p, N, counts().em, counts().pat, packed);
      HIPCHECK(hipGetLastError());
    }
    const int moved = total + (w_combined ? 1 : 0);            // (the reduce flag rides behind the pre-combined buffer)
    if (comm) RCCLCHECK(rccl().AllReduce(abi_sums.p, abi_sums.p, (size_t)moved, ncclFloat64, ncclSum, comm, stream));
    if (packed == abi_sums.p) HIPCHECK(hipMemcpyAsync(h_abi, abi_sums.p, moved * sizeof(double), hipMemcpyDeviceToHost, stream));
    flag_pending = w_combined != nullptr;
    sums_issued = std::chrono::steady_clock::now();
    sums_pending = true;
    sums_len = total;
  }
  void cohort_sums_end(double* o, int expect_len) {
    REQUIRE(sums_pending, "mmhn_cohort_sums_end without mmhn_cohort_sums_begin");
    REQUIRE(expect_len == sums_len, "mmhn_cohort_sums_end / mmhn_cohort_wsums_end does not match the _begin call");
    sums_pending = false;
    HIPCHECK(hipStreamSynchronize(stream));
    check_abort();
    std::memcpy(o, h_abi, (size_t)sums_len * sizeof(double));
    reduce_flag_sum = flag_pending ? h_abi[sums_len] : 0.0;
    if (cfg.trace_host)
      std::fprintf(stderr, "[mmhn] evaluation issued after %.1f us, complete after %.1f us\n",
                   std::chrono::duration<double, std::micro>(sums_issued - sums_t0).count(),
                   std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - sums_t0).count());
    finish_eval(sums_t0);
  }
  // (A hipGraph replay of the evaluation was measured on the LUAD-reduced cohort, ROCm 7.0.2: the host is free after
  // 75 us instead of 535 us, but the graph takes 660 us to execute against 550 us for the eager launches - dropped.)
  void cohort_sums(const double* lt, const double* ldp, const double* ldm, bool grad, double* o) {
    cohort_sums_begin(lt, ldp, ldm, grad);
    cohort_sums_end(o, 4 + 2 * N * N + 3 * N);
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

// ======================================================================================
// C ABI
// ======================================================================================
using namespace mmhn;

struct mmhn_engine {
  int dtype;
  int n;
  EngineBase* impl;
};

#define API_BEGIN try {
#define API_END                                   \
  return 0;                                       \
  }                                               \
  catch (const Fail& f) { g_err = f.msg; return 1; } \
  catch (const std::exception& e) { g_err = e.what(); return 2; }

// engine's device current for the rest of the entry point
#define GUARD(h)                            \
  REQUIRE(h && h->impl, "null handle");     \
  DevGuard dev_guard_(h->impl->device)

#define DISPATCH(h, call)                                             \
  do {                                                                \
    REQUIRE(h && h->impl, "null handle");                             \
    if (h->dtype == MMHN_F64) static_cast<Engine<double>*>(h->impl)->call; \
    else static_cast<Engine<float>*>(h->impl)->call;                  \
  } while (0)
// ... and a free function template over the engine (prims.h, orders_host.h, bench.h)
#define DISPATCH_FN(h, fn, ...)                                                            \
  do {                                                                                     \
    REQUIRE(h && h->impl, "null handle");                                                  \
    if (h->dtype == MMHN_F64) fn(*static_cast<Engine<double>*>(h->impl), __VA_ARGS__);     \
    else fn(*static_cast<Engine<float>*>(h->impl), __VA_ARGS__);                           \
  } while (0)

extern "C" {

const char* mmhn_last_error(void) { return g_err.c_str(); }

int mmhn_create(int device_id, int n_mut, int dtype, mmhn_handle* out) {
  API_BEGIN
  REQUIRE(out, "null out pointer");
  REQUIRE(dtype == MMHN_F64 || dtype == MMHN_F32, "dtype must be MMHN_F64 or MMHN_F32");
  int ndev = 0;
  HIPCHECK(hipGetDeviceCount(&ndev));
  REQUIRE(ndev > 0, "no HIP device visible: metmhn_amd needs a GPU (no CPU fallback)");
  REQUIRE(device_id >= 0 && device_id < ndev, "device_id out of range");
  auto* h = new mmhn_engine{dtype, n_mut, nullptr};
  try {
    if (dtype == MMHN_F64) h->impl = new Engine<double>(device_id, n_mut);
    else h->impl = new Engine<float>(device_id, n_mut);
  } catch (...) { delete h; throw; }
  h->impl->dtype = dtype;
  *out = h;
  API_END
}

void mmhn_destroy(mmhn_handle h) {
  if (!h) return;
  try {
    if (h->impl) {
      DevGuard guard(h->impl->device);     // device memory, stream and communicator are released on their GPU
      delete h->impl;
    }
  } catch (...) {
  }
  delete h;
}

int mmhn_set_workspace_limit(mmhn_handle h, size_t bytes) {
  API_BEGIN
  GUARD(h);
  REQUIRE(bytes >= (size_t)1 << 20, "workspace limit below 1 MiB");
  h->impl->cfg.plan.ws_limit = bytes;
  API_END
}

int mmhn_set_cohort(mmhn_handle h, const int8_t* dat, int64_t n_pat, int n_cols) {
  API_BEGIN
  GUARD(h);
  REQUIRE(dat || n_pat == 0, "null dat");
  DISPATCH(h, set_cohort(dat, n_pat, n_cols));
  API_END
}

// n_unknown: rows of dat type 4 - weight 1, outside the EM / NM balance (they ride in the NM sums)
static void weights(double n_em, double n_pat, double n_unknown, double perc_met, double* w, double* n_full) {
  const double n_nm = n_pat - n_em - n_unknown;           // regularized_optimization.py:121-128
  *w = (n_em * n_nm != 0) ? perc_met * n_nm / ((1 - perc_met) * n_em) : 1.0;
  *n_full = *w * n_em + n_nm + n_unknown;
}
static long long unknown_rows(mmhn_handle h) {
  return h->dtype == MMHN_F64 ? static_cast<Engine<double>*>(h->impl)->n_unknown : static_cast<Engine<float>*>(h->impl)->n_unknown;
}

int mmhn_set_row_weights(mmhn_handle h, const double* w, int64_t n) {
  API_BEGIN
  GUARD(h);
  DISPATCH_FN(h, set_row_weights, w, n);
  API_END
}

int mmhn_get_row_weight_sums(mmhn_handle h, double* out3) {
  API_BEGIN
  GUARD(h);
  REQUIRE(out3, "null pointer");
  DISPATCH(h, row_weight_sums(out3));
  API_END
}

int mmhn_set_row_groups(mmhn_handle h, const int64_t* ptr, int64_t n_groups, const int64_t* rows, const double* w) {
  API_BEGIN
  GUARD(h);
  DISPATCH_FN(h, set_row_groups, ptr, n_groups, rows, w);
  API_END
}

int mmhn_group_posteriors(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double* lp_group, double* rho) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && lp_group && rho, "null pointer");
  DISPATCH_FN(h, group_posteriors, lt, ldp, ldm, lp_group, rho);
  API_END
}

int mmhn_cohort_sums(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad,
                     double* sums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && sums, "null pointer");
  DISPATCH(h, cohort_sums(lt, ldp, ldm, with_grad != 0, sums));
  API_END
}

int mmhn_cohort_sums_begin(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm, "null pointer");
  DISPATCH(h, cohort_sums_begin(lt, ldp, ldm, with_grad != 0));
  API_END
}

int mmhn_cohort_sums_end(mmhn_handle h, double* sums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(sums, "null pointer");
  DISPATCH(h, cohort_sums_end(sums, 4 + 2 * (h->n + 1) * (h->n + 1) + 3 * (h->n + 1)));
  API_END
}

int mmhn_cohort_wsums_begin(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad, double w) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm, "null pointer");
  REQUIRE(std::isfinite(w), "w must be finite");
  DISPATCH(h, cohort_sums_begin(lt, ldp, ldm, with_grad != 0, &w));
  API_END
}

int mmhn_set_reduce_flag(mmhn_handle h, double value) {
  API_BEGIN
  GUARD(h);
  REQUIRE(std::isfinite(value), "the flag must be finite");
  DISPATCH(h, reduce_flag = value);
  API_END
}
int mmhn_get_reduce_flag(mmhn_handle h, double* summed) {
  API_BEGIN
  GUARD(h);
  REQUIRE(summed, "null pointer");
  if (h->dtype == MMHN_F64) *summed = static_cast<Engine<double>*>(h->impl)->reduce_flag_sum;
  else *summed = static_cast<Engine<float>*>(h->impl)->reduce_flag_sum;
  API_END
}

int mmhn_cohort_wsums_end(mmhn_handle h, double* wsums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(wsums, "null pointer");
  DISPATCH(h, cohort_sums_end(wsums, 1 + (h->n + 1) * (h->n + 1) + 2 * (h->n + 1)));
  API_END
}

int mmhn_score_and_grad(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double perc_met,
                        double* score, double* d_theta, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && score, "null pointer");
  const int N = h->n + 1;
  const bool grad = d_theta && d_dp && d_dm;
  std::vector<double> s(4 + 2 * N * N + 3 * N);
  DISPATCH(h, cohort_sums(lt, ldp, ldm, grad, s.data()));
  double w, nf;
  double c3[3];
  DISPATCH(h, row_weight_sums(c3));
  weights(s[2], s[3], c3[2], perc_met, &w, &nf);
  *score = (w * s[0] + s[1]) / nf;
  if (grad) {
    const double* gem = s.data() + 4;
    const double* gnm = gem + N * N;
    const double* pem = gnm + N * N;
    const double* pnm = pem + N;
    const double* mem_ = pnm + N;
    for (int e = 0; e < N * N; ++e) d_theta[e] = (w * gem[e] + gnm[e]) / nf;
    for (int i = 0; i < N; ++i) { d_dp[i] = (w * pem[i] + pnm[i]) / nf; d_dm[i] = w * mem_[i] / nf; }
  }
  API_END
}

int mmhn_score(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double perc_met,
               double* score) {
  return mmhn_score_and_grad(h, lt, ldp, ldm, perc_met, score, nullptr, nullptr, nullptr);
}

int mmhn_patient_grads(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double* lp,
                       double* d_theta, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && lp, "null pointer");
  const int N = h->n + 1, st = 1 + N * N + 2 * N;
  long long np = 0;
  if (h->dtype == MMHN_F64) np = static_cast<Engine<double>*>(h->impl)->n_pat;
  else np = static_cast<Engine<float>*>(h->impl)->n_pat;
  std::vector<double> rows((size_t)np * st), s(2 * st);
  const bool grad = d_theta != nullptr;
  DISPATCH(h, evaluate(lt, ldp, ldm, grad, s.data(), rows.data()));
  for (long long i = 0; i < np; ++i) {
    const double* r = rows.data() + (size_t)i * st;
    lp[i] = r[0];
    if (grad) {
      std::memcpy(d_theta + (size_t)i * N * N, r + 1, N * N * sizeof(double));
      if (d_dp) std::memcpy(d_dp + (size_t)i * N, r + 1 + N * N, N * sizeof(double));
      if (d_dm) std::memcpy(d_dm + (size_t)i * N, r + 1 + N * N + N, N * sizeof(double));
    }
  }
  API_END
}

int mmhn_patient_status(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double* lp, double* p_seeded) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && lp && p_seeded, "null pointer");
  DISPATCH(h, patient_status(lt, ldp, ldm, lp, p_seeded));
  API_END
}

int mmhn_get_unknown_rows(mmhn_handle h, int64_t* n_unknown) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_unknown, "null pointer");
  *n_unknown = unknown_rows(h);
  API_END
}

// ---- joint primitives
#define JOINT_DESC(state) make_joint(state, h->n)

int mmhn_kronvec(mmhn_handle h, const double* lt, const int8_t* state, const double* p, double* y, int diag,
                 int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_kronvec, d, p, y, diag != 0, transpose != 0);
  API_END
}
int mmhn_kronvec_batched(mmhn_handle h, const double* lt, const int8_t* state, int64_t batch, const double* p,
                         double* y, int diag, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  REQUIRE(batch >= 1, "batch must be positive");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_kronvec_batched, d, batch, p, y, diag != 0, transpose != 0);
  API_END
}
int mmhn_jacobi_step_batched(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, const int8_t* state,
                             int64_t batch, const double* p, const double* rhs, double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && state && p && rhs && y, "null pointer");
  REQUIRE(batch >= 1, "batch must be positive");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, ldp, ldm));
  DISPATCH_FN(h, api_jacobi_step_batched, d, batch, p, rhs, y, transpose != 0);
  API_END
}
int mmhn_kron_diag(mmhn_handle h, const double* lt, const int8_t* state, double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && out, "null pointer");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_diag, d, nullptr, out, KD_DQ);
  API_END
}
int mmhn_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p, double* y, int which) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_d && state && p && y, "null pointer");
  REQUIRE(which == 0 || which == 1, "which must be 0 (d_p) or 1 (d_m)");
  const Desc d = JOINT_DESC(state);
  REQUIRE(d.seedbit >= 0, "diag_scal needs an active seeding slot");
  const int N = h->n + 1;
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), which == 0 ? log_d : nullptr, which == 1 ? log_d : nullptr));
  DISPATCH_FN(h, api_diag, d, p, y, which == 0 ? KD_DP : KD_DM);
  API_END
}
int mmhn_obs_states(mmhn_handle h, const int8_t* state, int pt_first, int64_t* idx, int64_t* count) {
  API_BEGIN
  GUARD(h);
  REQUIRE(h && state && idx && count, "null pointer");
  obs_indices(JOINT_DESC(state), pt_first != 0, idx, count);
  API_END
}
int mmhn_resolvent(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, const int8_t* state,
                   const double* x, double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && state && x && y, "null pointer");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, ldp, ldm));
  DISPATCH_FN(h, api_resolvent, d, nullptr, x, y, transpose != 0);
  API_END
}
int mmhn_x_partial_Q_y(mmhn_handle h, const double* lt, const int8_t* state, const double* x, const double* y,
                       double* G) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y && G, "null pointer");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_xQy_joint, d, x, y, G);
  API_END
}
int mmhn_x_partial_D_y(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* x,
                       const double* y, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && x && y && d_dp && d_dm, "null pointer");
  const Desc d = JOINT_DESC(state);
  const int N = h->n + 1;
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), ldp, ldm));
  DISPATCH_FN(h, api_xDy_joint, d, x, y, d_dp, d_dm);
  API_END
}

int mmhn_partial_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p, int i, int which,
                           double* y) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_d && state && p && y, "null pointer");
  REQUIRE(which == 0 || which == 1, "which must be 0 (d_p) or 1 (d_m)");
  const int n = h->n, N = n + 1;
  REQUIRE(i >= 0 && i <= n, "event index out of range");
  const Desc d = JOINT_DESC(state);
  REQUIRE(d.seedbit >= 0, "partial_diag_scal needs an active seeding slot");
  // kronvec.py:632-644, :704-710: zero when the tumour's slot of event i is inactive; i == n: the seeding bit
  const int bit = i == n ? d.seedbit : (which == 0 ? d.bitP[i] : d.bitM[i]);
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), which == 0 ? log_d : nullptr, which == 1 ? log_d : nullptr));
  if (bit < 0) {
    std::memset(y, 0, sizeof(double) << d.k);
  } else {
    DISPATCH_FN(h, api_diag, d, p, y, which == 0 ? KD_DP : KD_DM, bit);
  }
  API_END
}

// ---- single-tumour primitives
int mmhn_v_kronvec(mmhn_handle h, const double* lt, const int8_t* state, const double* p, double* y, int diag,
                   int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_ONE);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_kronvec, d, p, y, diag != 0, transpose != 0);
  API_END
}
int mmhn_v_resolvent(mmhn_handle h, const double* lt, const int8_t* state, const double* d_rates, const double* x,
                     double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y, "null pointer");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_ONE);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_resolvent, d, d_rates, x, y, transpose != 0);
  API_END
}
int mmhn_v_x_partial_Q_y(mmhn_handle h, const double* lt, const int8_t* state, const double* x, const double* y,
                         double* G, double* d_diag) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y && G, "null pointer");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_ONE);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_xQy_single, d, x, y, G, d_diag);
  API_END
}

int mmhn_v_kron_diag(mmhn_handle h, const double* lt, const int8_t* state, const double* diag, double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && out, "null pointer");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_ONE);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  DISPATCH_FN(h, api_diag, d, diag, out, diag ? KD_QP : KD_DQ);
  API_END
}
int mmhn_v_scal_d_pt(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* vec,
                     double* out_p, double* out_m) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && vec && out_p && out_m, "null pointer");
  REQUIRE(state[h->n] == 1, "scal_d_pt needs the seeding event in the state (vanilla.py:142)");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_MET);
  const int N = h->n + 1;
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), ldp, ldm));
  DISPATCH_FN(h, api_diag, d, vec, out_p, KD_SDP);
  DISPATCH_FN(h, api_diag, d, vec, out_m, KD_DM);
  API_END
}
int mmhn_v_d_scal_d_pt(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* vec,
                       int i, double* out_p, double* out_m) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && vec && out_p && out_m, "null pointer");
  const int n = h->n, N = n + 1;
  REQUIRE(i >= 0 && i <= n, "event index out of range");
  REQUIRE(state[n] == 1, "d_scal_d_pt needs the seeding event in the state");
  const Desc d = make_single(state, n, PS_THETA, OBS_MET);
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), ldp, ldm));
  // vanilla.py:182-187: inactive event -> zeros; i == n -> (0, d_m part); otherwise both parts restricted to "i happened"
  if (d.bitP[i] < 0 || i == n) std::memset(out_p, 0, sizeof(double) << d.k);
  else DISPATCH_FN(h, api_diag, d, vec, out_p, KD_SDP, d.bitP[i]);
  if (d.bitP[i] < 0) std::memset(out_m, 0, sizeof(double) << d.k);
  else DISPATCH_FN(h, api_diag, d, vec, out_m, KD_DM, i == n ? -1 : d.bitP[i]);
  API_END
}
int mmhn_v_x_partial_D_y(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* x,
                         const double* y, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && x && y && d_dp && d_dm, "null pointer");
  REQUIRE(state[h->n] == 1, "x_partial_D_y needs the seeding event in the state");
  const Desc d = make_single(state, h->n, PS_THETA, OBS_MET);
  const int N = h->n + 1;
  std::vector<double> lt((size_t)N * N, 0.0);
  DISPATCH(h, build_params(lt.data(), ldp, ldm));
  DISPATCH_FN(h, api_xDy_single, d, x, y, d_dp, d_dm);
  API_END
}

// ---- patient shards on several GPUs: one RCCL communicator per engine
int mmhn_comm_unique_id(void* id128) {
  API_BEGIN
  REQUIRE(id128, "null pointer");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  RCCLCHECK(rccl().GetUniqueId(&id));
  std::memcpy(id128, &id, sizeof(id));
  API_END
}
int mmhn_comm_init(mmhn_handle h, const void* id128, int rank, int n_ranks) {
  API_BEGIN
  GUARD(h);
  REQUIRE(id128, "null pointer");
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  DISPATCH(h, comm_init(id, rank, n_ranks));
  API_END
}
int mmhn_comm_destroy(mmhn_handle h) {
  API_BEGIN
  GUARD(h);
  DISPATCH(h, comm_destroy());
  API_END
}

// ---- likeliest event orders of a cohort
int mmhn_likeliest_orders(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                          int64_t n_pat, int n_cols, int front_cap, int8_t* orders, double* prob, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && orders && prob && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "likeliest orders need an fp64 engine (MMHN_F64)");
  likeliest_orders(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, front_cap, orders, prob,
                                                         status);
  API_END
}

// ---- pre-seeding posteriors of a cohort: the sum over the orders mmhn_likeliest_orders maximises over
int mmhn_order_posteriors(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                          int64_t n_pat, int n_cols, double* log_evidence, double* pre, double* seed_pos, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && pre && seed_pos && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "order posteriors need an fp64 engine (MMHN_F64)");
  order_posteriors(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, log_evidence, pre,
                   seed_pos, status);
  API_END
}

// ---- pairwise precedence posteriors of a cohort: which of two events came first, over the same orders
int mmhn_order_precedences(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                           int64_t n_pat, int n_cols, double* log_evidence, double* prec, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && prec && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "order precedences need an fp64 engine (MMHN_F64)");
  order_precedences(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, log_evidence, prec,
                    status);
  API_END
}

// ---- posterior event positions of a cohort: where in its lineage every event happened, over the same orders
int mmhn_order_positions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                         int64_t n_pat, int n_cols, double* log_evidence, double* pos_pt, double* pos_mt, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && pos_pt && pos_mt && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "order positions need an fp64 engine (MMHN_F64)");
  order_positions(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, log_evidence, pos_pt,
                  pos_mt, status);
  API_END
}

// ---- posterior event and observation times of a cohort: when every event and observation happened, over the same orders
int mmhn_order_times(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                     int64_t n_pat, int n_cols, double* log_evidence, double* time, double* obs, double* pt_first,
                     int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && time && obs && pt_first && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "order times need an fp64 engine (MMHN_F64)");
  order_times(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, log_evidence, time, obs,
              pt_first, status);
  API_END
}

// ---- posterior genotypes at the first observation of a cohort's paired rows: what the two tumours held then, over the same orders
int mmhn_order_snapshots(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                         int64_t n_pat, int n_cols, double* log_evidence, double* held, double* late, int8_t* map_state,
                         int32_t* map_first, double* map_prob, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && held && late && map_state && map_first && map_prob && status,
          "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(h->dtype == MMHN_F64, "order snapshots need an fp64 engine (MMHN_F64)");
  order_snapshots(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, log_evidence, held, late,
                  map_state, map_first, map_prob, status);
  API_END
}

// ---- posterior samples of the event orders of a cohort: orders drawn with their exact probability given the row
int mmhn_order_samples(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                       int64_t n_pat, int n_cols, int64_t first, int64_t n_samples, uint64_t seed, double* log_evidence,
                       int8_t* orders, double* log_prob, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && status, "null pointer");
  REQUIRE(dat || n_pat == 0, "null dat");
  REQUIRE(n_pat >= 0 && n_pat < ((int64_t)1 << 31), "n_pat out of range");
  REQUIRE(first >= 0, "first must be non-negative");
  REQUIRE(n_samples >= 0 && n_samples < ((int64_t)1 << 31), "n_samples out of range");
  REQUIRE(n_samples <= INT64_MAX - first, "first + n_samples overflows 64 bits");
  REQUIRE((orders && log_prob) || n_samples == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "order samples need an fp64 engine (MMHN_F64)");
  order_samples(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, dat, n_pat, n_cols, first, n_samples, seed,
                log_evidence, orders, log_prob, status);
  API_END
}

// ---- seeding forecasts from a tumour's genotype: what comes before the seeding, how likely it is before the next look
int mmhn_seeding_forecasts(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes, int64_t n_rows,
                           int until, double* p_seed, double* time, double* before, double* with_seed, double* n_before,
                           int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows out of range");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && p_seed && time && before && with_seed && n_before && status) || n_rows == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "seeding forecasts need an fp64 engine (MMHN_F64)");
  seeding_forecasts(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, genotypes, n_rows, until, p_seed, time, before,
                    with_seed, n_before, status);
  API_END
}

// ---- seeding landscape: the forecast scalars of every genotype of the model from one backward sweep
int mmhn_seeding_landscape(mmhn_handle h, const double* log_theta, const double* obs1, int until, const int8_t* genotypes,
                           int64_t n_rows, double* values, int32_t* status, double* full) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows out of range");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "the seeding landscape needs an fp64 engine (MMHN_F64)");
  seeding_landscape(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, until, genotypes, n_rows, values, status, full);
  API_END
}

// ---- genotype distribution of the primary tumour: every genotype's probability, unseeded and seeded, from one forward sweep
int mmhn_genotype_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes,
                               int64_t n_rows, double* values, int32_t* status, double* summary, double* full) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows out of range");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "the genotype distribution needs an fp64 engine (MMHN_F64)");
  genotype_distribution(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, genotypes, n_rows, values, status, summary, full);
  API_END
}

// ---- genotype distribution of the metastasis and its founder: every genotype's Z, M, C from one forward sweep
int mmhn_metastasis_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                                 const int8_t* genotypes, int64_t n_rows, double* values, int32_t* status, double* summary,
                                 double* full) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows out of range");
  REQUIRE(log_theta && obs1 && obs2, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "the metastasis distribution needs an fp64 engine (MMHN_F64)");
  metastasis_distribution(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, genotypes, n_rows, values, status,
                          summary, full);
  API_END
}

// ---- genotype distribution of one tumour given the other: a row or column of the (PT x MT) table per query genotype
int mmhn_partner_distributions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int given,
                               const int8_t* genotypes, const int8_t* targets, int64_t n_rows, double* values,
                               int32_t* status, double* summaries, double* full) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_rows >= 0 && n_rows < ((int64_t)1 << 31), "n_rows out of range");
  REQUIRE(log_theta && obs1 && obs2, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "the partner distribution needs an fp64 engine (MMHN_F64)");
  partner_distributions(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, given, genotypes, targets, n_rows,
                        values, status, summaries, full);
  API_END
}

// ---- exact PT x MT co-occurrence and joint burden tables: the second moments of the (PT x MT) table through the founder
int mmhn_cross_table(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int with_burden,
                     double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && out, "null pointer");
  REQUIRE(h->dtype == MMHN_F64, "the cross table needs an fp64 engine (MMHN_F64)");
  cross_table(*static_cast<Engine<double>*>(h->impl), log_theta, obs1, obs2, with_burden != 0, out);
  API_END
}

// ---- Gillespie sampler
int mmhn_simulate(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t n_sim,
                  uint64_t seed, int8_t* dat_out, int8_t* orders_out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(h && lt && pt_d_ef && mt_d_ef && dat_out, "null pointer");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  const int N = h->n + 1;
  REQUIRE(N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate(h->impl->stream, lt, pt_d_ef, mt_d_ef, h->n, n_sim, seed, dat_out, orders_out);
  API_END
}

int mmhn_simulate_summary(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t first,
                          int64_t n_sim, uint64_t seed, int64_t* counts) {
  API_BEGIN
  GUARD(h);
  REQUIRE(h && lt && pt_d_ef && mt_d_ef && counts, "null pointer");
  REQUIRE(first >= 0, "first must be non-negative");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  REQUIRE(n_sim <= INT64_MAX - first, "first + n_sim overflows 64 bits");
  const int N = h->n + 1;
  REQUIRE(N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate_summary(h->impl->stream, h->impl->device, h->impl->cfg.sim_chunk, lt, pt_d_ef, mt_d_ef, h->n, first, n_sim, seed, counts);
  API_END
}

int mmhn_simulate_pairs(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t first,
                        int64_t n_sim, uint64_t seed, int64_t* n_class, int64_t* pairs, int64_t* burden) {
  API_BEGIN
  GUARD(h);
  REQUIRE(h && lt && pt_d_ef && mt_d_ef && n_class && pairs && burden, "null pointer");
  REQUIRE(first >= 0, "first must be non-negative");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  REQUIRE(n_sim <= INT64_MAX - first, "first + n_sim overflows 64 bits");
  const int N = h->n + 1;
  REQUIRE(N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate_pairs(h->impl->stream, h->impl->device, h->impl->cfg.sim_chunk, lt, pt_d_ef, mt_d_ef, h->n, first, n_sim, seed, n_class,
                 pairs, burden);
  API_END
}

// ---- measurement
int mmhn_bench_kronvec(mmhn_handle h, const double* lt, const int8_t* state, int64_t batch, int iters,
                       int transpose, int jacobi, double* ms_per_launch, int64_t* tiles) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && ms_per_launch, "null pointer");
  const Desc d = JOINT_DESC(state);
  DISPATCH(h, build_params(lt, nullptr, nullptr));
  long long tl[2] = {0, 0};
  if (h->dtype == MMHN_F64)
    *ms_per_launch = bench_kronvec(*static_cast<Engine<double>*>(h->impl), d, batch, iters, transpose != 0, jacobi != 0, tl);
  else
    *ms_per_launch = bench_kronvec(*static_cast<Engine<float>*>(h->impl), d, batch, iters, transpose != 0, jacobi != 0, tl);
  if (tiles) { tiles[0] = tl[0]; tiles[1] = tl[1]; }
  API_END
}
int mmhn_bench_stream(mmhn_handle h, size_t bytes, int iters, int kind, double* gbps) {
  API_BEGIN
  GUARD(h);
  REQUIRE(gbps, "null pointer");
  if (h->dtype == MMHN_F64) *gbps = bench_stream(*static_cast<Engine<double>*>(h->impl), bytes, iters, kind);
  else *gbps = bench_stream(*static_cast<Engine<float>*>(h->impl), bytes, iters, kind);
  API_END
}
#ifdef MMHN_STAMPS
// diagnostic builds only: shader cycles wave 0 of every k_psolve workgroup spent per phase ([0..7] forward, [8..15] adjoint)
int mmhn_debug_stamps(mmhn_handle h, double* out16, int reset) {
  API_BEGIN
  GUARD(h);
  unsigned long long v[16];
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_stamps), sizeof(v)));
  for (int i = 0; i < 16; ++i) out16[i] = (double)v[i];
  if (reset) { std::memset(v, 0, sizeof(v)); HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), v, sizeof(v))); }
  API_END
}
#endif
int mmhn_get_counters(mmhn_handle h, mmhn_counters* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(h && h->impl && out, "null pointer");
  if (h->dtype == MMHN_F64) *out = static_cast<Engine<double>*>(h->impl)->cnt;
  else *out = static_cast<Engine<float>*>(h->impl)->cnt;
  API_END
}
int mmhn_debug_lane_moves(mmhn_handle h, int transposed, int* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(out, "null pointer");
  DevArr<int> d;
  d.alloc(6 * 64);
  if (transposed) hipLaunchKernelGGL((k_lane_moves<true>), dim3(1), dim3(64), 0, h->impl->stream, d.p);
  else hipLaunchKernelGGL((k_lane_moves<false>), dim3(1), dim3(64), 0, h->impl->stream, d.p);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(out, d.p, 6 * 64 * sizeof(int), hipMemcpyDeviceToHost, h->impl->stream));
  HIPCHECK(hipStreamSynchronize(h->impl->stream));
  API_END
}

int mmhn_abi_version(void) { return MMHN_ABI_VERSION; }

int mmhn_reset_counters(mmhn_handle h) {
  API_BEGIN
  GUARD(h);
  DISPATCH(h, reset_counters());
  API_END
}

}  // extern "C"
