// The C ABI of include/metmhn_amd.h: every entry point checks its arguments, makes the engine's device current and calls
// the engine (engine.hip) or one of the host files around it.  Included last by engine.hip.
// An entry point that reads only what does not depend on the engine's dtype (EngineBase) uses h->impl; one that needs
// Engine<T> goes through with_engine, one that exists for fp64 alone through f64_engine.
#pragma once

using namespace mmhn;

struct mmhn_engine {
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

// f(E) with E the handle's Engine<double>& or Engine<float>& (behind GUARD(h)); returns what f returns
template <typename F>
static auto with_engine(mmhn_handle h, F&& f) {
  if (h->impl->dtype == MMHN_F64) return f(*static_cast<Engine<double>*>(h->impl));
  return f(*static_cast<Engine<float>*>(h->impl));
}
// the engine of an entry point that exists for fp64 alone; text: its refusal of an fp32 engine
static Engine<double>& f64_engine(mmhn_handle h, const char* text) {
  REQUIRE(h->impl->dtype == MMHN_F64, text);
  return *static_cast<Engine<double>*>(h->impl);
}
// a row count that the kernels index with 32 bits; name: "n_pat" / "n_rows"
static void count_in_range(int64_t count, const char* name) {
  REQUIRE(count >= 0 && count < ((int64_t)1 << 31), std::string(name) + " out of range");
}
// the rows of an order entry point
static void cohort_rows(const int8_t* dat, int64_t n_pat) {
  REQUIRE(dat || n_pat == 0, "null dat");
  count_in_range(n_pat, "n_pat");
}
// a single-problem primitive: the parameters (lt == nullptr: a zero log-theta, for the entry points that take observation
// rates only), then f(E)
template <typename F>
static void primitive(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, F&& f) {
  with_engine(h, [&](auto& E) { E.build_params(lt, ldp, ldm); f(E); });
}

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
  auto* h = new mmhn_engine{nullptr};
  try {
    if (dtype == MMHN_F64) h->impl = new Engine<double>(device_id, n_mut);
    else h->impl = new Engine<float>(device_id, n_mut);
  } catch (...) { delete h; throw; }
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
  with_engine(h, [&](auto& E) { E.set_cohort(dat, n_pat, n_cols); });
  API_END
}

// n_unknown: rows of dat type 4 - weight 1, outside the EM / NM balance (they ride in the NM sums)
static void weights(double n_em, double n_pat, double n_unknown, double perc_met, double* w, double* n_full) {
  const double n_nm = n_pat - n_em - n_unknown;           // regularized_optimization.py:121-128
  *w = (n_em * n_nm != 0) ? perc_met * n_nm / ((1 - perc_met) * n_em) : 1.0;
  *n_full = *w * n_em + n_nm + n_unknown;
}

int mmhn_set_row_weights(mmhn_handle h, const double* w, int64_t n) {
  API_BEGIN
  GUARD(h);
  with_engine(h, [&](auto& E) { set_row_weights(E, w, n); });
  API_END
}

int mmhn_get_row_weight_sums(mmhn_handle h, double* out3) {
  API_BEGIN
  GUARD(h);
  REQUIRE(out3, "null pointer");
  h->impl->row_weight_sums(out3);
  API_END
}

int mmhn_set_row_groups(mmhn_handle h, const int64_t* ptr, int64_t n_groups, const int64_t* rows, const double* w) {
  API_BEGIN
  GUARD(h);
  with_engine(h, [&](auto& E) { set_row_groups(E, ptr, n_groups, rows, w); });
  API_END
}

int mmhn_group_posteriors(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double* lp_group, double* rho) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && lp_group && rho, "null pointer");
  with_engine(h, [&](auto& E) { group_posteriors(E, lt, ldp, ldm, lp_group, rho); });
  API_END
}

int mmhn_cohort_sums(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad,
                     double* sums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && sums, "null pointer");
  with_engine(h, [&](auto& E) { E.cohort_sums(lt, ldp, ldm, with_grad != 0, sums); });
  API_END
}

int mmhn_cohort_sums_begin(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm, "null pointer");
  with_engine(h, [&](auto& E) { E.cohort_sums_begin(lt, ldp, ldm, with_grad != 0); });
  API_END
}

int mmhn_cohort_sums_end(mmhn_handle h, double* sums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(sums, "null pointer");
  with_engine(h, [&](auto& E) { E.cohort_sums_end(sums, E.full_len()); });
  API_END
}

int mmhn_cohort_wsums_begin(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, int with_grad, double w) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm, "null pointer");
  REQUIRE(std::isfinite(w), "w must be finite");
  with_engine(h, [&](auto& E) { E.cohort_sums_begin(lt, ldp, ldm, with_grad != 0, &w); });
  API_END
}

int mmhn_set_reduce_flag(mmhn_handle h, double value) {
  API_BEGIN
  GUARD(h);
  REQUIRE(std::isfinite(value), "the flag must be finite");
  h->impl->reduce_flag = value;
  API_END
}
int mmhn_get_reduce_flag(mmhn_handle h, double* summed) {
  API_BEGIN
  GUARD(h);
  REQUIRE(summed, "null pointer");
  *summed = h->impl->reduce_flag_sum;
  API_END
}

int mmhn_cohort_wsums_end(mmhn_handle h, double* wsums) {
  API_BEGIN
  GUARD(h);
  REQUIRE(wsums, "null pointer");
  with_engine(h, [&](auto& E) { E.cohort_sums_end(wsums, E.stride()); });
  API_END
}

int mmhn_score_and_grad(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, double perc_met,
                        double* score, double* d_theta, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && score, "null pointer");
  const int N = h->impl->N;
  const bool grad = d_theta && d_dp && d_dm;
  std::vector<double> s(h->impl->full_len());
  with_engine(h, [&](auto& E) { E.cohort_sums(lt, ldp, ldm, grad, s.data()); });
  double w, nf;
  weights(s[2], s[3], h->impl->counts().unknown, perc_met, &w, &nf);
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
  const int N = h->impl->N, st = h->impl->stride();
  const long long np = h->impl->n_pat;
  std::vector<double> rows((size_t)np * st), s(2 * st);
  const bool grad = d_theta != nullptr;
  with_engine(h, [&](auto& E) { E.evaluate(lt, ldp, ldm, grad, s.data(), rows.data()); });
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
  with_engine(h, [&](auto& E) { E.patient_status(lt, ldp, ldm, lp, p_seeded); });
  API_END
}

int mmhn_get_unknown_rows(mmhn_handle h, int64_t* n_unknown) {
  API_BEGIN
  GUARD(h);
  REQUIRE(n_unknown, "null pointer");
  *n_unknown = h->impl->n_unknown;
  API_END
}

// ---- joint primitives
// (an entry point that takes observation rates and no log-theta builds its parameters with lt = nullptr: a zero log-theta)
#define JOINT_DESC(state) make_joint(state, h->impl->n)

int mmhn_kronvec(mmhn_handle h, const double* lt, const int8_t* state, const double* p, double* y, int diag,
                 int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_kronvec(E, d, p, y, diag != 0, transpose != 0); });
  API_END
}
int mmhn_kronvec_batched(mmhn_handle h, const double* lt, const int8_t* state, int64_t batch, const double* p,
                         double* y, int diag, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  REQUIRE(batch >= 1, "batch must be positive");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_kronvec_batched(E, d, batch, p, y, diag != 0, transpose != 0); });
  API_END
}
int mmhn_jacobi_step_batched(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, const int8_t* state,
                             int64_t batch, const double* p, const double* rhs, double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && state && p && rhs && y, "null pointer");
  REQUIRE(batch >= 1, "batch must be positive");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, ldp, ldm, [&](auto& E) { api_jacobi_step_batched(E, d, batch, p, rhs, y, transpose != 0); });
  API_END
}
int mmhn_kron_diag(mmhn_handle h, const double* lt, const int8_t* state, double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && out, "null pointer");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_diag(E, d, nullptr, out, KD_DQ); });
  API_END
}
int mmhn_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p, double* y, int which) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_d && state && p && y, "null pointer");
  REQUIRE(which == 0 || which == 1, "which must be 0 (d_p) or 1 (d_m)");
  const Desc d = JOINT_DESC(state);
  REQUIRE(d.seedbit >= 0, "diag_scal needs an active seeding slot");
  primitive(h, nullptr, which == 0 ? log_d : nullptr, which == 1 ? log_d : nullptr,
            [&](auto& E) { api_diag(E, d, p, y, which == 0 ? KD_DP : KD_DM); });
  API_END
}
int mmhn_obs_states(mmhn_handle h, const int8_t* state, int pt_first, int64_t* idx, int64_t* count) {
  API_BEGIN
  GUARD(h);
  REQUIRE(state && idx && count, "null pointer");
  obs_indices(JOINT_DESC(state), pt_first != 0, idx, count);
  API_END
}
int mmhn_resolvent(mmhn_handle h, const double* lt, const double* ldp, const double* ldm, const int8_t* state,
                   const double* x, double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && ldp && ldm && state && x && y, "null pointer");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, ldp, ldm, [&](auto& E) { api_resolvent(E, d, nullptr, x, y, transpose != 0); });
  API_END
}
int mmhn_x_partial_Q_y(mmhn_handle h, const double* lt, const int8_t* state, const double* x, const double* y,
                       double* G) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y && G, "null pointer");
  const Desc d = JOINT_DESC(state);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_xQy_joint(E, d, x, y, G); });
  API_END
}
int mmhn_x_partial_D_y(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* x,
                       const double* y, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && x && y && d_dp && d_dm, "null pointer");
  const Desc d = JOINT_DESC(state);
  primitive(h, nullptr, ldp, ldm, [&](auto& E) { api_xDy_joint(E, d, x, y, d_dp, d_dm); });
  API_END
}

int mmhn_partial_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p, int i, int which,
                           double* y) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_d && state && p && y, "null pointer");
  REQUIRE(which == 0 || which == 1, "which must be 0 (d_p) or 1 (d_m)");
  const int n = h->impl->n;
  REQUIRE(i >= 0 && i <= n, "event index out of range");
  const Desc d = JOINT_DESC(state);
  REQUIRE(d.seedbit >= 0, "partial_diag_scal needs an active seeding slot");
  // kronvec.py:632-644, :704-710: zero when the tumour's slot of event i is inactive; i == n: the seeding bit
  const int bit = i == n ? d.seedbit : (which == 0 ? d.bitP[i] : d.bitM[i]);
  primitive(h, nullptr, which == 0 ? log_d : nullptr, which == 1 ? log_d : nullptr, [&](auto& E) {
    if (bit < 0) std::memset(y, 0, sizeof(double) << d.k);
    else api_diag(E, d, p, y, which == 0 ? KD_DP : KD_DM, bit);
  });
  API_END
}

// ---- single-tumour primitives
int mmhn_v_kronvec(mmhn_handle h, const double* lt, const int8_t* state, const double* p, double* y, int diag,
                   int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && p && y, "null pointer");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_ONE);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_kronvec(E, d, p, y, diag != 0, transpose != 0); });
  API_END
}
int mmhn_v_resolvent(mmhn_handle h, const double* lt, const int8_t* state, const double* d_rates, const double* x,
                     double* y, int transpose) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y, "null pointer");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_ONE);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_resolvent(E, d, d_rates, x, y, transpose != 0); });
  API_END
}
int mmhn_v_x_partial_Q_y(mmhn_handle h, const double* lt, const int8_t* state, const double* x, const double* y,
                         double* G, double* d_diag) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && x && y && G, "null pointer");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_ONE);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_xQy_single(E, d, x, y, G, d_diag); });
  API_END
}

int mmhn_v_kron_diag(mmhn_handle h, const double* lt, const int8_t* state, const double* diag, double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && state && out, "null pointer");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_ONE);
  primitive(h, lt, nullptr, nullptr, [&](auto& E) { api_diag(E, d, diag, out, diag ? KD_QP : KD_DQ); });
  API_END
}
int mmhn_v_scal_d_pt(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* vec,
                     double* out_p, double* out_m) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && vec && out_p && out_m, "null pointer");
  REQUIRE(state[h->impl->n] == 1, "scal_d_pt needs the seeding event in the state (vanilla.py:142)");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_MET);
  primitive(h, nullptr, ldp, ldm, [&](auto& E) { api_diag(E, d, vec, out_p, KD_SDP); api_diag(E, d, vec, out_m, KD_DM); });
  API_END
}
int mmhn_v_d_scal_d_pt(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* vec,
                       int i, double* out_p, double* out_m) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && vec && out_p && out_m, "null pointer");
  const int n = h->impl->n;
  REQUIRE(i >= 0 && i <= n, "event index out of range");
  REQUIRE(state[n] == 1, "d_scal_d_pt needs the seeding event in the state");
  const Desc d = make_single(state, n, PS_THETA, OBS_MET);
  primitive(h, nullptr, ldp, ldm, [&](auto& E) {
    // vanilla.py:182-187: inactive event -> zeros; i == n -> (0, d_m part); otherwise both parts restricted to "i happened"
    if (d.bitP[i] < 0 || i == n) std::memset(out_p, 0, sizeof(double) << d.k);
    else api_diag(E, d, vec, out_p, KD_SDP, d.bitP[i]);
    if (d.bitP[i] < 0) std::memset(out_m, 0, sizeof(double) << d.k);
    else api_diag(E, d, vec, out_m, KD_DM, i == n ? -1 : d.bitP[i]);
  });
  API_END
}
int mmhn_v_x_partial_D_y(mmhn_handle h, const double* ldp, const double* ldm, const int8_t* state, const double* x,
                         const double* y, double* d_dp, double* d_dm) {
  API_BEGIN
  GUARD(h);
  REQUIRE(ldp && ldm && state && x && y && d_dp && d_dm, "null pointer");
  REQUIRE(state[h->impl->n] == 1, "x_partial_D_y needs the seeding event in the state");
  const Desc d = make_single(state, h->impl->n, PS_THETA, OBS_MET);
  primitive(h, nullptr, ldp, ldm, [&](auto& E) { api_xDy_single(E, d, x, y, d_dp, d_dm); });
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
  h->impl->comm_init(id, rank, n_ranks);
  API_END
}
int mmhn_comm_destroy(mmhn_handle h) {
  API_BEGIN
  GUARD(h);
  h->impl->comm_destroy();
  API_END
}

// ---- likeliest event orders of a cohort
int mmhn_likeliest_orders(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                          int64_t n_pat, int n_cols, int front_cap, int8_t* orders, double* prob, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && orders && prob && status, "null pointer");
  cohort_rows(dat, n_pat);
  likeliest_orders(f64_engine(h, "likeliest orders need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
                   front_cap, orders, prob, status);
  API_END
}

// ---- pre-seeding posteriors of a cohort: the sum over the orders mmhn_likeliest_orders maximises over
int mmhn_order_posteriors(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                          int64_t n_pat, int n_cols, double* log_evidence, double* pre, double* seed_pos, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && pre && seed_pos && status, "null pointer");
  cohort_rows(dat, n_pat);
  order_posteriors(f64_engine(h, "order posteriors need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
                   log_evidence, pre, seed_pos, status);
  API_END
}

// ---- pairwise precedence posteriors of a cohort: which of two events came first, over the same orders
int mmhn_order_precedences(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                           int64_t n_pat, int n_cols, double* log_evidence, double* prec, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && prec && status, "null pointer");
  cohort_rows(dat, n_pat);
  order_precedences(f64_engine(h, "order precedences need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
                    log_evidence, prec, status);
  API_END
}

// ---- posterior event positions of a cohort: where in its lineage every event happened, over the same orders
int mmhn_order_positions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                         int64_t n_pat, int n_cols, double* log_evidence, double* pos_pt, double* pos_mt, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && pos_pt && pos_mt && status, "null pointer");
  cohort_rows(dat, n_pat);
  order_positions(f64_engine(h, "order positions need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
                  log_evidence, pos_pt, pos_mt, status);
  API_END
}

// ---- posterior event and observation times of a cohort: when every event and observation happened, over the same orders
int mmhn_order_times(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                     int64_t n_pat, int n_cols, double* log_evidence, double* time, double* obs, double* pt_first,
                     int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && time && obs && pt_first && status, "null pointer");
  cohort_rows(dat, n_pat);
  order_times(f64_engine(h, "order times need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
              log_evidence, time, obs, pt_first, status);
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
  cohort_rows(dat, n_pat);
  order_snapshots(f64_engine(h, "order snapshots need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols,
                  log_evidence, held, late, map_state, map_first, map_prob, status);
  API_END
}

// ---- posterior samples of the event orders of a cohort: orders drawn with their exact probability given the row
int mmhn_order_samples(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                       int64_t n_pat, int n_cols, int64_t first, int64_t n_samples, uint64_t seed, double* log_evidence,
                       int8_t* orders, double* log_prob, int32_t* status) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && log_evidence && status, "null pointer");
  cohort_rows(dat, n_pat);
  REQUIRE(first >= 0, "first must be non-negative");
  count_in_range(n_samples, "n_samples");
  REQUIRE(n_samples <= INT64_MAX - first, "first + n_samples overflows 64 bits");
  REQUIRE((orders && log_prob) || n_samples == 0, "null pointer");
  order_samples(f64_engine(h, "order samples need an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, dat, n_pat, n_cols, first,
                n_samples, seed, log_evidence, orders, log_prob, status);
  API_END
}

// ---- seeding forecasts from a tumour's genotype: what comes before the seeding, how likely it is before the next look
int mmhn_seeding_forecasts(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes, int64_t n_rows,
                           int until, double* p_seed, double* time, double* before, double* with_seed, double* n_before,
                           int32_t* status) {
  API_BEGIN
  GUARD(h);
  count_in_range(n_rows, "n_rows");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && p_seed && time && before && with_seed && n_before && status) || n_rows == 0, "null pointer");
  seeding_forecasts(f64_engine(h, "seeding forecasts need an fp64 engine (MMHN_F64)"), log_theta, obs1, genotypes, n_rows, until,
                    p_seed, time, before, with_seed, n_before, status);
  API_END
}

// ---- seeding landscape: the forecast scalars of every genotype of the model from one backward sweep
int mmhn_seeding_landscape(mmhn_handle h, const double* log_theta, const double* obs1, int until, const int8_t* genotypes,
                           int64_t n_rows, double* values, int32_t* status, double* full) {
  API_BEGIN
  GUARD(h);
  count_in_range(n_rows, "n_rows");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  seeding_landscape(f64_engine(h, "the seeding landscape needs an fp64 engine (MMHN_F64)"), log_theta, obs1, until, genotypes,
                    n_rows, values, status, full);
  API_END
}

// ---- genotype distribution of the primary tumour: every genotype's probability, unseeded and seeded, from one forward sweep
int mmhn_genotype_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes,
                               int64_t n_rows, double* values, int32_t* status, double* summary, double* full) {
  API_BEGIN
  GUARD(h);
  count_in_range(n_rows, "n_rows");
  REQUIRE(log_theta && obs1, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  genotype_distribution(f64_engine(h, "the genotype distribution needs an fp64 engine (MMHN_F64)"), log_theta, obs1, genotypes,
                        n_rows, values, status, summary, full);
  API_END
}

// ---- genotype distribution of the metastasis and its founder: every genotype's Z, M, C from one forward sweep
int mmhn_metastasis_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                                 const int8_t* genotypes, int64_t n_rows, double* values, int32_t* status, double* summary,
                                 double* full) {
  API_BEGIN
  GUARD(h);
  count_in_range(n_rows, "n_rows");
  REQUIRE(log_theta && obs1 && obs2, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  metastasis_distribution(f64_engine(h, "the metastasis distribution needs an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2,
                          genotypes, n_rows, values, status, summary, full);
  API_END
}

// ---- genotype distribution of one tumour given the other: a row or column of the (PT x MT) table per query genotype
int mmhn_partner_distributions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int given,
                               const int8_t* genotypes, const int8_t* targets, int64_t n_rows, double* values,
                               int32_t* status, double* summaries, double* full) {
  API_BEGIN
  GUARD(h);
  count_in_range(n_rows, "n_rows");
  REQUIRE(log_theta && obs1 && obs2, "null pointer");
  REQUIRE((genotypes && values && status) || n_rows == 0, "null pointer");
  partner_distributions(f64_engine(h, "the partner distribution needs an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, given,
                        genotypes, targets, n_rows, values, status, summaries, full);
  API_END
}

// ---- exact PT x MT co-occurrence and joint burden tables: the second moments of the (PT x MT) table through the founder
int mmhn_cross_table(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int with_burden,
                     double* out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(log_theta && obs1 && obs2 && out, "null pointer");
  cross_table(f64_engine(h, "the cross table needs an fp64 engine (MMHN_F64)"), log_theta, obs1, obs2, with_burden != 0, out);
  API_END
}

// ---- Gillespie sampler
int mmhn_simulate(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t n_sim,
                  uint64_t seed, int8_t* dat_out, int8_t* orders_out) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && pt_d_ef && mt_d_ef && dat_out, "null pointer");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  REQUIRE(h->impl->N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate(h->impl->stream, lt, pt_d_ef, mt_d_ef, h->impl->n, n_sim, seed, dat_out, orders_out);
  API_END
}

int mmhn_simulate_summary(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t first,
                          int64_t n_sim, uint64_t seed, int64_t* counts) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && pt_d_ef && mt_d_ef && counts, "null pointer");
  REQUIRE(first >= 0, "first must be non-negative");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  REQUIRE(n_sim <= INT64_MAX - first, "first + n_sim overflows 64 bits");
  REQUIRE(h->impl->N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate_summary(h->impl->stream, h->impl->device, h->impl->cfg.sim_chunk, lt, pt_d_ef, mt_d_ef, h->impl->n, first, n_sim, seed, counts);
  API_END
}

int mmhn_simulate_pairs(mmhn_handle h, const double* lt, const double* pt_d_ef, const double* mt_d_ef, int64_t first,
                        int64_t n_sim, uint64_t seed, int64_t* n_class, int64_t* pairs, int64_t* burden) {
  API_BEGIN
  GUARD(h);
  REQUIRE(lt && pt_d_ef && mt_d_ef && n_class && pairs && burden, "null pointer");
  REQUIRE(first >= 0, "first must be non-negative");
  REQUIRE(n_sim >= 0, "n_sim must be non-negative");
  REQUIRE(n_sim <= INT64_MAX - first, "first + n_sim overflows 64 bits");
  REQUIRE(h->impl->N < SIM_MAXN, "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)");
  simulate_pairs(h->impl->stream, h->impl->device, h->impl->cfg.sim_chunk, lt, pt_d_ef, mt_d_ef, h->impl->n, first, n_sim, seed, n_class,
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
  long long tl[2] = {0, 0};
  *ms_per_launch = with_engine(h, [&](auto& E) {
    E.build_params(lt, nullptr, nullptr);
    return bench_kronvec(E, d, batch, iters, transpose != 0, jacobi != 0, tl);
  });
  if (tiles) { tiles[0] = tl[0]; tiles[1] = tl[1]; }
  API_END
}
int mmhn_bench_stream(mmhn_handle h, size_t bytes, int iters, int kind, double* gbps) {
  API_BEGIN
  GUARD(h);
  REQUIRE(gbps, "null pointer");
  *gbps = with_engine(h, [&](auto& E) { return bench_stream(E, bytes, iters, kind); });
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
  REQUIRE(out, "null pointer");
  *out = h->impl->cnt;
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
  h->impl->reset_counters();
  API_END
}

}  // extern "C"
