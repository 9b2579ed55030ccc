/*
 * metmhn_amd C ABI - MI355X (gfx950) likelihood / gradient engine for metMHN.
 *
 * The reference (cbg-ethz/metMHN @ 2024_08_07) has no FFI layer: its boundary is the
 * Python call surface of metmhn/regularized_optimization.py and metmhn/jx/{kronvec,likelihood,vanilla}.py.  Every
 * entry point below replaces one of those Python functions; the ctypes binding lives in
 * metmhn_amd/_lib.py and the reference-side stub a maintainer would add is shown in
 * INTEGRATION.md.  All pointers are caller-owned HOST buffers, row-major, fp64 at the
 * interface whatever the engine's internal dtype; every function returns 0 on success
 * and a non-zero status otherwise (message: mmhn_last_error(), thread-local).  A handle
 * is bound to one GPU and is not thread-safe (the reference is single-threaded:
 * scipy.optimize.minimize calls score_and_grad_reg synchronously,
 * regularized_optimization.py:328-330).
 *
 * Layout conventions (regularized_optimization.py:63-66, metmhn/jx/kronvec.py:223-250):
 *   dat    int8 [n_pat][2n+3]  = PT_0,MT_0,...,PT_{n-1},MT_{n-1},seed, order, type
 *          type 0 "absent", 1 "present", 2 "isMetastasis", 3 "isPaired" as in the reference, and
 *          type 4: a primary tumour was sequenced and its metastatic status is unknown.  PT columns 0 / 1; every MT column and
 *          the seeding column must be 0 (mmhn_set_cohort refuses the cohort otherwise, naming the row); the order column is
 *          ignored.  With lp0 the log-probability of the same genotype as a type-0 row and lp1 as a type-1 row with seeding = 1,
 *          the row's lp = logaddexp(lp0, lp1), P(seeded | genotype) = exp(lp1 - lp), and its gradient is the mixture of the two
 *          rows' gradients under those posterior weights (d_dm = 0).  In the objective a type-4 row has weight 1: n_em (the sum
 *          of the seeding column) is not changed by it, n_nm = n_pat - n_em - n_unknown, w as before from n_em and n_nm,
 *          n_full = w n_em + n_nm + n_unknown, and its lp and gradient ride in the "NM" sums below.
 *          The mmhn_order_* / mmhn_likeliest_orders entry points take types 0..3 only: a type-4 row gets MMHN_ORD_BAD_STATUS
 *          there, filter such rows out first.
 *   state  int8 [2n+1]  joint observation;  [n+1] for the single-tumour functions
 *   vectors have 2^k entries, k = #ones in state; index bit b <-> b-th active slot.
 *   log_theta fp64 [n+1][n+1], log_d_p / log_d_m fp64 [n+1].
 *
 * Size limits (every one is checked on the host before anything is launched; the text is mmhn_last_error()):
 *   n_mut in [1, 31] for the engine, the single-vector functions and the mmhn_order_* / mmhn_likeliest_orders entry points:
 *     mmhn_create fails with "n_mut must be in [1, 31]".
 *   n_mut <= 30 for mmhn_simulate, mmhn_simulate_summary and mmhn_simulate_pairs; on an engine with n_mut = 31 they fail with
 *     "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)".
 *   At most 30 active slots (index bits) in any one restricted space.  For a row of dat that is its joint space (type 3: PT
 *     slots + MT slots + seeding) or its single-tumour space (types 0 / 1: PT slots + seeding, type 2: MT slots + seeding,
 *     type 4: PT slots + 1 - the message then ends with " (row R)"):
 *     mmhn_set_cohort fails with "too many active events for one patient" and leaves the engine without a cohort.  For a
 *     state of the single-vector functions: "too many active events".  The order entry points give such a row the status
 *     MMHN_ORD_TOO_LARGE.
 *   Verified sizes: spaces of up to 30 bits are accepted; the largest ones a test compares with a reference have k = 27
 *     (fp32 window route), k = 26 (tile route, fp64) and k = 25 (fp64 window route, both class sizes at their maximum), and
 *     n_mut = 31 is compared with small spaces (k <= 20).  Nothing above k = 27 has been compared with a reference: a vector
 *     of a 30-bit space is 8 GB per argument of the single-vector interface, and the CPU reference needs tens of seconds and
 *     tens of GB for one such row.
 */
#ifndef METMHN_AMD_H
#define METMHN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmhn_engine* mmhn_handle;

enum { MMHN_F64 = 0, MMHN_F32 = 1 };

/* ---- lifetime ------------------------------------------------------------------- */
int mmhn_create(int device_id, int n_mut, int dtype, mmhn_handle* out);
void mmhn_destroy(mmhn_handle h);
const char* mmhn_last_error(void);
/* upper bound on device workspace used per batch of patients (default: 70 % of free HBM) */
int mmhn_set_workspace_limit(mmhn_handle h, size_t bytes);

/* ---- cohort objective -------------------------------------------------------------
 * mmhn_set_cohort copies `dat`, derives every patient's bit layout and batches once.
 * mmhn_score            <-> regularized_optimization.score           (:55-130)
 * mmhn_score_and_grad   <-> regularized_optimization.score_and_grad  (:163-267)
 * mmhn_cohort_sums returns the UNWEIGHTED partial sums of this handle's patients so that
 * patient shards on several GPUs can be combined with one all-reduce:
 *   sums[0]            = sum of log-probs of the rows with type != 0 ("EM")
 *   sums[1]            = sum of log-probs of the rows with type == 0 ("NM") and of those with type == 4 (weight 1 as well)
 *   sums[2]            = number of rows with seeding == 1,  sums[3] = number of rows (type 4 included: mmhn_get_unknown_rows
 *                        says how many of them are)
 *   then d_theta_EM [N*N], d_theta_NM [N*N], d_dp_EM [N], d_dp_NM [N], d_dm_EM [N]
 * (N = n_mut + 1; 4 + 2*N*N + 3*N doubles; gradient blocks are zero if with_grad == 0).
 */
int mmhn_set_cohort(mmhn_handle h, const int8_t* dat, int64_t n_pat, int n_cols);
int mmhn_score(mmhn_handle h, const double* log_theta, const double* log_d_p, const double* log_d_m,
               double perc_met, double* score);
int mmhn_score_and_grad(mmhn_handle h, const double* log_theta, const double* log_d_p,
                        const double* log_d_m, double perc_met, double* score, double* d_theta,
                        double* d_dp, double* d_dm);
int mmhn_cohort_sums(mmhn_handle h, const double* log_theta, const double* log_d_p,
                     const double* log_d_m, int with_grad, double* sums);
/* The same in two halves: _begin issues the evaluation (and the all-reduce) and returns without waiting - the
 * parameter arrays may be reused at once -, _end waits and delivers.  In between the caller is free to do host work: the
 * reference computes its penalty terms on the host after the score (regularized_optimization.py:292-298), here they run
 * next to the GPU.  One evaluation in flight per handle. */
int mmhn_cohort_sums_begin(mmhn_handle h, const double* log_theta, const double* log_d_p,
                           const double* log_d_m, int with_grad);
int mmhn_cohort_sums_end(mmhn_handle h, double* sums);
/* The same evaluation with the EM / NM weighting of regularized_optimization.py:256-266 applied on the device:
 * wsums[1 + N*N + 2 N] = [w s_EM + s_NM, w G_EM + G_NM, w p_EM + p_NM, w m_EM]; the caller divides by
 * n_full = w n_em + n_nm (+ n_unknown, the rows of type 4, which ride in the NM terms).  w needs the GLOBAL counts only (known to every rank once the cohort is set), so with a
 * communicator attached the all-reduce carries 1 + N^2 + 2 N doubles (484 at n = 20). */
int mmhn_cohort_wsums_begin(mmhn_handle h, const double* log_theta, const double* log_d_p,
                            const double* log_d_m, int with_grad, double w);
int mmhn_cohort_wsums_end(mmhn_handle h, double* wsums);
/* One more double riding in the SAME all-reduce as the wsums buffer (ABI 5): the value set here travels with the NEXT
 * mmhn_cohort_wsums_begin, is summed over the ranks of the communicator, and is read back after its _end.  That call
 * takes the value (it is 0 again for the one after it), whether or not its evaluation succeeds; calls in between that are
 * no mmhn_cohort_wsums_begin - mmhn_cohort_sums, mmhn_cohort_sums_begin, mmhn_patient_grads - leave it where it is, and so
 * does a _begin that is refused because an evaluation is still pending.  After the _end of a plain
 * mmhn_cohort_sums_begin, mmhn_get_reduce_flag reads 0.  The Python host
 * uses it for the "this rank's cohort array was edited in place" bit of its layout cache, which used to be a second
 * collective per evaluation (metmhn_amd/regularized_optimization.py: _result). */
int mmhn_set_reduce_flag(mmhn_handle h, double value);
int mmhn_get_reduce_flag(mmhn_handle h, double* summed);
/* per-patient results of the current cohort (tests): lp[n_pat], and if non-NULL
 * d_theta[n_pat][N*N], d_dp[n_pat][N], d_dm[n_pat][N]  (ssr._g_coupled_*, _grad_*_obs) */
int mmhn_patient_grads(mmhn_handle h, const double* log_theta, const double* log_d_p,
                       const double* log_d_m, double* lp, double* d_theta, double* d_dp, double* d_dm);

/* score-only evaluation of the current cohort: lp[n_pat] of every row, p_seeded[n_pat] = P(the metastasis had been seeded |
 * PT genotype) for the rows of type 4 and NaN for every other row */
int mmhn_patient_status(mmhn_handle h, const double* log_theta, const double* log_d_p, const double* log_d_m,
                        double* lp, double* p_seeded);
/* rows of type 4 in the cohort the handle was given (this handle's shard: mmhn_score / mmhn_score_and_grad use it for
 * n_full, so with a communicator attached and type-4 rows present weight the all-reduced sums yourself from the global
 * counts - mmhn_cohort_wsums_begin) */
int mmhn_get_unknown_rows(mmhn_handle h, int64_t* n_unknown);

/* ---- per-row weights of the cohort objective (additive: the ABI version is unchanged) ----------------------------------
 * mmhn_set_row_weights gives row i of the current cohort the weight w[i] >= 0 (finite, not all zero; n = the cohort's row
 * count).  With weights set every cohort sum is the weighted sum of the per-row values v_i (lp, or an element of the
 * gradient row):
 *   S_EM = sum_{i in EM} w_i v_i      S_NM = sum_{i in NM or type 4} w_i v_i
 *   n_em = sum_i w_i [seeding == 1]   n_pat = sum_i w_i   n_unknown = sum_i w_i [type == 4]
 * and mmhn_score, mmhn_score_and_grad and slots [2], [3] of the mmhn_cohort_sums buffer use these real-valued counts in the
 * place of the integer ones.  For integer weights this is the objective of the cohort in which row i is written w_i times.
 * A row of weight 0 contributes exactly nothing, to the sums and to the counts: it is selected out, not multiplied by 0
 * (it is still solved: dropping it would need a new plan).  The plan, the solves and the per-row values do not change;
 * mmhn_patient_grads and mmhn_patient_status stay per row and UNWEIGHTED.
 * w == NULL removes the weights (n is ignored), and so does every mmhn_set_cohort.  The call is refused - the message of
 * mmhn_last_error names the first offending row, the weights held before stay - for a wrong n, a negative or non-finite
 * entry, an all-zero vector, an engine without cohort rows, and between a _begin and its _end.  The weights go to the device
 * here, once: an evaluation does no extra upload and no extra synchronisation, and without weights it launches what it
 * launched before this entry point existed. */
int mmhn_set_row_weights(mmhn_handle h, const double* w, int64_t n);
/* out3 = [n_em, n_pat, n_unknown] as defined above (this handle's shard), summed on the host in row order - exact for dyadic
 * weights; the integer counts of the cohort when no weights are set */
int mmhn_get_row_weight_sums(mmhn_handle h, double* out3);

/* ---- row groups: cohort rows as alternatives of one patient (additive: the ABI version is unchanged) -------------------
 * A row with m unobserved entries has the likelihood of the sum of its 2^m completions, each an ordinary cohort row.
 * mmhn_set_row_groups makes group g the list rows[ptr[g] .. ptr[g+1]) of row indices of the current cohort, with the weight
 * w[g] >= 0 (n_groups + 1 entries of ptr, ptr[n_groups] of rows, n_groups of w).  With groups set
 *   lp_g = log sum_{r in g} exp(lp_r)        rho_{g,r} = exp(lp_r - lp_g)
 *   sum of element 0      = sum_g w_g lp_g
 *   sum of element e >= 1 = sum_g w_g sum_{r in g} rho_{g,r} v_r[e]            (v_r: the row's gradient row)
 * in each of the two blocks (EM; NM with type 4), and the counts are the group-weighted ones: n_pat = sum_g w_g, n_em over the
 * groups whose rows have seeding = 1, n_unknown over the groups of type-4 rows (mmhn_get_row_weight_sums returns them;
 * mmhn_score, mmhn_score_and_grad and slots [2], [3] of mmhn_cohort_sums use them).  The groups enter only in the cohort
 * reduction, in fp64 whatever the engine's dtype: per row omega_r = sum_g w_g rho_{g,r} and lambda_r = sum_g w_g rho_{g,r} lp_g
 * over the groups that hold r, then the reduction of the row weights with the addend omega_r v_r[e] (lambda_r for e = 0).
 * Plan, solves and per-row values do not change: mmhn_patient_grads and mmhn_patient_status stay per row and UNMIXED.
 * A row may be in any number of groups.  A row in no group, or only in groups of weight 0, is absent - selected out, its values
 * may be anything - but it is still solved.  A cohort of several batches with a gradient is evaluated in two sweeps (a
 * score-only one first: a group may span batches and lp_g must be known before a row is added).
 * n_groups == 0 or null pointers remove the groups, and so does every mmhn_set_cohort.  The call is refused - the message
 * names the first offending group or row, what was held before stays - for: ptr not non-decreasing from 0; an empty group;
 * a row index outside the cohort; a negative or non-finite weight; all weights zero; a group whose rows are not all in one
 * block of the sums (types 1-3, or types 0 and 4) or do not agree in "is type 4"; a call between a _begin and its _end; an
 * engine without cohort rows; an engine that holds row weights (and mmhn_set_row_weights is refused while groups are held:
 * the group weights take the role of the row weights); a communicator of more than one rank (sharding cuts through groups).
 * Limits: one rank; rows of weight 0 or in no group are still solved; the cost of m unobserved entries is 2^m rows (the Python
 * layer's Utilityfunctions.expand_missing builds the groups and refuses a row with more than max_alternatives = 1024 of them).
 * Without groups an evaluation launches what it launched before these entry points existed. */
int mmhn_set_row_groups(mmhn_handle h, const int64_t* ptr, int64_t n_groups, const int64_t* rows, const double* w);
/* a score-only evaluation: lp_group[g] = lp_g, rho[ptr[g] + s] = rho of the s-th alternative of group g (also of groups of
 * weight 0) */
int mmhn_group_posteriors(mmhn_handle h, const double* log_theta, const double* log_d_p, const double* log_d_m,
                          double* lp_group, double* rho);

/* ---- joint PT/MT primitives (metmhn/jx/kronvec.py, likelihood.py) ------------------
 * mmhn_kronvec        <-> kronvec.kronvec        (:499-539)   y = Q p, flags diag / transpose
 * mmhn_kron_diag      <-> kronvec.kron_diag      (:964-999)
 * mmhn_diag_scal      <-> kronvec.diag_scal_p/m  (:574-602, :646-671)  which: 0 = p, 1 = m
 * mmhn_obs_states     <-> kronvec.obs_states + jnp.where(size=) (:1056-1095, likelihood.py:280)
 *                         ascending compatible indices; *count receives how many
 * mmhn_resolvent      <-> likelihood.R_i_inv_vec (:231-262)   (D_p + D_m - Q)^-1 x
 * mmhn_x_partial_Q_y  <-> likelihood.x_partial_Q_y (:163-201) G[N][N]
 * mmhn_x_partial_D_y  <-> likelihood.x_partial_D_y (:204-228) (takes log_d_p, log_d_m in THAT order)
 * mmhn_partial_diag_scal <-> kronvec.partial_diag_scal_p / _m (:605-644, :674-710): (dD/dlog d[i]) * p,
 *                         which: 0 = p, 1 = m; i in [0, n_mut] (n_mut = the seeding entry)
 * mmhn_kronvec_batched: the same product for `batch` vectors p[b][2^k] of ONE restricted space (what a vmapped
 *   kronvec.kronvec does; SURVEY 8b "+ _batched"): one launch over every tile of every vector into y[b][2^k].  The
 *   device output starts as a NaN pattern and is written completely by that launch (tiles where Q_off has no entries
 *   are zeroed inside it) - it is the launch sequence mmhn_bench_kronvec times.
 */
int mmhn_kronvec_batched(mmhn_handle h, const double* log_theta, const int8_t* state, int64_t batch, const double* p,
                         double* y, int diag, int transpose);
/* one sweep of likelihood.R_i_inv_vec's Jacobi iteration (likelihood.py:253-255), batched as above:
 * y[b] = lidg * (Q_off p[b] + rhs[b]) (transpose: Q_off^T), lidg = 1 / (D_p + D_m - diag Q); the launch
 * mmhn_bench_kronvec times with jacobi != 0 */
int mmhn_jacobi_step_batched(mmhn_handle h, const double* log_theta, const double* log_d_p, const double* log_d_m,
                             const int8_t* state, int64_t batch, const double* p, const double* rhs, double* y,
                             int transpose);
int mmhn_kronvec(mmhn_handle h, const double* log_theta, const int8_t* state, const double* p,
                 double* y, int diag, int transpose);
int mmhn_kron_diag(mmhn_handle h, const double* log_theta, const int8_t* state, double* out);
int mmhn_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p,
                   double* y, int which);
int mmhn_obs_states(mmhn_handle h, const int8_t* state, int pt_first, int64_t* idx, int64_t* count);
int mmhn_resolvent(mmhn_handle h, const double* log_theta, const double* log_d_p,
                   const double* log_d_m, const int8_t* state, const double* x, double* y,
                   int transpose);
int mmhn_x_partial_Q_y(mmhn_handle h, const double* log_theta, const int8_t* state, const double* x,
                       const double* y, double* G);
int mmhn_x_partial_D_y(mmhn_handle h, const double* log_d_p, const double* log_d_m,
                       const int8_t* state, const double* x, const double* y, double* d_dp,
                       double* d_dm);
int mmhn_partial_diag_scal(mmhn_handle h, const double* log_d, const int8_t* state, const double* p,
                           int i, int which, double* y);

/* ---- single-tumour primitives (metmhn/jx/vanilla.py); state has n+1 entries ---------
 * mmhn_v_kronvec       <-> vanilla.kronvec        (:78-106)
 * mmhn_v_resolvent     <-> vanilla.R_inv_vec      (:269-305)  d_rates == NULL means 1
 * mmhn_v_x_partial_Q_y <-> vanilla.x_partial_Q_y  (:328-393)  G[N][N], d_diag[N]
 * mmhn_v_kron_diag     <-> vanilla.kron_diag      (:247-260)  diag(Q) * diag  (diag == NULL means ones)
 * mmhn_v_scal_d_pt     <-> vanilla.scal_d_pt      (:125-142)  observation rates of an MT-only datapoint:
 *                          out_p = [seeding clear] prod d_p * vec, out_m = [seeding set] d_m[n] prod d_m * vec
 * mmhn_v_d_scal_d_pt   <-> vanilla.d_scal_d_pt    (:144-187)  their derivatives w.r.t. log d[i]
 * mmhn_v_x_partial_D_y <-> vanilla.x_partial_D_y  (:190-203)  (d_dp[N], d_dm[N]); argument order (log_d_p, log_d_m)
 * The three scal_d_pt functions need state[n_mut] == 1 (the reference applies a 2-state factor to the seeding bit).
 */
int mmhn_v_kronvec(mmhn_handle h, const double* log_theta, const int8_t* state, const double* p,
                   double* y, int diag, int transpose);
int mmhn_v_resolvent(mmhn_handle h, const double* log_theta, const int8_t* state,
                     const double* d_rates, const double* x, double* y, int transpose);
int mmhn_v_x_partial_Q_y(mmhn_handle h, const double* log_theta, const int8_t* state,
                         const double* x, const double* y, double* G, double* d_diag);
int mmhn_v_kron_diag(mmhn_handle h, const double* log_theta, const int8_t* state, const double* diag,
                     double* out);
int mmhn_v_scal_d_pt(mmhn_handle h, const double* log_d_p, const double* log_d_m, const int8_t* state,
                     const double* vec, double* out_p, double* out_m);
int mmhn_v_d_scal_d_pt(mmhn_handle h, const double* log_d_p, const double* log_d_m, const int8_t* state,
                       const double* vec, int i, double* out_p, double* out_m);
int mmhn_v_x_partial_D_y(mmhn_handle h, const double* log_d_p, const double* log_d_m,
                         const int8_t* state, const double* x, const double* y, double* d_dp,
                         double* d_dm);

/* ---- patient shards on several GPUs (one process and one engine per GPU) ----------------
 * The reference is single-process; its cohort sum (regularized_optimization.py:256-266) is what shards.
 * Rank 0 draws an id (mmhn_comm_unique_id, 128 bytes) and hands it to every rank by any host channel; after
 * mmhn_comm_init every mmhn_cohort_sums / mmhn_score / mmhn_score_and_grad of the handle returns the sums over
 * ALL ranks' cohorts: one RCCL all-reduce of the 4 + 2 N^2 + 3 N doubles on the engine's stream per evaluation,
 * no host staging.  Every rank must make the same calls in the same order (collective semantics).
 */
int mmhn_comm_unique_id(void* id128);
int mmhn_comm_init(mmhn_handle h, const void* id128, int rank, int n_ranks);
int mmhn_comm_destroy(mmhn_handle h);

/* ---- simulation ---------------------------------------------------------
 * mmhn_simulate: Gillespie sampler of the joint PT/MT process, one trajectory per thread; replaces
 * metmhn/simulations.py:117-147 (`simulate_dat`) and :87-114 (`simulate_orders`).
 *   log_theta [N][N], pt_d_ef / mt_d_ef [N]: log-parameters as the reference passes them (N = n_mut + 1)
 *   seed: Philox key; the samples depend on (seed, n_sim index) only
 *   dat_out    int8 [n_sim][2 n_mut + 2] = [PT_0, MT_0, ..., seeding, order (0 unpaired / 1 PT first / 2 MT first)]
 *   orders_out int8 [n_sim][2 N + 2] event sequences padded with -99 (events numbered as simulations.py:100-107), or NULL
 */
int mmhn_simulate(mmhn_handle h, const double* log_theta, const double* pt_d_ef, const double* mt_d_ef,
                  int64_t n_sim, uint64_t seed, int8_t* dat_out, int8_t* orders_out);
/* mmhn_simulate_summary: the same trajectories, counted on the device instead of written out (metmhn/simulations.py:150-240
 * `preseeding_probs`, Utilityfunctions.py:116-155 `marg_frequs` without the per-sample arrays).  Simulates the sample
 * indices [first, first + n_sim) - sample i is the i-th row mmhn_simulate returns under the same seed - in launches of
 * MMHN_SIM_CHUNK samples (default 2^26), so n_sim is bounded by time, not memory.  first >= 0, n_sim >= 0 and
 * first + n_sim < 2^63.  counts int64 [4 + 5 n_mut] (overwritten; seeding = event n_mut):
 *   [0] n_sim  [1] seeded  [2] seeded, PT observed first  [3] seeded, MT observed first  (dat_out's order 1 / 2)
 *   [4 + 0 n_mut + m] pre     seeded, mutation m occurred before the seeding (the PT set when it seeded)
 *   [4 + 1 n_mut + m] pt      seeded, final PT bit of m
 *   [4 + 2 n_mut + m] mt      seeded, final MT bit of m
 *   [4 + 3 n_mut + m] shared  seeded, final PT and MT bits of m
 *   [4 + 4 n_mut + m] pt_nm   unseeded, final PT bit of m
 * Integer counts: the result does not depend on the chunking or the launch geometry.
 */
int mmhn_simulate_summary(mmhn_handle h, const double* log_theta, const double* pt_d_ef, const double* mt_d_ef,
                          int64_t first, int64_t n_sim, uint64_t seed, int64_t* counts);
/* mmhn_simulate_pairs: the same trajectories again, counted to second order: which events occur together, per class of
 * sample, and how many mutations a tumour carries.  The model-side counterpart of a cohort's co-occurrence table; exact
 * pairwise marginals do not exist (2^(2 n_mut + 1) joint states), this is their Monte-Carlo estimate.  Sample indices, seed,
 * chunking (MMHN_SIM_CHUNK) and the argument checks are those of mmhn_simulate_summary; works on fp32 engines too (the
 * sampler is fp64 throughout).  With G the genotype columns [PT_0, MT_0, PT_1, MT_1, ...] of the rows mmhn_simulate
 * returns for these indices, B = 2 n_mut, and the class of a row = its last column (0 unseeded / 1 seeded, PT observed
 * first / 2 seeded, MT observed first), all outputs overwritten:
 *   n_class int64 [3]                 rows of each class
 *   pairs   int64 [3][B][B]           pairs[c] = G_c^T G_c over the rows of class c: full and symmetric, the diagonal holds
 *                                     the marginal counts, pairs[c][2i][2i+1] the rows with event i in both tumours
 *   burden  int64 [3][5][n_mut + 1]   per class the histogram of |PT|, |MT|, |PT & MT|, |PT & ~MT|, |MT & ~PT| over the
 *                                     mutations of a row (seeding and diagnosis excluded); every row of it sums to n_class[c]
 * Integer counts: the result does not depend on the chunking or the launch geometry.
 */
int mmhn_simulate_pairs(mmhn_handle h, const double* log_theta, const double* pt_d_ef, const double* mt_d_ef,
                        int64_t first, int64_t n_sim, uint64_t seed, int64_t* n_class, int64_t* pairs, int64_t* burden);

/* ---- likeliest event orders -------------------------------------------------
 * mmhn_likeliest_orders: MetMHN.likeliest_order (metmhn/model.py:213-293) of every row of a reference-format `dat`
 * [n_pat][2 n_mut + 3] in one call, exact (max-product Viterbi / Pareto-front DP over each row's 2^k sub-states).
 *   status per row of dat[:, -1] (type) and dat[:, -2] (diagnosis order): 0 "absent", 1 "present", 2 "isMetastasis",
 *   3 "isPaired" with first observation 0 "unknown", 1 "PT", any other value "Met" (as mmhn_set_cohort reads it).
 *   log_theta [N][N], obs1 / obs2 [N] (N = n_mut + 1), fp64 engines only.
 *   front_cap: candidates kept per sub-state of a paired row (0: MMHN_ORD_DEFAULT_FRONT_CAP, at most 65536).
 *   orders [n_pat][2 N - 1] event codes (2i PT, 2i+1 MT, 2 n_mut seeding) padded with -1; prob [n_pat];
 *   status [n_pat]: MMHN_ORD_OK, MMHN_ORD_OVERFLOW (a front outgrew front_cap: no result, recompute elsewhere),
 *   MMHN_ORD_INVALID (orders[i][0] holds the MMHN_ORD_* reason), MMHN_ORD_TOO_LARGE (the row's lattice does not fit the
 *   workspace limit on its own).  prob is NaN and the order all -1 wherever status != 0.
 * Rows are cut into batches that fit mmhn_set_workspace_limit; the call leaves a loaded cohort as it was.
 */
enum { MMHN_ORD_OK = 0, MMHN_ORD_OVERFLOW = 1, MMHN_ORD_INVALID = 2, MMHN_ORD_TOO_LARGE = 3 };
enum { MMHN_ORD_BAD_STATUS = 1,       /* type not in 0..3 */
       MMHN_ORD_UNREACHABLE = 2,      /* paired row without the seeding whose tumours differ */
       MMHN_ORD_NO_SEEDING = 3,       /* paired row without the seeding */
       MMHN_ORD_MT_PT_PART = 4,       /* "isMetastasis" row with primary-tumour events */
       MMHN_ORD_MT_NO_SEEDING = 5,    /* "isMetastasis" row without the seeding */
       MMHN_ORD_ABSENT_MET = 6,       /* "absent" row with metastasis events or the seeding */
       MMHN_ORD_PRESENT_MET = 7 };    /* "present" row whose metastasis part is not the seeding alone */
enum { MMHN_ORD_DEFAULT_FRONT_CAP = 64 };
int mmhn_likeliest_orders(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                          const int8_t* dat, int64_t n_pat, int n_cols, int front_cap, int8_t* orders, double* prob,
                          int32_t* status);

/* ---- pre-seeding posteriors of a cohort ------------------------------------------------------
 * mmhn_order_posteriors: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it) the sum over
 * ALL admissible orders where mmhn_likeliest_orders takes the maximum - exact sum-product over the row's 2^k sub-states,
 * forward and backward.  No reference counterpart (the reference derives such statements from likeliest orders and
 * simulation).  fp64 engines only.
 *   log_evidence [n_pat]        log of the summed order likelihoods = the row's log-probability under the model
 *   pre [n_pat][n_mut]          P(mutation m occurred before the seeding | the row); 0 for mutations the row does not carry
 *                               (paired rows: not in both tumours)
 *   seed_pos [n_pat][n_mut + 1] P(j mutations preceded the seeding | the row); sums to 1
 *   status [n_pat]: low half MMHN_ORD_OK, MMHN_ORD_INVALID (the MMHN_ORD_* reason is in the HIGH half: status >> 16) or
 *   MMHN_ORD_TOO_LARGE (the row's lattice - 2^k x 64 + 2^(k-1) x 24 B paired, 2^k x 16 B one tumour - does not fit the
 *   workspace limit on its own); never MMHN_ORD_OVERFLOW.  Every output of a row is NaN where its status != 0; pre and
 *   seed_pos are also NaN for rows of type 0 ("absent": no seeding in the observation), whose log_evidence is valid.
 * No atomics: two calls return the same bits, whatever the batching.  Rows are cut into batches that fit
 * mmhn_set_workspace_limit (allocated once per call); the call leaves a loaded cohort as it was.
 */
int mmhn_order_posteriors(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                          const int8_t* dat, int64_t n_pat, int n_cols, double* log_evidence, double* pre,
                          double* seed_pos, int32_t* status);

/* ---- pairwise precedence posteriors of a cohort ---------------------------------------------
 * mmhn_order_precedences: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it), over the
 * same admissible orders as mmhn_order_posteriors: which of two events came first.  Event codes as in the orders of
 * mmhn_likeliest_orders (2i event i in the primary tumour, 2i+1 in the metastasis, 2 n_mut the seeding; a one-tumour row
 * carries the codes its likeliest order is written in).  No reference counterpart.  fp64 engines only.
 *   log_evidence [n_pat]                        as mmhn_order_posteriors
 *   prec [n_pat][2 n_mut + 1][2 n_mut + 1]      prec[c][d] = P(code c happened strictly earlier than code d | the row).
 *                                               The two codes of an event that occurred before the seeding of a paired
 *                                               row happen at the same moment: neither precedes the other, so
 *                                               prec[c][d] + prec[d][c] = 1 - pre for them and 1 for every other pair.
 *                                               NaN where c or d is not in the row, 0 on the diagonal of those that are.
 *   status [n_pat]: as mmhn_order_posteriors - low half MMHN_ORD_OK, MMHN_ORD_INVALID (reason in the HIGH half) or
 *   MMHN_ORD_TOO_LARGE (the row does not fit the workspace limit on its own); every output of a row is NaN where its
 *   status != 0.  Workspace of a row of k slots, in doubles: the lattice of mmhn_order_posteriors (8 x 2^k + 3 x 2^(k-1)
 *   paired, 2 x 2^k one tumour) + the chunk partials of the reduction, k x sum over its levels of (c_l + 1) 2^(m_l - c_l)
 *   with m_0 = k - 2 paired / k - 1 one tumour, m_(l+1) = m_l - c_l, c_l = min(m_l, 10) past the first level and
 *   c_0 = min(m_0, max(6, min(10, m_0 - 2))) below 15 slots, min(m_0, max(6, min(10, m_0 - 4))) from there up: under 3 %
 *   on top of the lattice.
 * No atomics: two calls return the same bits, whatever the batching.  Rows are cut into batches that fit
 * mmhn_set_workspace_limit (allocated once per call); the call leaves a loaded cohort as it was.
 */
int mmhn_order_precedences(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                           const int8_t* dat, int64_t n_pat, int n_cols, double* log_evidence, double* prec,
                           int32_t* status);

/* ---- posterior event positions of a cohort --------------------------------------------------
 * mmhn_order_positions: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it), over the same
 * admissible orders as mmhn_order_posteriors: at which position of its lineage every event happened.  An order has two
 * lineages: the metastasis' (the order without its even codes other than the seeding: the events before the seeding, the
 * seeding, the metastasis' own events) and the primary tumour's (the order without its odd codes).  No reference
 * counterpart (the reference reads positions off the likeliest order).  fp64 engines only.
 *   log_evidence [n_pat]                        as mmhn_order_posteriors
 *   pos_pt [n_pat][n_mut + 1][n_mut + 1]        pos_pt[e][j] = P(event e - n_mut: the seeding - is the j-th (0-based) entry
 *                                               of the primary tumour's lineage | the row)
 *   pos_mt [n_pat][n_mut + 1][n_mut + 1]        the same for the metastasis' lineage
 *                                               A row of type 2 has the metastasis' lineage only, rows of type 0 and 1 the
 *                                               primary tumour's (type 0 without the seeding).  NaN for an event the row
 *                                               does not carry in that lineage and throughout a lineage the row does not
 *                                               have; for a carried event 0 at the positions past the lineage's length.
 *                                               The seeding's row equals seed_pos of mmhn_order_posteriors.
 *   status [n_pat]: as mmhn_order_precedences, with the same workspace per row or less (the same rows fit); every output
 *   of a row is NaN where its status != 0.
 * No atomics: two calls return the same bits, whatever the batching.  Rows are cut into batches that fit
 * mmhn_set_workspace_limit (allocated once per call); the call leaves a loaded cohort as it was.
 */
int mmhn_order_positions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                         const int8_t* dat, int64_t n_pat, int n_cols, double* log_evidence, double* pos_pt,
                         double* pos_mt, int32_t* status);

/* ---- posterior event and observation times of a cohort ---------------------------------------
 * mmhn_order_times: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it), over the same
 * admissible orders as mmhn_order_posteriors and every point of them at which the first observation can fall: the
 * posterior mean of the time at which every event and every observation happened.  Time 0 is the event-free state, the unit
 * the one in which an event-free tumour is observed at rate 1.  Given a path the chain holds in a state x for an
 * Exp(den[x]) time, so a mean time is a sum over the lattice of occupancy / den (metmhn_amd/csrc/ordertime.h).  No
 * reference counterpart.  fp64 engines only.
 *   log_evidence [n_pat]                        as mmhn_order_posteriors
 *   time [n_pat][2 n_mut + 1]                   E(time of the event with code c | the row), event codes as in
 *                                               mmhn_order_precedences; the two codes of an event that occurred before the
 *                                               seeding share its moment.  NaN where c is not in the row.
 *   obs [n_pat][2]                              E(time of the first observation | the row), E(time of the second); a
 *                                               one-tumour row has (its observation, NaN)
 *   pt_first [n_pat]                            P(the primary tumour was observed first | the row): exactly 1 / 0 for a
 *                                               paired row of diagnosis order 1 / neither 0 nor 1, NaN for a one-tumour row
 *   status [n_pat]: as mmhn_order_precedences - low half MMHN_ORD_OK, MMHN_ORD_INVALID (reason in the HIGH half) or
 *   MMHN_ORD_TOO_LARGE (the row does not fit the workspace limit on its own, or has more than 10 joint events); every
 *   output of a row is NaN where its status != 0.  Workspace of a row of k slots, in doubles: the lattice of
 *   mmhn_order_posteriors + the chunk partials of mmhn_order_precedences' reduction for 2 vectors of k - 1 index bits
 *   (paired) or 1 vector of k (one tumour) instead of k vectors: less than mmhn_order_precedences' from 4 slots on.
 * No atomics: two calls return the same bits, whatever the batching.  Rows are cut into batches that fit
 * mmhn_set_workspace_limit (allocated once per call); the call leaves a loaded cohort as it was.
 */
int mmhn_order_times(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                     int64_t n_pat, int n_cols, double* log_evidence, double* time, double* obs, double* pt_first,
                     int32_t* status);

/* ---- posterior genotypes at the first observation of a cohort's paired rows ------------------
 * mmhn_order_snapshots: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it), over the same
 * admissible orders as mmhn_order_posteriors and every point of them at which the first observation can fall: what the two
 * tumours held at the moment of the first observation.  The first observation of a paired row falls in a seeded state x
 * that holds every event of the tumour it is made of; with r = 0 the primary tumour observed first and r = 1 the metastasis,
 * mass(r, x) / evidence is the posterior probability that the first observation was of tumour r and found the chain in x
 * (metmhn_amd/csrc/ordersnap.h).  No reference counterpart (the reference sums the observation point away).  fp64 engines
 * only.
 *   log_evidence [n_pat]                        as mmhn_order_posteriors
 *   held [n_pat][2][2 n_mut + 1]                held[r][c] = P(the first observation was of tumour r and the event with code
 *                                               c had happened by then | the row), event codes as in mmhn_order_precedences.
 *                                               held[0][2 n_mut] + held[1][2 n_mut] = 1, held[0][2 n_mut] is pt_first of
 *                                               mmhn_order_times, and held[r][c] = held[r][2 n_mut] for the codes of tumour r.
 *                                               Exactly 0 throughout the r that the row's diagnosis order excludes (1: r = 1;
 *                                               neither 0 nor 1: r = 0).  NaN where c is not in the row.
 *   late [n_pat][2][n_mut + 1]                  late[r][j] = P(the first observation was of tumour r and exactly j events of
 *                                               the other tumour happened after it | the row); 0 past the number of events the
 *                                               other tumour has; the 2 (n_mut + 1) entries sum to 1
 *   map_first [n_pat], map_state [n_pat][2 n_mut + 1], map_prob [n_pat]
 *                                               the single most probable (r, x): r; per code 1 = held in x, 0 = in the row and
 *                                               still to come, -1 = not in the row; mass(r, x) / evidence.  Of equal masses
 *                                               r = 0 wins over r = 1, then the x that is the smaller number over the row's
 *                                               occupied columns of dat (the first column the lowest bit).
 *   A one-tumour row (types 0, 1, 2) has one observation: a valid log_evidence, NaN in held, late and map_prob, -1 in
 *   map_first and map_state.
 *   status [n_pat]: as mmhn_order_posteriors - low half MMHN_ORD_OK, MMHN_ORD_INVALID (reason in the HIGH half) or
 *   MMHN_ORD_TOO_LARGE (the row does not fit the workspace limit on its own; the number of joint events does not matter
 *   here); where it is not 0 every double of the row is NaN and every integer -1.  Workspace of a row of k slots, in doubles:
 *   the lattice of mmhn_order_posteriors, for a paired row + the chunk partials of mmhn_order_precedences' reduction for 2
 *   vectors of k - 1 index bits, as mmhn_order_times'.
 * No atomics: two calls return the same bytes, whatever the batching.  Rows are cut into batches that fit
 * mmhn_set_workspace_limit (allocated once per call); the call leaves a loaded cohort as it was.
 */
int mmhn_order_snapshots(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                         int64_t n_pat, int n_cols, double* log_evidence, double* held, double* late, int8_t* map_state,
                         int32_t* map_first, double* map_prob, int32_t* status);

/* ---- posterior samples of the event orders of a cohort ---------------------------------------
 * mmhn_order_samples: for every row of a reference-format `dat` (read as mmhn_likeliest_orders reads it), orders drawn from
 * the exact posterior over the admissible orders mmhn_order_posteriors sums over: an order comes with the probability
 * likelihood(order) / evidence.  The draw is metmhn_amd/model.py MetMHN.sample_order, move by move on the backward weights of
 * the row's lattice (metmhn_amd/csrc/ordersample.h).  Samples first ... first + n_samples - 1 of every row; Philox4x32-10, key
 * = `seed`, counter = (sample index low word, high word, move number, cohort row + 1) - a sample depends on (seed, cohort row,
 * sample index) only, not on n_samples or the batching; counter word 3 = 0 is mmhn_simulate's stream.  No reference
 * counterpart.  fp64 engines only.
 *   log_evidence [n_pat]                        as mmhn_order_posteriors
 *   orders [n_pat][n_samples][2 n_mut + 1]      event codes as in mmhn_likeliest_orders, padded with -1
 *   log_prob [n_pat][n_samples]                 log P(order | the row); log_evidence + log_prob = log likelihood(order)
 *   status [n_pat]: as mmhn_order_precedences (rows of more than 10 joint events are MMHN_ORD_TOO_LARGE); where it is not 0
 *   the row's orders are all -1 and its log_prob NaN.  Workspace of a row: the lattice of mmhn_order_posteriors plus its
 *   share of the output, n_samples x (2 n_mut + 1 + 8) bytes.
 * n_samples = 0 is valid and returns the evidence only (orders and log_prob may be null).  No atomics: two calls return the
 * same bytes, whatever the batching.  Rows are cut into batches that fit mmhn_set_workspace_limit; the call leaves a loaded
 * cohort as it was.
 */
int mmhn_order_samples(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, const int8_t* dat,
                       int64_t n_pat, int n_cols, int64_t first, int64_t n_samples, uint64_t seed, double* log_evidence,
                       int8_t* orders, double* log_prob, int32_t* status);

/* ---- seeding forecasts from a tumour's genotype ---------------------------------------------
 * mmhn_seeding_forecasts: the forward question.  A primary tumour holds the mutations of genotypes[r] and has not seeded;
 * until the seeding (until = 0), or until the seeding or the model's own clock of the first observation, whichever comes
 * first (until = 1), its chain runs on the supersets y of the genotype - a lattice over the f mutations it does NOT hold:
 *   lambda_j(y) = exp(theta[j][j] + sum over i in y of theta[j][i])   j not in y
 *   sigma(y)    = exp(theta[n][n] + sum over i in y of theta[n][i])   the seeding (theta[i][n], i < n, is never read)
 *   kappa(y)    = until ? exp(sum over i in y of obs1[i]) : 0         the clock
 *   den = sum of lambda_j + sigma + kappa,  F(genotype) = 1,  F(y) = sum over b of F(y - b) lambda_b(y - b) / den(y - b),
 *   G = F / den (the expected time spent in y)
 * One forward sum-product over the lattice, one launch per level over every row of the batch
 * (metmhn_amd/csrc/forecast.h).  No reference counterpart.  fp64 engines only; independent of mmhn_set_cohort.
 *   genotypes [n_rows][n_mut]                   int8, 1 = held, 0 = not
 *   p_seed [n_rows]                             sum G sigma: P(the seeding comes before the clock); 1 for until = 0
 *   time [n_rows]                               sum G: the expected time until the seeding or the clock (mmhn_order_times' unit)
 *   before [n_rows][n_mut]                      sum over y without j of G lambda_j: P(mutation j arises before the end);
 *                                               NaN for a held mutation
 *   with_seed [n_rows][n_mut]                   sum over y with j of G sigma: P(the seeding comes first and the seeding cell
 *                                               carries j); NaN for a held mutation
 *   n_before [n_rows][n_mut + 1]                sum over |y - genotype| = m of G sigma: P(the seeding comes first, after exactly
 *                                               m new mutations); exactly 0 for m > f
 *   status [n_rows]: low half MMHN_ORD_OK, MMHN_ORD_INVALID (high half MMHN_ORD_BAD_ENTRY: an entry other than 0 / 1) or
 *   MMHN_ORD_TOO_LARGE (f > 30, or the row's workspace - 8 B x 2^f and, per 2^14 states, 3 f + 3 doubles of partials -
 *   does not fit the workspace limit on its own); every output of a row is NaN where its status != 0.
 * The call fails (return 1) for until = 0 when the seeding rate of the full genotype underflows to 0 (theta[n][n] of
 * -1e10, as a fit without seeded samples leaves it): the full state would have no exit.  Mutation rates of 0 are fine.
 * n_rows = 0 is valid.  No atomics: two calls return the same bytes, whatever the batching and the other rows.  Rows are
 * cut into batches that fit mmhn_set_workspace_limit (allocated once per call).
 */
enum { MMHN_ORD_BAD_ENTRY = 8 };     /* mmhn_seeding_forecasts: a genotype entry other than 0 / 1 */
int mmhn_seeding_forecasts(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes,
                           int64_t n_rows, int until, double* p_seed, double* time, double* before, double* with_seed,
                           double* n_before, int32_t* status);

/* ---- seeding landscape: the forecast scalars of every genotype ------------------------------
 * mmhn_seeding_landscape: ONE backward sweep over all 2^n_mut genotypes of the model gives every genotype's scalar answers of
 * mmhn_seeding_forecasts.  x is a genotype code, bit j = mutation j held (the order of genotypes[r][j]); with the rates of
 * mmhn_seeding_forecasts and j over the mutations x does not hold
 *   p_seed(x)      = (sigma(x) + sum_j lambda_j(x) p_seed(x + j)) / den(x)
 *   time(x)        = (1        + sum_j lambda_j(x) time(x + j)) / den(x)
 *   new_events(x)  = (           sum_j lambda_j(x) (1 + new_events(x + j))) / den(x)                  = the sum of `before`
 *   seed_events(x) = (           sum_j lambda_j(x) (p_seed(x + j) + seed_events(x + j))) / den(x)     = the sum of `with_seed`
 * from the full genotype down (metmhn_amd/csrc/landscape.h: tiles of 2^10 codes finished in LDS, one launch per popcount of
 * the tile number).  No reference counterpart.  fp64 engines only; independent of mmhn_set_cohort.
 *   genotypes [n_rows][n_mut]                   int8 queries, 1 = held, 0 = not; n_rows = 0 is valid
 *   values [n_rows][4]                          p_seed, time, new_events, seed_events of every query
 *   status [n_rows]                             MMHN_ORD_OK, or MMHN_ORD_INVALID with MMHN_ORD_BAD_ENTRY in the high half for
 *                                               an entry other than 0 / 1: that row's values are NaN, the others unaffected
 *   full                                        null, or [4][2^n_mut]: the four values of every genotype by code
 * The call fails (return 1, mmhn_last_error names the bytes needed) when 32 B x 2^n_mut, the rate tables and the tile list
 * (4 B per 2^10 codes) exceed mmhn_set_workspace_limit: there is no partial landscape and nothing is launched.  It fails
 * for until = 0 when the seeding rate of the full genotype underflows to 0, as mmhn_seeding_forecasts does.  Mutation rates
 * of 0 are fine and give exact zeros.  Every shape depends on n_mut alone and there are no atomics: a genotype's four
 * values do not depend on the queries or on an earlier call.
 */
int mmhn_seeding_landscape(mmhn_handle h, const double* log_theta, const double* obs1, int until, const int8_t* genotypes,
                           int64_t n_rows, double* values, int32_t* status, double* full);

/* ---- genotype distribution of the primary tumour ---------------------------------------------
 * mmhn_genotype_distribution: ONE forward sweep over all 2^n_mut genotypes gives the probability that the primary tumour
 * is observed with genotype x and has not seeded (U), or has seeded by then (S).  The primary tumour is an autonomous chain
 * on (genotype, seeded or not): theta[i][n], i < n, is not read.  With the rates of the seeding forecasts, j over the
 * mutations x does not hold and b over the ones it holds
 *   kappa0(x) = exp(sum over i in x of obs1[i]),  kappa1(x) = kappa0(x) exp(obs1[n]),  L(x) = sum_j lambda_j(x)
 *   F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                    G0 = F0 / (L + sigma + kappa0)
 *                   F1(y) = G0(y) sigma(y) + sum_b G1(y - b) lambda_b(y - b),   G1 = F1 / (L + kappa1)
 *   U = kappa0 G0 = exp(lp) of the cohort row of type 0 with that genotype,  S = kappa1 G1 = the same of type 1
 * from the empty genotype up (metmhn_amd/csrc/genodist.h: the tiles of the seeding landscape, one launch per popcount of the
 * tile number, ascending).  fp64 engines only; independent of the loaded cohort.
 *   genotypes [n_rows][n_mut]                   int8 queries, 1 = held, 0 = not; n_rows = 0 is valid
 *   values [n_rows][2]                          U, S of every query
 *   status [n_rows]                             MMHN_ORD_OK, or MMHN_ORD_INVALID with MMHN_ORD_BAD_ENTRY in the high half for
 *                                               an entry other than 0 / 1: that row's values are NaN, the others unaffected
 *   summary                                     null, or [2][1 + n_mut * n_mut + n_mut + 1], per plane s (0: U, 1: S):
 *                                               mass = sum_x P_s(x), pairs [n_mut][n_mut] = sum_x P_s(x) x_i x_j (the
 *                                               marginals on the diagonal), burden [n_mut + 1] = sum over |x| = m of P_s(x)
 *   full                                        null, or [2][2^n_mut]: U and S of every genotype by code (bit j = mutation j)
 * The call fails (return 1, the last error names the bytes needed) when 16 B x 2^n_mut, the rate tables, the tile list
 * (4 B per 2^10 codes) and, with a summary, the tiles' partial sums (1 072 B per 2^10 codes) exceed the workspace limit:
 * there is no partial distribution and nothing is launched.  Mutation rates of 0 give exact zeros on every genotype that
 * holds the mutation; a seeding rate of 0 gives S = 0 throughout and is no failure.  Every shape depends on n_mut alone and
 * there are no atomics: no byte of an output depends on the queries or on an earlier call.
 */
int mmhn_genotype_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const int8_t* genotypes,
                               int64_t n_rows, double* values, int32_t* status, double* summary, double* full);

/* ---- genotype distribution of the metastasis and its founder ---------------------------------
 * mmhn_metastasis_distribution: ONE forward sweep over all 2^n_mut genotypes gives the probability that the seeding happens
 * before the primary tumour's observation and the seeding cell (the founder) holds exactly y (Z), the probability that the
 * metastasis is observed with genotype z (M), and M weighted by the number of z's mutations the founder held (C).  The
 * metastasis is an autonomous chain: the common lineage until the seeding, then its own rates, which carry the seeding's
 * effect theta[j][n], until its own clock obs2; nothing the primary tumour does afterwards reaches it.  With the notation of
 * mmhn_genotype_distribution, j over the mutations a code does not hold and b over the ones it holds
 *   mu_j(z) = lambda_j(z) exp(theta[j][n]),  Lm(z) = sum_j mu_j(z),  kappam(z) = exp(obs2[n] + sum over i in z of obs2[i])
 *   F0(empty) = 1,  F0(y) = sum_b G0(y - b) lambda_b(y - b),                      G0 = F0 / (L + sigma + kappa0)
 *                   FM(y) = G0(y) sigma(y)     + sum_b GM(y - b) mu_b(y - b),     GM = FM / (Lm + kappam)
 *                   FC(y) = G0(y) sigma(y) |y| + sum_b GC(y - b) mu_b(y - b),     GC = FC / (Lm + kappam)
 *   Z = sigma G0,  M = kappam GM = exp(lp) of the cohort row of type 2 with that MT genotype,  C = kappam GC
 * from the empty genotype up (metmhn_amd/csrc/metdist.h, on the tiles of mmhn_genotype_distribution).  sum Z = sum M = the
 * mass[1] of mmhn_genotype_distribution; C / M is the expected number of z's mutations that were already in the founder,
 * 0 <= C <= |z| M.  fp64 engines only; independent of the loaded cohort.
 *   genotypes [n_rows][n_mut]                   int8 queries, 1 = held, 0 = not; n_rows = 0 is valid
 *   values [n_rows][3]                          Z, M, C of every query
 *   status [n_rows]                             as for mmhn_genotype_distribution: MMHN_ORD_OK, or MMHN_ORD_INVALID with
 *                                               MMHN_ORD_BAD_ENTRY in the high half (that row's values are NaN)
 *   summary                                     null, or [2][1 + n_mut * n_mut + n_mut + 1]: mass, pairs [n_mut][n_mut],
 *                                               burden [n_mut + 1] of the founder plane Z and then of the metastasis plane M
 *   full                                        null, or [3][2^n_mut]: Z, M and C of every genotype by code
 * The call fails (return 1, the last error names the bytes needed) when 24 B x 2^n_mut, the two sets of rate tables, the
 * tile list and, with a summary, the tiles' partial sums exceed the workspace limit: there is no partial distribution and
 * nothing is launched.  A mutation rate of 0 gives exact zeros on every genotype that holds the mutation; a seeding rate of
 * 0 gives all three planes 0 and is no failure.  Every shape depends on n_mut alone and there are no atomics: no byte of an
 * output depends on the queries or on an earlier call.
 */
int mmhn_metastasis_distribution(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2,
                                 const int8_t* genotypes, int64_t n_rows, double* values, int32_t* status, double* summary,
                                 double* full);

/* ---- genotype distribution of one tumour given the other -------------------------------------
 * mmhn_partner_distributions: for every query genotype q the joint probability of q in the GIVEN tumour - the primary tumour
 * observed seeded (given = 0) or the metastasis (given = 1) - with EVERY genotype of the other tumour, the partner: one row or
 * column of the (PT x MT) table, exp(lp) of the cohort row of type 3 with unknown order of observation for all 2^n_mut
 * partners at once.  After the seeding the two tumours are independent chains, each stopped by its own clock, so the joint
 * factorises through the founder z.  With the notation of the two distributions above, kappa1 = kappa0 exp(obs1[n]),
 * den1 = L + kappa1, denm = Lm + kappam, and for given = 0 (given = 1 exchanges the chains: mu, kappam, denm behind the
 * seeding for B and lambda, kappa1, den1 for F)
 *   G0(z), z a subset of q:  as in mmhn_genotype_distribution
 *   B(q) = kappa1(q) / den1(q),  B(z) = sum over j in q - z of lambda_j(z) B(z + j) / den1(z)    (L over ALL mutations z lacks)
 *   W(z) = sigma(z) G0(z) B(z) on the subsets of q, 0 elsewhere     = P(founder z, the given tumour observed as q)
 *   F(y) = W(y) + sum_b G(y - b) mu_b(y - b),  G = F / denm,  J(y) = kappam(y) G(y)     = P(PT = q seeded, MT = y)
 * sum W = sum J = S(q) of mmhn_genotype_distribution (given = 0) or M(q) of mmhn_metastasis_distribution (given = 1), and
 * J of q given as PT at y = J of y given as MT at q.  Per DISTINCT query: a backward pass and a forward pass over the
 * 2^|q| subsets of q and one forward sweep of one plane over all 2^n_mut genotypes (metmhn_amd/csrc/partner.h).  The device
 * returns joint probabilities; the conditionals are J / mass.  fp64 engines only; independent of the loaded cohort.
 *   given                                       0: the queries are primary tumours, 1: metastases
 *   genotypes [n_rows][n_mut]                   int8 queries, 1 = held, 0 = not; n_rows = 0 is valid
 *   targets                                     null, or [n_rows][n_mut]: a partner genotype per row
 *   values [n_rows][3]                          mass = sum J - the sum over the tiles (thread t of 256 the tiles t, t + 256, ...
 *                                               ascending, then a tree) of the tile masses of the summary's fold, the bytes of
 *                                               the summary's mass of the partner, formed with or without summaries -, W and J
 *                                               at the row's target (NaN without targets)
 *   status [n_rows]                             as for mmhn_genotype_distribution: MMHN_ORD_OK, or MMHN_ORD_INVALID with
 *                                               MMHN_ORD_BAD_ENTRY in the high half for an entry of the query or the target
 *                                               other than 0 / 1 (that row's values and summaries are NaN)
 *   summaries                                   null, or [n_rows][2][1 + n_mut * n_mut + n_mut + 1]: mass, pairs, burden of
 *                                               the founder plane W and then of the partner plane J of every row
 *   full                                        null, or [2][2^n_mut]: W and J of every genotype by code; n_rows must be 1
 * The call fails (return 1, the last error names the bytes needed) when 16 B x 2^n_mut, the two sets of rate tables, the
 * two tile lists and the tiles' partial sums exceed the workspace limit, whatever the rows (the per-row buffers, 28 B per valid
 * row for the target code and the values, fall outside the limit as the gather buffers of the sweeps above do): there is no partial distribution
 * and nothing is launched.  A query that holds a mutation of rate 0 gives exact zeros; no byte of a row's outputs depends
 * on the other rows or on an earlier call.
 */
int mmhn_partner_distributions(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int given,
                               const int8_t* genotypes, const int8_t* targets, int64_t n_rows, double* values,
                               int32_t* status, double* summaries, double* full);

/* ---- exact PT x MT co-occurrence and joint burden tables --------------------------------------
 * mmhn_cross_table: the second moments of the (PT x MT) table of which mmhn_partner_distributions gives one row or column:
 * P(the primary tumour holds mutation i, the metastasis holds mutation j, seeded) for every i, j and P(|PT| = k, |MT| = l,
 * seeded) for every k, l, exactly.  After the seeding the two tumours are independent chains, each stopped by its own clock,
 * so every bilinear statistic of the pair factorises through the founder z:
 *   E[phi(PT) psi(MT); seeded] = sum_z Z(z) a_phi(z) b_psi(z),    Z = sigma G0 of mmhn_metastasis_distribution,
 *   a_phi(z) = (kappa1(z) phi(z) + sum over j not in z of lambda_j(z) a_phi(z + j)) / den1(z)      from the full genotype down,
 *   b_psi(z) the same with mu_j, kappam, denm
 * (the notation of mmhn_partner_distributions).  The features of a chain are the n_mut gene indicators [mutation i held] and
 * the n_mut + 1 burden indicators [|x| = k]: 2 ceil((2 n_mut + 1) / 4) backward sweeps of four planes over all 2^n_mut
 * genotypes when every plane fits, one forward plane for Z, and a fold per pair of blocks (metmhn_amd/csrc/cross.h).
 * Everything is a JOINT probability with "seeded"; the conditionals are the outputs over `mass`.  fp64 engines only;
 * independent of the loaded cohort.
 *   with_burden                                 0: only the n_mut gene features are swept, the burden outputs are NaN and
 *                                               the gene outputs have the bytes they have with the burden
 *   out [1 + 2 n + n n + (n + 1)(n + 1) + 2 n (n + 1)], n = n_mut, in this order:
 *     mass                                      sum Z = P(seeded)
 *     pt [n], mt [n]                            sum Z a_i = P(PT holds i, seeded), sum Z b_j = P(MT holds j, seeded)
 *     cross [n][n]                              sum Z a_i b_j
 *     burden [n + 1][n + 1]                     [k][l] = P(|PT| = k, |MT| = l, seeded)
 *     gene_burden [2][n][n + 1]                 [0][i][l] = P(PT holds i, |MT| = l, seeded), [1][j][k] = P(MT holds j, |PT| = k, seeded)
 * The planes are planned against the workspace limit: Z, one block of the metastasis and as many blocks of the primary tumour
 * as fit are resident, 1 + 4 + 4 ceil((2 n + 1) / 4) planes of 8 B x 2^n_mut at the most; blocks that do not fit are swept again
 * per block of the metastasis.  The call fails (return 1, the last error names the bytes needed) when the minimum - 72 B x
 * 2^n_mut, the two sets of rate tables, the tile list and the tiles' partial sums - exceeds the workspace limit: there is no
 * partial table and nothing is launched.  A mutation of rate 0 gives exact zeros in its pt entry and its rows of cross and
 * gene_burden[0].  Every shape depends on n_mut alone and there are no atomics: no byte of the output depends on the
 * workspace limit, on how many blocks were held or swept again, or on an earlier call.
 */
int mmhn_cross_table(mmhn_handle h, const double* log_theta, const double* obs1, const double* obs2, int with_burden,
                     double* out);

/* ---- measurement -------------------------------------------------------------------
 * mmhn_bench_kronvec: `batch` resident copies of a 2^k vector, `iters` back-to-back
 * launches of mmhn_kronvec_batched's launch (diag = 0: y = Q_off p into a NaN-filled y, every tile of every vector,
 * structurally zero tiles zeroed inside the launch) or of the fused Jacobi step if jacobi != 0, timed
 * with HIP events on the engine's stream; returns the average launch duration in ms.
 * tiles (optional): [0] = tiles per launch where Q_off has entries, [1] = tiles per launch.
 * mmhn_get_counters: cumulative figures since mmhn_reset_counters, per class of dominant kernel (events recorded
 * on the engine's stream around every launch).
 */
enum { MMHN_K_OTHER_SOLVE = 0,  /* tile solves / Jacobi sweeps of the single-tumour problems (k_csolve, k_tsolve, k_sweep), API calls */
       MMHN_K_PSOLVE_FWD = 1,   /* k_wsolve / k_psolve2 forward: a chain of patients / one patient per workgroup, (D - Q) pi = e_0 */
       MMHN_K_PSOLVE_ADJ = 2,   /* ... adjoint: (D - Q)^T q = rhs */
       MMHN_K_PCLASS = 3,       /* k_wclass / k_pclass: class marginals of pi (x) q */
       MMHN_K_CSOLVE_FWD = 4,   /* k_csolve forward: the tiles of the joint problems on the tile route, one cooperative launch */
       MMHN_K_CSOLVE_ADJ = 5,   /* ... adjoint */
       MMHN_K_COUNT = 6 };
typedef struct {
  double ms;         /* total duration of the launches (HIP events on the engine's stream) */
  int64_t launches;
  double alg_bytes;  /* algorithmic bytes of those launches: solves = the solution written once (live tiles),
                        marginals = pi and q read once, Jacobi sweep = 4 * 2^k * sizeof(dtype) per vector */
} mmhn_kernel_counter;
typedef struct {
  mmhn_kernel_counter kernel[MMHN_K_COUNT];
  double eval_ms;    /* host wall time spent inside evaluations */
  int64_t evals;
  int32_t comm_ranks; /* ranks of the RCCL communicator attached by mmhn_comm_init as RCCL itself reports them (ncclCommCount), 0: none */
  int32_t comm_rank;  /* this engine's rank in it (ncclCommUserRank), -1: none */
} mmhn_counters;
/* ABI version of this header: bumped whenever an exported signature or structure changes (4: mmhn_bench_kronvec has its
 * `tiles` argument, mmhn_debug_lane_moves exists; 5: mmhn_counters has six kernel classes and the communicator's size / rank; 6: mmhn_likeliest_orders exists; 7: mmhn_simulate_summary exists; 8: mmhn_order_posteriors exists; mmhn_order_precedences, mmhn_order_positions, mmhn_order_samples, mmhn_simulate_pairs, mmhn_order_times, mmhn_order_snapshots, mmhn_seeding_forecasts, mmhn_seeding_landscape, mmhn_genotype_distribution, mmhn_metastasis_distribution, mmhn_partner_distributions and mmhn_cross_table were added within version 8, purely additive changes).  A client built against another header must refuse to run:
 * mmhn_abi_version() != MMHN_ABI_VERSION (metmhn_amd/_lib.py checks it on load). */
#define MMHN_ABI_VERSION 8
int mmhn_abi_version(void);
int mmhn_bench_kronvec(mmhn_handle h, const double* log_theta, const int8_t* state, int64_t batch,
                       int iters, int transpose, int jacobi, double* ms_per_launch, int64_t* tiles);
/* device-memory bandwidth of this GPU for a plain 16-byte-per-lane stream over arrays of `bytes` each
 * (kind 0: copy, 1: triad a = b + s c), GB/s of the 2 x / 3 x bytes moved: the measured denominator next to the
 * nominal HBM peak */
int mmhn_bench_stream(mmhn_handle h, size_t bytes, int iters, int kind, double* gbps);
int mmhn_get_counters(mmhn_handle h, mmhn_counters* out);
int mmhn_reset_counters(mmhn_handle h);
/* diagnostic of the window-layout solve (csrc/wsolve.h): out[6][64], out[i][lane] = the lane whose value `lane` receives
 * through the exchange along lane bit i (DPP / swizzle / permute forms) - lane ^ (1 << i) on every lane that has the
 * move (forward: bit i set, transposed: bit i clear).  No reference counterpart (the reference has no lanes). */
int mmhn_debug_lane_moves(mmhn_handle h, int transposed, int* out);

#ifdef __cplusplus
}
#endif
#endif /* METMHN_AMD_H */
