"""What the tests of the cohort reduction share (test_cohort_reduction.py, test_row_weights.py, test_row_groups.py,
test_unknown_status.py): the two packed layouts of include/metmhn_amd.h, the reference of a cohort buffer with its bound
(derived in tests/test_cohort_reduction.py), and the cohorts they reduce.  Imported as a module (`import reduction_common as RC`):
its names are short."""
import math

import numpy as np

from eval_common import row
from unknown_common import unknown_row

U = 2.0 ** -53
RED_MAX_CHUNKS = 128            # csrc/assemble.h
N4 = 4
PERC_MET = 0.3
W_PM = 0.37                                                   # EM / NM weight of the pre-combined buffer
WEIGHT_VALUES = np.array([0.0, 0.5, 1.0, 2.0, 3.0, 7.25])
MULTI_BATCH = (4, 4097)                                       # in at least three batches
MULTI_BATCH_WS = 1 << 20                                   # its workspace limit in bytes (test_cohort_reduction.py: test_multi_batch_reduction)


def red_per(npat):
    """Rows per chunk of k_reduce_rows (csrc/assemble.h: red_per)."""
    return max(32, (npat + RED_MAX_CHUNKS - 1) // RED_MAX_CHUNKS)


def stride(N):
    return 1 + N * N + 2 * N


def raw_len(N):
    return 4 + 2 * N * N + 3 * N


# ---- the two layouts of include/metmhn_amd.h ---------------------------------------------------------------------------

def raw_layout(em, nm, n_em, n_pat, N):
    """[s_EM, s_NM, n_em, n_pat, G_EM, G_NM, p_EM, p_NM, m_EM] from two rows [lp, G, d_dp, d_dm] (mmhn_cohort_sums)."""
    NN = N * N
    return np.concatenate(([em[0], nm[0], n_em, n_pat], em[1:1 + NN], nm[1:1 + NN], em[1 + NN:1 + NN + N],
                           nm[1 + NN:1 + NN + N], em[1 + NN + N:]))


def wsums_layout(em, nm, w, N):
    """[w s_EM + s_NM, w G_EM + G_NM, w p_EM + p_NM, w m_EM] (mmhn_cohort_wsums_begin / _end)."""
    head = 1 + N * N + N
    return np.concatenate((w * em[:head] + nm[:head], w * em[head:]))


# ---- the reference and its bound -----------------------------------------------------------------------------------------

def colsum(a):
    """Correctly rounded column sums of a [P, st] array."""
    return np.array([math.fsum(c) for c in a.T]) if a.shape[0] else np.zeros(a.shape[1])


class Reference:
    """Exact per-class sums of the rows [P, st] of a cohort.  nm_rows: the rows of type 0 (all-zero rows among them);
    n_seed: rows with the seeding event (sums[2]); spread (optional, [P, st]): |difference| of two downloads of the rows."""

    def __init__(self, rows, nm_rows, n_seed, N, spread=None):
        rows = np.asarray(rows, dtype=np.float64)
        nm_rows = np.asarray(nm_rows, dtype=bool)
        assert rows.shape == (nm_rows.shape[0], stride(N)), (rows.shape, nm_rows.shape, stride(N))
        self.N, self.P, self.n_seed = N, rows.shape[0], float(n_seed)
        self.p_em, self.p_nm = int((~nm_rows).sum()), int(nm_rows.sum())
        self.em, self.nm = colsum(rows[~nm_rows]), colsum(rows[nm_rows])
        self.abs_em, self.abs_nm = colsum(np.abs(rows[~nm_rows])), colsum(np.abs(rows[nm_rows]))
        z = np.zeros(stride(N))
        self.sp_em = z if spread is None else colsum(spread[~nm_rows])
        self.sp_nm = z if spread is None else colsum(spread[nm_rows])

    def raw(self):
        """(reference, bound) of the mmhn_cohort_sums buffer; the bound of the two counts is 0."""
        ref = raw_layout(self.em, self.nm, self.n_seed, float(self.P), self.N)
        bound = raw_layout((self.p_em + 2) * U * self.abs_em + self.sp_em, (self.p_nm + 2) * U * self.abs_nm + self.sp_nm,
                           0.0, 0.0, self.N)
        return ref, bound

    def wsums(self, w):
        """(reference, bound) of the pre-combined buffer."""
        ref = wsums_layout(self.em, self.nm, w, self.N)
        bound = (self.P + 4) * U * wsums_layout(self.abs_em, self.abs_nm, abs(w), self.N) + \
            wsums_layout(self.sp_em, self.sp_nm, abs(w), self.N)
        return ref, bound


def within(got, ref, bound, what):
    """Every element within its bound (exactly equal where the bound is 0, NaN never passes); the worst error / bound."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: {got.shape} doubles, expected {ref.shape}"
    err = np.abs(got - ref)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements outside the bound, first at {bad[0]}: got {got[bad[0]]!r}, "
                           f"reference {ref[bad[0]]!r}, error {err[bad[0]]:.3e}, bound {bound[bad[0]]:.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def check_raw(got, reference, what="cohort_sums"):
    return within(got, *reference.raw(), what)


def check_wsums(got_and_tail, reference, w, flag, what="cohort_wsums"):
    """got_and_tail: the 1 + N^2 + 2N doubles and the slot behind them, which must hold the flag itself."""
    got_and_tail = np.asarray(got_and_tail, dtype=np.float64)
    st = stride(reference.N)
    assert got_and_tail.shape == (st + 1,), f"{what}: {got_and_tail.shape}"
    ratio = within(got_and_tail[:st], *reference.wsums(w), what)
    assert got_and_tail[st] == flag, f"{what}: the slot behind the buffer holds {got_and_tail[st]!r}, flag {flag!r}"
    return ratio


# ---- cohorts ---------------------------------------------------------------------------------------------------------------

def hand_rows(n):
    """all-zero type 0; seeding-only rows of types 1, 2, 3 (diagnosis order 0); paired rows of orders 1 and 2 with one event each side."""
    return {"zero": row(n, [], [], 0, -99, 0), "t1": row(n, [], [], 1, -99, 1), "t2": row(n, [], [], 1, -99, 2),
            "t3_o0": row(n, [], [], 1, 0, 3), "t3_o1": row(n, [0], [1], 1, 1, 3), "t3_o2": row(n, [1], [0, 2], 1, 2, 3)}


MAX_PAIRED_EVENTS = 6


def few_events(dat):
    """Paired rows keep their first MAX_PAIRED_EVENTS events: a joint space of up to 2^6 states beside the seeding bit is one
    row of 64 states to k_pclass (csrc/classmarg.h), whose class-marginal entries one wave adds up.  With more, several
    waves meet in the floating-point atomics of its flush and two evaluations of a row may differ in the last bit - the
    reference rows would no longer be those of the evaluation under test."""
    n = (dat.shape[1] - 3) // 2
    for r in np.flatnonzero((dat[:, -1] == 3) & (dat[:, :2 * n].sum(axis=1) > MAX_PAIRED_EVENTS)):
        dat[r, np.flatnonzero(dat[r, :2 * n])[MAX_PAIRED_EVENTS:]] = 0
    return dat


def cohort(n, P, kind="mixed"):
    """synthetic.mixed_cohort with few events per row (small spaces), the hand-written rows at its start, an order-1 paired row
    as the last row of the first chunk and an all-zero row as the last row of the cohort."""
    from metmhn_amd import synthetic
    p_event = 0.25 if n <= 6 else 0.08
    hand = hand_rows(n)
    if P == 0:
        return np.zeros((0, 2 * n + 3), dtype=np.int8)
    if P == 1:
        return hand["t3_o1"][None, :].copy()
    if kind != "mixed":
        pool = synthetic.mixed_cohort(n, 40 * P, seed=P + n, p_event=p_event)
        dat = few_events(pool[(pool[:, -1] == 0) == (kind == "all_nm")][:P].copy())
        assert dat.shape[0] == P, (dat.shape, P)
        if kind == "all_nm":
            dat[P - 1] = hand["zero"]
        return dat
    dat = few_events(synthetic.mixed_cohort(n, P, seed=P + n, p_event=p_event))
    for i, name in enumerate(("t1", "t2", "t3_o0", "t3_o2")):
        dat[i] = hand[name]
    dat[P - 1] = hand["zero"]
    edge = min(red_per(P), P) - 1
    dat[edge if edge < P - 1 else P - 2] = hand["t3_o1"]
    assert (dat[:, -1] == 0).any() and all(((dat[:, -1] == 3) & (dat[:, -2] == o)).any() for o in (0, 1, 2)), "a row type or order is missing"
    return dat


def typed_cohort(n, P, seed):
    """cohort() with every seventh row replaced by a row of type 4 (the empty genotype among them)."""
    dat = cohort(n, P).copy()
    rng = np.random.default_rng(seed)
    for k, r in enumerate(range(3, P, 7)):
        dat[r] = unknown_row(n, [] if k == 0 else rng.choice(n, size=int(rng.integers(1, n)), replace=False))
    return dat


def params(n):
    from metmhn_amd import synthetic
    return synthetic.random_params(n)


def nm_class(dat):
    """Rows of the NM sums: type 0 and type 4 (unknown status, weight 1 of their own)."""
    return (dat[:, -1] == 0) | (dat[:, -1] == 4)


# ---- what an engine returns ------------------------------------------------------------------------------------------------

def rows_of(e, lt, dp, dm, with_grad=True):
    """The engine's per-patient rows [P, st] = [lp, G, d_dp, d_dm] (with_grad=False: lp and zeros): never weighted or mixed."""
    P, N = e.n_pat, e.N
    if P == 0:
        return np.zeros((0, stride(N)))
    if not with_grad:
        rows = np.zeros((P, stride(N)))
        rows[:, 0] = e.patient_grads(lt, dp, dm, with_grad=False)
        return rows
    lp, g, gp, gm = e.patient_grads(lt, dp, dm)
    return np.concatenate((lp[:, None], g.reshape(P, N * N), gp, gm), axis=1)


def wsums(e, lt, dp, dm, w_pm, with_grad=True):
    """One weighted evaluation: the pre-combined buffer."""
    e.cohort_wsums_begin(lt, dp, dm, w_pm, with_grad=with_grad)
    return e.cohort_wsums_end()


def flat(res):
    """(score, d_theta, d_dp, d_dm) as one vector in the order of the pre-combined buffer."""
    return np.concatenate(([float(res[0])], np.ravel(res[1]), np.ravel(res[2]), np.ravel(res[3])))
