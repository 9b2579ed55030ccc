"""Row groups (mmhn_set_row_groups, csrc/rowmix.h: k_mix_gather, k_group_lse, k_mix_weights, k_reduce_rows_mix) and the host code on
top of them (Utilityfunctions.expand_missing, regularized_optimization's `groups=`, impute_missing).

Definition (include/metmhn_amd.h): group g is a list of cohort rows, alternatives of one patient, with weight w_g:
    lp_g = log sum_{r in g} exp(lp_r)      rho_{g,r} = exp(lp_r - lp_g)
    sum of element 0 = sum_g w_g lp_g      sum of element e >= 1 = sum_g w_g sum_{r in g} rho_{g,r} v_r[e]
per block (EM; NM with type 4); n_pat = sum w_g, n_em over the groups of seeded rows, n_unknown over the groups of type-4 rows.
The device forms, per cohort row, omega_r = sum_g w_g rho_{g,r} and lambda_r = sum_g w_g rho_{g,r} lp_g over the groups that
hold r and then reduces the rows as k_reduce_rows_w does, with the addend omega_r v_r[e] (lambda_r for e = 0).

Reference (MixReference): the same quantities in NumPy long double from the engine's own per-row values (Engine.patient_grads,
which stays unmixed), the per-class sums with math.fsum over the float64 addends.

Bound, to first order in u = 2^-53, with exp and log of the device taken as accurate to E = 3 ulps (6 u relative: the OpenCL
full-profile limit the device library is written to) and L alternatives in group g, m = max lp_r:
  * a_r = lp_r - m is rounded once (relative u, i.e. |a_r| u absolute in the argument of exp), exp adds 2 E u: the addends of s
    = sum exp(a_r) carry (|a_r| + 2 E) u relative; they are positive, so any tree over L of them adds (L - 1) u:
        |ds| / s <= (L - 1 + 2 E + A_g) u,   A_g = sum_r rho_r |lp_r - m|;
  * lp_g = m + log(s): log passes |ds| / s on, adds 2 E u |log s| <= 2 E u log L, the addition rounds once:
        D_g = |d lp_g| <= (L - 1 + 2 E + A_g) u + 2 E u log L + u |lp_g|;
  * rho = exp(lp_r - lp_g): the argument is rounded once - that enters rho scaled by |lp_r - lp_g| - and is off by D_g, exp adds
    2 E u:   eta_{g,r} = |d rho| / rho <= |lp_r - lp_g| u + D_g + 2 E u;
  * omega_r: the product w_g rho rounds once, the M_r memberships (positive addends) are added in list order:
        |d omega_r| <= sum_g w_g rho_{g,r} (eta_{g,r} + M_r u);
  * lambda_r: the addend w_g rho lp_g rounds twice and inherits D_g through lp_g:
        |d lambda_r| <= sum_g w_g rho_{g,r} (|lp_g| (eta_{g,r} + (M_r + 1) u) + D_g);
  * the reduction is the one of the row weights: recursive summation of P_cls addends of which each is a product rounded
    once, against a reference that rounds each addend and the sum once (test_row_weights.py: WeightedReference with omega_r in the
    place of w_i):  (P_cls + 3) u S,  S = sum_r |omega_r v_r| (|lambda_r| for e = 0), plus sum_r |d omega_r| |v_r| (|d lambda_r|);
    the pre-combined buffer (P + 5) u (|w_pm| S_EM + S_NM) plus the same terms.
A rho below the subnormal range is 0 on both sides (the reference rounds rho to float64); the cases keep away from the
subnormal range itself: lp_r - lp_g is above -700 or is -inf.  Where two downloads of the rows differ (lp of a score-only and of
a gradient evaluation, or the fixture's lp in the LUAD case) the difference d_r of lp_r enters as d_r + max_{r' in g} d_r' in
eta and max d in D_g; it is 0 when the precondition (reproducible rows) holds.  lp_group is compared under D_g + u |lp_g|,
rho under rho (eta + u), sum_r rho - 1 under sum_r rho eta + L u."""
import ctypes as C
import importlib.util
import itertools
import math
import os

import numpy as np
import pytest

import reduction_common as RC
from eval_common import engine_pool
from reduction_common import MULTI_BATCH, MULTI_BATCH_WS, N4, PERC_MET, W_PM, WEIGHT_VALUES, Reference, U, raw_layout, red_per, stride, wsums_layout
from unknown_common import relabel, unknown_row

LD = np.longdouble
E_ULPS = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = -1


# ---- the reference and its bound ------------------------------------------------------------------------------------------------

def _group_counts(dat, ptr, idx, w):
    """(n_em, n_pat, n_unknown) by the definition, one group at a time."""
    n_em = n_pat = n_unknown = 0.0
    for g, wg in enumerate(w):
        r = dat[idx[ptr[g]]]
        n_em += wg if r[-3] == 1 else 0.0
        n_pat += wg
        n_unknown += wg if r[-1] == 4 else 0.0
    return n_em, n_pat, n_unknown


class MixReference:
    """lp_g, rho, omega, lambda and the two class sums of the module docstring, with their bounds.  lp [P], rows [P, st]: the
    per-row values (rows of no group or of weight-0 groups only may hold anything); spread [P, st], lp_spread [P]: |difference|
    between downloads of the rows / of lp."""

    def __init__(self, lp, rows, dat, ptr, idx, w, N, spread=None, lp_spread=None):
        P, G, st = lp.shape[0], len(w), stride(N)
        E2 = 2 * E_ULPS
        lpL = np.asarray(lp, dtype=np.float64).astype(LD)
        dl = np.zeros(P) if lp_spread is None else np.asarray(lp_spread, dtype=np.float64)
        spread = np.zeros((P, st)) if spread is None else spread
        self.N, self.ptr, self.idx, self.w = N, ptr, idx, w
        self.lpg, self.lpg_bound = np.zeros(G), np.zeros(G)
        self.rho, self.rho_bound, self.rho_sum_bound = np.zeros(len(idx)), np.zeros(len(idx)), np.zeros(G)
        omega, lam = np.zeros(P, dtype=LD), np.zeros(P, dtype=LD)
        d_om, d_la, abs_la, M = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
        for g in range(G):
            r = idx[ptr[g]:ptr[g + 1]]
            L = len(r)
            x = lpL[r]
            m = x.max()
            lg = m + np.log(np.exp(x - m).sum())
            rho = np.exp(x - lg)
            gap = np.where(rho > 0, np.abs(x - lg), 0).astype(np.float64)       # (a row at -inf has rho = 0: no share)
            A = float((rho * np.where(rho > 0, np.abs(x - m), 0)).sum())
            D = (L - 1 + E2 + A) * U + E2 * U * math.log(L) + U * abs(float(lg)) + dl[r].max()
            eta = gap * U + D + E2 * U + dl[r]
            rho64 = rho.astype(np.float64)
            self.lpg[g], self.lpg_bound[g] = float(lg), D + U * abs(float(lg))
            self.rho[ptr[g]:ptr[g + 1]], self.rho_bound[ptr[g]:ptr[g + 1]] = rho64, rho64 * (eta + U)
            self.rho_sum_bound[g] = float((rho64 * eta).sum()) + L * U
            if w[g] != 0:
                assert np.isfinite(float(lg)), f"group {g} has no finite alternative"
                t = w[g] * rho
                np.add.at(omega, r, t)
                np.add.at(lam, r, t * lg)
                np.add.at(d_om, r, t.astype(np.float64) * eta)
                np.add.at(d_la, r, t.astype(np.float64) * (abs(float(lg)) * eta + D))
                np.add.at(abs_la, r, t.astype(np.float64) * abs(float(lg)))
                np.add.at(M, r, 1.0)
        d_om += omega.astype(np.float64) * M * U
        d_la += abs_la * (M + 1) * U
        self.omega, self.lam = omega.astype(np.float64), lam.astype(np.float64)
        keep = self.omega != 0
        self.keep = keep
        assert np.isfinite(rows[keep]).all(), "a row that counts is not finite"
        R, sp = np.zeros((P, st)), np.zeros((P, st))
        R[keep, 0] = self.lam[keep]
        R[keep, 1:] = (omega[keep, None] * rows[keep, 1:].astype(LD)).astype(np.float64)
        sp[keep, 0] = d_la[keep]
        sp[keep, 1:] = d_om[keep, None] * np.abs(rows[keep, 1:]) + self.omega[keep, None] * spread[keep, 1:]
        self.counts = _group_counts(dat, ptr, idx, w)
        self.r = Reference(R[keep], RC.nm_class(dat)[keep], self.counts[0], N, sp[keep])

    def raw(self):
        r = self.r
        ref = raw_layout(r.em, r.nm, self.counts[0], self.counts[1], self.N)
        bound = raw_layout((r.p_em + 3) * U * r.abs_em + r.sp_em, (r.p_nm + 3) * U * r.abs_nm + r.sp_nm, 0.0, 0.0, self.N)
        return ref, bound

    def wsums(self, w_pm):
        r = self.r
        ref = wsums_layout(r.em, r.nm, w_pm, self.N)
        bound = (r.P + 5) * U * wsums_layout(r.abs_em, r.abs_nm, abs(w_pm), self.N) + wsums_layout(r.sp_em, r.sp_nm, abs(w_pm), self.N)
        return ref, bound

    def objective_bound(self, perc_met):
        from metmhn_amd import distributed as D
        w_pm, n_full = D.em_weight(*self.counts[:2], perc_met, self.counts[2])
        return self.wsums(w_pm)[1] / n_full, (w_pm, n_full)


def _make_groups(dat, sizes, seed, hub=0, leave_out=0.1, singles=False):
    """(ptr, idx, w) over the rows of `dat`: one group of every size in `sizes` (drawn from one class of rows: EM, type 0 or
    type 4 - whichever holds enough rows, in turn), `hub` groups of two that all hold one EM row (a row in hub groups), every
    other row that is not left out (a share `leave_out` of the rows, in no group) as a singleton when `singles`.  Weights from
    WEIGHT_VALUES with at least one group of weight 0; the first group's rows are also a group of weight 0."""
    rng = np.random.default_rng(seed)
    typ = dat[:, -1]
    out = rng.random(dat.shape[0]) < leave_out
    classes = [np.flatnonzero(((typ >= 1) & (typ <= 3)) & ~out), np.flatnonzero((typ == 0) & ~out), np.flatnonzero((typ == 4) & ~out)]
    lists, turn = [], 0
    for L in sizes:
        for k in range(3):
            c = classes[(turn + k) % 3]
            if len(c) >= L:
                lists.append(rng.choice(c, size=L, replace=False))
                turn += k + 1
                break
        else:
            raise AssertionError(f"no class of rows holds {L} rows")
    if len(classes[2]) >= 2:
        lists.append(classes[2][:2].copy())                    # a type-4 group in every case that has such rows
    if hub:
        em = classes[0]
        for k in range(hub):
            lists.append(np.array([em[0], em[1 + k % (len(em) - 1)]]))
    if singles:
        used = set(np.concatenate(lists).tolist())
        lists += [np.array([r]) for r in range(dat.shape[0]) if r not in used and not out[r]]
    lists.append(lists[0].copy())
    w = rng.choice(WEIGHT_VALUES[1:], size=len(lists))
    w[-1] = 0.0
    if len(lists) > 3:
        w[1] = 0.0
    w[0] = 7.25
    ptr = np.concatenate(([0], np.cumsum([len(x) for x in lists]))).astype(np.int64)
    return ptr, np.concatenate(lists).astype(np.int64), w


# ---- CPU: expand_missing against brute force ------------------------------------------------------------------------------------

def _entries_row(n, pt, mt, seeding, order, typ):
    r = np.zeros(2 * n + 3, dtype=np.int64)
    r[0:2 * n:2], r[1:2 * n:2] = pt, mt
    r[2 * n], r[2 * n + 1], r[2 * n + 2] = seeding, order, typ
    return r


def _hand_missing_cohort():
    n, m = 4, MISSING
    rows = [_entries_row(n, [1, m, 0, m], [0, 0, 0, 0], 0, -99, 0),    # A: type 0, two missing
            _entries_row(n, [m, 1, 0, 0], [0, 0, m, 0], 1, -99, 1),    # B: type 1, a missing MT entry is ignored
            _entries_row(n, [m, 0, 0, 0], [1, m, m, 0], 1, -99, 2),    # C: type 2, a missing PT entry is ignored
            _entries_row(n, [1, m, 0, 0], [m, 1, m, 0], 1, 1, 3),      # D: paired, PT and MT missing independently
            _entries_row(n, [m, 1, 0, 0], [0, 0, 0, 0], 0, -99, 4),    # E: type 4
            _entries_row(n, [1, 1, 0, m], [0, 0, 0, 0], 0, -99, 0),    # F: shares its completions with A
            _entries_row(n, [1, 0, 0, 0], [0, 0, 0, 0], 0, -99, 0),    # G: nothing missing, a completion of A
            _entries_row(n, [1, 0, 0, 0], [0, 1, 0, 0], 1, 2, 3)]      # H: paired, nothing missing
    return np.array(rows)


def _brute_completions(row, missing=MISSING):
    """Every completion of one row as a list of tuples: the missing entries of the columns its type reads take both values, a
    missing entry elsewhere 0."""
    n = (len(row) - 3) // 2
    typ = row[-1]
    read = [c for c in range(2 * n) if (c % 2 == 0 and typ in (0, 1, 3, 4)) or (c % 2 == 1 and typ in (2, 3))]
    free = [c for c in read if row[c] == missing]
    out = []
    for vals in itertools.product((0, 1), repeat=len(free)):
        r = np.where(row == missing, 0, row)
        r[free] = vals
        out.append(tuple(int(v) for v in r))
    return out


def _check_expansion(dat, G):
    P = dat.shape[0]
    assert G.rows.dtype == np.int8 and G.ptr.shape == (P + 1,) and G.idx.shape == (G.ptr[-1],) and G.ptr[0] == 0
    np.testing.assert_array_equal(G.weights, np.ones(P))
    assert len({r.tobytes() for r in G.rows}) == G.rows.shape[0], "a completed row occurs twice"
    first = [np.flatnonzero(G.idx == u)[0] for u in range(G.rows.shape[0])]
    assert (np.diff(first) > 0).all(), "the completed rows are not in order of first occurrence"
    for g in range(P):
        want = _brute_completions(dat[g])
        got = [tuple(int(v) for v in G.rows[i]) for i in G.idx[G.ptr[g]:G.ptr[g + 1]]]
        assert len(got) == len(want) == len(set(got)) and set(got) == set(want), f"group {g}"
    n = (dat.shape[1] - 3) // 2
    want_entries = {(r, c) for r in range(P) for c in range(2 * n) if dat[r, c] == MISSING}
    assert {(r, c) for r, c, _ in G.entries} == want_entries and len(G.entries) == len(want_entries)
    for r, c, alts in G.entries:
        members = G.idx[G.ptr[r]:G.ptr[r + 1]]
        ones = {s for s in range(len(members)) if G.rows[members[s], c] == 1}
        assert set(int(a) for a in alts) == ones, f"entry ({r}, {c})"
        typ = dat[r, -1]
        ignored = (c % 2 == 1 and typ in (0, 1, 4)) or (c % 2 == 0 and typ == 2)
        assert (len(alts) == 0) == ignored                     # (ignored: written as 0 in every alternative)
        assert ignored or len(alts) * 2 == len(members)        # (expanded: set in half of them)


def test_expand_missing_against_brute_force():
    from metmhn_amd import Utilityfunctions as UF
    dat = _hand_missing_cohort()
    G = UF.expand_missing(dat)
    _check_expansion(dat, G)
    assert np.diff(G.ptr).tolist() == [4, 2, 4, 8, 2, 2, 1, 1] and G.n_groups == 8
    a, f, g7 = (set(G.idx[G.ptr[g]:G.ptr[g + 1]].tolist()) for g in (0, 5, 6))
    assert f < a and g7 < a and G.rows.shape[0] == 4 + 2 + 4 + 8 + 2 + 1       # F and G add no row of their own
    np.testing.assert_array_equal(G.rows[0], np.where(dat[0] == MISSING, 0, dat[0]))
    rng = np.random.default_rng(3)
    big = RC.typed_cohort(N4, 60, 4).astype(np.int64)
    big[:, :2 * N4] = np.where(rng.random((60, 2 * N4)) < 0.2, MISSING, big[:, :2 * N4])
    _check_expansion(big, UF.expand_missing(big))
    other = np.where(dat == MISSING, 9, dat)                   # another marker
    np.testing.assert_array_equal(UF.expand_missing(other, missing=9).rows, G.rows)


def test_expand_missing_refusals():
    import pandas as pd
    from metmhn_amd import Utilityfunctions as UF
    dat = _hand_missing_cohort()
    with pytest.raises(ValueError, match=r"row 3 has 3 unobserved entries.*max_alternatives = 4"):
        UF.expand_missing(dat, max_alternatives=4)
    df = pd.DataFrame(dat, index=[f"pat_{c}" for c in "ABCDEFGH"])
    with pytest.raises(ValueError, match=r"row 'pat_D' has 3 unobserved"):
        UF.expand_missing(df, max_alternatives=7)
    assert UF.expand_missing(df, max_alternatives=8).rows.shape[0] == 21
    for col, what in ((-3, "seeding"), (-2, "order"), (-1, "type")):
        bad = dat.copy()
        bad[5, col] = MISSING
        with pytest.raises(ValueError, match=rf"{what} column of row 5"):
            UF.expand_missing(bad)


# ---- CPU: the definition against the dense oracle ---------------------------------------------------------------------------------

def _compatible(bits, obs):
    """Is the full state `bits` (0 / 1 per event) compatible with the observation `obs` (0 / 1 / MISSING per event)?"""
    return all(o == MISSING or o == b for b, o in zip(bits, obs))


def _dense_single_states(lt, dp, dm, typ, seeding):
    """P(the tumour is observed in state x) for every x of the FULL single-tumour space (bit j = event j, bit n = seeding) of a
    row of type 0 / 1 (PT) or 2 (MT), from oracle.dense's generator and observation rates: one dense solve."""
    from oracle import dense
    n = lt.shape[0] - 1
    th, edp, edm = np.exp(lt), np.exp(dp), np.exp(dm)
    full = np.ones(n + 1, dtype=np.int64)
    if typ in (0, 1):
        th_pt = th.copy()
        th_pt[:n, n] = 1.0
        Q, D = dense.single_Q(th_pt, full), dense.single_D(edp, full)
    else:
        Q = dense.single_Q(th, full)
        half = 2 ** n
        D = np.concatenate((dense.single_D(np.append(edp[:n], 1.0), full)[:half], dense.single_D(edm, full)[half:]))
    e0 = np.zeros(Q.shape[0])
    e0[0] = 1.0
    return D * np.linalg.solve(np.diag(D) - Q, e0)


def _dense_row_marginal(lt, dp, dm, row, fix=None):
    """P(the observed entries of a single-tumour row) summed over the compatible full states; fix = (column, value): only
    the states with that entry."""
    n = lt.shape[0] - 1
    typ = int(row[-1])
    obs = list(row[0:2 * n:2] if typ in (0, 1) else row[1:2 * n:2]) + [1 if typ == 2 else int(row[2 * n])]
    if fix is not None:
        obs[fix[0] // 2] = fix[1]
    p = _dense_single_states(lt, dp, dm, typ, obs[-1])
    return sum(p[x] for x in range(2 ** (n + 1)) if _compatible([(x >> j) & 1 for j in range(n + 1)], obs))


def _dense_paired_marginal(lt, dp, dm, row, fix=None):
    """The same for a paired row of order 1 (PT observed first): the joint chain on the full space of 2n + 1 slots up to the PT
    observation, every seeded state whose PT part is compatible handed to the MT chain, which runs to the MT observation."""
    from oracle import dense
    n = lt.shape[0] - 1
    assert row[-1] == 3 and row[-2] == 1 and row[2 * n] == 1
    obs = [int(v) for v in row[:2 * n]]
    if fix is not None:
        obs[fix[0]] = fix[1]
    full = np.ones(2 * n + 1, dtype=np.int64)
    Q = dense.joint_Q(lt, full)
    Dp, Dm = dense.joint_D(dp, dm, full)
    e0 = np.zeros(Q.shape[0])
    e0[0] = 1.0
    pi = np.linalg.solve(np.diag(Dp + Dm) - Q, e0)
    th, edm = np.exp(lt), np.exp(dm)
    ones = np.ones(n + 1, dtype=np.int64)
    QM, DM = dense.single_Q(th, ones), dense.single_D(edm, ones)
    v = np.zeros(2 ** (n + 1))
    for x in range(2 ** (2 * n + 1)):
        if not (x >> (2 * n)) & 1:
            continue
        pt = [(x >> (2 * j)) & 1 for j in range(n)]
        mt = [(x >> (2 * j + 1)) & 1 for j in range(n)]
        if _compatible(pt, obs[0::2]):
            v[sum(b << j for j, b in enumerate(mt)) | 1 << n] += Dp[x] * pi[x]
    z = DM * np.linalg.solve(np.diag(DM) - QM, v)
    return sum(z[y] for y in range(2 ** n, 2 ** (n + 1)) if _compatible([(y >> j) & 1 for j in range(n)], obs[1::2]))


def _oracle_group_lp(lt, dp, dm, G, g):
    from oracle import metmhn_oracle as O
    lps = np.array([float(O.patient_lp(lt, dp, dm, G.rows[i])[0]) for i in G.idx[G.ptr[g]:G.ptr[g + 1]]])
    return lps, float(np.logaddexp.reduce(lps))


def test_mixture_is_the_marginal_of_the_dense_oracle():
    """logsumexp of the oracle's lp over the completions = log of the dense oracle's probability summed over the compatible
    states of the full space: two independent fp64 computations, 1e-12 relative as in the dense-oracle tests."""
    from metmhn_amd import Utilityfunctions as UF
    lt, dp, dm = RC.params(N4)
    dat = _hand_missing_cohort()
    dat = np.vstack((dat[[0, 1, 2, 5, 6]], _entries_row(N4, [MISSING, 0, MISSING, 0], [0, 0, 0, 0], 0, -99, 0)[None, :]))   # (the empty genotype among the completions)
    G = UF.expand_missing(dat)
    for g in range(dat.shape[0]):
        _, lp_mix = _oracle_group_lp(lt, dp, dm, G, g)
        lp_dense = math.log(_dense_row_marginal(lt, dp, dm, dat[g]))
        assert abs(lp_mix - lp_dense) <= 1e-12 * abs(lp_dense), f"row {g}: {lp_mix!r} against {lp_dense!r}"


def test_mixture_of_a_paired_row_is_the_marginal_of_the_dense_oracle():
    from metmhn_amd import Utilityfunctions as UF
    lt, dp, dm = RC.params(N4)
    dat = _hand_missing_cohort()[[3]]
    G = UF.expand_missing(dat)
    assert G.ptr[-1] == 8
    _, lp_mix = _oracle_group_lp(lt, dp, dm, G, 0)
    lp_dense = math.log(_dense_paired_marginal(lt, dp, dm, dat[0]))
    assert abs(lp_mix - lp_dense) <= 1e-12 * abs(lp_dense), f"{lp_mix!r} against {lp_dense!r}"


# ---- CPU: the kernels' order of operations ----------------------------------------------------------------------------------------

def _butterfly(lanes, op):
    v = lanes.copy()
    o = 32
    while o:
        v = op(v, v[np.arange(64) ^ o])
        o >>= 1
    assert (v == v[0]).all()
    return v[0]


def _mix_replay(lp, rows, kinds, ptr, idx, w, batches, order, N, mode, a, b, reverse=False, defect=False):
    """What the device writes, in float64 NumPy: k_group_lse (lane l takes the alternatives l, l + 64, ..., butterfly over the
    lanes), k_mix_weights (the memberships of a row in group order; reverse: in the opposite order), k_reduce_rows_mix in the
    chunks and batch order of test_row_weights.py: _replay_w.  defect: one row's rho is taken from the wrong group."""
    P, G, st = lp.shape[0], len(w), stride(N)
    lpg = np.zeros(G)
    for g in range(G):
        x = lp[idx[ptr[g]:ptr[g + 1]]]
        mx = np.full(64, -np.inf)
        for k, v in enumerate(x):
            mx[k % 64] = max(mx[k % 64], v)
        m = _butterfly(mx, np.maximum)
        s = np.zeros(64)
        for k, v in enumerate(x):
            s[k % 64] += np.exp(v - m)
        lpg[g] = m + np.log(_butterfly(s, np.add))
    members = [[] for _ in range(P)]
    for g in range(G):
        for r in idx[ptr[g]:ptr[g + 1]]:
            members[r].append(g)
    victim = idx[ptr[0]] if defect else -1
    omega, lam = np.zeros(P), np.zeros(P)
    for r in range(P):
        for g in (members[r][::-1] if reverse else members[r]):
            if w[g] == 0:
                continue
            lg = lpg[(g + 1) % G] if r == victim else lpg[g]
            t = w[g] * np.exp(lp[r] - lg)
            omega[r] += t
            lam[r] += t * lg
    sums = np.zeros((2, st))
    r0 = 0
    for npat, perm in zip(batches, order):
        per = red_per(npat)
        pats = r0 + perm
        acc = np.zeros((2, st))
        for c in range((npat + per - 1) // per):
            part = np.zeros((2, st))
            for i in range(c * per, min(npat, (c + 1) * per)):
                r = pats[i]
                if omega[r] == 0:
                    continue
                add = omega[r] * rows[r]
                add[0] = lam[r]
                part[1 if kinds[r] in (0, 4, 5) else 0] += add
            acc += part
        sums += acc
        r0 += npat
    em, nm = sums
    return raw_layout(em, nm, a, b, N) if mode == 1 else wsums_layout(em, nm, a, N)


def _replay_case(P, batches, sizes, seed, **how):
    N = N4 + 1
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((P, stride(N))) * 10.0 ** rng.uniform(-3, 3, size=(P, stride(N)))
    lp = -rng.uniform(1.0, 30.0, size=P)
    rows[:, 0] = lp
    kinds = rng.integers(0, 6, size=P)
    dat = np.zeros((P, 2 * N4 + 3), dtype=np.int8)
    dat[:, -1] = np.where(kinds == 4, 0, np.where(kinds == 5, 4, kinds))
    dat[:, -3] = (kinds >= 1) & (kinds <= 3)
    ptr, idx, w = _make_groups(dat, sizes, seed + 1, hub=40 if P > 64 else 3, singles=P <= 64)
    order = [rng.permutation(nb) for nb in batches]
    ref = MixReference(lp, rows, dat, ptr, idx, w, N)
    c = ref.counts
    r1 = RC.within(_mix_replay(lp, rows, kinds, ptr, idx, w, batches, order, N, 1, c[0], c[1], **how), *ref.raw(), "replayed raw")
    r2 = RC.within(_mix_replay(lp, rows, kinds, ptr, idx, w, batches, order, N, 2, W_PM, 0.0, **how), *ref.wsums(W_PM), "replayed pre-combined")
    return max(r1, r2)


BIG_SIZES = (1, 2, 63, 64, 65, 257)
REPLAY_SHAPES = [(32, [32], (1, 2, 5)), (33, [33], (1, 2, 5)), (4097, [4097], BIG_SIZES), (4097, [1400, 1400, 1297], BIG_SIZES)]
REPLAY_IDS = [f"P{P}-{len(b)}batches" for P, b, _ in REPLAY_SHAPES]


@pytest.mark.parametrize("P,batches,sizes", REPLAY_SHAPES, ids=REPLAY_IDS)
def test_replayed_mixing_is_within_the_bound(P, batches, sizes):
    """The reference and the bound alone: the kernels' operations in float64 NumPy pass at the shapes of the GPU test - and so
    do they with the memberships of every row added in the opposite order."""
    a = _replay_case(P, batches, sizes, seed=300 + P)
    b = _replay_case(P, batches, sizes, seed=300 + P, reverse=True)
    print(f"mixing replay P={P} {batches}: worst error / bound {a:.3f}, memberships reversed {b:.3f}")
    assert max(a, b) <= 1.0


@pytest.mark.parametrize("P,batches,sizes", REPLAY_SHAPES, ids=REPLAY_IDS)
def test_rho_of_the_wrong_group_breaks_the_bound(P, batches, sizes):
    with pytest.raises(AssertionError):
        _replay_case(P, batches, sizes, seed=300 + P, defect=True)


def test_group_counts_against_a_loop():
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    dat = RC.typed_cohort(N4, 97, 3)
    for seed in range(3):
        ptr, idx, w = _make_groups(dat, (1, 2, 5, 9), seed, hub=3, singles=seed == 1)
        assert ro._group_counts(dat, ptr, idx, w) == _group_counts(dat, ptr, idx, w)
    ptr, idx, w = np.arange(98), np.arange(97), np.ones(97)    # singletons of weight one: the counts of the cohort
    assert ro._group_counts(dat, ptr, idx, w) == ro._global_counts(dat)
    t4 = np.flatnonzero(dat[:, -1] == 4)[:2]
    assert ro._group_counts(dat, np.array([0, 2]), t4, np.array([3.0])) == (0.0, 3.0, 3.0)
    G = UF.expand_missing(_hand_missing_cohort())
    assert ro._group_counts(G.rows, *ro._group_arrays(G, G.rows.shape[0])) == (4.0, 8.0, 1.0)
    with pytest.raises(ValueError, match="outside the 3 rows"):
        ro._group_arrays(G, 3)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def make_engine():
    yield from engine_pool()


def _all_outputs(e, lt, dp, dm):
    return [e.cohort_sums(lt, dp, dm), e.cohort_sums(lt, dp, dm, with_grad=False), RC.wsums(e, lt, dp, dm, W_PM),
            RC.wsums(e, lt, dp, dm, W_PM, with_grad=False), RC.flat(e.score_and_grad(lt, dp, dm, PERC_MET)), e.score(lt, dp, dm, PERC_MET)]


def _at_least_three_batches(dat, n):
    """test_cohort_reduction.py: test_multi_batch_reduction's count of the least number of batches under MULTI_BATCH_WS."""
    N = n + 1
    all_zero = (dat[:, -1] == 0) & (dat[:, 0:2 * n + 1:2].sum(axis=1) == 0)
    charged = dat.shape[0] * ((stride(N) + 1) * 8 + 2 * 8) + int((~all_zero).sum()) * ((N * N + 65) * 8 + 4 * 8)
    assert -(-charged // MULTI_BATCH_WS) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("how", ("zerocopy", "zerocopy0", "multibatch"))
def test_singleton_groups_of_weight_one_change_nothing(make_engine, how):
    """Every row its own group, weight 1: the same bits as without groups in both buffers and in mmhn_score_and_grad - and
    again after the groups are removed.  (lp_g = lp + log 1, rho = exp 0: every step is exact.)"""
    lt, dp, dm = RC.params(N4)
    P = 4097
    dat = RC.cohort(N4, P)
    e = make_engine(N4, zerocopy=how != "zerocopy0", workspace=MULTI_BATCH_WS if how == "multibatch" else None)
    e.set_cohort(dat)
    assert e.row_groups is None
    plain = _all_outputs(e, lt, dp, dm)
    rows_plain = RC.rows_of(e, lt, dp, dm)
    counts = e.row_weight_sums
    ptr, idx = np.arange(P + 1), np.arange(P)
    other = _make_groups(dat, BIG_SIZES, 5, hub=40)
    for groups in ((ptr, idx, None), None, other, (ptr, idx[::-1].copy(), np.ones(P))):
        if groups is None:
            e.set_row_groups(None, None)
            assert e.row_groups is None
        else:
            e.set_row_groups(*groups)
            assert np.array_equal(e.row_groups[0], groups[0]) and np.array_equal(e.row_groups[1], groups[1])
        got = _all_outputs(e, lt, dp, dm)
        same = all(np.array_equal(a, b) for a, b in zip(got, plain))
        if groups is other:
            assert not same and e.row_weight_sums != counts   # (the groups in between do reach the sums)
        else:
            assert same and e.row_weight_sums == counts
        np.testing.assert_array_equal(RC.rows_of(e, lt, dp, dm), rows_plain)        # patient_grads stays per row and unmixed
    e.set_row_groups(None, None)
    assert e.row_groups is None and e.row_weights is None


def _check_mixed(e, dat, groups, lt, dp, dm, tag, lp_fixture=None):
    """Both buffers of `e` (holding dat and the groups) with and without gradient against the reference of its own rows."""
    ptr, idx, w = groups
    r1, r2 = RC.rows_of(e, lt, dp, dm), RC.rows_of(e, lt, dp, dm)
    s1, s2 = RC.rows_of(e, lt, dp, dm, False), RC.rows_of(e, lt, dp, dm, False)
    with np.errstate(invalid="ignore"):
        dl = np.nan_to_num(np.maximum(np.maximum(np.abs(r1[:, 0] - r2[:, 0]), np.abs(s1[:, 0] - s2[:, 0])), np.abs(r1[:, 0] - s1[:, 0])), nan=0.0)
        sp, sp0 = np.nan_to_num(np.abs(r1 - r2), nan=0.0), np.nan_to_num(np.abs(s1 - s2), nan=0.0)
    ref = MixReference(r1[:, 0], r1, dat, ptr, idx, w, e.N, sp, dl)
    ref0 = MixReference(s1[:, 0], s1, dat, ptr, idx, w, e.N, sp0, dl)
    s = e.cohort_sums(lt, dp, dm)
    a = RC.within(s, *ref.raw(), tag + " cohort_sums")
    s0 = e.cohort_sums(lt, dp, dm, with_grad=False)
    RC.within(s0, *ref0.raw(), tag + " cohort_sums(with_grad=False)")
    assert not s0[4:].any(), f"{tag}: gradient entries of a score-only evaluation"
    b = RC.within(RC.wsums(e, lt, dp, dm, W_PM), *ref.wsums(W_PM), tag + " cohort_wsums")
    ws0 = RC.wsums(e, lt, dp, dm, W_PM, with_grad=False)
    RC.within(ws0, *ref0.wsums(W_PM), tag + " cohort_wsums(with_grad=False)")
    assert not ws0[1:].any(), f"{tag}: gradient entries of a score-only pre-combined evaluation"
    assert (s[2], s[3]) == ref.counts[:2] and e.row_weight_sums == ref.counts, f"{tag}: counts {s[2:4]}, {e.row_weight_sums}"
    lpg, rho = e.group_posteriors(lt, dp, dm)
    c = RC.within(lpg, ref0.lpg, ref0.lpg_bound, tag + " lp_group")
    d = RC.within(rho, ref0.rho, ref0.rho_bound, tag + " rho")
    tot = np.array([rho[ptr[g]:ptr[g + 1]].sum() for g in range(len(w))])
    RC.within(tot, np.ones(len(w)), ref0.rho_sum_bound + U * np.diff(ptr), tag + " sum of rho")
    print(f"{tag}: worst error / bound: raw {a:.3f}, pre-combined {b:.3f}, lp_group {c:.3f}, rho {d:.3f}; dropped rows {int((~ref.keep).sum())}")
    return s, ref


MIXED_SHAPES = [(32, "f64", None), (33, "f64", None), (4097, "f64", None), (MULTI_BATCH[1], "f64", MULTI_BATCH_WS), (33, "f32", None),
                (MULTI_BATCH[1], "f32", MULTI_BATCH_WS)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,dtype,workspace", MIXED_SHAPES, ids=[f"P{P}-{d}-{'multibatch' if ws else 'onebatch'}" for P, d, ws in MIXED_SHAPES])
def test_mixed_sums_against_the_reference(make_engine, P, dtype, workspace):
    """Groups of 1, 2, 63, 64, 65 and 257 rows (EM, NM and type-4 groups), a row in 40 groups, rows in no group, groups of weight
    0, weights from WEIGHT_VALUES: both buffers, with and without gradient, lp_group and rho under the derived bound.  The
    MULTI_BATCH cohort under MULTI_BATCH_WS takes at least three batches, its groups span them: two sweeps with a gradient."""
    n = MULTI_BATCH[0] if workspace else N4
    lt, dp, dm = RC.params(n)
    dat = RC.typed_cohort(n, P, 11)
    if workspace:
        _at_least_three_batches(dat, n)
    big = P > 64
    groups = _make_groups(dat, BIG_SIZES if big else (1, 2, 5), 20 + P, hub=40 if big else 3, singles=not big)
    assert (np.bincount(groups[1], minlength=P) == 0).any() and (np.bincount(groups[1], minlength=P) >= (40 if big else 3)).any()
    assert (dat[groups[1][groups[0][:-1]], -1] == 4).any() and (groups[2] == 0).sum() >= 2
    e = make_engine(n, dtype=dtype, workspace=workspace)
    e.set_cohort(dat)
    e.set_row_groups(*groups)
    _check_mixed(e, dat, groups, lt, dp, dm, f"P={P} {dtype} ws={workspace}")
    second = _make_groups(dat, (2, 3, 64) if big else (3, 2), 21 + P, hub=2, singles=True)      # other groups on the same plan
    e.set_row_groups(*second)
    _check_mixed(e, dat, second, lt, dp, dm, f"P={P} {dtype} ws={workspace} second groups")


@pytest.mark.gpu
def test_an_alternative_of_probability_zero(make_engine):
    """theta_00 = exp(-800) is 0 in float64: every row with event 0 has probability 0, lp = -inf, more than 745 below its
    group's other alternative.  rho is exactly (1, 0), nothing becomes NaN, and the sums are those of the other rows."""
    lt, dp, dm = RC.params(N4)
    lt = np.array(lt, copy=True)
    lt[0, 0] = -800.0
    dat = np.array([_entries_row(N4, [0, 1, 0, 0], [0, 0, 0, 0], 0, -99, 0), _entries_row(N4, [1, 1, 0, 0], [0, 0, 0, 0], 0, -99, 0),
                    _entries_row(N4, [0, 0, 1, 0], [0, 0, 0, 0], 1, -99, 1), _entries_row(N4, [1, 0, 1, 0], [0, 0, 0, 0], 1, -99, 1),
                    _entries_row(N4, [0, 0, 0, 1], [0, 0, 0, 0], 0, -99, 0)], dtype=np.int8)
    e = make_engine(N4, tag=4)
    e.set_cohort(dat)
    lp = e.patient_grads(lt, dp, dm, with_grad=False)
    assert np.isfinite(lp[[0, 2, 4]]).all() and (lp[[1, 3]] == -np.inf).all(), lp
    groups = (np.array([0, 2, 4, 5, 7]), np.array([0, 1, 2, 3, 4, 1, 4]), np.array([2.0, 0.5, 1.0, 0.0]))
    e.set_row_groups(*groups)
    lpg, rho = e.group_posteriors(lt, dp, dm)
    np.testing.assert_array_equal(rho[:5], [1.0, 0.0, 1.0, 0.0, 1.0])
    np.testing.assert_array_equal(lpg[:3], lp[[0, 2, 4]])
    s, _ = _check_mixed(e, dat, groups, lt, dp, dm, "an alternative of probability 0")
    assert np.isfinite(s).all() and np.isfinite(RC.flat(e.score_and_grad(lt, dp, dm, PERC_MET))).all()


@pytest.mark.gpu
def test_posteriors_of_a_status_pair_are_p_seeded(make_engine):
    """A type-4 row is the mixture of its genotype as a type-0 and as a type-1 row.  The two lie in different blocks of the
    sums, so they cannot share a group (refused); their lp_group as singletons give rho = exp(lp1 - logaddexp(lp0, lp1)), which
    reproduces patient_status's p_seeded of the type-4 row.  Bound: r1 = 1 / (1 + exp(lp0 - lp1)) has |d r1 / d lp| <= 1 / 4; each
    lp is a logarithm, E ulps of its own size off, on either route: 0.25 * 2 * 2 E u (|lp0| + |lp1|), and 8 u for the
    handful of roundings of the two closed forms."""
    lt, dp, dm = RC.params(N4)
    t4 = np.array([unknown_row(N4, ev) for ev in ([1], [0, 2], [0, 1, 2, 3])], dtype=np.int8)
    dat = np.vstack((t4, [relabel(r, 0) for r in t4], [relabel(r, 1) for r in t4]))
    e = make_engine(N4, tag=5)
    e.set_cohort(dat)
    _, p_seeded = e.patient_status(lt, dp, dm)
    with pytest.raises(RuntimeError, match=r"group 0 mixes the two blocks.*row 3.*row 6"):
        e.set_row_groups([0, 2], [3, 6])
    e.set_row_groups(np.arange(10), np.arange(9))
    lpg, rho = e.group_posteriors(lt, dp, dm)
    np.testing.assert_array_equal(rho, np.ones(9))
    lp0, lp1 = lpg[3:6], lpg[6:9]
    r1 = np.exp(lp1 - np.logaddexp(lp0, lp1))
    bound = 0.25 * 2 * 2 * E_ULPS * U * (np.abs(lp0) + np.abs(lp1)) + 8 * U
    ratio = RC.within(r1, p_seeded[:3], bound, "rho of the status pair against p_seeded")
    print(f"status pair: worst error / bound {ratio:.3f}")
    np.testing.assert_allclose(lpg[:3], np.logaddexp(lp0, lp1), rtol=1e-14)


# ---- GPU: the objective by the definition ---------------------------------------------------------------------------------------

def _masked_cohort(n, P, seed, frac=0.15, most=3):
    """synthetic.mixed_cohort (types 0 - 3) with a share `frac` of the event entries missing, at most `most` per row."""
    from metmhn_amd import synthetic
    dat = np.asarray(synthetic.mixed_cohort(n, P, seed=seed, p_event=0.35)).astype(np.int64)
    rng = np.random.default_rng(seed + 1)
    for r in range(P):
        cols = np.flatnonzero(rng.random(2 * n) < frac)[:most]
        dat[r, cols] = MISSING
    return dat


def _mixed_objective(lt, dp, dm, G, dat, perc_met):
    """(score, d_theta, d_dp, d_dm) by the definition: oracle.cref's rows of the completions mixed in NumPy, then
    unknown_common.objective over the groups as patients."""
    from oracle import cref
    from unknown_common import objective
    N = lt.shape[0]
    lp, g, a, b = cref.patients(lt, dp, dm, G.rows)
    rows = np.concatenate((lp[:, None], g.reshape(-1, N * N), a, b), axis=1)
    mixed = np.zeros((G.n_groups, rows.shape[1]))
    for k in range(G.n_groups):
        r = G.idx[G.ptr[k]:G.ptr[k + 1]]
        lg = np.logaddexp.reduce(lp[r])
        mixed[k] = (np.exp(lp[r] - lg)[:, None] * rows[r]).sum(axis=0)
        mixed[k, 0] = lg
    return objective(mixed, dat, perc_met)[:4]


def _mixed_objective_reg(params, G, dat, perc_met, w_penal):
    from oracle import metmhn_oracle as O
    N = (dat.shape[1] - 3) // 2 + 1
    lt, dp, dm = params[:N * N].reshape(N, N), params[N * N:N * N + N], params[N * N + N:]
    sc, g, a, b = _mixed_objective(lt, dp, dm, G, dat, perc_met)
    pen, pen_ = O.symmetric_penal(params, N)
    return -sc + w_penal * pen, -np.concatenate((g.flatten(), a, b)) + w_penal * pen_


@pytest.mark.gpu
def test_objective_with_missing_entries_by_definition():
    """score_and_grad_reg(..., groups=expand_missing(dat)) against oracle.cref's rows mixed in NumPy (1e-9 on the value, 1e-7 on the
    gradient), and the gradient as central differences of score_reg(..., groups=) along four random directions (step and
    tolerance of test_gpu_parity.py: test_full_size_gradient_is_directional_difference_of_score)."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    n = N4
    lt, dp, dm = RC.params(n)
    dat = _masked_cohort(n, 48, 31)
    G = UF.expand_missing(dat)
    assert G.ptr[-1] > 2 * 48 and G.rows.shape[0] < G.ptr[-1] and {0, 1, 2, 3} <= set(dat[:, -1].tolist())
    params = np.concatenate((np.asarray(lt).flatten(), dp, dm))
    try:
        v, g = ro.score_and_grad_reg(params, G.rows, PERC_MET, ro.symmetric_penal, 1e-2, groups=G)
        v_ref, g_ref = _mixed_objective_reg(params, G, dat, PERC_MET, 1e-2)
        np.testing.assert_allclose(float(v), v_ref, rtol=1e-9)
        np.testing.assert_allclose(g, g_ref, rtol=1e-7, atol=1e-10)
        sc = ro.score(lt, dp, dm, G.rows, PERC_MET, groups=G)
        np.testing.assert_allclose(float(sc), _mixed_objective(lt, dp, dm, G, dat, PERC_MET)[0], rtol=1e-9)
        res = ro.score_and_grad(lt, dp, dm, G.rows, PERC_MET, groups=G)
        assert float(res[0]) == float(sc) or abs(float(res[0]) - float(sc)) <= 1e-12 * abs(float(sc))
        rng = np.random.default_rng(5)
        h = 1e-5
        for _ in range(4):
            u = rng.standard_normal(params.size)
            u /= np.linalg.norm(u)
            fd = (float(ro.score_reg(params + h * u, G.rows, PERC_MET, ro.symmetric_penal, 1e-2, groups=G))
                  - float(ro.score_reg(params - h * u, G.rows, PERC_MET, ro.symmetric_penal, 1e-2, groups=G))) / (2 * h)
            np.testing.assert_allclose(float(g @ u), fd, rtol=2e-6, atol=1e-9)
        with pytest.raises(ValueError, match="exclude each other"):
            ro.score(lt, dp, dm, G.rows, PERC_MET, weights=np.ones(G.rows.shape[0]), groups=G)
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_impute_missing_against_the_dense_oracle():
    """P(entry = 1 | the row's observed entries) and lp of every original row against the dense oracle on the full space
    (single-tumour rows and the paired row of the hand cohort; n = 4, 1e-12 relative).  An entry in an ignored column: NaN."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    lt, dp, dm = RC.params(N4)
    dat = _hand_missing_cohort()[[0, 1, 2, 3, 5, 6]]
    G = UF.expand_missing(dat)
    try:
        p, lp = ro.impute_missing(lt, dp, dm, G)
        assert p.shape == (len(G.entries),) and lp.shape == (dat.shape[0],)
        marg = [_dense_paired_marginal if r[-1] == 3 else _dense_row_marginal for r in dat]
        for g in range(dat.shape[0]):
            want = math.log(marg[g](lt, dp, dm, dat[g]))
            assert abs(lp[g] - want) <= 1e-12 * abs(want), f"lp of row {g}: {lp[g]!r} against {want!r}"
        seen = 0
        for k, (r, c, alts) in enumerate(G.entries):
            if len(alts) == 0:
                assert np.isnan(p[k])
                continue
            want = marg[r](lt, dp, dm, dat[r], fix=(c, 1)) / marg[r](lt, dp, dm, dat[r])
            assert abs(p[k] - want) <= 1e-12 * want, f"entry ({r}, {c}): {p[k]!r} against {want!r}"
            seen += 1
        assert seen >= 8
    finally:
        ro.invalidate()


# ---- GPU: refusals, guard, cache ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(make_engine):
    """Every refused call raises with a message that names the group or row and leaves the groups held before in place; the
    next evaluation is the one of the groups held."""
    from metmhn_amd import Engine, _lib
    from metmhn_amd.engine import unique_id
    lt, dp, dm = RC.params(N4)
    dat = RC.typed_cohort(N4, 33, 2)
    e = make_engine(N4, tag=3)
    e.set_cohort(dat)
    good = _make_groups(dat, (1, 2, 5), 3, hub=3, singles=True)
    e.set_row_groups(*good)
    held = e.cohort_sums(lt, dp, dm)
    em = np.flatnonzero((dat[:, -1] >= 1) & (dat[:, -1] <= 3))
    nm = np.flatnonzero(dat[:, -1] == 0)
    t4 = np.flatnonzero(dat[:, -1] == 4)

    def c_call(ptr, rows, w):
        ptr, rows, w = np.asarray(ptr, dtype=np.int64), np.asarray(rows, dtype=np.int64), np.asarray(w, dtype=np.float64)
        i64 = C.POINTER(C.c_int64)
        status = e.lib.mmhn_set_row_groups(e.h, ptr.ctypes.data_as(i64), len(ptr) - 1, rows.ctypes.data_as(i64), w.ctypes.data_as(C.POINTER(C.c_double)))
        return status, e.lib.mmhn_last_error().decode()

    def still_held():
        for a, b in zip(e.row_groups, good):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(e.cohort_sums(lt, dp, dm), held)

    cases = [(([1, 2, 3], [0, 1, 2], None), r"ptr\[0\] must be 0 \(group 0\)"),
             (([0, 2, 1, 3], [0, 1, 2], None), r"group 1: ptr is decreasing"),
             (([0, 1, 1, 2], [em[0], em[1]], None), r"group 1 is empty"),
             (([0, 1, 3], [em[0], em[1], 33], None), r"group 1 holds row 33, outside the cohort of 33 rows"),
             (([0, 1, 2], [em[0], -1], None), r"group 1 holds row -1"),
             (([0, 1, 2, 3], [em[0], em[1], em[2]], [1.0, -0.5, -1.0]), r"weight of group 1 is negative"),
             (([0, 1, 2, 3], [em[0], em[1], em[2]], [1.0, 1.0, np.nan]), r"weight of group 2 is not finite"),
             (([0, 1, 2], [em[0], em[1]], [np.inf, 1.0]), r"weight of group 0 is not finite"),
             (([0, 1, 2], [em[0], em[1]], [0.0, 0.0]), r"every weight is 0 \(group 0"),
             (([0, 1, 3], [em[0], em[1], nm[0]], None), rf"group 1 mixes the two blocks.*row {em[1]} is EM, row {nm[0]} is not"),
             (([0, 2], [nm[0], em[0]], None), rf"group 0 mixes the two blocks.*row {nm[0]} is NM"),
             (([0, 1, 3], [nm[0], nm[1], t4[0]], None), rf"group 1 mixes rows of type 4 with others \(rows {nm[1]} and {t4[0]}\)")]
    for args, pattern in cases:
        with pytest.raises(RuntimeError, match=pattern):
            e.set_row_groups(*args)
        still_held()
    with pytest.raises(ValueError, match="one weight per group"):
        e.set_row_groups([0, 1, 2], [0, 1], [1.0])
    with pytest.raises(ValueError, match=r"points outside rows \(length 2\): group 1"):
        e.set_row_groups([0, 1, 3], [em[0], em[1]])
    status, msg = c_call([0, 2, 1], [em[0], em[1], em[2]], [1.0, 1.0])
    assert status != 0 and "group 1: ptr is decreasing" in msg, msg
    still_held()
    # row weights and row groups exclude each other
    with pytest.raises(RuntimeError, match=r"holds row groups \(group 0"):
        e.set_row_weights(np.ones(33))
    e.set_row_weights(None)                                    # nothing to remove: fine
    still_held()
    e.set_row_groups(None, None)
    e.set_row_weights(np.ones(33))
    with pytest.raises(RuntimeError, match=r"holds row weights \(row 0\)"):
        e.set_row_groups(*good)
    assert e.row_groups is None and np.array_equal(e.row_weights, np.ones(33))
    e.set_row_weights(None)
    e.set_row_groups(*good)
    # between _begin and _end
    e.cohort_sums_begin(lt, dp, dm)
    with pytest.raises(RuntimeError, match="has not been collected"):
        e.set_row_groups(np.arange(34), np.arange(33))
    with pytest.raises(RuntimeError, match="has not been collected"):
        e.set_row_groups(None, None)
    np.testing.assert_array_equal(e.cohort_sums_end(), held)
    still_held()
    # a communicator of one rank is fine (the refusal of more than one rank needs a second GPU to make such a communicator;
    # the host-side refusal of sharded groups is test_sharded_groups_are_refused)
    e.comm_init(unique_id(), 0, 1)
    still_held()
    e.comm_destroy()
    # set_cohort clears them; group_posteriors needs groups
    e.set_cohort(dat)
    assert e.row_groups is None and e.row_weight_sums == (float(dat[:, -3].sum()), 33.0, float(len(t4)))
    with pytest.raises(RuntimeError, match="needs row groups"):
        e.group_posteriors(lt, dp, dm)
    # an engine without a cohort
    with Engine(N4) as fresh:
        with pytest.raises(RuntimeError, match=r"holds no cohort \(row 0 of group 0"):
            fresh.set_row_groups([0, 1], [0])
        fresh.set_row_groups(None, None)
        assert fresh.row_groups is None
    assert _lib.ABI_VERSION == e.lib.mmhn_abi_version() == 8


@pytest.mark.gpu
def test_guard_rebuild_keeps_the_groups():
    """groups.rows edited in place between two ro.score(..., groups=G): the guard's rebuild (set_cohort clears the groups) applies
    them again - the second value is that of a fresh engine on the edited rows with the groups."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    lt, dp, dm = RC.params(N4)
    G = UF.expand_missing(_masked_cohort(N4, 33, 8))
    try:
        before = ro.score(lt, dp, dm, G.rows, PERC_MET, groups=G)
        eng = ro._engine_for(G.rows, check=False)
        assert eng._groups is not None and np.array_equal(eng.row_groups[1], G.idx)
        solo = int(np.flatnonzero(np.bincount(G.idx, minlength=G.rows.shape[0]) == 1)[0])
        g_of = int(np.searchsorted(G.ptr, np.flatnonzero(G.idx == solo)[0], side="right") - 1)
        free = [c for c in range(0, 2 * N4, 2) if G.rows[solo, c] == 0 and G.rows[solo, -1] in (0, 1)] or \
               [c for c in range(1, 2 * N4, 2) if G.rows[solo, c] == 0]
        G.rows[solo, free[0]] = 1                              # one more event in one completion: same class, same seeding
        after = ro.score(lt, dp, dm, G.rows, PERC_MET, groups=G)
        assert ro._engine_for(G.rows, check=False) is eng and np.array_equal(eng.row_groups[1], G.idx)
        fresh = UF.RowGroups(G.rows.copy(), G.ptr, G.idx, G.weights, G.entries)
        assert after == ro.score(lt, dp, dm, fresh.rows, PERC_MET, groups=fresh) and after != before
        assert ro._engine_for(fresh.rows, check=False) is not eng and g_of >= 0
        # other weights on the cached rows: no new engine, the counts follow; None removes the groups
        G2 = UF.RowGroups(G.rows, G.ptr, G.idx, np.where(np.arange(G.n_groups) % 2, 2.0, 0.5), G.entries)
        s2 = ro.score(lt, dp, dm, G.rows, PERC_MET, groups=G2)
        assert ro._engine_for(G.rows, check=False) is eng and s2 != after
        assert eng._global_counts == _group_counts(G.rows, G2.ptr, G2.idx, G2.weights) == eng.row_weight_sums
        plain = ro.score(lt, dp, dm, G.rows, PERC_MET)
        assert eng.row_groups is None and eng._groups is None and eng._global_counts == ro._global_counts(G.rows)
        assert plain == ro.score(lt, dp, dm, fresh.rows, PERC_MET)
        w = np.full(G.rows.shape[0], 2.0)
        ro.score(lt, dp, dm, G.rows, PERC_MET, groups=G)
        sw = ro.score(lt, dp, dm, G.rows, PERC_MET, weights=w)  # from groups to weights on the same engine
        assert eng.row_groups is None and np.array_equal(eng.row_weights, w) and sw == ro.score(lt, dp, dm, fresh.rows, PERC_MET, weights=w)
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_sharded_groups_are_refused(monkeypatch):
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    G = UF.expand_missing(_masked_cohort(N4, 33, 8))
    lt, dp, dm = RC.params(N4)
    try:
        ro.score(lt, dp, dm, G.rows, PERC_MET)
        eng = ro._engine_for(G.rows, check=False)
        with pytest.raises(ValueError, match="more than one rank"):
            ro._set_groups(eng, G.rows, ro._group_arrays(G, G.rows.shape[0]), 2)
        assert eng.row_groups is None
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_learn_mhn_with_groups_matches_the_oracle_optimizer():
    """learn_mhn(..., groups=) under SciPy's L-BFGS-B reaches the objective the same optimizer reaches on the NumPy-mixed oracle
    objective (test_gpu_parity.py: test_learn_mhn_matches_oracle_optimizer's settings and tolerance)."""
    import scipy.optimize as opt
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    n = N4
    N = n + 1
    dat = _masked_cohort(n, 60, 21, frac=0.1, most=2)
    G = UF.expand_missing(dat)
    th0 = np.diag(np.full(N, -1.0))
    dp0, dm0 = np.zeros(N), np.zeros(N)
    try:
        th, dp, dm = ro.learn_mhn(th0, dp0, dm0, G.rows, 0.3, ro.symmetric_penal, 0.05, opt_iter=200, opt_ftol=1e-10, opt_v=False, groups=G)
        x0 = np.concatenate((th0.flatten(), dp0, dm0))
        ref = opt.minimize(fun=_mixed_objective_reg, jac=True, x0=x0, method="L-BFGS-B", args=(G, dat, 0.3, 0.05),
                           options={"maxiter": 200, "ftol": 1e-10})
        got = np.concatenate((th.flatten(), dp, dm))
        f_got = float(_mixed_objective_reg(got, G, dat, 0.3, 0.05)[0])
        assert abs(f_got - float(ref.fun)) < 1e-7 * max(1.0, abs(float(ref.fun)))
        np.testing.assert_allclose(got, ref.x, atol=5e-4)
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_luad28_with_a_three_gene_panel_mask(golden):
    """The 28-event LUAD cohort with the 3-gene mask of scripts/luad28_missing.py at the published fit, one score-only
    evaluation: the two sums against sum_g w_g logsumexp over lp of the completions - the fixture's fit_lp where a completion
    is a row of the fixture, the engine's own patient_grads otherwise - under the derived bound (the difference between
    the fixture's lp and the engine's is part of it)."""
    from metmhn_amd import Engine, Utilityfunctions as UF
    spec = importlib.util.spec_from_file_location("luad28_missing", os.path.join(ROOT, "scripts", "luad28_missing.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    g = golden("luad28")
    dat = g["dat"]
    masked, hit = script.panel_mask(dat, script.GENES3)
    assert 0.25 * dat.shape[0] < hit.sum() < 0.45 * dat.shape[0]
    G = UF.expand_missing(masked, max_alternatives=64)
    assert G.n_groups == 4852 and G.rows.shape[0] < G.ptr[-1] and np.diff(G.ptr).max() == 64
    lt, a, b = g["fit_theta"], g["fit_dp"], g["fit_dm"]
    known = {r.tobytes(): i for i, r in enumerate(dat)}
    with Engine(28) as e:
        e.set_cohort(G.rows)
        lp_own = e.patient_grads(lt, a, b, with_grad=False)
        lp = lp_own.copy()
        at = np.array([known.get(r.tobytes(), -1) for r in G.rows])
        lp[at >= 0] = g["fit_lp"][at[at >= 0]]
        assert (at >= 0).sum() > 1000 and (at < 0).sum() > 1000
        e.set_row_groups(G.ptr, G.idx, G.weights)
        assert e.row_weight_sums == (float(dat[:, -3].sum()), 4852.0, 0.0)
        rows = np.zeros((lp.shape[0], stride(29)))
        rows[:, 0] = lp
        ref = MixReference(lp, rows, G.rows, G.ptr, G.idx, G.weights, 29, lp_spread=np.abs(lp - lp_own))
        s = e.cohort_sums(lt, a, b, with_grad=False)
        ratio = RC.within(s, *ref.raw(), "LUAD-28, 3-gene mask: score-only sums")
        print(f"LUAD-28, 3-gene mask: {G.rows.shape[0]} distinct completed rows of {int(G.ptr[-1])}, {int((at >= 0).sum())} of them fixture rows; "
              f"worst error / bound {ratio:.3f}, largest |fit_lp - lp| {np.abs(lp - lp_own).max():.2e}")
