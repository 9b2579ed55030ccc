"""Per-row weights of the cohort objective (mmhn_set_row_weights, csrc/assemble.h: k_reduce_rows_w), the host code on top of
them (regularized_optimization's `weights=`, Utilityfunctions.collapse_rows / bootstrap_fits).

Definition (include/metmhn_amd.h): with weights w_i every cohort sum is sum_i w_i v_i over the per-row values, and the three
counts are n_em = sum w_i [seeding = 1], n_pat = sum w_i, n_unknown = sum w_i [type 4]; for integer weights that is the objective
of the cohort in which row i is written w_i times.  A row of weight 0 is absent.

Reference of a weighted buffer: reduction_common.Reference over the engine's own per-row values (Engine.patient_grads, which
stays unweighted) times the weights, rows of weight 0 left out.  The float64 products w_i v_i are the addends, and the device may
fuse the product into the addition, so every addend carries one rounding more than in the unweighted bound: (P_cls + 3) u S for
the raw buffer, (P + 5) u (|w_pm| S_EM + S_NM) for the pre-combined one, S over |w_i v_i|, P_cls the rows of the class with
w_i != 0.  The counts are compared exactly: every weight is one of {0, 0.5, 1, 2, 3, 7.25}, whose sums are exact in any order."""
import ctypes as C
import os

import numpy as np
import pytest

import reduction_common as RC
from eval_common import GOLDEN, close, close_grads, engine_pool
from reduction_common import MULTI_BATCH, MULTI_BATCH_WS, N4, PERC_MET, W_PM, WEIGHT_VALUES, Reference, U, raw_layout, red_per, stride, wsums_layout
from unknown_common import unknown_row


def _weights(P, seed, zeros=True):
    """P weights from WEIGHT_VALUES (zeros=False: from its non-zero entries), never all zero."""
    rng = np.random.default_rng(seed)
    w = rng.choice(WEIGHT_VALUES if zeros and P > 1 else WEIGHT_VALUES[1:], size=P)
    if P > 1:
        w[0], w[1] = 7.25, 0.5                                # (neighbours that differ: a shifted or permuted weight shows)
    return w


def _counts(dat, w):
    """(n_em, n_pat, n_unknown) by the definition, one row at a time."""
    n_em = n_pat = n_unknown = 0.0
    for r, wi in zip(dat, w):
        n_em += wi if r[-3] == 1 else 0.0
        n_pat += wi
        n_unknown += wi if r[-1] == 4 else 0.0
    return n_em, n_pat, n_unknown


class WeightedReference:
    """Exact weighted per-class sums of the rows [P, st] with the bound of the module docstring (weights None: all one, the
    unweighted bound of tests/test_cohort_reduction.py)."""

    def __init__(self, rows, w, dat, N, spread=None):
        self.N = N
        self.extra = 0 if w is None else 1
        w = np.ones(rows.shape[0]) if w is None else np.asarray(w, dtype=np.float64)
        keep = w != 0
        self.counts = _counts(dat, w)
        sp = None if spread is None else spread[keep] * w[keep, None]
        self.r = Reference(rows[keep] * w[keep, None], RC.nm_class(dat)[keep], self.counts[0], N, sp)

    def raw(self):
        r, x = self.r, self.extra
        ref = raw_layout(r.em, r.nm, self.counts[0], self.counts[1], self.N)
        bound = raw_layout((r.p_em + 2 + x) * U * r.abs_em + r.sp_em, (r.p_nm + 2 + x) * U * r.abs_nm + r.sp_nm, 0.0, 0.0, self.N)
        return ref, bound

    def wsums(self, w_pm):
        r = self.r
        ref = wsums_layout(r.em, r.nm, w_pm, self.N)
        bound = (r.P + 4 + self.extra) * U * wsums_layout(r.abs_em, r.abs_nm, abs(w_pm), self.N) + \
            wsums_layout(r.sp_em, r.sp_nm, abs(w_pm), self.N)
        return ref, bound

    def objective_bound(self, perc_met):
        """Bound of (score, d_theta, d_dp, d_dm) as one vector in the order of the pre-combined buffer, and (w_pm, n_full)."""
        from metmhn_amd import distributed as D
        w_pm, n_full = D.em_weight(*self.counts[:2], perc_met, self.counts[2])
        return self.wsums(w_pm)[1] / n_full, (w_pm, n_full)


# ---- CPU: collapse_rows -------------------------------------------------------------------------------------------------------

def _check_collapse(dat):
    from metmhn_amd import Utilityfunctions as UF
    rows, counts, inverse = UF.collapse_rows(dat)
    assert counts.dtype == np.float64 and inverse.dtype == np.int64 and rows.dtype == dat.dtype
    assert rows.shape[1] == dat.shape[1] and counts.shape == (rows.shape[0],) and inverse.shape == (dat.shape[0],)
    np.testing.assert_array_equal(rows[inverse], dat)
    np.testing.assert_array_equal(counts, np.bincount(inverse, minlength=rows.shape[0]))
    assert len({r.tobytes() for r in rows}) == rows.shape[0], "a row occurs twice among the distinct rows"
    first = np.array([np.flatnonzero(inverse == u)[0] for u in range(rows.shape[0])]) if rows.shape[0] <= 4096 else \
        np.unique(inverse, return_index=True)[1]
    assert (np.diff(first) > 0).all(), "the distinct rows are not in order of first occurrence"
    return rows, counts, inverse


def test_collapse_rows_hand_cohort():
    n = N4
    base = RC.cohort(n, 33)
    t4 = np.array([unknown_row(n, []), unknown_row(n, [1, 3]), unknown_row(n, [])], dtype=np.int8)
    dat = np.vstack((base[5:8], t4, base[:12], base[5:8], t4[1:], base[30:]))
    rows, counts, inverse = _check_collapse(dat)
    np.testing.assert_array_equal(rows[0], dat[0])            # first occurrence, not sorted
    assert not np.array_equal(rows, np.unique(dat, axis=0))
    assert rows.shape[0] < dat.shape[0] and counts.sum() == dat.shape[0]
    u4 = np.flatnonzero(rows[:, -1] == 4)
    assert u4.size == 2 and sorted(counts[u4]) == [2.0, 3.0]  # type-4 rows collapse like any others
    rows0, counts0, inverse0 = _check_collapse(dat[:0])
    assert rows0.shape == (0, dat.shape[1]) and counts0.size == 0 and inverse0.size == 0


def test_collapse_rows_luad28(golden):
    dat = golden("luad28")["dat"]
    rows, counts, _ = _check_collapse(dat)
    assert dat.shape[0] == 4852 and rows.shape[0] == 3297 and counts.max() == 102.0 and counts.sum() == 4852.0
    assert int((rows[:, -1] == 3).sum()) == 444


# ---- CPU: the kernel's order of additions ----------------------------------------------------------------------------------

def _replay_w(rows, kinds, w, batches, order, N, mode, a, b, defect=False):
    """What the device writes with weights: the cohort rows cut into consecutive `batches` (row counts); inside a batch the
    patients stand in the order `order` (a permutation of the batch's cohort rows, as PatRec::row gives it) and wrow holds
    w[order]; chunks of red_per(rows of the batch) patients in batch order (k_reduce_rows_w), the chunk sums in chunk order,
    the batches in order, the pack (mode 1: a = n_em, b = n_pat; mode 2: a = w_pm).  defect: wrow holds the weights in ROW order
    (w of the batch's rows, not permuted) while the rows are read in batch order."""
    st = stride(N)
    sums = np.zeros((2, st))
    r0 = 0
    for npat, perm in zip(batches, order):
        per = red_per(npat)
        pats = r0 + perm
        wrow = w[r0:r0 + npat] if defect else w[pats]
        acc = np.zeros((2, st))
        for c in range((npat + per - 1) // per):
            part = np.zeros((2, st))
            for i in range(c * per, min(npat, (c + 1) * per)):
                nm = kinds[pats[i]] in (0, 4, 5)
                part[1 if nm else 0] += 0.0 if wrow[i] == 0 else wrow[i] * rows[pats[i]]
            acc += part
        sums += acc
        r0 += npat
    em, nm = sums
    return raw_layout(em, nm, a, b, N) if mode == 1 else wsums_layout(em, nm, a, N)


def _replay_case(P, batches, seed, defect=False):
    N = N4 + 1
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((P, stride(N))) * 10.0 ** rng.uniform(-3, 3, size=(P, stride(N)))
    kinds = rng.integers(0, 6, size=P)                        # planner kinds 0 .. 5 (4: all-zero type 0, 5: dat type 4)
    dat = np.zeros((P, 2 * N4 + 3), dtype=np.int8)            # the columns the reference reads: seeding and type
    dat[:, -1] = np.where(kinds == 4, 0, np.where(kinds == 5, 4, kinds))
    dat[:, -3] = (kinds >= 1) & (kinds <= 3)
    w = _weights(P, seed + 1)
    order = [rng.permutation(nb) for nb in batches]
    ref = WeightedReference(rows, w, dat, N)
    r1 = RC.within(_replay_w(rows, kinds, w, batches, order, N, 1, ref.counts[0], ref.counts[1], defect), *ref.raw(), "replayed raw")
    r2 = RC.within(_replay_w(rows, kinds, w, batches, order, N, 2, W_PM, 0.0, defect), *ref.wsums(W_PM), "replayed pre-combined")
    return max(r1, r2)


REPLAY_SHAPES = [(1, [1]), (32, [32]), (33, [33]), (4097, [4097]), (4097, [1400, 1400, 1297]), (4097, [33, 4000, 64])]


@pytest.mark.parametrize("P,batches", REPLAY_SHAPES, ids=[f"P{P}-{len(b)}batches" for P, b in REPLAY_SHAPES])
def test_replayed_weighted_order_is_within_the_bound(P, batches):
    """The reference and the bound alone: k_reduce_rows_w's additions in float64 NumPy pass at the shapes of the GPU test."""
    ratio = _replay_case(P, batches, seed=200 + P)
    print(f"weighted replay P={P} {batches}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("P,batches", REPLAY_SHAPES[1:], ids=[f"P{P}-{len(b)}batches" for P, b in REPLAY_SHAPES[1:]])
def test_weights_in_row_order_break_the_bound(P, batches):
    """The defect the batch order invites: wrow filled in row order while the kernel reads the rows in batch order."""
    with pytest.raises(AssertionError):
        _replay_case(P, batches, seed=200 + P, defect=True)


# ---- CPU: the host code around the engine -----------------------------------------------------------------------------------

def test_shard_weight_slices_cover_the_vector():
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import distributed as D
    dat = RC.typed_cohort(N4, 97, 3)
    w = _weights(97, 5)
    w = w + np.arange(97) * 2.0 ** -20                        # (all different: a slice taken with other indices shows)
    for world in (1, 2, 3, 8):
        back = np.full(97, np.nan)
        idx = D.shard_rows(dat, world)
        for rank in range(world):
            part = ro._shard_weights(w, dat, rank, world)
            assert part.shape == (dat[idx[rank]].shape[0],) if world > 1 else part is w
            back[idx[rank] if world > 1 else slice(None)] = part
        np.testing.assert_array_equal(back, w)


def test_weighted_global_counts_against_a_loop():
    import metmhn_amd.regularized_optimization as ro
    dat = RC.typed_cohort(N4, 97, 3)
    assert ro._global_counts(dat) == _counts(dat, np.ones(97)) == (float(dat[:, -3].sum()), 97.0, float((dat[:, -1] == 4).sum()))
    for seed in range(4):
        w = _weights(97, seed)
        assert ro._global_counts(dat, w) == _counts(dat, w)
    w = np.zeros(97)
    w[np.flatnonzero(dat[:, -1] == 4)[0]] = 3.0               # only a type-4 row counts
    assert ro._global_counts(dat, w) == (0.0, 3.0, 3.0)
    with pytest.raises(ValueError, match="one per row"):
        ro._check_weights(np.ones(96), 97)
    assert ro._check_weights(None, 97) is None


def test_bootstrap_result_summaries():
    from metmhn_amd import Utilityfunctions as UF
    B, N = 40, 3
    rng = np.random.default_rng(0)
    th = rng.standard_normal((B, N, N))
    th[:, 0, 1] = np.abs(th[:, 0, 1]) + 0.1                   # always positive
    th[:30, 1, 0], th[30:, 1, 0] = -1.0, 2.0                  # 30 of 40 with the sign of the median
    res = UF.BootstrapFits(th, rng.standard_normal((B, N)), rng.standard_normal((B, N)), np.ones((B, 2)), np.zeros((2, 2 * N + 1)))
    lo, hi = res.interval(0.9)["theta"]
    np.testing.assert_allclose(lo, np.percentile(th, 5, axis=0))
    np.testing.assert_allclose(hi, np.percentile(th, 95, axis=0))
    assert (res.interval()["d_p"][0] <= res.interval()["d_p"][1]).all()
    s = res.sign_stability()["theta"]
    assert s[0, 1] == 1.0 and s[1, 0] == 0.75 and s.shape == (N, N) and res.sign_stability()["d_m"].shape == (N,)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def make_engine():
    yield from engine_pool()


def _references(e, dat, w, lt, dp, dm, score_only=True):
    """(reference of a gradient evaluation, of a score-only one - None with score_only=False) of engine `e` holding `dat` with
    weights `w` (None: none), each with the spread of two downloads of the rows in its bound."""
    keep = slice(None) if w is None else np.asarray(w) != 0
    r1, r2 = RC.rows_of(e, lt, dp, dm), RC.rows_of(e, lt, dp, dm)
    assert np.isfinite(r1[keep]).all()
    ref = WeightedReference(r1, w, dat, e.N, np.abs(r1 - r2))
    if not score_only:
        return ref, None
    s1, s2 = RC.rows_of(e, lt, dp, dm, False), RC.rows_of(e, lt, dp, dm, False)
    assert np.isfinite(s1[keep]).all()
    return ref, WeightedReference(s1, w, dat, e.N, np.abs(s1 - s2))


def _check_weighted(e, dat, w, lt, dp, dm, tag):
    """Both buffers of `e` (holding dat and w) with and without gradients against its own rows; the raw sums."""
    ref, ref0 = _references(e, dat, w, lt, dp, dm)
    s = e.cohort_sums(lt, dp, dm)
    a = RC.within(s, *ref.raw(), tag + " cohort_sums")
    s0 = e.cohort_sums(lt, dp, dm, with_grad=False)
    RC.within(s0, *ref0.raw(), tag + " cohort_sums(with_grad=False)")
    assert not s0[4:].any(), f"{tag}: gradient entries of a score-only evaluation"
    b = RC.within(RC.wsums(e, lt, dp, dm, W_PM), *ref.wsums(W_PM), tag + " cohort_wsums")
    ws0 = RC.wsums(e, lt, dp, dm, W_PM, with_grad=False)
    RC.within(ws0, *ref0.wsums(W_PM), tag + " cohort_wsums(with_grad=False)")
    assert not ws0[1:].any(), f"{tag}: gradient entries of a score-only weighted evaluation"
    assert (s[2], s[3]) == ref.counts[:2] and e.row_weight_sums == ref.counts, f"{tag}: counts {s[2:4]}, {e.row_weight_sums}"
    print(f"{tag}: worst error / bound: raw {a:.3f}, pre-combined {b:.3f}")
    return s, ref


@pytest.mark.gpu
@pytest.mark.parametrize("zerocopy", (True, False), ids=("zerocopy", "zerocopy0"))
def test_weights_of_one_change_nothing(make_engine, zerocopy):
    """w = 1 everywhere: the same bits as without weights in both buffers and in mmhn_score_and_grad - and again after the
    weights are removed."""
    lt, dp, dm = RC.params(N4)
    dat = RC.cohort(N4, 4097)
    e = make_engine(N4, zerocopy=zerocopy)
    e.set_cohort(dat)
    assert e.row_weights is None
    plain = [e.cohort_sums(lt, dp, dm), e.cohort_sums(lt, dp, dm, with_grad=False), RC.wsums(e, lt, dp, dm, W_PM),
             RC.wsums(e, lt, dp, dm, W_PM, with_grad=False), RC.flat(e.score_and_grad(lt, dp, dm, PERC_MET)), e.score(lt, dp, dm, PERC_MET)]
    counts = e.row_weight_sums
    assert counts == (float(dat[:, -3].sum()), 4097.0, 0.0)
    for w in (np.ones(4097), None, _weights(4097, 1), np.ones(4097)):
        e.set_row_weights(w)
        assert (e.row_weights is None) if w is None else np.array_equal(e.row_weights, w)
        got = [e.cohort_sums(lt, dp, dm), e.cohort_sums(lt, dp, dm, with_grad=False), RC.wsums(e, lt, dp, dm, W_PM),
               RC.wsums(e, lt, dp, dm, W_PM, with_grad=False), RC.flat(e.score_and_grad(lt, dp, dm, PERC_MET)), e.score(lt, dp, dm, PERC_MET)]
        same = all(np.array_equal(a, b) for a, b in zip(got, plain))
        if w is not None and not (w == 1).all():
            assert not same and e.row_weight_sums != counts   # (the weights in between do reach the sums)
        else:
            assert same and e.row_weight_sums == counts
    e.row_weights[0] = 5.0                                    # a copy: writing to it does not reach the engine
    assert e.row_weights[0] == 1.0


WEIGHTED_SHAPES = [(1, "f64", None), (32, "f64", None), (33, "f64", None), (4097, "f64", None), (MULTI_BATCH[1], "f64", MULTI_BATCH_WS),
                   (33, "f32", None), (MULTI_BATCH[1], "f32", MULTI_BATCH_WS)]


@pytest.mark.gpu
@pytest.mark.parametrize("P,dtype,workspace", WEIGHTED_SHAPES, ids=[f"P{P}-{d}-{'multibatch' if ws else 'onebatch'}" for P, d, ws in WEIGHTED_SHAPES])
def test_weighted_sums_against_the_reference(make_engine, P, dtype, workspace):
    """Both buffers, with and without gradient, against the weighted reference under the bound; the MULTI_BATCH cohort under
    MULTI_BATCH_WS is cut into at least three batches (test_cohort_reduction.py: test_multi_batch_reduction), where the order of
    the patients of a batch and the order of the cohort's rows part."""
    n = MULTI_BATCH[0] if workspace else N4
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, P)
    w = _weights(P, 10 + P)
    e = make_engine(n, dtype=dtype, workspace=workspace)
    e.set_cohort(dat)
    e.set_row_weights(w)
    s, _ = _check_weighted(e, dat, w, lt, dp, dm, f"P={P} {dtype} ws={workspace}")
    if P > 1:                                                 # a second vector on the same plan, then none
        w2 = _weights(P, 11 + P)[::-1].copy()
        e.set_row_weights(w2)
        _check_weighted(e, dat, w2, lt, dp, dm, f"P={P} {dtype} ws={workspace} second weights")
    e.set_row_weights(None)
    _check_weighted(e, dat, None, lt, dp, dm, f"P={P} {dtype} ws={workspace} weights removed")


def _definition_case(u, c, tag, with_collapse=True):
    """Distinct rows u with integer counts c as weights against np.repeat(u, c) without weights, through ro.score_and_grad."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    n = (u.shape[1] - 3) // 2
    lt, dp, dm = RC.params(n)
    full = np.repeat(u, c.astype(np.int64), axis=0)
    try:
        got_w = ro.score_and_grad(lt, dp, dm, u, PERC_MET, weights=c)
        ew = ro._engine_for(u, check=False)
        np.testing.assert_array_equal(ew.row_weights, c)
        got_f = ro.score_and_grad(lt, dp, dm, full, PERC_MET)
        ef = ro._engine_for(full, check=False)
        assert ef.row_weights is None and ef.n_pat == full.shape[0] and ew.n_pat == u.shape[0]
        assert ew._global_counts == ef._global_counts == _counts(full, np.ones(full.shape[0])) == ew.row_weight_sums
        ref_w, _ = _references(ew, u, c, lt, dp, dm)
        ref_f, _ = _references(ef, full, None, lt, dp, dm)
        bw, (w_pm, n_full) = ref_w.objective_bound(PERC_MET)
        bf, (w_pm_f, n_full_f) = ref_f.objective_bound(PERC_MET)
        assert (w_pm, n_full) == (w_pm_f, n_full_f)
        ratio = RC.within(RC.flat(got_w), RC.flat(got_f), bw + bf, tag + ": weighted against repeated rows")
        print(f"{tag}: worst |weighted - repeated| / (sum of the bounds) {ratio:.3f}, w_pm {w_pm:.4f}, n_full {n_full}")
        if with_collapse:
            rows, counts, inverse = UF.collapse_rows(full)
            np.testing.assert_array_equal(rows, u)
            np.testing.assert_array_equal(counts, c)
            got_c = ro.score_and_grad(lt, dp, dm, rows, PERC_MET, weights=counts)
            ref_c, _ = _references(ro._engine_for(rows, check=False), rows, counts, lt, dp, dm)
            RC.within(RC.flat(got_c), RC.flat(got_f), ref_c.objective_bound(PERC_MET)[0] + bf, tag + ": collapse_rows fed back")
            ro.invalidate(rows)
    finally:
        ro.invalidate(u)
        ro.invalidate(full)


def _distinct(dat):
    return dat[np.sort(np.unique(dat, axis=0, return_index=True)[1])]


@pytest.mark.gpu
@pytest.mark.parametrize("U_rows", (1, 33, 100))
def test_integer_weights_are_repeated_rows(U_rows):
    """The definition: integer weights c on distinct rows u give the objective of np.repeat(u, c), within the sum of the two
    sides' bounds over n_full; collapse_rows of the repeated array, fed back, gives it too."""
    u = _distinct(RC.cohort(N4, 1500))[:U_rows]
    assert u.shape[0] == U_rows
    rng = np.random.default_rng(U_rows)
    c = rng.choice([1.0, 2.0, 3.0, 7.0, 40.0], size=U_rows)
    _definition_case(u, c, f"U={U_rows}")


@pytest.mark.gpu
def test_weighted_rows_of_unknown_status():
    """Rows of type 4 with weights, among rows of types 0 - 3 and with the empty genotype: the weighted n_unknown of
    mmhn_get_row_weight_sums and the objective by the definition."""
    from metmhn_amd import Engine
    u = _distinct(RC.typed_cohort(N4, 120, 9))
    t4 = u[:, -1] == 4
    assert t4.sum() >= 5 and (t4 & (u[:, :2 * N4].sum(axis=1) == 0)).any() and set(np.unique(u[:, -1])) == {0, 1, 2, 3, 4}
    c = np.random.default_rng(4).choice([1.0, 2.0, 3.0, 5.0], size=u.shape[0])
    _definition_case(u, c, "with type-4 rows")
    w = _weights(u.shape[0], 8)
    w[np.flatnonzero(t4)[:3]] = (7.25, 0.0, 0.5)
    lt, dp, dm = RC.params(N4)
    with Engine(N4) as e:
        e.set_cohort(u)
        assert e.n_unknown == int(t4.sum()) and e.row_weight_sums[2] == float(t4.sum())
        e.set_row_weights(w)
        assert e.row_weight_sums[2] == w[t4].sum() and e.n_unknown == int(t4.sum())
        _, ref = _check_weighted(e, u, w, lt, dp, dm, "type-4 rows, fractional weights")
        # mmhn_score_and_grad weights with the real-valued n_unknown
        bound, (w_pm, n_full) = ref.objective_bound(PERC_MET)
        exact = ref.wsums(w_pm)[0] / n_full
        RC.within(RC.flat(e.score_and_grad(lt, dp, dm, PERC_MET)), exact, bound + 2 * U * np.abs(exact), "mmhn_score_and_grad with type-4 weights")


@pytest.mark.gpu
@pytest.mark.parametrize("zero", ("some", "every_em", "every_nm"))
def test_weight_zero_is_absence(make_engine, zero):
    """A cohort with weights equals the cohort of its rows with w != 0 (with their weights): sums under the two bounds, counts
    equal.  every_em: no EM row is left, the objective takes the w = 1 branch of em_weight."""
    from metmhn_amd import distributed as D
    lt, dp, dm = RC.params(N4)
    dat = RC.typed_cohort(N4, 200, 2)
    w = _weights(200, 21)
    if zero == "every_em":
        w[dat[:, -3] == 1] = 0.0
    elif zero == "every_nm":
        w[dat[:, -1] == 0] = 0.0
    keep = w != 0
    assert 0 < keep.sum() < 200 and (w == 0).sum() >= 20
    a, b = make_engine(N4, tag=1), make_engine(N4, tag=2)
    a.set_cohort(dat)
    a.set_row_weights(w)
    b.set_cohort(dat[keep])
    b.set_row_weights(w[keep])
    sa, ref_a = _check_weighted(a, dat, w, lt, dp, dm, f"zero={zero} whole cohort")
    sb, ref_b = _check_weighted(b, dat[keep], w[keep], lt, dp, dm, f"zero={zero} rows with w != 0")
    assert a.row_weight_sums == b.row_weight_sums and tuple(sa[2:4]) == tuple(sb[2:4])
    RC.within(sa, sb, ref_a.raw()[1] + ref_b.raw()[1], f"zero={zero}: raw sums of the two cohorts")
    bound_a, (w_pm, n_full) = ref_a.objective_bound(PERC_MET)
    bound_b, same = ref_b.objective_bound(PERC_MET)
    assert same == (w_pm, n_full)
    if zero != "some":
        assert w_pm == 1.0 and n_full == a.row_weight_sums[1]
    got_a, got_b = RC.flat(a.score_and_grad(lt, dp, dm, PERC_MET)), RC.flat(b.score_and_grad(lt, dp, dm, PERC_MET))
    RC.within(got_a, got_b, bound_a + bound_b, f"zero={zero}: objective of the two cohorts")
    # weight 1 on the kept rows: the plain cohort of those rows, no weights at all
    ones = keep.astype(np.float64)
    a.set_row_weights(ones)
    b.set_row_weights(None)
    assert a.row_weight_sums == b.row_weight_sums == _counts(dat[keep], np.ones(int(keep.sum())))
    ra, _ = _references(a, dat, ones, lt, dp, dm)
    rb, _ = _references(b, dat[keep], None, lt, dp, dm)
    RC.within(a.cohort_sums(lt, dp, dm), b.cohort_sums(lt, dp, dm), ra.raw()[1] + rb.raw()[1], f"zero={zero}: 0 / 1 weights against the sub-cohort")
    assert D.em_weight(*a.row_weight_sums[:2], PERC_MET, a.row_weight_sums[2]) == D.em_weight(*b.row_weight_sums[:2], PERC_MET, b.row_weight_sums[2])


@pytest.mark.gpu
def test_refusals(make_engine):
    """Every refused vector raises with a message that names the row and leaves the weights held before in place; a call
    between _begin and _end is refused and the pending evaluation delivers the old result; set_cohort clears the weights."""
    from metmhn_amd import Engine, _lib
    lt, dp, dm = RC.params(N4)
    dat = RC.cohort(N4, 33)
    e = make_engine(N4, tag=3)
    e.set_cohort(dat)
    w = _weights(33, 3)
    e.set_row_weights(w)
    held = e.cohort_sums(lt, dp, dm)

    def c_call(vec, n=None):
        vec = np.ascontiguousarray(vec, dtype=np.float64)
        status = e.lib.mmhn_set_row_weights(e.h, vec.ctypes.data_as(C.POINTER(C.c_double)), vec.shape[0] if n is None else n)
        return status, e.lib.mmhn_last_error().decode()

    for bad, row, word in ((-1.0, 5, "negative"), (np.nan, 7, "finite"), (np.inf, 32, "finite"), (-np.inf, 0, "finite")):
        v = w.copy()
        v[row] = bad
        v[min(row + 3, 32)] = bad                             # (the FIRST offending row is named)
        with pytest.raises(RuntimeError, match=rf"row {row} .*{word}"):
            e.set_row_weights(v)
    with pytest.raises(RuntimeError, match=r"every weight is 0 \(row 0"):
        e.set_row_weights(np.zeros(33))
    for n_bad, text in ((32, "row 32 has no weight"), (34, "row 33 does not exist"), (0, "row 0 has no weight")):
        with pytest.raises(ValueError, match=r"one weight per cohort row \(row \d+"):
            e.set_row_weights(np.ones(n_bad))
        with pytest.raises(ValueError):
            e.set_row_weights(np.ones((n_bad, 1)))
        status, msg = c_call(np.ones(max(n_bad, 1)), n_bad)   # the library's own check of n
        assert status != 0 and text in msg and "33 rows" in msg, msg
    np.testing.assert_array_equal(e.row_weights, w)
    np.testing.assert_array_equal(e.cohort_sums(lt, dp, dm), held)
    # between _begin and _end
    e.cohort_sums_begin(lt, dp, dm)
    with pytest.raises(RuntimeError, match="has not been collected"):
        e.set_row_weights(np.ones(33))
    with pytest.raises(RuntimeError, match="has not been collected"):
        e.set_row_weights(None)
    np.testing.assert_array_equal(e.cohort_sums_end(), held)
    np.testing.assert_array_equal(e.row_weights, w)
    # set_cohort clears them
    e.set_cohort(dat)
    assert e.row_weights is None and e.row_weight_sums == (float(dat[:, -3].sum()), 33.0, 0.0)
    assert tuple(e.cohort_sums(lt, dp, dm)[2:4]) == (float(dat[:, -3].sum()), 33.0)
    # an engine without a cohort, and one whose cohort is empty
    with Engine(N4) as fresh:
        for _ in range(2):
            with pytest.raises(RuntimeError, match=r"holds no cohort \(row 0"):
                fresh.set_row_weights(np.ones(33))
            fresh.set_row_weights(None)                       # nothing to remove: fine
            assert fresh.row_weights is None and fresh.row_weight_sums == (0.0, 0.0, 0.0)
            fresh.set_cohort(dat[:0])
    assert _lib.ABI_VERSION == e.lib.mmhn_abi_version() == 8


@pytest.mark.gpu
def test_guard_rebuild_keeps_the_weights():
    """dat edited in place between two ro.score(..., weights=w): the guard's rebuild (set_cohort clears the weights) applies
    them again - the second value is that of a fresh engine on the edited array with w."""
    import metmhn_amd.regularized_optimization as ro
    lt, dp, dm = RC.params(N4)
    dat = RC.cohort(N4, 33).copy()
    w = _weights(33, 6)
    w[2] = 3.0
    try:
        before = ro.score(lt, dp, dm, dat, PERC_MET, weights=w)
        eng = ro._engine_for(dat, check=False)
        dat[2] = dat[32]                                      # a seeding-only paired row becomes an all-zero NM row: counts change
        after = ro.score(lt, dp, dm, dat, PERC_MET, weights=w)
        assert ro._engine_for(dat, check=False) is eng and np.array_equal(eng.row_weights, w)
        assert eng._global_counts == _counts(dat, w)
        fresh_dat = dat.copy()
        fresh = ro.score(lt, dp, dm, fresh_dat, PERC_MET, weights=w)
        assert ro._engine_for(fresh_dat, check=False) is not eng
        assert after == fresh and after != before
        g_after = RC.flat(ro.score_and_grad(lt, dp, dm, dat, PERC_MET, weights=w))
        np.testing.assert_array_equal(g_after, RC.flat(ro.score_and_grad(lt, dp, dm, fresh_dat, PERC_MET, weights=w)))
        # other weights on the cached cohort: no new engine, the counts follow; None removes them
        w2 = w[::-1].copy()
        s2 = ro.score(lt, dp, dm, dat, PERC_MET, weights=w2)
        assert ro._engine_for(dat, check=False) is eng and eng._global_counts == _counts(dat, w2) and s2 != after
        plain = ro.score(lt, dp, dm, dat, PERC_MET)
        assert eng.row_weights is None and eng._weights is None and eng._global_counts == _counts(dat, np.ones(33))
        assert plain == ro.score(lt, dp, dm, fresh_dat, PERC_MET)
        with pytest.raises(ValueError, match="one per row"):
            ro.score(lt, dp, dm, dat, PERC_MET, weights=np.ones(32))
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_one_rank_collective_path(monkeypatch):
    """MMHN_FORCE_ALLREDUCE=1: the weighted objective through the in-library all-reduce of one rank equals the plain path."""
    import metmhn_amd.regularized_optimization as ro
    lt, dp, dm = RC.params(N4)
    dat = RC.typed_cohort(N4, 200, 5)
    w = _weights(200, 12)
    try:
        plain = RC.flat(ro.score_and_grad(lt, dp, dm, dat, PERC_MET, weights=w))
        assert not ro._engine_for(dat, check=False)._sharded
        monkeypatch.setenv("MMHN_FORCE_ALLREDUCE", "1")
        monkeypatch.setenv("MMHN_STRICT_COMM", "1")
        other = dat.copy()
        forced = RC.flat(ro.score_and_grad(lt, dp, dm, other, PERC_MET, weights=w))
        eng = ro._engine_for(other, check=False)
        assert eng._sharded and eng._device_comm and np.array_equal(eng.row_weights, w)
        np.testing.assert_array_equal(forced, plain)
        assert ro.score(lt, dp, dm, other, PERC_MET, weights=w) == plain[0]
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_bootstrap_fits():
    """60 rows, 3 replicates of 5 iterations: reproducible by key, the documented draw, every replicate the weighted fit."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    dat = RC.typed_cohort(N4, 60, 1)
    dat[40:50] = dat[10:20]                                   # duplicates: fewer distinct rows than rows
    pm, lam, N = PERC_MET, 1e-2, N4 + 1
    try:
        a = UF.bootstrap_fits(dat, 3, pm, ro.symmetric_penal, lam, key=7, opt_iter=5)
        b = UF.bootstrap_fits(dat, 3, pm, ro.symmetric_penal, lam, key=7, opt_iter=5)
        rows, counts, inverse = UF.collapse_rows(dat)
        Un = rows.shape[0]
        assert Un < 60 and a.theta.shape == (3, N, N) and a.d_p.shape == a.d_m.shape == (3, N) and a.weights.shape == (3, Un)
        for x, y in ((a.theta, b.theta), (a.d_p, b.d_p), (a.d_m, b.d_m), (a.weights, b.weights)):
            assert x.tobytes() == y.tobytes()
        draw = np.random.default_rng(7).multinomial(60, np.full(60, 1 / 60), size=3)
        want = np.stack([np.bincount(inverse, weights=d, minlength=Un) for d in draw])
        np.testing.assert_array_equal(a.weights, want)
        assert (a.weights.sum(axis=1) == 60).all() and (a.weights == 0).any() and a.weights.dtype == np.float64
        np.testing.assert_array_equal(a.rows, rows)
        other = UF.bootstrap_fits(dat, 3, pm, ro.symmetric_penal, lam, key=8, opt_iter=5)
        assert not np.array_equal(other.weights, a.weights) and not np.array_equal(other.theta, a.theta)
        th0, dp0, dm0 = UF.indep(dat)
        for k in range(3):
            th, d_p, d_m = ro.learn_mhn(th0, dp0, dm0, rows, pm, ro.symmetric_penal, lam, opt_iter=5, opt_v=False, weights=a.weights[k])
            assert th.tobytes() == a.theta[k].tobytes() and d_p.tobytes() == a.d_p[k].tobytes() and d_m.tobytes() == a.d_m[k].tobytes()
        assert not np.array_equal(a.theta[0], a.theta[1])
        lo, hi = a.interval()["theta"]
        assert lo.shape == (N, N) and (lo <= hi).all() and a.sign_stability()["theta"].shape == (N, N)
        # a start of the caller's, and weights of one against the plain fit
        s = UF.bootstrap_fits(dat, 1, pm, ro.symmetric_penal, lam, key=7, start=(a.theta[0], a.d_p[0], a.d_m[0]), opt_iter=2)
        assert not np.array_equal(s.theta[0], a.theta[0]) and np.array_equal(s.weights[0], a.weights[0])
        plain = ro.learn_mhn(th0, dp0, dm0, dat, pm, ro.symmetric_penal, lam, opt_iter=5, opt_v=False)
        ones = ro.learn_mhn(th0, dp0, dm0, dat, pm, ro.symmetric_penal, lam, opt_iter=5, opt_v=False, weights=np.ones(60))
        for x, y in zip(plain, ones):
            assert x.tobytes() == y.tobytes()
    finally:
        ro.invalidate()


@pytest.mark.gpu
def test_luad28_collapsed(golden):
    """The 28-event LUAD cohort as its 3 297 distinct rows with their counts as weights, against the fixture of
    test_gpu_parity.py: test_luad28_real_workload with its tolerances; with the 1 227 primaries of unknown status appended, the
    collapsed cohort against the uncollapsed one, each side under the bound of its own rows."""
    from metmhn_amd import Engine, Utilityfunctions as UF
    g = golden("luad28")
    rows, counts, _ = UF.collapse_rows(g["dat"])
    assert rows.shape == (3297, 59) and counts.sum() == 4852.0
    pm = float(g["perc_met"])
    with Engine(28) as e:
        e.set_cohort(rows)
        e.set_row_weights(counts)
        assert e.row_weight_sums == (float(g["dat"][:, -3].sum()), 4852.0, 0.0)
        for pt in ("indep", "fit"):
            lt, a, b = g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"]
            close_grads(f"collapsed LUAD-28 {pt}", e.score_and_grad(lt, a, b, pm), [g[pt + s] for s in ("_score", "_d_th", "_d_dp", "_d_dm")],
                        (1e-9, 0.0), (1e-7, 1e-10))
            close(f"collapsed LUAD-28 {pt} score", float(e.score(lt, a, b, pm)), g[pt + "_score"], 1e-9)
    unknown = np.load(os.path.join(GOLDEN, "luad28_unknown_rows.npy"))
    dat = np.vstack((g["dat"], unknown))
    rows, counts, _ = UF.collapse_rows(dat)
    assert rows.shape[0] < dat.shape[0] and counts[rows[:, -1] == 4].sum() == 1227.0
    lt, a, b = g["fit_theta"], g["fit_dp"], g["fit_dm"]
    with Engine(28) as e, Engine(28) as full:
        e.set_cohort(rows)
        e.set_row_weights(counts)
        full.set_cohort(dat)
        assert e.row_weight_sums == full.row_weight_sums == (float(dat[:, -3].sum()), float(dat.shape[0]), 1227.0)
        ref_c, _ = _references(e, rows, counts, lt, a, b, score_only=False)
        ref_f, _ = _references(full, dat, None, lt, a, b, score_only=False)
        sc, sf = e.cohort_sums(lt, a, b), full.cohort_sums(lt, a, b)
        r1 = RC.within(sc, *ref_c.raw(), "LUAD-28 + unknown, collapsed, against its own rows")
        r2 = RC.within(sc, sf, ref_c.raw()[1] + ref_f.raw()[1], "LUAD-28 + unknown: collapsed against uncollapsed sums")
        bc, (w_pm, n_full) = ref_c.objective_bound(pm)
        bf, same = ref_f.objective_bound(pm)
        assert same == (w_pm, n_full)
        r3 = RC.within(RC.flat(e.score_and_grad(lt, a, b, pm)), RC.flat(full.score_and_grad(lt, a, b, pm)), bc + bf,
                     "LUAD-28 + unknown: collapsed against uncollapsed objective")
        print(f"LUAD-28 + unknown rows, {rows.shape[0]} distinct of {dat.shape[0]}: worst error / bound {r1:.3f} (own rows), "
              f"{r2:.3f} (sums), {r3:.3f} (objective)")
