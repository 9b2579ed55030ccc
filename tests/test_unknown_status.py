"""Cohort rows of type 4: a primary tumour was sequenced, its metastatic status is unknown.  The engine scores the PT genotype
x as the sum over both statuses, lp = logaddexp(lp0, lp1) with lp0 what a type-0 row of x scores and lp1 what a type-1 row with
seeding = 1 scores, reports r1 = P(seeded | x) = exp(lp1 - lp) and mixes the two gradients with (1 - r1, r1).  Reference, bars
and helpers: tests/unknown_common.py (the oracle on the relabelled rows, combined in NumPy)."""
import os

import numpy as np
import pytest

import reduction_common as RC
import unknown_common as UC
from eval_common import GOLDEN

PERC_MET = 0.3


# ---------------------------------------------------------------------------------------------------------------- CPU

def _write_csvs(tmp_path):
    """Six patients, two events: absent, present, isMetastasis, paired, and two unpaired primaries of unknown status (one of
    them with a stray MT entry in the table), plus a paired patient of unknown status (no type in either mode)."""
    ev = tmp_path / "events.csv"
    an = tmp_path / "annot.csv"
    ev.write_text(",P.A (M),M.A (M),P.B (M),M.B (M),P.AgeAtSeqRep,M.AgeAtSeqRep,paired\n"
                  "p0,1,0,0,0,50,No metastasis included,0\n"
                  "p1,0,0,1,0,60,No metastasis included,0\n"
                  "p2,0,1,0,1,No primary included,61,0\n"
                  "p3,1,1,0,1,55,57,1\n"
                  "p4,1,0,1,0,58,No metastasis included,0\n"
                  "p5,0,1,0,0,40,No metastasis included,0\n"
                  "p6,1,1,0,0,41,42,2\n")
    an.write_text("patientID,metaStatus\np0,absent\np1,present\np2,isMetastasis\np3,isPaired\np4,unknown\np5,unknown\np6,unknown\n")
    return str(ev), str(an)


def test_loader_keeps_unknown_primaries_on_request(tmp_path):
    from metmhn_amd import Utilityfunctions as U
    ev, an = _write_csvs(tmp_path)
    known, events = U.load_cohort(ev, an)
    assert events == ["A (M)", "B (M)", "Seeding"]
    assert known.tolist() == [[1, 0, 0, 0, 0, -99, 0], [0, 0, 1, 0, 1, -99, 1], [0, 1, 0, 1, 1, -99, 2], [1, 1, 0, 1, 1, 1, 3]]
    both, events2 = U.load_cohort(ev, an, keep_unknown=True)
    assert events2 == events
    assert both[:4].tolist() == known.tolist()
    assert both[4:, :5].tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 0, 0]] and both[4:, -1].tolist() == [4, 4]   # MT and seeding cleared
    assert U.load_cohort(ev, an, keep_unknown=False)[0].tolist() == known.tolist()
    import pandas as pd
    assert U.categorize({"paired": 0, "metaStatus": "unknown"}) is pd.NA                                   # categorize is unchanged


def test_weights_with_unknown_rows():
    from metmhn_amd import distributed as D
    n_em, n_pat = 70.0, 100.0
    assert D.em_weight(n_em, n_pat, PERC_MET, 0) == D.em_weight(n_em, n_pat, PERC_MET)
    w0, nf0 = D.em_weight(n_em, n_pat, PERC_MET)
    w, nf = D.em_weight(n_em, n_pat + 25, PERC_MET, 25)
    assert w == w0 and nf == nf0 + 25                          # the known rows' weight; the unknown rows count once each
    assert D.em_weight(0.0, 40.0, PERC_MET, 40) == (1.0, 40.0)
    N = 3
    rng = np.random.default_rng(0)
    sums = rng.standard_normal(4 + 2 * N * N + 3 * N)
    sums[2], sums[3] = n_em, n_pat
    for a, b in zip(D.combine_sums(sums, N, PERC_MET, 0), D.combine_sums(sums, N, PERC_MET)):
        assert np.array_equal(a, b)
    plus = sums.copy()
    plus[3] += 25
    got, ref = D.combine_sums(plus, N, PERC_MET, 25), D.combine_sums(sums, N, PERC_MET)
    for a, b in zip(got, ref):
        np.testing.assert_allclose(a, b * nf0 / (nf0 + 25), rtol=1e-14)
    # the definition, spelled out
    w, nf = D.em_weight(n_em, n_pat + 25, PERC_MET, 25)
    assert got[0] == (w * plus[0] + plus[1]) / nf and nf == w * n_em + (n_pat - n_em) + 25


def test_indep_with_unknown_rows():
    from metmhn_amd import Utilityfunctions as U, synthetic
    n = 5
    known = synthetic.mixed_cohort(n, 80, seed=3)
    unknown = np.array([UC.unknown_row(n, ev) for ev in ([], [0], [0, 2], [1, 2, 4], [0], [3])], dtype=np.int8)
    dat = np.vstack((known[:40], unknown, known[40:]))
    th, dp, dm = U.indep(dat)
    th0, _, _ = U.indep(known)
    assert not dp.any() and not dm.any()
    assert th[n, n] == th0[n, n]                                # the seeding's rate: the rows of known status alone
    n_coupled, n_single = int((dat[:, -1] == 3).sum()), int((dat[:, -1] != 3).sum())
    for i in range(n):                                          # type-4 rows are single PT observations
        cnt = int(dat[:, 2 * i].sum()) + int(dat[:, 2 * i + 1].sum())
        assert th[i, i] == np.log(cnt / (2 * n_coupled + n_single - cnt + 1e-10))
    assert np.array_equal(U.indep(known)[0], th0)
    # the strata tables ignore the rows of type 4
    ev = [f"e{i}" for i in range(n)] + ["Seeding"]
    assert U.marg_frequs(dat, ev).equals(U.marg_frequs(known, ev))
    for a, b in zip(U.pair_counts(dat), U.pair_counts(known)):
        assert np.array_equal(a, b)


def test_mixture_reference_against_finite_differences_of_its_lp():
    """The NumPy mixture of tests/unknown_common.py: its gradient against central differences of its own lp through the oracle
    (n = 4, h = 1e-6: truncation ~1e-12, rounding ~1e-10 relative to lp), every entry of theta and d_p; d_dm is 0."""
    n = 4
    lt, dp, dm = UC.params(n)
    N = n + 1
    h = 1e-6
    for events in ([], [2], [0, 3], [0, 1, 2, 3]):
        row = UC.unknown_row(n, events)
        m = UC.mixture(lt, dp, dm, row)
        assert 0.0 < m["r1"] < 1.0 and not m["b"].any()
        assert abs(m["lp"] - UC.mixture_lp(lt, dp, dm, row)[0]) <= 1e-12 * abs(m["lp"])
        fd_g, fd_a = np.zeros((N, N)), np.zeros(N)
        for i in range(N):
            for j in range(N):
                d = np.zeros((N, N)); d[i, j] = h
                fd_g[i, j] = (UC.mixture_lp(lt + d, dp, dm, row)[0] - UC.mixture_lp(lt - d, dp, dm, row)[0]) / (2 * h)
            d = np.zeros(N); d[i] = h
            fd_a[i] = (UC.mixture_lp(lt, dp + d, dm, row)[0] - UC.mixture_lp(lt, dp - d, dm, row)[0]) / (2 * h)
        worst = max(UC.ratio(m["g"], fd_g, 1e-6, 1e-8, f"|x| = {len(events)} d_theta"), UC.ratio(m["a"], fd_a, 1e-6, 1e-8, f"|x| = {len(events)} d_dp"))
        assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine(monkeypatch, n, dtype="f64", env=None, workspace=None):
    from metmhn_amd import Engine
    for k_ in ("MMHN_SMALL", "MMHN_POISON"):
        monkeypatch.delenv(k_, raising=False)
    for k_, v_ in (env or {}).items():
        monkeypatch.setenv(k_, v_)                               # (read when the engine is created)
    return Engine(n, dtype=dtype, workspace_bytes=workspace)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ({}, {"MMHN_SMALL": "0"}, {"MMHN_POISON": "1"}), ids=("default", "staged", "poison"))
@pytest.mark.parametrize("dtype", ("f64", "f32"))
def test_shapes_against_the_oracle(monkeypatch, dtype, env):
    """One type-4 row for each |x| in SHAPE_SIZES at n = 13: the larger part at and just past every size class of the small-space
    path (6, 9, TB bits), the last row (|x| + 1 = TB + 1) on the staged kernels, |x| = 0 with the closed-form share;
    patient_grads and patient_status against the oracle's mixture.  MMHN_SMALL=0: everything staged."""
    lt, dp, dm, rows, ref = UC.shape_reference()
    with _engine(monkeypatch, UC.N_SHAPES, dtype, env) as e:
        e.set_cohort(rows)
        assert e.n_unknown == len(rows)
        got = e.patient_grads(lt, dp, dm)
        lp, ps = e.patient_status(lt, dp, dm)
    assert np.array_equal(lp, got[0]), "patient_status and patient_grads disagree on lp"
    UC.check_rows(got, ps, ref, dtype, f"{dtype} {env}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("f64", "f32"))
def test_shapes_against_the_engines_own_rows(monkeypatch, dtype):
    """The same rows against the engine's own type-0 and type-1 rows of the same genotypes in the same cohort, mixed in NumPy."""
    lt, dp, dm, rows, _ = UC.shape_reference()
    P = len(rows)
    dat = np.vstack((rows, [UC.relabel(r, 0) for r in rows], [UC.relabel(r, 1) for r in rows]))
    with _engine(monkeypatch, UC.N_SHAPES, dtype) as e:
        e.set_cohort(dat)
        assert e.n_unknown == P
        lp, g, a, b = e.patient_grads(lt, dp, dm)
        _, ps = e.patient_status(lt, dp, dm)
    assert np.isnan(ps[P:]).all(), "p_seeded of a row of known status is not NaN"
    mlp, r1, mg = UC.combine(lp[P:2 * P], lp[2 * P:], g[P:2 * P], g[2 * P:])
    ma = UC.combine(lp[P:2 * P], lp[2 * P:], a[P:2 * P], a[2 * P:])[2]
    ref = dict(lp=mlp, r1=r1, lp0=lp[P:2 * P], lp1=lp[2 * P:], g=mg, a=ma, b=np.zeros_like(ma))
    eps = np.finfo(np.float64 if dtype == "f64" else np.float32).eps
    print(f"{dtype}: lp differs from the mixture of the engine's own rows by {np.abs(lp[:P] - mlp).max() / eps:.2f} eps (absolute), "
          f"p_seeded by {np.abs(ps[:P] - r1).max() / eps:.2f} eps")
    UC.check_rows((lp[:P], g[:P], a[:P], b[:P]), ps[:P], ref, dtype, f"{dtype} own rows")


def _mixed(n=6, P=60, n_unknown=20, seed=11):
    """reduction_common.cohort's mixed cohort (every type and order code) with type-4 rows of 0 .. n events dealt between its rows."""
    known = RC.cohort(n, P)
    rng = np.random.default_rng(seed)
    unknown = np.array([UC.unknown_row(n, rng.choice(n, size=i % (n + 1), replace=False)) for i in range(n_unknown)], dtype=np.int8)
    at = np.sort(rng.choice(P + 1, size=n_unknown, replace=True))
    dat = np.insert(known, at, unknown, axis=0)
    assert (dat[:, -1] == 4).sum() == n_unknown and dat.shape[0] == P + n_unknown
    return dat


@pytest.mark.gpu
def test_mixed_cohort_sums_and_objective(monkeypatch):
    """cohort_sums = the per-patient rows added per class (type-4 rows in the weight-1 class), within the recursive-summation
    bound of tests/test_cohort_reduction.py; score_and_grad = the definition built from the rows and the counts; score = its
    first output; the objective layer (regularized_optimization) gives the same numbers."""
    from metmhn_amd import distributed as D, regularized_optimization as ro
    n = 6
    lt, dp, dm = UC.params(n)
    dat = _mixed(n)
    with _engine(monkeypatch, n) as e:
        e.set_cohort(dat)
        assert e.n_unknown == 20
        r1, r2 = RC.rows_of(e, lt, dp, dm), RC.rows_of(e, lt, dp, dm)
        assert np.array_equal(r1, r2) and np.isfinite(r1).all()
        cls1 = np.isin(dat[:, -1], (0, 4))
        ref = RC.Reference(r1, cls1, float(dat[:, -3].sum()), n + 1)
        sums = e.cohort_sums(lt, dp, dm)
        print(f"cohort_sums: worst error / bound {RC.check_raw(sums, ref, 'cohort_sums with type-4 rows'):.3f}")
        s, g, a, b = e.score_and_grad(lt, dp, dm, PERC_MET)
        s_only = e.score(lt, dp, dm, PERC_MET)
    want = UC.objective(r1, dat, PERC_MET)
    w, n_full = want[4]
    assert (w, n_full) == D.em_weight(float(dat[:, -3].sum()), float(dat.shape[0]), PERC_MET, 20)
    # bound, as for the pre-combined buffer of tests/test_cohort_reduction.py: the class sums are within (P_cls + 2) u S of the
    # exact ones, the weighting and the division add four roundings: (P + 8) u (w S_EM + S_NM) / n_full per element
    flat = lambda t: np.concatenate(([t[0]], np.ravel(t[1]), t[2], t[3]))
    bound = (dat.shape[0] + 8) * RC.U * (w * ref.abs_em + ref.abs_nm) / n_full
    want_v = flat(want)
    for name, got_v in (("Engine.score_and_grad", flat((s, g, a, b))), ("distributed.combine_sums", flat(D.combine_sums(sums, n + 1, PERC_MET, 20))),
                        ("regularized_optimization.score_and_grad", flat(ro.score_and_grad(lt, dp, dm, dat, PERC_MET)))):
        print(f"{name} against the definition: worst error / bound {RC.within(got_v, want_v, bound, name):.3f}")
    assert abs(s_only - s) <= bound[0] and abs(ro.score(lt, dp, dm, dat, PERC_MET) - s) <= bound[0], "score and score_and_grad disagree"
    ro.invalidate()


@pytest.mark.gpu
def test_known_rows_do_not_move(monkeypatch):
    """The mixed cohort without its type-4 rows gives per-patient rows equal (==) to the same rows inside the mixed cohort."""
    n = 6
    lt, dp, dm = UC.params(n)
    dat = _mixed(n)
    keep = dat[:, -1] != 4
    with _engine(monkeypatch, n) as e:
        e.set_cohort(dat)
        with_unknown = RC.rows_of(e, lt, dp, dm)
        e.set_cohort(dat[keep])
        assert e.n_unknown == 0
        without = RC.rows_of(e, lt, dp, dm)
        _, ps = e.patient_status(lt, dp, dm)
    assert np.isnan(ps).all()
    assert np.array_equal(with_unknown[keep], without)


@pytest.mark.gpu
def test_known_rows_do_not_move_across_batches(monkeypatch):
    """The same for a cohort in several batches (workspace limit 1 MiB), a type-4 row after every third row: type-4 rows on both
    sides of every batch edge, the batches of the two cohorts cut at different rows.  The type-4 rows themselves against a
    one-batch engine, ==."""
    n, P = 6, 1500
    lt, dp, dm = UC.params(n)
    known = RC.cohort(n, P)
    rng = np.random.default_rng(5)
    pool = np.array([UC.unknown_row(n, rng.choice(n, size=i % (n + 1), replace=False)) for i in range(P // 3)], dtype=np.int8)
    dat = np.insert(known, np.arange(3, P + 1, 3)[:len(pool)], pool, axis=0)
    keep = dat[:, -1] != 4
    # (plan.h: footprint() charges every row (stride + 1) doubles and two T, and every problem N^2 + 65 T and four vectors: at
    # least three batches under 1 MiB)
    some = dat[:, 0:2 * n + 1:2].sum(axis=1) + (dat[:, -1] != 0) > 0
    assert dat.shape[0] * ((RC.stride(n + 1) + 1) * 8 + 16) + int(some.sum()) * (((n + 1) ** 2 + 65) * 8 + 32) >= 2.5 * (1 << 20)
    with _engine(monkeypatch, n, workspace=1 << 20) as e:
        e.set_cohort(dat)
        cut = RC.rows_of(e, lt, dp, dm)
        _, ps_cut = e.patient_status(lt, dp, dm)
        e.set_cohort(dat[keep])
        cut_known = RC.rows_of(e, lt, dp, dm)
    with _engine(monkeypatch, n) as e:
        e.set_cohort(dat)
        one = RC.rows_of(e, lt, dp, dm)
        _, ps_one = e.patient_status(lt, dp, dm)
    assert np.isfinite(cut).all()
    assert np.array_equal(cut[keep], cut_known)
    assert np.array_equal(cut[~keep], one[~keep])
    assert np.array_equal(ps_cut, ps_one, equal_nan=True) and np.isfinite(ps_cut[~keep]).all() and np.isnan(ps_cut[keep]).all()


@pytest.mark.gpu
def test_objective_gradient_against_central_differences(monkeypatch):
    """The mixed cohort: the gradient of the regularised objective against central differences of score_reg along four random
    directions (h = 1e-5, rtol 2e-6, atol 1e-9: the step and bar of test_gpu_parity.py's finite-difference test)."""
    from metmhn_amd import regularized_optimization as ro
    n = 6
    lt, dp, dm = UC.params(n)
    dat = _mixed(n)
    params = np.concatenate((lt.flatten(), dp, dm))
    v, g = ro.score_and_grad_reg(params, dat, PERC_MET, ro.symmetric_penal, 1e-2)
    assert np.isfinite(v) and np.isfinite(g).all()
    rng = np.random.default_rng(5)
    h = 1e-5
    for _ in range(4):
        u = rng.standard_normal(params.size)
        u /= np.linalg.norm(u)
        fd = (float(ro.score_reg(params + h * u, dat, PERC_MET, ro.symmetric_penal, 1e-2))
              - float(ro.score_reg(params - h * u, dat, PERC_MET, ro.symmetric_penal, 1e-2))) / (2 * h)
        print(f"directional derivative {float(g @ u):.12e}, central difference {fd:.12e}, "
              f"error / bar {abs(float(g @ u) - fd) / (2e-6 * abs(fd) + 1e-9):.3e}")
        np.testing.assert_allclose(float(g @ u), fd, rtol=2e-6, atol=1e-9)
    ro.invalidate()


@pytest.mark.gpu
def test_refusals_name_the_row(monkeypatch):
    from metmhn_amd import Engine
    n = 4
    ok = UC.unknown_row(n, [0, 2])
    with _engine(monkeypatch, n) as e:
        for what, edit, text in (("an MT bit", lambda r: r.__setitem__(3, 1), "must have no MT event"),
                                 ("the seeding", lambda r: r.__setitem__(2 * n, 1), "must have seeding = 0"),
                                 ("type 5", lambda r: r.__setitem__(-1, 5), "type column must be 0..4")):
            bad = ok.copy()
            edit(bad)
            with pytest.raises(RuntimeError, match=r"row 2\b") as err:
                e.set_cohort(np.array([ok, ok, bad, ok]))
            assert text in str(err.value), what
            assert e.n_pat == 0 and e.n_unknown == 0
        e.set_cohort(np.array([ok, ok]))
        assert e.n_unknown == 2
    with Engine(31) as e:                                       # |x| + 1 = 31 > MAXK = 30
        wide = UC.unknown_row(31, range(30))
        with pytest.raises(RuntimeError, match=r"too many active events for one patient \(row 1\)"):
            e.set_cohort(np.array([UC.unknown_row(31, [1]), wide]))
        assert e.n_pat == 0
    # the order entry points keep refusing every type outside 0 .. 3: the row's own status, the others unaffected
    lt, dp, dm = UC.params(n)
    dat = np.array([UC.relabel(ok, 1), ok, UC.relabel(ok, 0)])
    with Engine(n) as e:
        le, pre, pos, status = e.order_posteriors(lt, dp, dm, dat)
    assert status[0] == 0 and status[2] == 0 and (status[1] & 0xFFFF) == 2 and (status[1] >> 16) == 1      # MMHN_ORD_BAD_STATUS
    assert np.isnan(le[1]) and np.isfinite(le[[0, 2]]).all()


@pytest.mark.gpu
def test_met_status_posterior(monkeypatch):
    """One genotype as a row of type 0, 1 and 4: three equal values; NaN on types 2 and 3; the values are patient_status'."""
    from metmhn_amd import regularized_optimization as ro, synthetic
    n = 6
    lt, dp, dm = UC.params(n)
    x = UC.unknown_row(n, [0, 3, 4])
    paired = synthetic.full_k_cohort(n, 2, k=4, seed=1)
    mt_only = UC.relabel(x, 1); mt_only[0:2 * n:2] = 0; mt_only[1] = 1; mt_only[-1] = 2
    dat = np.vstack((UC.relabel(x, 0), UC.relabel(x, 1), x, paired, mt_only, UC.unknown_row(n, [])))
    got = ro.met_status_posterior(lt, dp, dm, dat)
    assert got.shape == (7,) and got[0] == got[1] == got[2] and np.isnan(got[3:6]).all()
    ref = [UC.mixture_lp(lt, dp, dm, r) for r in (x, UC.unknown_row(n, []))]
    for i, m in ((2, ref[0]), (6, ref[1])):
        assert abs(got[i] - m[1]) <= UC.p_bar(m[2], m[3], "f64"), (i, got[i], m[1])
    assert np.isnan(ro.met_status_posterior(lt, dp, dm, paired)).all()


MC_N, MC_SAMPLES, MC_KEY, MC_MIN = 6, 2_000_000, 7, 2000


@pytest.mark.gpu
def test_met_status_posterior_monte_carlo():
    """simulate_dat at n = 6, 2 10^6 trajectories under a fixed key: for every PT genotype with at least 2 000 samples the share
    with the seeding set against p_seeded, bar 5 binomial standard errors sqrt(p (1 - p) / m) under the model.
    What corresponds (csrc/sampler.h): the primary tumour stops at its own diagnosis, in every class of simulate_dat's order
    column - unseeded, seeded and PT observed first, seeded and MT observed first -, so the PT columns are the PT genotype at the
    PT's observation, and the seeding column says whether the seeding had happened by then (it is an event of the primary
    tumour: it cannot happen after the PT's diagnosis).  All three classes therefore enter the anchor.
    The CPU sampler (oracle/gillespie.py, 2 10^6 draws, seed 123) against the oracle's mixture stays inside the same cut: worst
    2.67 standard errors over its 37 genotypes with at least 2 000 samples (the same 2.67 over the 28 with at least 5 000), so
    the threshold of 2 000 stands."""
    from metmhn_amd import regularized_optimization as ro, simulations as S
    n = MC_N
    lt, dp, dm = UC.params(n)
    sim = S.simulate_dat(lt, dp, dm, MC_SAMPLES, MC_KEY)
    worst, used = _mc_worst(sim, n, lambda rows: ro.met_status_posterior(lt, dp, dm, rows))
    print(f"{used} PT genotypes with at least {MC_MIN} samples; worst deviation {worst:.2f} binomial standard errors")
    assert used >= 20 and worst <= 5.0


def _mc_worst(sim, n, posterior):
    """(worst |share - p| / sqrt(p (1 - p) / m), genotypes used) over the PT genotypes of `sim` with at least MC_MIN samples."""
    pt = sim[:, 0:2 * n:2].astype(np.int64)
    key = pt @ (1 << np.arange(n))
    seeded = sim[:, 2 * n] == 1
    m = np.bincount(key, minlength=1 << n)
    k1 = np.bincount(key[seeded], minlength=1 << n)
    use = np.flatnonzero(m >= MC_MIN)
    rows = np.array([UC.unknown_row(n, [j for j in range(n) if (x >> j) & 1]) for x in use], dtype=np.int8)
    p = posterior(rows)
    assert np.isfinite(p).all() and ((p > 0) & (p < 1)).all()
    z = np.abs(k1[use] / m[use] - p) / np.sqrt(p * (1 - p) / m[use])
    return float(z.max()), int(use.size)


@pytest.mark.gpu
def test_luad28_with_unknown_primaries(monkeypatch, golden):
    """The 28-event LUAD cohort with its 1 227 primaries of unknown status (tests/golden/luad28_unknown_rows.npy, made by
    tests/tools/make_golden_luad_unknown.py) at the reference's published fit: lp and p_seeded of a fixed sample of 100 of these
    rows and of the 10 widest against the oracle's mixture; the whole cohort of 6 079 rows evaluated in the three dispatches of
    test_gpu_parity.py's LUAD test, finite throughout."""
    from metmhn_amd import Engine
    g = golden("luad28")
    unknown = np.load(os.path.join(GOLDEN, "luad28_unknown_rows.npy"))
    assert unknown.dtype == np.int8 and unknown.shape == (1227, 59) and (unknown[:, -1] == 4).all()
    dat = np.vstack((g["dat"], unknown))
    P0 = g["dat"].shape[0]
    lt, dp, dm = g["fit_theta"], g["fit_dp"], g["fit_dm"]
    width = unknown[:, 0:56:2].sum(axis=1)
    pick = np.unique(np.concatenate((np.random.default_rng(28).choice(1227, size=100, replace=False), np.argsort(width, kind="stable")[-10:])))
    ref = [UC.mixture_lp(lt, dp, dm, unknown[i]) for i in pick]
    ref = {k: np.array([r[j] for r in ref]) for j, k in enumerate(("lp", "r1", "lp0", "lp1"))}
    pm = float(g["perc_met"])
    for env in ({}, {"MMHN_COOP": "0"}, {"MMHN_PSOLVE_MIN": "1", "MMHN_POISON": "1"}):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        with Engine(28) as e:
            e.set_cohort(dat)
            assert e.n_unknown == 1227
            lp, ps = e.patient_status(lt, dp, dm)
            s, G, ga, gb = e.score_and_grad(lt, dp, dm, pm)
        for k_ in env:
            monkeypatch.delenv(k_)
        assert np.isfinite(lp).all() and np.isfinite(ps[P0:]).all() and np.isnan(ps[:P0]).all(), env
        assert np.isfinite(s) and np.isfinite(G).all() and np.isfinite(ga).all() and np.isfinite(gb).all(), env
        np.testing.assert_allclose(lp[:P0], g["fit_lp"], rtol=1e-9, atol=1e-11, err_msg=f"known rows {env}")
        worst = UC.ratio(lp[P0 + pick], ref["lp"], *UC.LP_BAR["f64"], f"LUAD-28 {env} lp of {pick.size} type-4 rows")
        err = np.abs(ps[P0 + pick] - ref["r1"]) / UC.p_bar(ref["lp0"], ref["lp1"], "f64")
        print(f"LUAD-28 {env} p_seeded: worst error / bar {err.max():.3e}; p_seeded over the 1 227 rows: "
              f"min {ps[P0:].min():.3f}, median {np.median(ps[P0:]):.3f}, max {ps[P0:].max():.3f}")
        assert worst <= 1.0 and err.max() <= 1.0
