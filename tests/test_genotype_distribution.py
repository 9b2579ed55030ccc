"""The genotype distribution of the primary tumour: the probability of every genotype to be the observed one, unseeded
(U) and seeded by then (S), from one forward sweep (MetMHN.genotype_distribution / genotype_distribution_at,
GenotypeDistribution, GenotypeSummary, mmhn_genotype_distribution, regularized_optimization.genotype_fit;
metmhn_amd/csrc/genodist.h).

CPU: the host definition against exp(oracle.dense.patient_lp) of every genotype as a type-0 and a type-1 row (1e-12
relative), its identities, the recursion re-evaluated in long double, the host summary against brute force in long
double, rates of 0, compare / genotype_fit against their formulas, the refusals.

GPU: the device against the host definition, against the engine's own cohort rows, against the backward sweep
(landscape.h, whose recursion shares no line with the forward one), the reduction alone, the bytes whatever the queries.

The bound of the device against the host (lattice_common.genodist_bound): chain_bound with the primary tumour's eps (pt_eps, obs1 with
the clock's entry).  One step of the chain, on one side: the numerator takes a product and at most n + 1 additions (the n
pulls and, for the seeded plane, G0 sigma); the den takes at most n + 2 additions and, for kappa1 = kappa0 exp(obs1_n),
one product and the exponential's own 2 u; the division: (2 n + 7) u, both sides 4 n + 14 a step.  The chain behind a value
is at most n + 1 states deep and n + 2 steps through the seeding (G0 sigma of the same state is one more step); on the way
out kappa times G.  Every value of both planes agrees within relative
    bound(n) = (n + 2) (4 eps + (4 n + 14) u) + 2 eps + 8 u,
the summary within bound(n) + (RED(n) + n + 19) u.  The device's summary against the long-double sums of the device's own
`full` output has the reduction's term alone: RED(n) u (1 % on top for the long-double side).

Measured on an MI355X, worst error / bound per test: device against host 3.1e-3 for the planes (n = 1; 1.5e-3 at
n = c + 3) and 2.7e-3 for the summary; exp(lp) of the engine's own rows 5.4e-6 and p_seeded 1.1e-6 of the 1e-9 bar; mass[1]
against the device landscape 0 (n = c + 6) and 7.3e-6 (n = 22); the reduction alone 0.11; a mutation of rate 0 1.7e-3.
CPU: the host definition against the dense oracle 2.0e-15 relative at the worst, p_seeded against the oracle's mixture
1.1e-7 of its bar, the recursion's residual 3.6 u against 26 u, the host summary 0.14 of (n + 19) u.
"""
import re

import numpy as np
import pytest

import metmhn_amd.model as model_mod
from metmhn_amd import regularized_optimization as ro
from metmhn_amd.model import GenotypeDistribution, GenotypeSummary, MetMHN
from lattice_common import (C, U, bits, brute_summary, check_same_bytes, fit_cohort, host_once, landscape_bound, ld_rel, no_library,
                            note, red, rel, summary_rel, without)
from lattice_common import genodist_bound as bound, genodist_summary_bound as summary_bound
from order_common import model


@host_once
def host(n, seed):
    """(planes [2, 2^n], GenotypeSummary) of order_common.model(n, seed) by the host definition."""
    mod = model(n, seed=seed)
    whole = mod._genodist_host()
    return whole, mod._genodist_summary_host(whole)


def rows_of(n, codes, typ):
    """Cohort rows of type 0 / 1 / 4 with the PT genotypes `codes`."""
    codes = np.asarray(codes, dtype=np.int64)
    dat = np.zeros((len(codes), 2 * n + 3), dtype=np.int8)
    dat[:, 0:2 * n:2] = bits(n, codes)
    dat[:, -3], dat[:, -2], dat[:, -1] = (1 if typ == 1 else 0), -99, typ
    return dat


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_host_definition_against_the_dense_oracle_of_every_genotype():
    from oracle import dense
    worst = 0.0
    for n in range(1, 7):
        mod = model(n, seed=n)
        got = mod.genotype_distribution(backend="host")
        assert isinstance(got, GenotypeDistribution) and np.array_equal(got.codes, np.arange(1 << n))
        whole = np.stack((got.unseeded, got.seeded))
        assert whole.shape == (2, 1 << n) and np.array_equal(whole, host(n, n)[0])
        args = (mod.log_theta, mod.obs1, mod.obs2)
        for typ in (0, 1):
            ref = np.exp([dense.patient_lp(*args, r) for r in rows_of(n, np.arange(1 << n), typ)])
            worst = max(worst, rel(whole[typ], ref))
        empty = 1.0 / (1.0 + np.trace(np.exp(mod.log_theta)))
        assert abs(got.unseeded[0] - empty) <= 1e-12 * empty
    print(f"host definition against exp(dense.patient_lp) of every genotype, n = 1 .. 6: worst relative {worst:.2e}")
    assert worst <= 1e-12


def test_identities():
    for n, seed in ((3, 3), (7, 7), (10, 10)):
        mod = model(n, seed=seed)
        whole, summary = host(n, seed)
        got = GenotypeDistribution(whole[0], whole[1], np.arange(1 << n), summary)
        # 1 in exact arithmetic: the host's own share of the bound is the bar
        assert abs(got.total.sum() - 1.0) <= summary_bound(mod)
        assert abs(summary.mass.sum() - 1.0) <= summary_bound(mod)
        back = mod._landscape_host("observation")[0, 0]
        assert abs(summary.mass[1] - back) <= 1e-12 * back, (n, summary.mass[1], back)
        assert (whole > 0).all() and ((got.p_seeded > 0) & (got.p_seeded < 1)).all()
        for s, stratum in enumerate(("NM", "EM-PT")):
            assert abs(summary.burden_pmf(stratum).sum() - 1.0) <= summary_bound(mod)
            assert np.array_equal(summary.frequencies(stratum), summary.pairs[s] / summary.mass[s])
        f = summary.frequencies("unknown")
        assert np.array_equal(f, (summary.pairs[0] + summary.pairs[1]) / (summary.mass[0] + summary.mass[1]))
        lo = summary.log_odds("unknown")
        assert np.isnan(np.diag(lo)).all() and np.isfinite(lo[~np.eye(n, dtype=bool)]).all()
        m = np.diag(f)
        assert abs(lo[0, 1] - np.log(f[0, 1] * (1 - m[0] - m[1] + f[0, 1]) / ((m[0] - f[0, 1]) * (m[1] - f[0, 1])))) <= 1e-12
    with pytest.raises(ValueError, match="stratum must be one of"):
        summary.frequencies("paired")


def test_p_seeded_against_the_oracles_mixture():
    import unknown_common as UC
    n = 6
    lt, dp, dm = UC.params(n)
    got = MetMHN(lt, dp, dm).genotype_distribution(backend="host")
    worst = 0.0
    for x in range(1 << n):
        lp, r1, lp0, lp1 = UC.mixture_lp(lt, dp, dm, UC.unknown_row(n, [j for j in range(n) if x >> j & 1]))
        worst = max(worst, abs(got.p_seeded[x] - r1) / UC.p_bar(lp0, lp1, "f64"))
        assert abs(got.total[x] - np.exp(lp)) <= 1e-12 * np.exp(lp)
    print(f"p_seeded against the oracle's type-4 mixture, n = {n}: worst error / bar {worst:.3e}")
    assert worst <= 1.0


def test_recursion_in_long_double():
    """Every state of one n = 10 model: the right-hand side of the recursion from the host's own fp64 rates and its values
    at the predecessors (and, for the seeded plane, its unseeded value at the state), evaluated in np.longdouble, against
    the host's value at the state.  With G = P / kappa: U(y) = kappa0 (sum_b U(y-b) / kappa0(y-b) lambda_b(y-b)) / den0,
    S(y) = kappa1 (U(y) / kappa0 sigma + sum_b S(y-b) / kappa1(y-b) lambda_b(y-b)) / den1.  The fp64 evaluation rounds along a
    path of the non-negative sum-product: the G of a predecessor against the value it returned (1), its product (1), at most
    n + 1 additions of the numerator, at most n + 2 additions of den, the division (1), kappa times G (1): 2 n + 6, so the
    residual is within (2 n + 6) u relative; the long double side adds 2^-64 terms, below the 1 % allowed on top."""
    n, seed, ld = 10, 10, np.longdouble
    mod = model(n, seed=seed)
    th = mod._pt_log_theta
    P = host(n, seed)[0]
    sums = model_mod._subset_sums
    lam = [np.exp(th[j, j] + sums(np.where(np.arange(n) == j, 0.0, th[j, :n]))) for j in range(n)]
    sig = np.exp(th[n, n] + sums(th[n, :n]))
    kap0 = np.exp(sums(mod.obs1[:n]))
    kap1 = kap0 * np.exp(mod.obs1[n])
    worst = 0.0
    for y in range(1, 1 << n):
        f0, f1, L = ld(0), ld(P[0, y]) / ld(kap0[y]) * ld(sig[y]), ld(0)
        for b in range(n):
            if y >> b & 1:
                x, r = y ^ 1 << b, ld(lam[b][y ^ 1 << b])
                f0 += ld(P[0, x]) / ld(kap0[x]) * r
                f1 += ld(P[1, x]) / ld(kap1[x]) * r
            else:
                L += ld(lam[b][y])
        ref = (ld(kap0[y]) * f0 / (L + ld(sig[y]) + ld(kap0[y])), ld(kap1[y]) * f1 / (L + ld(kap1[y])))
        for s in range(2):
            worst = max(worst, float(abs(ld(P[s, y]) - ref[s]) / ref[s]))
    print(f"residual of the recursion in long double, n = {n}: {worst / U:.2f} u, bar {2 * n + 6} u")
    assert worst <= 1.01 * (2 * n + 6) * U


def test_host_summary_against_brute_force_in_long_double():
    worst = 0.0
    for n in range(1, 9):
        whole, summary = host(n, n)
        assert summary.mass.shape == (2,) and summary.pairs.shape == (2, n, n) and summary.burden.shape == (2, n + 1)
        assert np.array_equal(summary.pairs, summary.pairs.transpose(0, 2, 1))
        ref = brute_summary(whole)
        err = max(ld_rel(a, b) for a, b in zip((summary.mass, summary.pairs, summary.burden), ref))
        worst = max(worst, err / ((n + 19) * U))
    print(f"host summary against long-double brute force, n = 1 .. 8: worst error / ((n + 19) u) {worst:.3e}")
    assert worst <= 1.01


def check_dead_mutation(a, b, codes, small, j, bar):
    """a: the distribution with mutation j of rate 0, b: the one of the model without it."""
    holds = np.setdiff1d(a.codes, codes)
    keep = [i for i in range(a.summary.n_mut) if i != j]
    worst = 0.0
    for name in ("unseeded", "seeded"):
        assert np.isfinite(getattr(a, name)).all() and (getattr(a, name)[holds] == 0.0).all(), name
        worst = max(worst, rel(getattr(a, name)[codes], getattr(b, name)[small]) / bar)
    assert (a.summary.pairs[:, j, :] == 0.0).all() and (a.summary.pairs[:, :, j] == 0.0).all()
    assert (a.summary.burden[:, -1] == 0.0).all()
    worst = max(worst, rel(a.summary.pairs[np.ix_([0, 1], keep, keep)], b.summary.pairs) / bar,
                rel(a.summary.mass, b.summary.mass) / bar, rel(a.summary.burden[:, :-1], b.summary.burden) / bar)
    return worst


def test_a_mutation_of_rate_zero():
    n, j = 6, 2
    dead, less, codes, small = without(model(n, seed=35), j)
    worst = check_dead_mutation(dead.genotype_distribution(backend="host"), less.genotype_distribution(backend="host"),
                                codes, small, j, 1e-12)
    print(f"a mutation of rate 0 against the model without it (host): worst error / 1e-12 {worst:.3e}")
    assert worst <= 1.0


def test_a_seeding_of_rate_zero():
    n = 6
    mod = model(n, seed=36)
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    got = MetMHN(th, mod.obs1, mod.obs2).genotype_distribution(backend="host")
    assert (got.seeded == 0.0).all() and np.isfinite(got.unseeded).all() and (got.unseeded > 0).all()
    assert got.summary.mass[1] == 0.0 and not got.summary.pairs[1].any() and not got.summary.burden[1].any()
    assert np.isfinite(got.summary.mass).all() and abs(got.summary.mass[0] - 1.0) <= 1e-12
    assert (got.p_seeded == 0.0).all() and np.array_equal(got.total, got.unseeded)


def check_fit(fit, mod, dat, whole, summary, bar):
    """genotype_fit's result against the formulas written out from the planes `whole` and `summary`."""
    n = mod.n
    typ = dat[:, -1]
    codes = dat[:, 0:2 * n:2].astype(np.int64) @ (1 << np.arange(n))
    own = np.isin(typ, (0, 1, 4))
    assert own.any() and not own.all() and (typ == 4).any()
    assert np.array_equal(fit.codes, np.where(own, codes, -1)) and np.isnan(fit.prob[~own]).all()
    ref = np.where(typ == 0, whole[0, codes] / summary.mass[0], np.where(typ == 1, whole[1, codes] / summary.mass[1],
                                                                          whole[0, codes] + whole[1, codes]))
    worst = rel(fit.prob[own], ref[own]) / bar
    res = summary.compare(dat)
    assert set(fit.residuals) == set(res) == {"NM", "EM-PT", "unknown"} == set(fit.table)
    for stratum, ty in (("NM", 0), ("EM-PT", 1), ("unknown", 4)):
        g = dat[typ == ty][:, 0:2 * n:2].astype(np.float64)
        rows = g.shape[0]
        p = {"NM": summary.pairs[0] / summary.mass[0], "EM-PT": summary.pairs[1] / summary.mass[1],
             "unknown": (summary.pairs[0] + summary.pairs[1]) / (summary.mass[0] + summary.mass[1])}[stratum]
        want = (g.T @ g - rows * p) / np.sqrt(rows * p * (1 - p))
        assert np.array_equal(res[stratum], want) and np.isfinite(want).all()
        assert np.allclose(fit.residuals[stratum], want, rtol=1e-6, atol=0)
        uniq, observed, expected = fit.table[stratum]
        assert np.array_equal(uniq, np.unique(codes[typ == ty])) and observed.sum() == rows
        assert np.array_equal(observed, [(codes[typ == ty] == x).sum() for x in uniq])
        worst = max(worst, rel(expected, [rows * ref[typ == ty][codes[typ == ty] == x][0] for x in uniq]) / bar)
    return worst


def test_compare_and_genotype_fit_on_a_mixed_cohort():
    n = 5
    mod = model(n, seed=48)
    dat = fit_cohort(n)
    fit = ro.genotype_fit(mod.log_theta, mod.obs1, mod.obs2, dat, backend="host")
    whole = mod._genodist_host()
    summary = mod._genodist_summary_host(whole)
    assert summary_rel(fit.summary, summary) == 0.0
    worst = check_fit(fit, mod, dat, whole, summary, 1e-12)
    print(f"genotype_fit against its formulas (host): worst error / 1e-12 {worst:.3e}")
    assert worst <= 1.0
    with pytest.raises(ValueError, match=r"dat must have shape \(n_pat, 13\)"):
        summary.compare(dat[:, 1:])
    only = ro.genotype_fit(mod.log_theta, mod.obs1, mod.obs2, dat[np.isin(dat[:, -1], (2, 3))][:2], backend="host")
    assert np.isnan(only.prob).all() and only.table == {} and only.residuals == {}


def test_refusals(monkeypatch):
    no_library(monkeypatch)
    n = 5
    mod = model(n, seed=36)
    G = bits(n, [1, 10, 0])
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.genotype_distribution(backend="cpu")
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.genotype_distribution_at(G, backend="cpu")
    for bad in (G[0], G[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=rf"genotypes must have shape \[R, {n}\]") as e1:
            mod.genotype_distribution_at(bad)
        with pytest.raises(ValueError) as e2:
            mod.seeding_landscape_at(bad)
        assert str(e1.value) == str(e2.value)
    H = G.copy()
    H[1, 4] = 2
    with pytest.raises(ValueError, match=r"^row 1: ") as e1:
        mod.genotype_distribution_at(H)
    with pytest.raises(ValueError) as e2:
        mod.seeding_landscape_at(H)
    assert str(e1.value) == str(e2.value)
    wide = model(25, seed=1)
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.genotype_distribution(backend="host")
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.genotype_distribution_at(np.zeros((1, 25), dtype=np.int8), backend="host")
    with pytest.raises(ValueError, match=rf"needs {16 << n} bytes, more than max_bytes = 511"):
        mod.genotype_distribution(backend="host", max_bytes=(16 << n) - 1)
    with pytest.raises(ValueError, match=rf"needs {16 << 28} bytes, more than max_bytes = {2 ** 31}"):
        model(28, seed=1).genotype_distribution()                      # the default: 2 GiB, n <= 27; before any library
    with pytest.raises(ValueError, match=rf"needs {16 << 31} bytes"):
        model(31, seed=1).genotype_distribution(max_bytes=2 ** 34)
    whole = mod.genotype_distribution(backend="host", max_bytes=16 << n)
    assert whole.unseeded.shape == (1 << n,) and whole.seeded.shape == (1 << n,)
    some = mod.genotype_distribution_at(G, backend="host")
    assert some.codes.tolist() == [1, 10, 0]
    assert np.array_equal(some.unseeded, whole.unseeded[[1, 10, 0]]) and np.array_equal(some.seeded, whole.seeded[[1, 10, 0]])
    assert np.array_equal(some.total, some.unseeded + some.seeded) and np.array_equal(some.p_seeded, some.seeded / some.total)
    assert summary_rel(some.summary, whole.summary) == 0.0
    empty = mod.genotype_distribution_at(np.zeros((0, n), dtype=np.int8), backend="host")
    assert empty.unseeded.shape == (0,) and empty.codes.shape == (0,) and summary_rel(empty.summary, whole.summary) == 0.0


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 3, C, C + 1, C + 3))
def test_device_against_the_host_definition(n):
    """One partial tile (n = 1, 3), exactly one tile (n = c), two tiles and one high bit (c + 1), several tiles on a level
    (c + 3).  Bounds: module docstring."""
    from metmhn_amd.jx import engine
    seed = 40 + n
    mod = model(n, seed=seed)
    values, status, sums, whole = engine(n).genotype_distribution(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8),
                                                                  summary=True, full=True)
    assert values.shape == (0, 2) and status.shape == (0,) and whole.shape == (2, 1 << n)
    assert sums[0].shape == (2,) and sums[1].shape == (2, n, n) and sums[2].shape == (2, n + 1)
    ref, ref_summary = host(n, seed)
    note(f"device planes against host, n = {n}", rel(whole, ref) / bound(mod))
    note(f"device summary against host, n = {n}", summary_rel(sums, ref_summary) / summary_bound(mod))
    assert np.array_equal(sums[1], sums[1].transpose(0, 2, 1))
    got = mod.genotype_distribution()
    assert np.stack((got.unseeded, got.seeded)).tobytes() == whole.tobytes()
    for a, b in zip((got.summary.mass, got.summary.pairs, got.summary.burden), sums):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_device_against_the_engines_own_rows():
    """n = c + 4, 24 genotypes, each as a row of type 0, 1 and 4 of one cohort: exp of the evaluation's log-probabilities
    and its P(seeded | genotype) against the sweep, at the project's 1e-9 (relative)."""
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    n = C + 4
    mod = model(n, seed=70)
    G = (np.random.default_rng(71).random((24, n)) < 0.5).astype(np.int8)
    assert (G.sum(axis=1) <= 14).all() and len(np.unique(G, axis=0)) == 24
    codes = G.astype(np.int64) @ (1 << np.arange(n))
    values, status, _, _ = engine(n).genotype_distribution(mod.log_theta, mod.obs1, G, summary=False)
    assert (status == 0).all() and (values > 0).all()
    dat = np.vstack([rows_of(n, codes, typ) for typ in (0, 1, 4)])
    with Engine(n) as eng:
        eng.set_cohort(dat)
        lp = eng.patient_grads(mod.log_theta, mod.obs1, mod.obs2, with_grad=False)
        lp2, ps = eng.patient_status(mod.log_theta, mod.obs1, mod.obs2)
    ref = np.concatenate((values[:, 0], values[:, 1], values.sum(axis=1)))
    note("exp(lp) of the engine's rows of types 0, 1, 4 against the sweep, over 1e-9", rel(np.exp(lp), ref) / 1e-9)
    assert np.isnan(ps[:48]).all()
    note("patient_status' p_seeded against S / (U + S), over 1e-9", rel(ps[48:], values[:, 1] / values.sum(axis=1)) / 1e-9)
    at = mod.genotype_distribution_at(G)
    assert np.stack((at.unseeded, at.seeded), axis=1).tobytes() == values.tobytes() and np.array_equal(at.codes, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (C + 6, 22))
def test_seeded_mass_against_the_backward_sweep(n):
    """mass[1] = the seeding landscape's p_seed of the empty genotype until the observation: the forward sweep meets the
    backward one in one number (n = 22: 64 MiB here, 128 MiB there).  The bar is the sum of the two bounds - this file's
    summary bound and tests/test_seeding_landscape.py's (n + 1) (4 eps + (2 n + 8) u)."""
    from metmhn_amd.jx import engine
    mod = model(n, seed=50 + n)
    _, _, sums, _ = engine(n).genotype_distribution(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8))
    back, status, _ = engine(n).seeding_landscape(mod.log_theta, mod.obs1, np.zeros((1, n), dtype=np.int8), "observation")
    assert status.tolist() == [0]
    note(f"mass[1] against the landscape's p_seed of the empty genotype, n = {n}",
         rel(sums[0][1], back[0, 0]) / (summary_bound(mod) + landscape_bound(mod, clock=True)))
    assert abs(sums[0].sum() - 1.0) <= summary_bound(mod)


@pytest.mark.gpu
def test_the_reduction_alone():
    """n = c + 3: the device summary against the long-double sums over the device's own `full` output; only the
    reduction's term of the bound applies."""
    from metmhn_amd.jx import engine
    n = C + 3
    mod = model(n, seed=40 + n)
    _, _, sums, whole = engine(n).genotype_distribution(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8), full=True)
    ref = brute_summary(whole)
    note(f"the reduction alone, n = {n}", max(ld_rel(a, b) for a, b in zip(sums, ref)) / (1.01 * red(n) * U))


@pytest.mark.gpu
def test_same_bytes_whatever_the_queries():
    from metmhn_amd.jx import engine
    n = C + 1
    mod = model(n, seed=41 + C)
    check_same_bytes(lambda G, **kw: engine(n).genotype_distribution(mod.log_theta, mod.obs1, G, **kw), 2, n,
                     mod.genotype_distribution_at)


@pytest.mark.gpu
def test_rates_of_zero_on_the_device():
    n, j = C + 1, C                                                    # the dead mutation is the high bit: whole tiles of zeros
    mod = model(n, seed=80)
    for jj in (j, 2):
        dead, less, codes, small = without(mod, jj)
        a, b = dead.genotype_distribution(), less.genotype_distribution(backend="host")
        note(f"a mutation of rate 0 (bit {jj}) on the device against the host model without it",
             check_dead_mutation(a, b, codes, small, jj, summary_bound(less)))
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    got = MetMHN(th, mod.obs1, mod.obs2).genotype_distribution()
    assert (got.seeded == 0.0).all() and np.isfinite(got.unseeded).all() and (got.unseeded > 0).all()
    assert got.summary.mass[1] == 0.0 and not got.summary.pairs[1].any() and not got.summary.burden[1].any()
    assert np.isfinite(got.summary.pairs).all() and np.isfinite(got.summary.burden).all()
    assert abs(got.summary.mass[0] - 1.0) <= summary_bound(mod)


@pytest.mark.gpu
def test_genotype_fit_on_the_device():
    """genotype_fit against its formulas from the device's own planes and summary."""
    m5 = model(5, seed=48)
    dat = fit_cohort(5)
    fit = ro.genotype_fit(m5.log_theta, m5.obs1, m5.obs2, dat)
    whole = m5.genotype_distribution()
    note("genotype_fit on the device against its formulas, over 1e-12",
         check_fit(fit, m5, dat, np.stack((whole.unseeded, whole.seeded)), whole.summary, 1e-12))


@pytest.mark.gpu
def test_a_distribution_that_does_not_fit_is_refused_with_its_bytes():
    from metmhn_amd.engine import Engine
    n = 31
    mod = model(n, seed=3)
    row = bits(n, [1 | 1 << 30])
    with Engine(n, workspace_bytes=1 << 30) as small:
        with pytest.raises(RuntimeError, match=r"31 mutations need (\d+) bytes.*limit is 1073741824 bytes") as err:
            small.genotype_distribution(mod.log_theta, mod.obs1, row)
        need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
        partials = 2 * 67 * 8 << (n - C)
        assert (16 << n) + (4 << (n - C)) + partials <= need <= (16 << n) + (4 << (n - C)) + partials + (1 << 16)
        with pytest.raises(RuntimeError, match=r"need (\d+) bytes") as err:
            small.genotype_distribution(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8), summary=False)
        need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
        assert 16 << n <= (16 << n) + (4 << (n - C)) <= need <= (16 << n) + (4 << (n - C)) + (1 << 16)
    with pytest.raises(ValueError, match=rf"needs {16 << n} bytes"):
        mod.genotype_distribution()
