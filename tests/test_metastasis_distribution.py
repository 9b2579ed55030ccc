"""The genotype distribution of the metastasis and of its founder: the probability of every genotype to be the seeding
cell's (Z), the metastasis' observed one (M) and M weighted by the founder's share of its mutations (C), from one forward
sweep (MetMHN.metastasis_distribution / metastasis_distribution_at, MetastasisDistribution, MetastasisSummary,
mmhn_metastasis_distribution, regularized_optimization.metastasis_fit; metmhn_amd/csrc/metdist.h).

CPU: the host definition's M against exp(oracle.dense.patient_lp) of every genotype as a type-2 row (1e-12 relative),
its identities, founder_events against the order posteriors of the type-2 rows, the model whose two chains coincide
against genotype_distribution's seeded plane, the recursion re-evaluated in long double, the host summary against brute
force in long double, rates of 0, the summary's methods and metastasis_fit against their formulas, the refusals.

GPU: the device against the host definition, against the engine's own type-2 rows, against the device's order posteriors
(which share no code with the sweep), against the device's genotype distribution and landscape, the reduction alone, the
bytes whatever the queries, Monte Carlo.

The bound of the device against the host: lattice_common's chain_bound with the pair's eps (pair_eps).  One step of the
chain, on one side: the numerator takes a product and at most n + 1 additions (the n pulls and G0 sigma), and for FC one
more product (G0 sigma times |y|); the den takes at most n + 2 additions; the division: (2 n + 8) u, both sides 4 n + 16 a
step.  The chain behind a value is n + 1 states and the seeding step: n + 2 steps; on the way out sigma or kappam times G.
Every value of the three planes agrees within relative
    bound(n) = (n + 2) (4 eps + (4 n + 16) u) + 2 eps + 8 u,
the summary, whose reductions are genodist.h's, within bound(n) + (RED(n) + n + 19) u; the device's summary against the
long-double sums of its own `full` planes: RED(n) u (1 % on top for the long-double side).  founder_events = C / M is a
quotient of two such values: 2 bound(n) + u.  Against the primary tumour's sweeps the bar adds their files' bounds
(lattice_common's genodist_bound, genodist_summary_bound and landscape_bound).

Measured on an MI355X, worst error / bound per test: device against host 3.2e-3 for the planes (n = 1; 1.7e-3 at
n = c + 3) and 2.9e-3 for the summary; exp(lp) of the engine's own type-2 rows 9.5e-6 of the 1e-9 bar; founder_events
against the device order posteriors 5.3e-6 and log M against their log_evidence 7.1e-6 of the 1e-9 bar; coinciding chains
against the device's seeded plane 1.1e-4; the masses against the other two sweeps 1.3e-5 and sum C against sum |y| Z 3.8e-5
(n = c + 6, 22); the reduction alone 0.14; a mutation of rate 0 1.7e-3; metastasis_fit device against host 7.8e-4; Monte
Carlo 2.02 standard errors over 28 entries (93 947 seeded samples) against the bar of 5.
CPU: the host definition against the dense oracle 2.9e-15 relative at the worst, founder_events against the host order
posteriors 1.3e-15 absolute, coinciding chains 6.8e-16 relative, the recursion's residual 3.8 u against 27 u, the host summary
0.17 of (n + 19) u.
"""
import numpy as np
import pytest

import metmhn_amd.model as model_mod
from metmhn_amd import regularized_optimization as ro
from metmhn_amd.model import GenotypeSummary, MetastasisDistribution, MetastasisSummary, MetMHN
from lattice_common import (C, U, bits, brute_summary, chain_bound, check_same_bytes, genodist_bound, genodist_summary_bound,
                            host_once, landscape_bound, ld_rel, no_library, note, pair_eps, red, rel, summary_rel, without)
from lattice_common import fit_cohort as pt_fit_cohort
from order_common import mixed_cohort, model

PLANES = ("founder", "metastasis", "founder_weighted")


def bound(mod):
    """Any plane of the device against the host definition (module docstring)."""
    return chain_bound(pair_eps(mod), mod.n + 2, 4 * mod.n + 16, out=True)


def summary_bound(mod):
    return chain_bound(pair_eps(mod), mod.n + 2, 4 * mod.n + 16, out=True, summed=mod.n)


@host_once
def host(n, seed):
    """(planes [3, 2^n], MetastasisSummary) of order_common.model(n, seed) by the host definition."""
    mod = model(n, seed=seed)
    whole = mod._metdist_host()
    return whole, mod._metdist_summary_host(whole)


def mt_rows(n, codes):
    """Cohort rows of type 2 with the MT genotypes `codes`."""
    codes = np.asarray(codes, dtype=np.int64)
    dat = np.zeros((len(codes), 2 * n + 3), dtype=np.int8)
    dat[:, 1:2 * n:2] = bits(n, codes)
    dat[:, -3], dat[:, -2], dat[:, -1] = 1, -99, 2
    return dat


def coinciding(mod):
    """The model with theta[:n, n] = 0 and obs2 = obs1: the metastasis' chain after the seeding is the primary tumour's."""
    th = mod.log_theta.copy()
    th[:mod.n, mod.n] = 0.0
    return MetMHN(th, mod.obs1, mod.obs1)


def popcounts(n):
    return bits(n, np.arange(1 << n)).sum(axis=1)


def planes_of(got):
    return np.stack([getattr(got, name) for name in PLANES])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_host_definition_against_the_dense_oracle_of_every_genotype():
    from oracle import dense
    worst = 0.0
    for n in range(1, 7):
        mod = model(n, seed=n)
        got = mod.metastasis_distribution(backend="host")
        assert isinstance(got, MetastasisDistribution) and np.array_equal(got.codes, np.arange(1 << n))
        assert isinstance(got.summary, MetastasisSummary) and isinstance(got.summary, GenotypeSummary)
        whole = planes_of(got)
        assert whole.shape == (3, 1 << n) and np.array_equal(whole, host(n, n)[0])
        ref = np.exp([dense.patient_lp(mod.log_theta, mod.obs1, mod.obs2, r) for r in mt_rows(n, np.arange(1 << n))])
        worst = max(worst, rel(got.metastasis, ref))
    print(f"host M against exp(dense.patient_lp) of every genotype as a type-2 row, n = 1 .. 6: worst relative {worst:.2e}")
    assert worst <= 1e-12


def test_identities():
    for n, seed in ((3, 3), (7, 7), (10, 10)):
        mod = model(n, seed=seed)
        (Z, M, Cw), summary = host(n, seed)
        mass1 = mod._genodist_summary_host(mod._genodist_host()).mass[1]
        back = mod._landscape_host("observation")[0, 0]
        for v in (Z.sum(), M.sum(), summary.mass[0], summary.mass[1], back):
            assert abs(v - mass1) <= 1e-12 * mass1, (n, v, mass1)
        pc = popcounts(n)
        want = (pc * Z).sum()
        assert abs(Cw.sum() - want) <= 1e-12 * want
        assert (Cw >= 0).all() and (Cw <= pc * M * (1 + 1e-12)).all() and Cw[0] == 0.0
        assert (Z > 0).all() and (M > 0).all()
        th = mod.log_theta
        z0 = np.exp(th[n, n]) / (np.exp(np.diag(th)[:n]).sum() + np.exp(th[n, n]) + 1.0)
        assert abs(Z[0] - z0) <= 1e-12 * z0
        got = MetastasisDistribution(Z, M, Cw, np.arange(1 << n), summary)
        fe = got.founder_events
        assert fe[0] == 0.0 and (fe >= 0).all() and (fe <= pc * (1 + 1e-12)).all()
        for s, stratum in enumerate(("founder", "MT")):
            assert abs(summary.burden_pmf(stratum).sum() - 1.0) <= 1e-12
            assert np.array_equal(summary.frequencies(stratum), summary.pairs[s] / summary.mass[s])
        lo = summary.log_odds("MT")
        assert np.isnan(np.diag(lo)).all() and np.isfinite(lo[~np.eye(n, dtype=bool)]).all()
    for stratum in ("NM", "EM-PT", "unknown", "paired"):
        with pytest.raises(ValueError, match="stratum must be one of"):
            summary.frequencies(stratum)
    assert model_mod.GENOTYPE_STRATA == ("NM", "EM-PT", "unknown")
    plain = GenotypeSummary(summary.mass, summary.pairs, summary.burden)
    assert np.array_equal(plain.frequencies("EM-PT"), summary.frequencies("MT"))


def test_founder_events_against_the_order_posteriors():
    """C / M of every genotype against the type-2 rows' exact order posteriors on the host, which sum over the orders of one
    observation and share nothing with the lattice recursion: the sum of pre (P(event before the seeding | row)) and the
    mean of seed_pos, at 1e-12 absolute."""
    worst = 0.0
    for n in (3, 5):
        mod = model(n, seed=n)
        got = mod.metastasis_distribution(backend="host")
        post = mod.order_posteriors(mt_rows(n, np.arange(1 << n)), backend="host")
        worst = max(worst, np.abs(got.founder_events - np.nansum(post.pre, axis=1)).max(),
                    np.abs(got.founder_events - np.nansum(post.seed_pos * np.arange(n + 1), axis=1)).max())
        lp = np.log(got.metastasis)
        assert np.abs(post.log_evidence - lp).max() <= 1e-12 * np.abs(lp).max()
    print(f"founder_events against the host order posteriors of every type-2 row, n = 3, 5: worst absolute {worst:.2e}")
    assert worst <= 1e-12


def test_coinciding_chains_give_the_seeded_plane():
    for n in (4, 8):
        mod = coinciding(model(n, seed=20 + n))
        got = mod.metastasis_distribution(backend="host")
        seeded = mod._genodist_host()[1]
        err = rel(got.metastasis, seeded)
        print(f"M against genotype_distribution's seeded plane with coinciding chains, n = {n}: {err:.2e}")
        assert err <= 1e-12


def test_recursion_in_long_double():
    """Every state of one n = 10 model: the right-hand side of the recursion from the host's own fp64 rates and its values
    at the predecessors (and, for M and C, its founder value Z at the state), evaluated in np.longdouble, against the host's
    value at the state.  With G0 = Z / sigma, GM = M / kappam, GC = C / kappam:
    Z(y) = sigma (sum_b Z(y-b) / sigma(y-b) lambda_b(y-b)) / den0,  M(y) = kappam (Z(y) + sum_b M(y-b) / kappam(y-b) mu_b(y-b))
    / denm,  C the same with Z(y) |y|.  The fp64 evaluation rounds along a path of the non-negative sum-product: the G of a
    predecessor against the value it returned (1), its product (1), at most n + 1 additions of the numerator, at most n + 2
    additions of den, the division (1), kappa times G (1), and for C the product Z |y| (1): 2 n + 7, so the residual is
    within (2 n + 7) u relative; the long double side adds 2^-64 terms, below the 1 % allowed on top."""
    n, seed, ld = 10, 10, np.longdouble
    mod = model(n, seed=seed)
    th = mod._pt_log_theta
    P = host(n, seed)[0]
    sums = model_mod._subset_sums
    lam = [np.exp(th[j, j] + sums(np.where(np.arange(n) == j, 0.0, th[j, :n]))) for j in range(n)]
    mu = [lam[j] * np.exp(mod.log_theta[j, n]) for j in range(n)]
    sig = np.exp(th[n, n] + sums(th[n, :n]))
    kap0 = np.exp(sums(mod.obs1[:n]))
    kapm = np.exp(mod.obs2[n] + sums(mod.obs2[:n]))
    worst = 0.0
    for y in range(1, 1 << n):
        pc = bin(y).count("1")
        f0, fm, fc, L, Lm = ld(0), ld(P[0, y]), ld(P[0, y]) * pc, ld(0), ld(0)
        for b in range(n):
            if y >> b & 1:
                x = y ^ 1 << b
                f0 += ld(P[0, x]) / ld(sig[x]) * ld(lam[b][x])
                fm += ld(P[1, x]) / ld(kapm[x]) * ld(mu[b][x])
                fc += ld(P[2, x]) / ld(kapm[x]) * ld(mu[b][x])
            else:
                L += ld(lam[b][y])
                Lm += ld(mu[b][y])
        denm = Lm + ld(kapm[y])
        ref = (ld(sig[y]) * f0 / (L + ld(sig[y]) + ld(kap0[y])), ld(kapm[y]) * fm / denm, ld(kapm[y]) * fc / denm)
        for s in range(3):
            worst = max(worst, float(abs(ld(P[s, y]) - ref[s]) / ref[s]))
    print(f"residual of the recursion in long double, n = {n}: {worst / U:.2f} u, bar {2 * n + 7} u")
    assert worst <= 1.01 * (2 * n + 7) * U


def test_host_summary_against_brute_force_in_long_double():
    worst = 0.0
    for n in range(1, 9):
        whole, summary = host(n, n)
        assert summary.mass.shape == (2,) and summary.pairs.shape == (2, n, n) and summary.burden.shape == (2, n + 1)
        assert np.array_equal(summary.pairs, summary.pairs.transpose(0, 2, 1))
        ref = brute_summary(whole[:2])
        err = max(ld_rel(a, b) for a, b in zip((summary.mass, summary.pairs, summary.burden), ref))
        worst = max(worst, err / ((n + 19) * U))
    print(f"host summary against long-double brute force, n = 1 .. 8: worst error / ((n + 19) u) {worst:.3e}")
    assert worst <= 1.01


def check_dead_mutation(a, b, codes, small, j, bar):
    """a: the distribution with mutation j of rate 0, b: the one of the model without it."""
    holds = np.setdiff1d(a.codes, codes)
    keep = [i for i in range(a.summary.n_mut) if i != j]
    worst = 0.0
    for name in PLANES:
        assert np.isfinite(getattr(a, name)).all() and (getattr(a, name)[holds] == 0.0).all(), name
        worst = max(worst, rel(getattr(a, name)[codes], getattr(b, name)[small]) / bar)
    assert np.isnan(a.founder_events[holds]).all() and np.isfinite(a.founder_events[codes]).all()
    assert (a.summary.pairs[:, j, :] == 0.0).all() and (a.summary.pairs[:, :, j] == 0.0).all()
    assert (a.summary.burden[:, -1] == 0.0).all()
    worst = max(worst, rel(a.summary.pairs[np.ix_([0, 1], keep, keep)], b.summary.pairs) / bar,
                rel(a.summary.mass, b.summary.mass) / bar, rel(a.summary.burden[:, :-1], b.summary.burden) / bar)
    return worst


def check_dead_seeding(got):
    for name in PLANES:
        assert (getattr(got, name) == 0.0).all(), name
    assert np.isnan(got.founder_events).all()
    s = got.summary
    assert not s.mass.any() and not s.pairs.any() and not s.burden.any()
    assert np.isfinite(s.mass).all() and np.isfinite(s.pairs).all() and np.isfinite(s.burden).all()


def test_rates_of_zero():
    n, j = 6, 2
    dead, less, codes, small = without(model(n, seed=35), j)
    worst = check_dead_mutation(dead.metastasis_distribution(backend="host"), less.metastasis_distribution(backend="host"),
                                codes, small, j, 1e-12)
    print(f"a mutation of rate 0 against the model without it (host): worst error / 1e-12 {worst:.3e}")
    assert worst <= 1.0
    mod = model(n, seed=36)
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    check_dead_seeding(MetMHN(th, mod.obs1, mod.obs2).metastasis_distribution(backend="host"))


def fit_cohort(n=5):
    return np.vstack((mixed_cohort(n), mixed_cohort(n)[4:9], pt_fit_cohort(n)[-4:])).astype(np.int8)


def check_fit(fit, mod, dat, whole, summary, bar):
    """metastasis_fit's result and the summary's methods against the formulas written out from `whole` and `summary`."""
    n = mod.n
    typ = dat[:, -1]
    codes = dat[:, 1:2 * n:2].astype(np.int64) @ (1 << np.arange(n))
    own = np.isin(typ, (2, 3))
    assert own.any() and not own.all() and (typ == 2).any() and (typ == 3).any() and (typ == 4).any()
    assert np.array_equal(fit.codes, np.where(own, codes, -1))
    assert np.isnan(fit.prob[~own]).all() and np.isnan(fit.founder_events[~own]).all()
    ref = whole[1, codes] / summary.mass[1]
    worst = max(rel(fit.prob[own], ref[own]), rel(fit.founder_events[own], (whole[2, codes] / whole[1, codes])[own])) / bar
    p = summary.pairs[1] / summary.mass[1]
    acquired = np.diag(p) - np.diag(summary.pairs[0] / summary.mass[0])
    assert np.array_equal(summary.acquired(), acquired) and (acquired > 0).all() and (acquired < 1).all()
    events = float((np.arange(n + 1) * (summary.burden[0] / summary.mass[0])).sum())
    assert abs(summary.expected_founder_events() - events) <= 1e-15 * events and 0 < events < n
    res = summary.compare(dat)
    assert set(fit.residuals) == set(res) == {"EM-MT", "paired"} == set(fit.table)
    for stratum, ty in (("EM-MT", 2), ("paired", 3)):
        g = dat[typ == ty][:, 1:2 * n:2].astype(np.float64)
        rows = g.shape[0]
        want = (g.T @ g - rows * p) / np.sqrt(rows * p * (1 - p))
        assert np.array_equal(res[stratum], want) and np.isfinite(want).all()
        assert np.allclose(fit.residuals[stratum], want, rtol=1e-6, atol=0)
        uniq, observed, expected = fit.table[stratum]
        assert np.array_equal(uniq, np.unique(codes[typ == ty])) and observed.sum() == rows
        assert np.array_equal(observed, [(codes[typ == ty] == x).sum() for x in uniq])
        worst = max(worst, rel(expected, [rows * ref[typ == ty][codes[typ == ty] == x][0] for x in uniq]) / bar)
    return worst


def test_summary_methods_and_metastasis_fit_on_a_mixed_cohort():
    n = 5
    mod = model(n, seed=48)
    dat = fit_cohort(n)
    fit = ro.metastasis_fit(mod.log_theta, mod.obs1, mod.obs2, dat, backend="host")
    whole = mod._metdist_host()
    summary = mod._metdist_summary_host(whole)
    assert isinstance(fit.summary, MetastasisSummary) and summary_rel(fit.summary, summary) == 0.0
    worst = check_fit(fit, mod, dat, whole, summary, 1e-12)
    print(f"metastasis_fit against its formulas (host): worst error / 1e-12 {worst:.3e}")
    assert worst <= 1.0
    # sum_j acquired_j = E|MT| - E|founder|: the founder's mutations all stay
    gained = (np.arange(n + 1) * summary.burden_pmf("MT")).sum() - summary.expected_founder_events()
    assert abs(summary.acquired().sum() - gained) <= 1e-12
    with pytest.raises(ValueError, match=r"dat must have shape \(n_pat, 13\)"):
        summary.compare(dat[:, 1:])
    only = ro.metastasis_fit(mod.log_theta, mod.obs1, mod.obs2, dat[np.isin(dat[:, -1], (0, 1, 4))][:3], backend="host")
    assert np.isnan(only.prob).all() and (only.codes == -1).all() and only.table == {} and only.residuals == {}


def test_refusals(monkeypatch):
    no_library(monkeypatch)
    n = 5
    mod = model(n, seed=36)
    G = bits(n, [1, 10, 0])
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.metastasis_distribution(backend="cpu")
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.metastasis_distribution_at(G, backend="cpu")
    for bad in (G[0], G[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=rf"genotypes must have shape \[R, {n}\]"):
            mod.metastasis_distribution_at(bad)
    H = G.copy()
    H[1, 4] = 2
    for backend in ("device", "host"):
        with pytest.raises(ValueError, match=r"^row 1: ") as e1:
            mod.metastasis_distribution_at(H, backend=backend)
        with pytest.raises(ValueError) as e2:
            mod.seeding_landscape_at(H)
        assert str(e1.value) == str(e2.value)
    wide = model(25, seed=1)
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.metastasis_distribution(backend="host")
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.metastasis_distribution_at(np.zeros((1, 25), dtype=np.int8), backend="host")
    with pytest.raises(ValueError, match=rf"needs {24 << n} bytes, more than max_bytes = 767"):
        mod.metastasis_distribution(backend="host", max_bytes=(24 << n) - 1)
    with pytest.raises(ValueError, match=rf"needs {24 << 27} bytes, more than max_bytes = {2 ** 31}"):
        model(27, seed=1).metastasis_distribution()                    # the default: 2 GiB, n <= 26; before any library
    with pytest.raises(ValueError, match=rf"needs {24 << 31} bytes"):
        model(31, seed=1).metastasis_distribution(max_bytes=2 ** 34)
    whole = mod.metastasis_distribution(backend="host", max_bytes=24 << n)
    some = mod.metastasis_distribution_at(G, backend="host")
    assert some.codes.tolist() == [1, 10, 0]
    for name in PLANES:
        assert getattr(whole, name).shape == (1 << n,)
        assert np.array_equal(getattr(some, name), getattr(whole, name)[[1, 10, 0]])
    assert np.array_equal(some.founder_events, whole.founder_events[[1, 10, 0]])
    assert summary_rel(some.summary, whole.summary) == 0.0
    empty = mod.metastasis_distribution_at(np.zeros((0, n), dtype=np.int8), backend="host")
    assert empty.metastasis.shape == (0,) and empty.codes.shape == (0,) and summary_rel(empty.summary, whole.summary) == 0.0


# ------------------------------------------------------------------------------------------------------------------ GPU
def device(mod, G=None, **kw):
    from metmhn_amd.jx import engine
    G = np.zeros((0, mod.n), dtype=np.int8) if G is None else G
    return engine(mod.n).metastasis_distribution(mod.log_theta, mod.obs1, mod.obs2, G, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 3, C, C + 1, C + 3))
def test_device_against_the_host_definition(n):
    """One partial tile (n = 1, 3), exactly one tile (n = c), two tiles and one high-bit pull (c + 1), several levels
    (c + 3).  Bounds: module docstring."""
    seed = 40 + n
    mod = model(n, seed=seed)
    values, status, sums, whole = device(mod, summary=True, full=True)
    assert values.shape == (0, 3) and status.shape == (0,) and whole.shape == (3, 1 << n)
    assert sums[0].shape == (2,) and sums[1].shape == (2, n, n) and sums[2].shape == (2, n + 1)
    ref, ref_summary = host(n, seed)
    for s, name in enumerate(PLANES):
        note(f"device {name} against host, n = {n}", rel(whole[s], ref[s]) / bound(mod))
    note(f"device summary against host, n = {n}", summary_rel(sums, ref_summary) / summary_bound(mod))
    assert np.array_equal(sums[1], sums[1].transpose(0, 2, 1))
    assert (whole[2] <= popcounts(n) * whole[1] * (1 + 2 * bound(mod))).all() and (whole[2, 0] == 0.0)
    got = mod.metastasis_distribution()
    assert planes_of(got).tobytes() == whole.tobytes() and isinstance(got.summary, MetastasisSummary)
    for a, b in zip((got.summary.mass, got.summary.pairs, got.summary.burden), sums):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_device_against_the_engines_own_rows():
    """n = 14, 24 genotypes as rows of type 2 of one cohort: exp of the evaluation's log-probabilities against M, at the
    project's 1e-9 (relative)."""
    from metmhn_amd.engine import Engine
    n = 14
    mod = model(n, seed=70)
    G = (np.random.default_rng(71).random((24, n)) < 0.5).astype(np.int8)
    assert len(np.unique(G, axis=0)) == 24
    codes = G.astype(np.int64) @ (1 << np.arange(n))
    values, status, _, _ = device(mod, G, summary=False)
    assert (status == 0).all() and (values[:, :2] > 0).all()
    with Engine(n) as eng:
        eng.set_cohort(mt_rows(n, codes))
        lp = eng.patient_grads(mod.log_theta, mod.obs1, mod.obs2, with_grad=False)
    note("exp(lp) of the engine's rows of type 2 against M, over 1e-9", rel(np.exp(lp), values[:, 1]) / 1e-9)
    at = mod.metastasis_distribution_at(G)
    assert np.stack([getattr(at, name) for name in PLANES], axis=1).tobytes() == values.tobytes()
    assert np.array_equal(at.codes, codes)


@pytest.mark.gpu
def test_founder_events_against_the_device_order_posteriors():
    """n = c + 2: C / M against the sum of pre and the mean of seed_pos of the device's order posteriors of type-2 rows - a
    kernel per row over the row's own events, no line shared with the sweep - rows that hold all n mutations included, at
    1e-9 absolute."""
    n = C + 2
    mod = model(n, seed=72)
    G = (np.random.default_rng(73).random((20, n)) < 0.45).astype(np.int8)
    G[0], G[1], G[2, :], G[2, 3] = 1, 0, 1, 0
    codes = G.astype(np.int64) @ (1 << np.arange(n))
    at = mod.metastasis_distribution_at(G)
    post = mod.order_posteriors(mt_rows(n, codes))
    assert mod.posteriors_fallback_rows == 0
    assert at.founder_events[1] == 0.0
    note("founder_events against the device order posteriors' sum of pre, over 1e-9",
         np.abs(at.founder_events - np.nansum(post.pre, axis=1)).max() / 1e-9)
    note("founder_events against the device order posteriors' mean of seed_pos, over 1e-9",
         np.abs(at.founder_events - np.nansum(post.seed_pos * np.arange(n + 1), axis=1)).max() / 1e-9)
    note("log M against the order posteriors' log_evidence, over 1e-9",
         np.abs(np.log(at.metastasis) - post.log_evidence).max() / 1e-9)


@pytest.mark.gpu
def test_coinciding_chains_against_the_device_seeded_plane():
    """theta[:n, n] = 0 and obs2 = obs1 at n = c + 6: M against genotype_distribution's seeded plane (genodist.h), within
    the sum of the two files' bounds."""
    n = C + 6
    mod = coinciding(model(n, seed=74))
    got = mod.metastasis_distribution()
    seeded = mod.genotype_distribution().seeded
    note(f"M against the device's seeded plane with coinciding chains, n = {n}",
         rel(got.metastasis, seeded) / (bound(mod) + genodist_bound(mod)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (C + 6, 22))
def test_masses_against_the_other_sweeps(n):
    """sum Z, sum M and the summary's masses = genotype_distribution's mass[1] = the landscape's p_seed of the empty genotype
    until the observation, within the summed bounds."""
    from metmhn_amd.jx import engine
    mod = model(n, seed=50 + n)
    _, _, sums, whole = device(mod, full=True)
    _, _, gsums, _ = engine(n).genotype_distribution(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8))
    back, status, _ = engine(n).seeding_landscape(mod.log_theta, mod.obs1, np.zeros((1, n), dtype=np.int8), "observation")
    assert status.tolist() == [0]
    for what, v in (("sum Z", whole[0].sum()), ("sum M", whole[1].sum()), ("mass[0]", sums[0][0]), ("mass[1]", sums[0][1])):
        note(f"{what} against genotype_distribution's mass[1], n = {n}",
             rel(v, gsums[0][1]) / (summary_bound(mod) + genodist_summary_bound(mod)))
        note(f"{what} against the landscape's p_seed of the empty genotype, n = {n}",
             rel(v, back[0, 0]) / (summary_bound(mod) + landscape_bound(mod, clock=True)))
    want = (popcounts(n) * whole[0]).sum()
    note(f"sum C against sum |y| Z, n = {n}", rel(whole[2].sum(), want) / (2 * summary_bound(mod)))


@pytest.mark.gpu
def test_the_reduction_alone():
    """n = c + 3: the device summary against the long-double sums over the device's own `full` planes Z and M; only the
    reduction's term of the bound applies."""
    n = C + 3
    mod = model(n, seed=40 + n)
    _, _, sums, whole = device(mod, full=True)
    ref = brute_summary(whole[:2])
    note(f"the reduction alone, n = {n}", max(ld_rel(a, b) for a, b in zip(sums, ref)) / (1.01 * red(n) * U))


@pytest.mark.gpu
def test_same_bytes_whatever_the_queries():
    n = C + 1
    mod = model(n, seed=41 + C)
    check_same_bytes(lambda G, **kw: device(mod, G, **kw), 3, n, mod.metastasis_distribution_at)


@pytest.mark.gpu
def test_rates_of_zero_on_the_device():
    n, j = C + 1, C                                                    # the dead mutation is the high bit: whole tiles of zeros
    mod = model(n, seed=80)
    for jj in (j, 2):
        dead, less, codes, small = without(mod, jj)
        a, b = dead.metastasis_distribution(), less.metastasis_distribution(backend="host")
        note(f"a mutation of rate 0 (bit {jj}) on the device against the host model without it",
             check_dead_mutation(a, b, codes, small, jj, summary_bound(less)))
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    check_dead_seeding(MetMHN(th, mod.obs1, mod.obs2).metastasis_distribution())


@pytest.mark.gpu
def test_a_distribution_that_does_not_fit_is_refused_with_its_bytes():
    import re
    from metmhn_amd.engine import Engine
    n = 31
    mod = model(n, seed=3)
    row = bits(n, [1 | 1 << 30])
    with Engine(n, workspace_bytes=1 << 30) as small:
        before = small.counters()
        with pytest.raises(RuntimeError, match=r"31 mutations need (\d+) bytes.*limit is 1073741824 bytes") as err:
            small.metastasis_distribution(mod.log_theta, mod.obs1, mod.obs2, row)
        need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
        partials = 2 * 67 * 8 << (n - C)
        assert (24 << n) + (4 << (n - C)) + partials <= need <= (24 << n) + (4 << (n - C)) + partials + (1 << 16)
        with pytest.raises(RuntimeError, match=r"need (\d+) bytes") as err:
            small.metastasis_distribution(mod.log_theta, mod.obs1, mod.obs2, np.zeros((0, n), dtype=np.int8), summary=False)
        need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
        assert (24 << n) + (4 << (n - C)) <= need <= (24 << n) + (4 << (n - C)) + (1 << 16)
        assert small.counters() == before                              # nothing was launched or allocated through the engine
    with pytest.raises(ValueError, match=rf"needs {24 << n} bytes"):
        mod.metastasis_distribution()


@pytest.mark.gpu
def test_metastasis_fit_on_the_device():
    """metastasis_fit on the device against its formulas from the device's own planes and summary, and against the host."""
    m5 = model(5, seed=48)
    dat = fit_cohort(5)
    fit = ro.metastasis_fit(m5.log_theta, m5.obs1, m5.obs2, dat)
    whole = m5.metastasis_distribution()
    note("metastasis_fit on the device against its formulas, over 1e-12",
         check_fit(fit, m5, dat, planes_of(whole), whole.summary, 1e-12))
    ref = ro.metastasis_fit(m5.log_theta, m5.obs1, m5.obs2, dat, backend="host")
    own = np.isin(dat[:, -1], (2, 3))
    assert np.array_equal(fit.codes, ref.codes) and set(fit.table) == set(ref.table)
    note("metastasis_fit device against host: prob", rel(fit.prob[own], ref.prob[own]) / (bound(m5) + summary_bound(m5)))
    note("metastasis_fit device against host: founder_events",
         rel(fit.founder_events[own], ref.founder_events[own]) / (2 * bound(m5) + U))
    note("metastasis_fit device against host: summary", summary_rel(fit.summary, ref.summary) / summary_bound(m5))


@pytest.mark.gpu
def test_monte_carlo():
    """n = 6, 10^6 samples under a fixed key: the exact "MT" frequencies and burden against simulate_pairs' "EM-MT"
    frequencies and "mt" burden, at most 5 binomial standard errors over the entries with 0 < p < 1 (21 pair frequencies
    and 7 burden cells: a correct implementation crosses 5 standard errors on one of them with probability below 1e-4; with
    the key fixed the test is deterministic)."""
    from metmhn_amd.simulations import simulate_pairs
    n = 6
    mod = model(n, seed=90)
    summary = mod.metastasis_distribution().summary
    sim = simulate_pairs(mod.log_theta, mod.obs1, mod.obs2, 10 ** 6, original_key=5)
    rows = int(sim.n_class[1] + sim.n_class[2])
    assert rows > 10 ** 4
    exact = np.concatenate((summary.frequencies("MT")[np.triu_indices(n)], summary.burden_pmf("MT")))
    est = np.concatenate((sim.frequencies("EM-MT")[1::2, 1::2][np.triu_indices(n)], sim.burden_pmf("mt", "EM-MT")))
    inside = (exact > 0) & (exact < 1)
    assert inside.sum() >= 25 and np.isfinite(est).all()
    z = np.abs(est - exact)[inside] / np.sqrt(exact[inside] * (1 - exact[inside]) / rows)
    print(f"Monte Carlo, n = {n}, {rows} seeded samples, {int(inside.sum())} entries: worst deviation {z.max():.3f} standard errors")
    assert z.max() <= 5.0
    mass = abs(rows / 10 ** 6 - summary.mass[1]) / np.sqrt(summary.mass[1] * (1 - summary.mass[1]) / 10 ** 6)
    print(f"share of seeded samples against mass[1]: {mass:.3f} standard errors")
