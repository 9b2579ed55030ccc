"""The exact PT x MT co-occurrence and joint burden tables of a seeded pair: MetMHN.cross_distribution / paired_summary,
CrossSummary, PairedSummary, mmhn_cross_table, regularized_optimization.paired_fit; metmhn_amd/csrc/cross.h.

CPU: the host definition against exp(oracle.dense.patient_lp) of the paired rows of unknown order summed over every pair
of genotypes (1e-12 relative), against the sums over all queries of the host partner distribution, its identities, the
recursion in long double, a mutation of rate 0, the Python layer against its formulas, the refusals.

GPU: the device against the host definition, against the device's one-tumour sweeps and its partner distributions (which
share no backward code with the new kernels), against simulate_pairs, the same bytes under a workspace limit that forces
blocks to be swept again and with or without the burden, a mutation of rate 0, paired_fit.

The bound of the device against the host: lattice_common's chain_bound with the pair's eps (pair_eps).  One step of a
chain costs, both sides together, 4 n + 16 roundings (a product, at most n + 1 additions of the numerator, at most n + 2
additions of den, the division, on either side).  The path behind a term Z(z) a(z) b(z): G0's chain to z (|z| + 1 steps),
the two value functions from z to the full genotype (n - |z| + 1 steps each), the product (one step): 2 n - |z| + 4 <=
2 n + 4 steps; on the way the clock times the feature.  Every term agrees within relative
    bound(n) = (2 n + 4) (4 eps + (4 n + 16) u) + 2 eps + 8 u
and the tables add the reductions - on the device 4 states a thread, 8 levels of the block sum, ceil(tiles / 256) + 8 across
the tiles: below lattice_common.red -:
    table_bound(n) = bound(n) + (RED(n) + n + 19) u.
The device's one-tumour summaries against their host definitions stay within test_metastasis_distribution.py's n + 2 steps
of 4 n + 16 with the reductions (sweep_summary_bound); the device's partner summaries within table_bound, which is
test_partner_distribution.py's expression for them.

The bars of the CPU identities: lattice_common.identity_bar, two host evaluations of one quantity, and the additions of
the sums - 11 u for a NumPy sum of at most 64 terms, so 11 u for a table entry, 22 u for the double sum over the queries and
the partners of the partner distributions.

Measured, CPU: host against the dense oracle 3.1e-15 relative at the worst (n = 1 .. 4); against the sums of the host
partner distributions 0.017 of the bar at the worst (n = 1); the identities 0.011 of the bar at the worst (3.8 u of 572 u at
n = 6); the recursion's residual in long double 3.6 u of 20 u, the fold 3.9 u of 21 u; a mutation of rate 0 2.8e-4 of the
1e-12 bar.
Measured on an MI355X, worst error / bound per test: device against host 1.8e-3 (n = 1; 8.7e-4 at n = c + 3), without the
burden 6.8e-4 (n = 4); marginals and mass against the device's one-tumour sweeps 2.5e-5 (n = c + 6); cross against the
device's partner distributions 1.8e-4; Monte Carlo 2.53 standard errors at the worst of 36 entries; a mutation of rate 0
5.8e-4; paired_fit device against host 1.8e-4 (frequencies), 1.4e-4 (expected counts), 5.1e-5 (residuals).
The siblings' reduction-alone test (the device's tables against long-double sums over planes copied out) is not built: the
ABI call has no output of the planes, which a slot's next block overwrites.
"""
import re

import numpy as np
import pytest

from metmhn_amd import regularized_optimization as ro
from metmhn_amd.results import CrossSummary, GenotypeSummary, MetastasisSummary, PairedSummary
from lattice_common import (C, U, bits, chain_bound, fit_cohort, host_once, identity_bar, ld_rel, no_library, note, pair_eps, rel,
                            without)
from order_common import model, paired

FIELDS = ("mass", "pt", "mt", "cross", "burden", "gene_burden")
GENES = ("mass", "pt", "mt", "cross")


def table_bound(mod):
    """An entry of the device's tables against the host definition (module docstring)."""
    return chain_bound(pair_eps(mod), 2 * mod.n + 4, 4 * mod.n + 16, out=True, summed=mod.n)


def sweep_summary_bound(mod):
    """A summary entry of a one-tumour sweep on the device against its host definition, with the pair's eps."""
    return chain_bound(pair_eps(mod), mod.n + 2, 4 * mod.n + 16, out=True, summed=mod.n)


@host_once
def host(n, seed):
    """_cross_host of order_common.model(n, seed) with its planes."""
    return model(n, seed=seed)._cross_host(planes=True)


def worst_rel(got, ref, names=FIELDS):
    """Worst relative difference of the named arrays of two results (CrossSummary, a namespace or a tuple in FIELDS' order)."""
    as_tuple = lambda r: r if isinstance(r, tuple) else tuple(getattr(r, k) for k in FIELDS)
    a, b = as_tuple(got), as_tuple(ref)
    return max(rel(a[FIELDS.index(k)], b[FIELDS.index(k)]) for k in names)


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_host_definition_against_the_dense_oracle():
    """cross and burden against exp(dense.patient_lp) of the paired row (x, y) with order code 0 (unknown order: the oracle
    adds both order terms), summed over EVERY pair of genotypes with the features written out, n = 1 .. 4; mass, pt, mt and
    gene_burden on the way.  Bar 1e-12 relative."""
    from oracle import dense
    worst = 0.0
    for n in range(1, 5):
        mod = model(n, seed=n)
        size = 1 << n
        ev = lambda v: [j for j in range(n) if v >> j & 1]
        J = np.array([[np.exp(dense.patient_lp(mod.log_theta, mod.obs1, mod.obs2, paired(n, ev(x), ev(y), 0)))
                       for y in range(size)] for x in range(size)])
        g = bits(n, np.arange(size)).astype(np.float64)                      # [2^n, n]
        h = (g.sum(axis=1)[:, None] == np.arange(n + 1)[None, :]).astype(np.float64)     # [2^n, n + 1]
        got = host(n, n)
        ref = (J.sum(), g.T @ J.sum(axis=1), g.T @ J.sum(axis=0), g.T @ J @ g, h.T @ J @ h, np.stack((g.T @ J @ h, g.T @ J.T @ h)))
        worst = max(worst, worst_rel(got, ref))
    print(f"host tables against the sums of exp(dense.patient_lp) over every pair, n = 1 .. 4: worst relative {worst:.2e}")
    assert worst <= 1e-12


def test_host_tables_against_the_host_partner_distributions():
    """n = 1 .. 6: every table against the sums over all 2^n queries x of the host partner distribution J_x(y) (given "PT")
    with the features written out, under identity_bar(n, 33): two paths, 11 u for the table's own sum over the founders and
    22 u for the double sum over queries and partners (module docstring)."""
    worst = 0.0
    for n in range(1, 7):
        mod = model(n, seed=n)
        size = 1 << n
        rates = mod._partner_rates()
        J = np.stack([mod._partner_host(q, "PT", rates)[1] for q in range(size)])        # [x, y]
        g = bits(n, np.arange(size)).astype(np.float64)
        h = (g.sum(axis=1)[:, None] == np.arange(n + 1)[None, :]).astype(np.float64)
        over = lambda w, v: float((w[:, None] * J * v[None, :]).sum(axis=1).sum())      # pairwise over y, then over x
        one = np.ones(size)
        ref = (over(one, one), np.array([over(g[:, i], one) for i in range(n)]), np.array([over(one, g[:, j]) for j in range(n)]),
               np.array([[over(g[:, i], g[:, j]) for j in range(n)] for i in range(n)]),
               np.array([[over(h[:, k], h[:, l]) for l in range(n + 1)] for k in range(n + 1)]),
               np.stack((np.array([[over(g[:, i], h[:, l]) for l in range(n + 1)] for i in range(n)]),
                         np.array([[over(h[:, k], g[:, j]) for k in range(n + 1)] for j in range(n)]))))
        err = worst_rel(host(n, n), ref) / (identity_bar(n, 33) * U)
        print(f"host tables against the sums of the host partner distributions, n = {n}: error / bar {err:.3f} (bar {identity_bar(n, 33)} u)")
        assert err <= 1.0
        worst = max(worst, err)
    print(f"host tables against the sums of the host partner distributions, n = 1 .. 6: worst error / bar {worst:.3f}")


def test_identities():
    """n = 1 .. 6, two host evaluations of one quantity under identity_bar(n, 22) (two sums of at most 64 terms): pt and mt
    against the diagonals of pairs[1] of the host genotype / metastasis summaries, the row and column sums of burden against
    their burden[1], sum burden = mass = their mass[1], gene_burden summed over the burden against pt and mt; and
    founder pairs <= cross <= min(pt_i, mt_j) up to the same bar."""
    worst = 0.0
    for n in range(1, 7):
        mod = model(n, seed=n)
        c = host(n, n)
        gs = mod.genotype_distribution(backend="host").summary
        ms = mod.metastasis_distribution(backend="host").summary
        bar = identity_bar(n, 22) * U
        err = max(rel(c.pt, np.diag(gs.pairs[1])), rel(c.mt, np.diag(ms.pairs[1])),
                  rel(c.burden.sum(axis=1), gs.burden[1]), rel(c.burden.sum(axis=0), ms.burden[1]),
                  rel(c.burden.sum(), c.mass), rel(c.mass, gs.mass[1]), rel(c.mass, ms.mass[1]), rel(c.mass, ms.mass[0]),
                  rel(c.gene_burden[0].sum(axis=1), c.pt), rel(c.gene_burden[1].sum(axis=1), c.mt))
        assert (ms.pairs[0] <= c.cross * (1 + bar)).all(), "the founder's mutations stay in both tumours"
        assert (c.cross <= np.minimum(c.pt[:, None], c.mt[None, :]) * (1 + bar)).all()
        assert (c.cross > 0).all() and (c.burden >= 0).all() and c.burden[0, 0] > 0
        # sum_i gene_burden[0][i][l] = E[|PT|; |MT| = l] = sum_k k burden[k][l]
        err = max(err, rel(c.gene_burden[0].sum(axis=0), np.arange(n + 1) @ c.burden),
                  rel(c.gene_burden[1].sum(axis=0), c.burden @ np.arange(n + 1)))
        print(f"identities of the host definition, n = {n}: {err / U:.1f} u, bar {identity_bar(n, 22)} u")
        assert err <= bar
        worst = max(worst, err / bar)
    print(f"identities of the host definition, n = 1 .. 6: worst error / bar {worst:.3f}")


def test_recursion_in_long_double():
    """n = 8, both chains, every feature and state: the right-hand side of the recursion from the host's own fp64 rates and
    its own values at the successors in np.longdouble against the value returned.  The fp64 evaluation rounds a product per
    move (1), at most n + 1 additions of the numerator, at most n + 1 of den and the division (1): 2 n + 4 u.  The fold: the
    tables against long-double sums of Z a_f b_g over the host's own planes: two products and a NumPy pairwise sum of 256
    terms (blocks of 128 in eight accumulators, 15 additions each and 3 to join them, one level above): 2 + 19 = 21 u.
    The long double side adds 2^-64 terms, below the 1 % allowed on top."""
    n, seed, ld = 8, 8, np.longdouble
    mod = model(n, seed=seed)
    R = mod._lattice_host_chains()
    c = host(n, seed)
    size = 1 << n
    phi = np.stack([(R.idx >> i & 1) for i in range(n)] + [(R.level == k) for k in range(n + 1)]).astype(ld)
    worst = 0.0
    for a, rate, kap in ((c.A, R.lam, R.kap1), (c.B, R.mu, R.kapm)):
        num, L = kap.astype(ld) * phi, np.zeros(size, dtype=ld)
        for j in range(n):
            free = np.flatnonzero((R.idx >> j & 1) == 0)
            num[:, free] += rate[j][free].astype(ld) * a[:, free | 1 << j].astype(ld)
            L[free] += rate[j][free].astype(ld)
        worst = max(worst, ld_rel(a, num / (L + kap.astype(ld))))
    za = c.Z.astype(ld) * c.A.astype(ld)
    M = np.array([[(za[f] * c.B[g].astype(ld)).sum() for g in range(2 * n + 1)] for f in range(2 * n + 1)])
    fold = max(ld_rel(c.cross, M[:n, :n]), ld_rel(c.burden, M[n:, n:]), ld_rel(c.gene_burden[0], M[:n, n:]),
               ld_rel(c.gene_burden[1], M[n:, :n].T), ld_rel(c.pt, za[:n].sum(axis=1)), ld_rel(np.float64(c.mass), c.Z.astype(ld).sum()))
    print(f"residual of the recursion in long double, n = {n}: {worst / U:.2f} u, bar {2 * n + 4} u; the fold {fold / U:.2f} u, bar 21 u")
    assert worst <= 1.01 * (2 * n + 4) * U and fold <= 1.01 * 21 * U


def check_dead_mutation(a, b, n, j, bar):
    """a: the tables of the model with mutation j of rate 0, b: of the model without it.  Exact zeros exactly; the rest
    over `bar`."""
    keep = [i for i in range(n) if i != j]
    assert a.pt[j] == 0.0 and (a.cross[j, :] == 0.0).all() and (a.gene_burden[0, j, :] == 0.0).all()
    assert a.mt[j] == 0.0 and (a.cross[:, j] == 0.0).all() and (a.gene_burden[1, j, :] == 0.0).all()    # mu_j = lambda_j exp(theta_jn) = 0
    assert (a.burden[n, :] == 0.0).all() and (a.burden[:, n] == 0.0).all() and (a.gene_burden[:, :, n] == 0.0).all()
    return max(rel(a.mass, b.mass), rel(a.pt[keep], b.pt), rel(a.mt[keep], b.mt), rel(a.cross[np.ix_(keep, keep)], b.cross),
               rel(a.burden[:n, :n], b.burden), rel(a.gene_burden[:, keep, :n], b.gene_burden)) / bar


def test_a_mutation_of_rate_zero():
    n, j = 6, 2
    dead, less, _, _ = without(model(n, seed=35), j)
    worst = check_dead_mutation(dead.cross_distribution(backend="host"), less.cross_distribution(backend="host"), n, j, 1e-12)
    print(f"a mutation of rate 0 against the model without it (host): worst error / 1e-12 {worst:.3e}")
    assert worst <= 1.0


def check_python_layer(mod, dat, backend):
    """CrossSummary's and PairedSummary's methods, compare and paired_fit against their formulas written out in NumPy."""
    n = mod.n
    c = mod.cross_distribution(backend=backend)
    assert isinstance(c, CrossSummary) and repr(c).startswith(f"CrossSummary(n_mut={n}, mass=")
    d = np.diag(c.cross)
    assert np.array_equal(c.shared(), d / c.mass) and np.array_equal(c.in_primary_given_metastasis(), d / c.mt)
    assert np.array_equal(c.in_metastasis_given_primary(), d / c.pt) and c.expected_shared() == np.trace(c.cross) / c.mass
    assert np.array_equal(c.burden_pmf(), c.burden / c.mass) and abs(c.burden_pmf().sum() - 1.0) <= 1e-12
    f, p, q = c.cross / c.mass, c.pt / c.mass, c.mt / c.mass
    want = np.log(f * (1 - p[:, None] - q[None, :] + f) / ((p[:, None] - f) * (q[None, :] - f)))
    assert np.isfinite(want).all() and rel(c.log_odds(), want) <= 1e-12
    assert (np.diag(c.log_odds()) > 0).all()                 # a mutation in one tumour makes it likelier in the other
    s = mod.paired_summary(backend=backend)
    assert isinstance(s, PairedSummary) and isinstance(s.primary, GenotypeSummary) and isinstance(s.metastasis, MetastasisSummary)
    assert worst_rel(s.cross, c) == 0.0 and s.mass == c.mass and s.n_mut == n
    F = s.frequencies("paired")
    assert F.shape == (2 * n, 2 * n) and np.array_equal(F, F.T) and np.array_equal(F, s.frequencies())
    assert np.array_equal(F[0::2, 0::2], s.primary.pairs[1] / s.primary.mass[1])
    assert np.array_equal(F[1::2, 1::2], s.metastasis.pairs[1] / s.metastasis.mass[1])
    assert np.array_equal(F[0::2, 1::2], f) and np.array_equal(F[np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2)], c.shared())
    m = np.diag(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = np.log(F * (1 - m[:, None] - m[None, :] + F) / ((m[:, None] - F) * (m[None, :] - F)))
    off = ~np.eye(2 * n, dtype=bool)
    assert np.isnan(np.diag(s.log_odds("paired"))).all() and rel(s.log_odds("paired")[off], lo[off]) <= 1e-12
    for stratum in ("EM-MT", "NM", "unknown"):
        with pytest.raises(ValueError, match="stratum must be one of"):
            s.frequencies(stratum)
    with pytest.raises(ValueError, match=rf"dat must have shape \(n_pat, {2 * n + 3}\)"):
        s.compare(dat[:, 1:])
    rows = dat[dat[:, -1] == 3]
    R = len(rows)
    assert R >= 10
    G = rows[:, :2 * n].astype(np.float64)
    want = (G.T @ G - R * F) / np.sqrt(R * F * (1 - F))
    res = s.compare(dat)
    assert set(res) == {"paired"} and np.isfinite(want).all() and np.array_equal(res["paired"], want)
    assert s.compare(dat[dat[:, -1] != 3]) == {}
    fit = ro.paired_fit(mod.log_theta, mod.obs1, mod.obs2, dat, backend=backend)
    pt, mt = rows[:, 0:2 * n:2].astype(bool), rows[:, 1:2 * n:2].astype(bool)
    assert fit.rows == R and np.array_equal(fit.residuals["paired"], want) and set(fit.residuals) == {"paired"}
    assert np.array_equal(fit.summary.frequencies(), F)
    for (obs, exp), o, e in ((fit.shared, pt & mt, c.shared()), (fit.pt_private, pt & ~mt, p - c.shared()),
                             (fit.mt_private, mt & ~pt, q - c.shared())):
        assert np.array_equal(obs, o.sum(axis=0)) and np.array_equal(exp, R * e) and (exp > 0).all()
    k = np.arange(n + 1)
    pmf = c.burden / c.mass
    for key, o, e in (("pt", pt.sum(axis=1).mean(), k @ pmf.sum(axis=1)), ("mt", mt.sum(axis=1).mean(), k @ pmf.sum(axis=0)),
                      ("shared", (pt & mt).sum(axis=1).mean(), np.trace(c.cross) / c.mass)):
        assert fit.burden[key][0] == o and abs(fit.burden[key][1] - e) <= 1e-12 * e
    assert abs(fit.burden["pt"][1] - p.sum()) <= 1e-12 * n       # E|PT| = sum_i P(PT holds i)
    assert abs(fit.burden["mt"][1] - q.sum()) <= 1e-12 * n
    none = ro.paired_fit(mod.log_theta, mod.obs1, mod.obs2, dat[dat[:, -1] != 3], backend=backend)
    assert none.rows == 0 and none.residuals == {} and np.isnan(none.burden["pt"][0]) and not none.shared[0].any()
    return fit


def test_python_layer_on_a_mixed_cohort():
    check_python_layer(model(5, seed=48), fit_cohort(5), "host")
    mod = model(4, seed=3)
    plain = mod.cross_distribution(backend="host", burden=False)
    whole = mod.cross_distribution(backend="host")
    assert np.isnan(plain.burden).all() and np.isnan(plain.gene_burden).all() and np.isnan(plain.burden_pmf()).all()
    assert worst_rel(plain, whole, GENES) == 0.0


def test_refusals(monkeypatch):
    from metmhn_amd.engine import Engine

    no_library(monkeypatch)
    mod = model(5, seed=36)
    for call in (mod.cross_distribution, mod.paired_summary):
        with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
            call(backend="cpu")
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        ro.paired_fit(mod.log_theta, mod.obs1, mod.obs2, fit_cohort(5), backend="cpu")
    wide = model(25, seed=1)
    for call in (wide.cross_distribution, wide.paired_summary):
        with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
            call(backend="host")
    eng = Engine.__new__(Engine)                                       # no device: only the argument checks are reached
    eng.n, eng.N, eng.h, eng.dtype = 5, 6, None, "f32"
    with pytest.raises(ValueError, match="the cross table needs an fp64 engine"):
        eng.cross_table(mod.log_theta, mod.obs1, mod.obs2)
    eng.dtype = "f64"
    with pytest.raises(ValueError, match=r"log_theta must have shape \(6, 6\)"):
        eng.cross_table(mod.log_theta[:5, :5], mod.obs1, mod.obs2)


# ------------------------------------------------------------------------------------------------------------------ GPU
def device(mod, burden=True, eng=None):
    from metmhn_amd.jx import engine
    return (eng or engine(mod.n)).cross_table(mod.log_theta, mod.obs1, mod.obs2, burden=burden)


def same_bytes(a, b, names=FIELDS):
    return all(np.asarray(a[FIELDS.index(k)]).tobytes() == np.asarray(b[FIELDS.index(k)]).tobytes() for k in names)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 3, C, C + 1, C + 3))
def test_device_against_the_host_definition(n):
    """One partial tile (n = 1, 3), exactly one tile (n = c), two tiles and one cross-tile pull (c + 1), eight tiles and
    four levels (c + 3); 2 n + 1 is no multiple of 4, so the last block is padded.  Bound: module docstring."""
    mod = model(n, seed=40 + n)
    got = device(mod)
    assert all(np.isfinite(np.asarray(a)).all() for a in got)
    note(f"device tables against host, n = {n}", worst_rel(got, host(n, 40 + n)) / table_bound(mod))
    c = mod.cross_distribution()
    assert same_bytes(tuple(getattr(c, k) for k in FIELDS), got)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (4, 8))
def test_device_without_the_burden_a_full_last_block(n):
    """burden=False at n = 4 and 8: n features, every block full; the gene outputs against the host, the burden outputs NaN."""
    mod = model(n, seed=40 + n)
    got = device(mod, burden=False)
    assert np.isnan(got[4]).all() and np.isnan(got[5]).all()
    note(f"device gene tables without the burden against host, n = {n}", worst_rel(got, host(n, 40 + n), GENES) / table_bound(mod))


@pytest.mark.gpu
def test_marginals_against_the_devices_one_tumour_sweeps():
    """n = c + 6: mass, pt, mt, the row and column sums of burden against the device's own genotype_distribution_at /
    metastasis_distribution_at summaries, which share no backward code with the new kernels; the bar is the sum of the two
    bounds (and n + 19 u for the sums of burden formed here)."""
    n = C + 6
    mod = model(n, seed=74)
    mass, pt, mt, cross, burden, gb = device(mod)
    none = np.zeros((0, n), dtype=np.int8)
    gs, ms = mod.genotype_distribution_at(none).summary, mod.metastasis_distribution_at(none).summary
    bar = table_bound(mod) + sweep_summary_bound(mod) + (n + 19) * U
    note(f"marginals and mass against the device's one-tumour sweeps, n = {n}",
         max(rel(mass, gs.mass[1]), rel(mass, ms.mass[1]), rel(mass, ms.mass[0]), rel(pt, np.diag(gs.pairs[1])),
             rel(mt, np.diag(ms.pairs[1])), rel(burden.sum(axis=1), gs.burden[1]), rel(burden.sum(axis=0), ms.burden[1]),
             rel(gb[0].sum(axis=1), np.diag(gs.pairs[1])), rel(gb[1].sum(axis=1), np.diag(ms.pairs[1]))) / bar)
    assert (ms.pairs[0] <= cross * (1 + bar)).all() and (cross <= np.minimum(pt[:, None], mt[None, :]) * (1 + bar)).all()


@pytest.mark.gpu
def test_cross_against_the_devices_partner_distributions():
    """n = 5: cross[i, j] against sum_x x_i P(PT = x seeded, MT holds j) from partner_distributions of all 2^n queries on the
    device; the bar is the two summary bounds and 11 u for the sum over the 32 queries."""
    n = 5
    mod = model(n, seed=45)
    G = bits(n, np.arange(1 << n))
    rows = mod.partner_distributions(G, "PT")
    marg = np.array([np.diag(s.pairs[1]) for s in rows.summaries])                   # [x, j]
    ref = (G.astype(np.float64)[:, :, None] * marg[:, None, :]).sum(axis=0)
    mass, pt, mt, cross, _, _ = device(mod)
    bar = 2 * table_bound(mod) + 11 * U
    note(f"cross against the device's partner distributions, n = {n}",
         max(rel(cross, ref), rel(mt, marg.sum(axis=0)), rel(mass, rows.mass.sum()), rel(pt, G.astype(np.float64).T @ rows.mass)) / bar)


@pytest.mark.gpu
def test_monte_carlo():
    """n = 6, 10^6 samples under a fixed key, the seeded classes summed: the n x n entries of the PT x MT block of
    simulate_pairs' "paired" frequencies against cross / mass, at most 5 binomial standard errors - the bar
    test_metastasis_distribution.py uses for the same sampler; with the key fixed the test is deterministic."""
    from metmhn_amd.simulations import simulate_pairs
    n = 6
    mod = model(n, seed=90)
    c = mod.cross_distribution()
    sim = simulate_pairs(mod.log_theta, mod.obs1, mod.obs2, 10 ** 6, original_key=5)
    rows = int(sim.n_class[1] + sim.n_class[2])
    assert rows > 10 ** 4
    exact, est = c.cross / c.mass, sim.frequencies("paired")[0::2, 1::2]
    assert ((exact > 0) & (exact < 1)).all() and np.isfinite(est).all()
    z = np.abs(est - exact) / np.sqrt(exact * (1 - exact) / rows)
    print(f"Monte Carlo, n = {n}, {rows} seeded samples, {n * n} cross entries: worst deviation {z.max():.3f} standard errors")
    assert z.max() <= 5.0
    pmf = c.burden_pmf().sum(axis=1)
    zb = np.abs(sim.burden_pmf("pt", "paired") - pmf) / np.sqrt(pmf * (1 - pmf) / rows)
    print(f"|PT| of the seeded samples against the row sums of burden: worst deviation {zb.max():.3f} standard errors")


@pytest.mark.gpu
def test_same_bytes_under_a_workspace_limit():
    """n = c + 6 (41 planes of 512 KiB to hold every block): the bytes of the unlimited call under the 9-plane minimum
    (every PT block swept again per MT block) and under a limit of 17 planes (two blocks held, one slot shared), one byte
    below the minimum refused as a whole naming the minimum's bytes, and two calls in a row with another model in between."""
    from metmhn_amd.engine import Engine
    n = C + 6
    mod, other = model(n, seed=74), model(n, seed=75)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    roomy = device(mod)
    device(other)
    assert same_bytes(device(mod), roomy)
    with Engine(n, workspace_bytes=1 << 20) as tiny:
        with pytest.raises(RuntimeError, match=rf"cross table: {n} mutations need (\d+) bytes of workspace \(72 B x 2\^n_mut.*"
                                               r"limit is 1048576 bytes; there is no partial table") as err:
            tiny.cross_table(*args)
    need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
    assert (72 << n) <= need <= (72 << n) + (1 << 16) + (25 * 8 << (n - C)) + 8 * (36 * 36 + 73)
    for limit in (need, need + (8 * 8 << n) + 5):
        assert need <= limit < need + (32 * 8 << n)                      # between the minimum and the 41 planes of all blocks
        with Engine(n, workspace_bytes=limit) as snug:
            assert same_bytes(snug.cross_table(*args), roomy), limit
            assert same_bytes(snug.cross_table(*args, burden=False), roomy, GENES), limit
    with Engine(n, workspace_bytes=need - 1) as small:
        before = small.counters()
        for kw in ({}, {"burden": False}):
            with pytest.raises(RuntimeError, match=rf"need {need} bytes.*limit is {need - 1} bytes; there is no partial table"):
                small.cross_table(*args, **kw)
        assert small.counters() == before                              # nothing was launched or allocated through the engine


@pytest.mark.gpu
@pytest.mark.parametrize("n", (3, C + 1))
def test_without_the_burden_the_same_gene_bytes(n):
    mod = model(n, seed=40 + n)
    whole, plain = device(mod), device(mod, burden=False)
    assert same_bytes(plain, whole, GENES) and np.isnan(plain[4]).all() and np.isnan(plain[5]).all()
    assert same_bytes(device(mod), whole)


@pytest.mark.gpu
def test_a_mutation_of_rate_zero_on_the_device():
    """n = c + 1, the dead mutation the high bit (whole tiles of zeros) and a low one, under the device-against-host bound
    against the HOST model without it; exact zeros are met exactly."""
    n = C + 1
    mod = model(n, seed=80)
    for j in (C, 2):
        dead, less, _, _ = without(mod, j)
        note(f"a mutation of rate 0 (bit {j}) on the device against the host model without it",
             check_dead_mutation(dead.cross_distribution(), less.cross_distribution(backend="host"), n, j, table_bound(less)))


@pytest.mark.gpu
def test_paired_fit_on_the_device():
    """paired_fit on the device against its formulas from the device's own tables, and against the host: the frequencies
    within the summary bounds; a private count's expectation rows (p - s) within the bounds of p and s over p + s; a
    residual (obs - R p) / sqrt(R p (1 - p)) moves by at most (sqrt(R p / (1 - p)) + |r|) 2 d (1 + d') for a relative
    change d of p, d' = p / (1 - p) d covering the denominator's 1 - p."""
    m5 = model(5, seed=48)
    dat = fit_cohort(5)
    fit = check_python_layer(m5, dat, "device")
    ref = ro.paired_fit(m5.log_theta, m5.obs1, m5.obs2, dat, backend="host")
    d = max(table_bound(m5), sweep_summary_bound(m5)) * 2 + 2 * U            # a frequency: a sum over its mass
    F, Fr = fit.summary.frequencies(), ref.summary.frequencies()
    note("paired_fit device against host: frequencies", rel(F, Fr) / d)
    worst = 0.0
    for name in ("shared", "pt_private", "mt_private"):
        (o, e), (o2, e2) = getattr(fit, name), getattr(ref, name)
        assert np.array_equal(o, o2)
        scale = fit.rows * (np.diag(Fr)[0::2] if name == "pt_private" else np.diag(Fr)[1::2]) + ref.shared[1]
        worst = max(worst, float(np.max(np.abs(e - e2) / (scale if name != "shared" else e2))) / d)
    note("paired_fit device against host: expected counts", worst)
    r, r2 = fit.residuals["paired"], ref.residuals["paired"]
    allowed = (np.sqrt(fit.rows * Fr / (1 - Fr)) + np.abs(r2)) * 2 * d * (1 + Fr / (1 - Fr) * d)
    note("paired_fit device against host: residuals", float(np.max(np.abs(r - r2) / allowed)))
    for key in ("pt", "mt", "shared"):
        assert fit.burden[key][0] == ref.burden[key][0]
        note(f"paired_fit device against host: expected {key} burden", rel(fit.burden[key][1], ref.burden[key][1]) / (d + (5 + 19) * U))
