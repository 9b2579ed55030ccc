"""The genotype distribution of one tumour given the other: for a primary tumour observed seeded with genotype x the joint
probability with every genotype of the metastasis and with every founder (given "PT"), for a metastasis observed with y the
same with every genotype of the primary tumour (given "MT") - MetMHN.partner_distribution / partner_distributions,
PartnerDistribution, PartnerSummary, mmhn_partner_distributions, regularized_optimization.partner_forecast;
metmhn_amd/csrc/partner.h.

CPU: the host definition's J against exp(oracle.dense.patient_lp) of the paired row with unknown order (1e-12 relative),
its identities, the recursion in long double, a mutation of rate 0, the Python layer against its formulas, the refusals.

GPU: the device against the host definition, against the engine's own paired rows (which share no code with the sweep),
against the device's one-tumour sweeps, the reduction alone, the bytes whatever the other rows, a mutation of rate 0.

The bound of the device against the host: lattice_common's chain_bound with the pair's eps (pair_eps).  One step of a
chain, on one side: the numerator takes a product and at most n + 1 additions (n pulls and the source), the den at most
n + 2 additions, the division: (2 n + 8) u, both sides 4 n + 16 a step.  The path behind J_q(y) through a founder z: G0's
chain to z (|z| + 1 states), B's chain from z to q (|q| - |z| + 1 states), the product sigma G0 B (one step: a rate and two
products), the partner's chain from z to y (|y| - |z| + 1 states): |q| + |y| - |z| + 4 steps, at most 2 n + 4 (z empty, q and y
full; the issue's 3 n + 4 counts |z| three times instead of taking it off twice); on the way out the clock times G.  Every
value of both planes agrees within relative
    bound(n) = (2 n + 4) (4 eps + (4 n + 16) u) + 2 eps + 8 u,
the summary and `mass` within bound(n) + (RED(n) + n + 19) u; the device's summary against long-double sums of its own
`full` planes: RED(n) u (1 % on top for the long-double side).  The one-tumour sweeps against their host definitions stay
within their files' bounds, which test_metastasis_distribution.py's n + 2 steps of 4 n + 16 with the pair's (larger) eps
cover (sweep_bound).

The bars of the CPU identities (lattice_common.identity_bar).  Both sides are host evaluations with the same fp64 rates:
P(n) = (2 n + 4) (2 n + 5) + 3 u a path, 275 u at n = 6.  A sum of at most 64 non-negative terms in NumPy's pairwise order
(eight accumulators, then a tree) adds at most 7 + 3 + 1 = 11 u and is as accurate as its worst term otherwise.  A sum
against a single value of a one-tumour sweep (whose own path, n + 2 steps, is shorter) or against another such sum:
2 P(n) + 11 u, 561 u at n = 6 and 101 u at n = 1; J_PT=x(y) against J_MT=y(x), two paths and no sum: 2 P(n) u.  These are
worst cases over paths of full length; "a few dozen u" is what is measured (printed per n).

Measured, CPU: the host definition against the dense oracle 3.1e-15 relative at the worst (n = 1 .. 5); the identities
1.1e-15 relative at the worst (9.8 u of 550 u at n = 6; 0.047 of its bar at the worst, n = 1); the recursion's residual in long double 4.3 u against the derived 2 n + 6 = 22 u
for J and 5.7 u against 213 u for W; a mutation of rate 0 3.3e-4 of the 1e-12 bar.
Measured on an MI355X, worst error / bound per test: device against host 2.7e-3 for the planes (n = 1; 2.0e-3 at n = c + 3)
and 2.5e-3 for the summaries and mass; at_target against exp(lp) of the engine's own paired rows 6.1e-6 of the 1e-9 bar;
mass against the device's one-tumour sweeps 1.5e-5 (n = c + 6); the reduction alone 0.10; a mutation of rate 0 1.7e-3;
partner_forecast device against host 2.1e-4.
"""
import functools

import numpy as np
import pytest

import metmhn_amd.model as model_mod
from metmhn_amd import regularized_optimization as ro
from metmhn_amd.model import GenotypeSummary, MetMHN, PartnerDistribution, PartnerSummary
from lattice_common import (C, U, bits, brute_summary, chain_bound, fit_cohort, host_once, identity_bar, ld_rel, no_library, note,
                            pair_eps, red, rel, summary_rel, without)
from order_common import model, paired

GIVEN = ("PT", "MT")


def bound(mod):
    """Either plane of the device against the host definition (module docstring)."""
    return chain_bound(pair_eps(mod), 2 * mod.n + 4, 4 * mod.n + 16, out=True)


def summary_bound(mod):
    """A summary entry or `mass`: bound with the reductions."""
    return chain_bound(pair_eps(mod), 2 * mod.n + 4, 4 * mod.n + 16, out=True, summed=mod.n)


def sweep_bound(mod):
    """A one-tumour sweep's value on the device against its host definition, with the pair's eps (module docstring)."""
    return chain_bound(pair_eps(mod), mod.n + 2, 4 * mod.n + 16, out=True)


def popcount(x):
    return bin(int(x)).count("1")


@functools.lru_cache(maxsize=None)
def host(n, seed, given):
    """{q: planes [2, 2^n]} of order_common.model(n, seed) by the host definition for every query code asked for so far:
    a query is computed once and never written to."""
    mod = model(n, seed=seed)
    rates = mod._partner_rates()

    return host_once(lambda q: mod._partner_host(q, given, rates))


def queries(n):
    """n <= 3: every genotype.  Larger n: a fixed dozen with the empty and the full genotype, low bits only, high bits only,
    the bits c - 1 and c together, a single high bit, all high bits with no low bit."""
    full = (1 << n) - 1
    if n <= 3:
        return list(range(1 << n))
    low = (1 << C) - 1
    fixed = [0, full, 0x155 & low, low, full & ~low, (3 << (C - 1)) & full, (1 << (n - 1)), (full & ~low) | 1,
             0x2A5 | (1 << C if n > C else 0), (full >> 1), (0x0F | 5 << (C - 1)) & full, (1 << (C - 1)) | (full & ~low & ~(1 << C))]
    more = np.random.default_rng(n).integers(0, full + 1, 24).tolist()        # (n = c has no high bits: some of `fixed` coincide)
    return list(dict.fromkeys(int(q) & full for q in fixed + more))[:12]


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_host_definition_against_the_dense_oracle():
    """partner[y] of the query x against exp(dense.patient_lp) of the paired row (x, y) with order code 0 (unknown order:
    the oracle adds both order terms), both `given`: every pair at n = 1 .. 4, 64 fixed pairs with the empty and the full
    genotype on either side at n = 5.  Worst relative difference 3.1e-15 against the bar 1e-12."""
    from oracle import dense
    worst = 0.0
    for n in range(1, 6):
        mod = model(n, seed=n)
        size = 1 << n
        if n < 5:
            pairs = [(x, y) for x in range(size) for y in range(size)]
        else:
            rng = np.random.default_rng(5)
            pairs = [(0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1)] + \
                [tuple(int(v) for v in rng.integers(0, size, 2)) for _ in range(60)]
            assert len(pairs) == 64
        got = mod.partner_distribution(bits(n, [pairs[0][0]])[0], "PT", backend="host")
        assert isinstance(got, PartnerDistribution) and np.array_equal(got.codes, np.arange(size))
        assert isinstance(got.summary, PartnerSummary) and isinstance(got.summary, GenotypeSummary)
        assert got.partner.tobytes() == host(n, n, "PT")(pairs[0][0])[1].tobytes()
        for x, y in pairs:
            ev = lambda v: [j for j in range(n) if v >> j & 1]
            ref = np.exp(dense.patient_lp(mod.log_theta, mod.obs1, mod.obs2, paired(n, ev(x), ev(y), 0)))
            worst = max(worst, rel(host(n, n, "PT")(x)[1, y], ref), rel(host(n, n, "MT")(y)[1, x], ref))
    print(f"host J against exp(dense.patient_lp) of the paired rows of unknown order, n = 1 .. 5: worst relative {worst:.2e}")
    assert worst <= 1e-12


def test_identities():
    """n = 1 .. 6, every query, each identity under its derived bar (module docstring): a sum against a single value or
    against another sum of at most 64 terms 2 P(n) + 11 u, J_PT=x(y) against J_MT=y(x) 2 P(n) u."""
    worst, worst_u = 0.0, 0.0
    for n in range(1, 7):
        mod = model(n, seed=n)
        size = 1 << n
        idx = np.arange(size)
        seeded = mod.genotype_distribution(backend="host").seeded
        met = mod.metastasis_distribution(backend="host")
        J, sums, over = {}, 0.0, lambda a: np.ascontiguousarray(a.T).sum(axis=1)      # (pairwise, as the 1-D sums are)
        for given, total in (("PT", seeded), ("MT", met.metastasis)):
            planes = np.stack([host(n, n, given)(q) for q in range(size)])                # [q, 2, 2^n]
            J[given] = planes[:, 1]
            for q in range(size):
                got = mod.partner_distribution(bits(n, [q])[0], given, backend="host")
                assert got.founder.tobytes() == planes[q, 0].tobytes() and got.genotype == q and got.given == given
                for v in (got.founder.sum(), got.partner.sum(), got.mass, got.summary.mass[0], got.summary.mass[1]):
                    sums = max(sums, abs(v - total[q]) / total[q])
                assert (got.founder[(idx & ~q) != 0] == 0.0).all() and (got.founder[(idx & ~q) == 0] > 0).all()
                assert (got.partner > 0).all()
                assert np.array_equal(got.conditional, got.partner / got.mass)
                assert np.array_equal(got.founder_conditional, got.founder / got.mass)
            sums = max(sums, rel(over(planes[:, 0]), met.founder),
                       rel(over(planes[:, 1]), met.metastasis if given == "PT" else seeded))
        sym = rel(J["PT"], J["MT"].T)
        print(f"identities of the host definition, n = {n}: sums {sums / U:.1f} u, bar {identity_bar(n, 11)} u; "
              f"J_PT=x(y) against J_MT=y(x) {sym / U:.1f} u, bar {identity_bar(n, 0)} u")
        assert sums <= identity_bar(n, 11) * U and sym <= identity_bar(n, 0) * U
        worst, worst_u = max(worst, sums, sym), max(worst_u, sums / (identity_bar(n, 11) * U), sym / (identity_bar(n, 0) * U))
    print(f"identities of the host definition, n = 1 .. 6: worst relative {worst:.2e} ({worst / U:.1f} u), worst error / bar {worst_u:.3f}")


def test_recursion_in_long_double():
    """n = 8, six queries, both `given`.  J: every state's right-hand side from the host's own fp64 rates, its W at the state
    and its J at the predecessors (G = J / clock) in np.longdouble against the host's J.  The fp64 evaluation rounds along a
    path of the non-negative sum-product: the G of a predecessor against the value returned (1), its product (1), at most
    n + 1 additions of the numerator, at most n + 1 of den, the division (1), the clock times G (1): 2 n + 6 u.  W: G0 and B
    and their product re-evaluated in long double from the fp64 rates: |q| + 2 <= n + 2 states, each a product, at most
    n + 1 additions, at most n + 2 of den and a division (2 n + 5 u), then sigma and two products (3 u): (n + 2) (2 n + 5) + 3 u.
    The long double side adds 2^-64 terms, below the 1 % allowed on top."""
    n, seed, ld = 8, 8, np.longdouble
    mod = model(n, seed=seed)
    idx, level, lam, sig, den0, chains = mod._partner_rates()
    size = 1 << n
    worst_j = worst_w = 0.0
    for given in GIVEN:
        (rq, kq, _), (rp, kp, _) = chains[given], chains["MT" if given == "PT" else "PT"]
        for q in (0, size - 1, 0x55, 0xF0, 0x81, 0x3C):
            W, J = host(n, seed, given)(q)
            for y in range(size):
                f, L = ld(W[y]), ld(0)
                for b in range(n):
                    if y >> b & 1:
                        x = y ^ 1 << b
                        f += ld(J[x]) / ld(kp[x]) * ld(rp[b][x])
                    else:
                        L += ld(rp[b][y])
                ref = ld(kp[y]) * f / (L + ld(kp[y]))
                worst_j = max(worst_j, float(abs(ld(J[y]) - ref) / ref))
            subs = [z for z in range(size) if z & ~q == 0]
            k0 = np.exp(model_mod._subset_sums(mod.obs1[:n]))
            G0, B = {}, {}
            for z in sorted(subs, key=popcount):
                f = ld(1) if z == 0 else sum(G0[z ^ 1 << b] * ld(lam[b][z ^ 1 << b]) for b in range(n) if z >> b & 1)
                L = sum((ld(lam[b][z]) for b in range(n) if not z >> b & 1), ld(0))
                G0[z] = f / (L + ld(sig[z]) + ld(k0[z]))
            for z in sorted(subs, key=popcount, reverse=True):
                L = sum((ld(rq[b][z]) for b in range(n) if not z >> b & 1), ld(0))
                num = ld(kq[z]) if z == q else sum(ld(rq[b][z]) * B[z | 1 << b] for b in range(n) if q >> b & 1 and not z >> b & 1)
                B[z] = num / (L + ld(kq[z]))
            for z in subs:
                ref = ld(sig[z]) * G0[z] * B[z]
                worst_w = max(worst_w, float(abs(ld(W[z]) - ref) / ref))
    bar_w = (n + 2) * (2 * n + 5) + 3
    print(f"residual of the recursion in long double, n = {n}: J {worst_j / U:.2f} u, bar {2 * n + 6} u; "
          f"W {worst_w / U:.2f} u, bar {bar_w} u")
    assert worst_j <= 1.01 * (2 * n + 6) * U and worst_w <= 1.01 * bar_w * U


def check_dead_mutation(a_of, b_of, mod_n, codes, small, j, bar):
    """a_of(q) / b_of(q): the PartnerDistribution of the model with mutation j of rate 0 / of the model without it."""
    worst = 0.0
    for q in (1 << j, (1 << mod_n) - 1):                                # the query holds the dead mutation
        a = a_of(q)
        assert (a.founder == 0.0).all() and (a.partner == 0.0).all() and a.mass == 0.0
        assert np.isnan(a.conditional).all() and np.isnan(a.founder_conditional).all()
        assert not a.summary.pairs.any() and not a.summary.burden.any() and not a.summary.mass.any()
    for q, qs in ((0, 0), (int(codes[-1]), int(small[-1])), (int(codes[5]), int(small[5]))):
        a, b = a_of(q), b_of(qs)
        holds = np.setdiff1d(a.codes, codes)
        for name in ("founder", "partner"):
            assert (getattr(a, name)[holds] == 0.0).all(), name
            worst = max(worst, rel(getattr(a, name)[codes], getattr(b, name)[small]) / bar)
        keep = [i for i in range(mod_n) if i != j]
        assert (a.summary.pairs[:, j, :] == 0.0).all() and (a.summary.pairs[:, :, j] == 0.0).all()
        worst = max(worst, rel(a.mass, b.mass) / bar, rel(a.summary.pairs[np.ix_([0, 1], keep, keep)], b.summary.pairs) / bar,
                    rel(a.summary.burden[:, :-1], b.summary.burden) / bar)
    return worst


def test_a_mutation_of_rate_zero():
    n, j = 6, 2
    dead, less, codes, small = without(model(n, seed=35), j)
    for given in GIVEN:
        worst = check_dead_mutation(lambda q: dead.partner_distribution(bits(n, [q])[0], given, backend="host"),
                                    lambda q: less.partner_distribution(bits(n - 1, [q])[0], given, backend="host"),
                                    n, codes, small, j, 1e-12)
        print(f"a mutation of rate 0 against the model without it (host, given {given}): worst error / 1e-12 {worst:.3e}")
        assert worst <= 1.0


def check_forecast(fc, mod, dat, backend):
    """partner_forecast's result against the formulas written out from partner_distribution of every row."""
    n = mod.n
    typ = dat[:, -1]
    assert set(typ.tolist()) >= {0, 1, 2, 3, 4}
    worst = 0.0
    for i, row in enumerate(dat):
        if typ[i] in (0, 3):
            assert np.isnan(fc.frequencies[i]).all() and np.isnan(fc.burden[i]) and np.isnan(fc.founder_burden[i])
            assert np.isnan(fc.mass[i]) and fc.given[i] == "" and fc.codes[i] == -1
            continue
        given = "MT" if typ[i] == 2 else "PT"
        g = row[1:2 * n:2] if typ[i] == 2 else row[0:2 * n:2]
        one = mod.partner_distribution(g, given, backend=backend)
        gb = bits(n, one.codes).astype(np.float64)
        assert fc.given[i] == given and fc.codes[i] == one.genotype
        worst = max(worst, rel(fc.mass[i], one.mass), rel(fc.frequencies[i], one.conditional @ gb),
                    rel(fc.burden[i], one.conditional @ gb.sum(axis=1)),
                    rel(fc.founder_burden[i], one.founder_conditional @ gb.sum(axis=1)))
    return worst


def test_python_layer_on_a_mixed_cohort():
    n = 5
    mod = model(n, seed=48)
    dat = fit_cohort(n)
    q = 0b01101
    g = bits(n, [q])[0]
    for given in GIVEN:
        got = mod.partner_distribution(g, given, backend="host")
        s, gb = got.summary, bits(n, got.codes).astype(np.float64)
        assert repr(s).startswith("PartnerSummary(n_mut=5") and model_mod.PARTNER_STRATA == ("founder", "partner")
        for k, (stratum, plane) in enumerate((("founder", got.founder), ("partner", got.partner))):
            assert np.array_equal(s.frequencies(stratum), s.pairs[k] / s.mass[k])
            assert np.array_equal(s.conditional_frequencies(stratum), np.diag(s.pairs[k]) / s.mass[k])
            assert rel(s.conditional_frequencies(stratum), (plane / plane.sum()) @ gb) <= 1e-12
            assert abs(s.burden_pmf(stratum).sum() - 1.0) <= 1e-12
            assert abs(s.expected_burden(stratum) - (plane / plane.sum()) @ gb.sum(axis=1)) <= 1e-12
        f = s.conditional_frequencies()
        assert np.array_equal(f, s.conditional_frequencies("partner"))
        held = g.astype(bool)
        assert np.array_equal(s.gained(g)[~held], f[~held]) and np.isnan(s.gained(g)[held]).all()
        assert np.array_equal(s.lost(g)[held], 1.0 - f[held]) and np.isnan(s.lost(g)[~held]).all()
        assert (s.conditional_frequencies("founder")[~held] == 0.0).all()          # the founder is a subset of the query
        lo = s.log_odds("partner")
        assert np.isnan(np.diag(lo)).all() and np.isfinite(lo[~np.eye(n, dtype=bool)]).all()
        for stratum in ("MT", "EM-PT", "unknown"):
            with pytest.raises(ValueError, match="stratum must be one of"):
                s.frequencies(stratum)
        with pytest.raises(ValueError, match="genotype must be 5 entries of 0 / 1"):
            s.gained(g[:-1])
        # the rows' form against the single query's
        G, T = bits(n, [q, 3, q, 0]), bits(n, [7, 3, 0, 31])
        rows = mod.partner_distributions(G, given, targets=T, backend="host")
        assert rows.codes.tolist() == [q, 3, q, 0] and len(rows.summaries) == 4 and rows.summaries[0] is rows.summaries[2]
        assert rows.mass[0] == got.mass and rows.at_target[0] == got.partner[7] and rows.founder_at_target[0] == got.founder[7]
        assert rows.at_target[2] == got.partner[0] and summary_rel(rows.summaries[0], s) == 0.0
        plain = mod.partner_distributions(G, given, backend="host")
        assert np.isnan(plain.at_target).all() and np.isnan(plain.founder_at_target).all() and np.array_equal(plain.mass, rows.mass)
    fc = ro.partner_forecast(mod.log_theta, mod.obs1, mod.obs2, dat, backend="host")
    worst = check_forecast(fc, mod, dat, "host")
    print(f"partner_forecast against its formulas (host): worst relative {worst:.2e}")
    assert worst <= 1e-12
    own = np.isin(dat[:, -1], (0, 1, 4))
    want = mod.genotype_distribution_at(dat[own][:, 0:2 * n:2], backend="host").p_seeded
    assert np.array_equal(fc.seeded[own], want) and np.isnan(fc.seeded[~own]).all()


def test_refusals(monkeypatch):
    no_library(monkeypatch)
    n = 5
    mod = model(n, seed=36)
    g = bits(n, [10])[0]
    G = bits(n, [1, 10, 0])
    for call in (lambda **kw: mod.partner_distribution(g, **kw), lambda **kw: mod.partner_distributions(G, **kw)):
        with pytest.raises(ValueError, match="given must be 'PT' or 'MT'"):
            call(given="pt")
        with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
            call(backend="cpu")
    for bad in (G, g[:-1]):
        with pytest.raises(ValueError, match=rf"genotype.* must have shape \[(R, )?{n}\]"):
            mod.partner_distribution(bad, backend="host")
    for bad in (g, G[:, :-1]):
        with pytest.raises(ValueError, match=rf"genotypes must have shape \[R, {n}\]"):
            mod.partner_distributions(bad)
    with pytest.raises(ValueError, match=rf"targets must have shape \[R, {n}\]"):
        mod.partner_distributions(G, targets=G[:2])
    H = G.copy()
    H[1, 4] = 2
    for backend in ("device", "host"):
        with pytest.raises(ValueError, match=r"^row 1: ") as e1:
            mod.partner_distributions(H, backend=backend)
        with pytest.raises(ValueError, match=r"^row 1: "):
            mod.partner_distributions(G, targets=H, backend=backend)
        with pytest.raises(ValueError) as e2:
            mod.seeding_landscape_at(H)
        assert str(e1.value) == str(e2.value)
        with pytest.raises(ValueError, match=r"^row 0: "):
            mod.partner_distribution(H[1], backend=backend)
    wide = model(25, seed=1)
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.partner_distribution(np.zeros(25, dtype=np.int8), backend="host")
    with pytest.raises(ValueError, match="host distribution stops at 24.*backend='device'"):
        wide.partner_distributions(np.zeros((1, 25), dtype=np.int8), backend="host")
    with pytest.raises(ValueError, match=rf"needs {16 << n} bytes, more than max_bytes = 511; partner_distributions reads"):
        mod.partner_distribution(g, backend="host", max_bytes=(16 << n) - 1)
    with pytest.raises(ValueError, match=rf"needs {16 << 28} bytes, more than max_bytes = {2 ** 31}"):
        model(28, seed=1).partner_distribution(np.zeros(28, dtype=np.int8))      # the default: 2 GiB, n <= 27; before any library
    assert mod.partner_distribution(g, backend="host", max_bytes=16 << n).partner.shape == (1 << n,)
    empty = mod.partner_distributions(np.zeros((0, n), dtype=np.int8), backend="host")
    assert empty.mass.shape == (0,) and empty.at_target.shape == (0,) and empty.summaries == []


def test_engine_refusals_before_the_library():
    """Engine.partner_distributions checks `given`, the shapes and full with R != 1 before it calls the library."""
    from metmhn_amd.engine import Engine
    n = 4
    mod = model(n, seed=2)
    eng = Engine.__new__(Engine)                                       # no device: only the argument checks are reached
    eng.n, eng.N, eng.h = n, n + 1, None
    args = (mod.log_theta, mod.obs1, mod.obs2)
    with pytest.raises(ValueError, match="given must be 'PT' or 'MT'"):
        eng.partner_distributions(*args, bits(n, [1]), given="both")
    with pytest.raises(ValueError, match=rf"genotypes must be a 2-D array \[R, {n}\]"):
        eng.partner_distributions(*args, bits(n, [1])[0])
    with pytest.raises(ValueError, match="targets must be a 2-D array"):
        eng.partner_distributions(*args, bits(n, [1, 2]), targets=bits(n, [1]))
    for G in (bits(n, [1, 2]), np.zeros((0, n), dtype=np.int8)):
        with pytest.raises(ValueError, match=rf"full=True returns the planes of one query.*got {len(G)}"):
            eng.partner_distributions(*args, G, full=True)


# ------------------------------------------------------------------------------------------------------------------ GPU
def device(mod, G, given="PT", **kw):
    from metmhn_amd.jx import engine
    return engine(mod.n).partner_distributions(mod.log_theta, mod.obs1, mod.obs2, G, given, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("given", GIVEN)
@pytest.mark.parametrize("n", (1, 3, C, C + 1, C + 3))
def test_device_against_the_host_definition(n, given):
    """One partial tile (n = 1, 3), exactly one tile (n = c), two tiles and one cross-tile pull (c + 1), eight tiles and
    several levels of the restricted list (c + 3).  Bounds: module docstring."""
    seed = 40 + n
    mod = model(n, seed=seed)
    qs = queries(n)
    assert n <= 3 or len(qs) == 12
    G = bits(n, qs)
    T = bits(n, qs[::-1])
    values, status, sums, none = device(mod, G, given, targets=T)
    assert none is None and (status == 0).all() and values.shape == (len(qs), 3)
    assert sums[0].shape == (len(qs), 2) and sums[1].shape == (len(qs), 2, n, n) and sums[2].shape == (len(qs), 2, n + 1)
    planes = ref_sum = 0.0
    for i, q in enumerate(qs):
        ref = host(n, seed, given)(q)
        one, st, s1, whole = device(mod, G[i:i + 1], given, targets=T[i:i + 1], full=True)
        assert st.tolist() == [0] and one.tobytes() == values[i:i + 1].tobytes() and whole.shape == (2, 1 << n)
        assert all(a[0].tobytes() == b[i].tobytes() for a, b in zip(s1, sums))
        t = qs[::-1][i]
        assert values[i, 1] == whole[0, t] and values[i, 2] == whole[1, t] and values[i, 0] == sums[0][i, 1]
        planes = max(planes, rel(whole, ref) / bound(mod))
        got = PartnerSummary(sums[0][i], sums[1][i], sums[2][i])
        ref_sum = max(ref_sum, summary_rel(got, mod._partner_summary_host(ref)) / summary_bound(mod),
                      rel(values[i, 0], ref[1].sum()) / summary_bound(mod))
        assert np.array_equal(got.pairs, got.pairs.transpose(0, 2, 1))
    note(f"device planes against host, given {given}, n = {n}", planes)
    note(f"device summary and mass against host, given {given}, n = {n}", ref_sum)
    whole_py = mod.partner_distribution(G[-1], given)
    assert whole_py.partner.tobytes() == whole[1].tobytes() and whole_py.founder.tobytes() == whole[0].tobytes()
    assert whole_py.mass == values[-1, 0] and isinstance(whole_py.summary, PartnerSummary)


@pytest.mark.gpu
def test_device_against_the_engines_own_paired_rows():
    """n = 14, 20 paired rows of unknown order with k up to 12 as targets of their own PT (given "PT") and of their own MT
    (given "MT"): at_target against exp of the evaluation's per-row log-probabilities, at the project's 1e-9 (relative)."""
    from metmhn_amd.engine import Engine
    n = 14
    mod = model(n, seed=70)
    rng = np.random.default_rng(71)
    PT = (rng.random((20, n)) < 0.3).astype(np.int8)
    MT = (rng.random((20, n)) < 0.3).astype(np.int8)
    PT[0], MT[0] = 0, 0
    PT[1, :6], MT[1, :] = 1, 0
    PT[2, C:], PT[2, :C], MT[2, C - 1:C + 1] = 1, 0, 1
    keep = (PT.sum(axis=1) + MT.sum(axis=1) + 1) <= 12
    PT, MT = PT[keep], MT[keep]
    assert len(PT) >= 16 and (PT.sum(axis=1) + MT.sum(axis=1) + 1).max() >= 10
    dat = np.array([paired(n, np.flatnonzero(p), np.flatnonzero(m), 0) for p, m in zip(PT, MT)], dtype=np.int8)
    with Engine(n) as eng:
        eng.set_cohort(dat)
        lp = eng.patient_grads(mod.log_theta, mod.obs1, mod.obs2, with_grad=False)
    for given, G, T in (("PT", PT, MT), ("MT", MT, PT)):
        rows = mod.partner_distributions(G, given, targets=T)
        assert (rows.at_target > 0).all()
        note(f"at_target against exp(lp) of the engine's paired rows, given {given}, over 1e-9",
             rel(rows.at_target, np.exp(lp)) / 1e-9)
        values, status, _, _ = device(mod, G, given, targets=T, summary=False)
        assert (status == 0).all() and values[:, 2].tobytes() == rows.at_target.tobytes()
        assert values[:, 0].tobytes() == rows.mass.tobytes() and values[:, 1].tobytes() == rows.founder_at_target.tobytes()


@pytest.mark.gpu
def test_mass_against_the_devices_one_tumour_sweeps():
    """n = c + 6, 8 queries: mass against genotype_distribution_at's seeded (given "PT") and metastasis_distribution_at's
    metastasis (given "MT"), within the sum of the two bounds."""
    n = C + 6
    mod = model(n, seed=74)
    full = (1 << n) - 1
    G = bits(n, [0, full, 0x3FF & full, full & ~0x3FF, 1 << (n - 1), 0x8421, 0x5A5A & full, (3 << (C - 1))])
    for given, ref in (("PT", mod.genotype_distribution_at(G).seeded), ("MT", mod.metastasis_distribution_at(G).metastasis)):
        rows = mod.partner_distributions(G, given)
        for i in range(len(G)):
            assert rows.summaries[i].mass[1] == rows.mass[i]
        note(f"mass against the device's one-tumour sweep, given {given}, n = {n}",
             max(rel(rows.mass, ref), rel([s.mass[0] for s in rows.summaries], ref)) / (summary_bound(mod) + sweep_bound(mod)))


@pytest.mark.gpu
def test_the_reduction_alone():
    """n = c + 3: the device summary and mass of one query against the long-double sums over the device's own `full` planes;
    only the reduction's term of the bound applies."""
    n = C + 3
    mod = model(n, seed=40 + n)
    q = (0x2A5 | 5 << C) & ((1 << n) - 1)
    values, _, sums, whole = device(mod, bits(n, [q]), "PT", full=True)
    assert (whole[0][(np.arange(1 << n) & ~q) != 0] == 0.0).all()
    ref = brute_summary(whole)
    note(f"the reduction alone, n = {n}", max(max(ld_rel(a[0], b) for a, b in zip(sums, ref)),
                                               ld_rel(values[:1, 0], ref[0][1:])) / (1.01 * red(n) * U))


@pytest.mark.gpu
def test_same_bytes_whatever_the_other_rows():
    """n = c + 1: a query's values, summary and full planes alone, among 300 permuted rows, duplicated, next to an invalid row,
    after a call with the other `given`; R = 0 returns empty arrays; the library's own refusals of full with R != 1 and of
    another `given`.  (The workspace limit is the next test: the engine takes no limit below 1 MiB, and a call at n = c + 1
    needs 0.1 MiB.)"""
    n = C + 1
    mod = model(n, seed=41 + C)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    size = 1 << n
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    perm = np.random.default_rng(7).permutation(size)[:300]
    perm[:5] = (0, size - 1, (1 << C) - 1, 1 << C, 0x2A5)
    tperm = np.random.default_rng(8).permutation(size)[:300]
    G, T = bits(n, perm), bits(n, tperm)
    for given in GIVEN:
        values, status, sums, _ = device(mod, G, given, targets=T)
        assert (status == 0).all() and np.isfinite(values).all()
        device(mod, G[:3], "MT" if given == "PT" else "PT")                       # an earlier call with the other `given`
        for i in range(5):
            one, st, s1, whole = device(mod, G[i:i + 1], given, targets=T[i:i + 1], full=True)
            assert st.tolist() == [0] and one.tobytes() == values[i:i + 1].tobytes()
            assert same([a[0] for a in s1], [b[i] for b in sums])
            assert one[0, 1] == whole[0, tperm[i]] and one[0, 2] == whole[1, tperm[i]]
            again = device(mod, G[i:i + 1], given, targets=T[i:i + 1], full=True)
            assert again[3].tobytes() == whole.tobytes() and again[0].tobytes() == one.tobytes()
        dup = np.vstack((G[4], G[2], G[4], G[4]))
        out, st, s2, _ = device(mod, dup, given, targets=np.vstack((T[4], T[2], T[0], T[4])))
        assert (st == 0).all() and out[[0, 1, 3]].tobytes() == values[[4, 2, 4]].tobytes() and out[2, 0] == values[4, 0]
        assert all(same([a[k] for a in s2], [b[4] for b in sums]) for k in (0, 2, 3))
        bad = np.vstack((G[4], G[3], G[2]))
        bad[1, 2] = 3
        out, st, s2, _ = device(mod, bad, given, targets=T[[4, 3, 2]])
        assert st.tolist() == [0, 2 | 8 << 16, 0] and np.isnan(out[1]).all() and all(np.isnan(a[1]).all() for a in s2)
        assert out[[0, 2]].tobytes() == values[[4, 2]].tobytes() and same([a[[0, 2]] for a in s2], [b[[4, 2]] for b in sums])
        bad_t = T[[4, 3, 2]].copy()
        bad_t[2, 0] = -1
        out, st, _, _ = device(mod, G[[4, 3, 2]], given, targets=bad_t)
        assert st.tolist() == [0, 0, 2 | 8 << 16] and np.isnan(out[2]).all() and out[:2].tobytes() == values[[4, 3]].tobytes()
        plain, st, none, _ = device(mod, G[:9], given, summary=False)
        assert none is None and plain[:, 0].tobytes() == values[:9, 0].tobytes() and np.isnan(plain[:, 1:]).all()
        v0, s0, e0, _ = device(mod, np.zeros((0, n), dtype=np.int8), given)
        assert v0.shape == (0, 3) and s0.shape == (0,) and e0[0].shape == (0, 2) and e0[1].shape == (0, 2, n, n)
        with pytest.raises(ValueError, match=r"^row 1: "):
            mod.partner_distributions(bad, given)
    from metmhn_amd import _lib
    from metmhn_amd.jx import engine
    eng = engine(n)                                                    # the library's own refusal of full with R != 1
    ptr = lambda a, t=_lib.f64p: a.ctypes.data_as(t)
    par = [np.ascontiguousarray(a, dtype=np.float64) for a in args]
    two, v2, s2, w2 = np.ascontiguousarray(G[:2]), np.empty((2, 3)), np.zeros(2, dtype=np.int32), np.empty((2, size))
    with pytest.raises(RuntimeError, match="full needs n_rows == 1"):
        _lib.check(eng.lib.mmhn_partner_distributions(eng.h, *(ptr(a) for a in par), 0, ptr(two, _lib.i8p), None, 2, ptr(v2),
                                                      ptr(s2, _lib.i32p), None, ptr(w2)))
    with pytest.raises(RuntimeError, match="given must be 0"):
        _lib.check(eng.lib.mmhn_partner_distributions(eng.h, *(ptr(a) for a in par), 2, ptr(two, _lib.i8p), None, 2, ptr(v2),
                                                      ptr(s2, _lib.i32p), None, None))


@pytest.mark.gpu
def test_a_workspace_limit_that_just_holds_the_call():
    """n = c + 6, the smallest n whose call needs more than the 1 MiB below which the engine takes no limit: the same bytes
    under a limit of exactly the bytes the refusal names, whatever the rows and with or without summaries; one byte less is
    refused as a whole with the byte count, before anything is launched or allocated."""
    import re
    from metmhn_amd.engine import Engine
    n = C + 6
    mod = model(n, seed=74)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    full = (1 << n) - 1
    G, T = bits(n, [0x8421, full, 0, 0x8421, 0x5A5A & full]), bits(n, [3, full, 1 << C, 0, 0x5A5A & full])
    values, status, sums, _ = device(mod, G, "MT", targets=T)
    assert (status == 0).all()
    roomy = device(mod, G[:1], "MT", targets=T[:1], full=True)[3]              # the planes of query 0 without a limit
    assert roomy[1, 3] == values[0, 2]
    with Engine(n, workspace_bytes=1 << 20) as tiny:
        with pytest.raises(RuntimeError, match=rf"partner distribution: {n} mutations need (\d+) bytes of workspace \(16 B x "
                                                r"2\^n_mut.*limit is 1048576 bytes; there is no partial distribution") as err:
            tiny.partner_distributions(*args, G[:1])
    need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
    partials = 2 * 67 * 8 << (n - C)
    assert (16 << n) + (8 << (n - C)) + partials <= need <= (16 << n) + (8 << (n - C)) + partials + (1 << 16)
    with Engine(n, workspace_bytes=need) as snug:
        out, st, s2, _ = snug.partner_distributions(*args, G, "MT", targets=T)
        assert (st == 0).all() and out.tobytes() == values.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(s2, sums))
        one, _, none, whole = snug.partner_distributions(*args, G[:1], "MT", targets=T[:1], summary=False, full=True)
        assert none is None and one.tobytes() == values[:1].tobytes() and whole.tobytes() == roomy.tobytes()
    with Engine(n, workspace_bytes=need - 1) as small:
        before = small.counters()
        for kw in ({}, {"summary": False}):
            with pytest.raises(RuntimeError, match=rf"need {need} bytes.*limit is {need - 1} bytes"):
                small.partner_distributions(*args, G[:1], "MT", **kw)
        with pytest.raises(RuntimeError, match=rf"need {need} bytes"):
            small.partner_distributions(*args, np.zeros((0, n), dtype=np.int8))
        assert small.counters() == before                              # nothing was launched or allocated through the engine


@pytest.mark.gpu
def test_a_mutation_of_rate_zero_on_the_device():
    """n = c + 1, the dead mutation the high bit (whole tiles of zeros) and a low one, under the device-against-host bound;
    exact zeros are met exactly (lattice_common.rel)."""
    n = C + 1
    mod = model(n, seed=80)
    for j in (C, 2):
        dead, less, codes, small = without(mod, j)
        for given in GIVEN:
            note(f"a mutation of rate 0 (bit {j}) on the device against the host model without it, given {given}",
                 check_dead_mutation(lambda q: dead.partner_distribution(bits(n, [q])[0], given),
                                     lambda q: less.partner_distribution(bits(n - 1, [q])[0], given, backend="host"),
                                     n, codes, small, j, summary_bound(less)))


@pytest.mark.gpu
def test_partner_forecast_on_the_device():
    """partner_forecast on the device against its formulas from the device's own planes, and against the host."""
    m5 = model(5, seed=48)
    dat = fit_cohort(5)
    fc = ro.partner_forecast(m5.log_theta, m5.obs1, m5.obs2, dat)
    note("partner_forecast on the device against its formulas, over 1e-12", check_forecast(fc, m5, dat, "device") / 1e-12)
    ref = ro.partner_forecast(m5.log_theta, m5.obs1, m5.obs2, dat, backend="host")
    own = ~np.isnan(ref.mass)
    assert np.array_equal(fc.codes, ref.codes) and np.array_equal(fc.given, ref.given)
    note("partner_forecast device against host", max(rel(fc.mass[own], ref.mass[own]), rel(fc.frequencies[own], ref.frequencies[own]),
                                                     rel(fc.burden[own], ref.burden[own])) / (2 * summary_bound(m5) + 2 * U))
    seen = np.isin(dat[:, -1], (0, 1, 4))
    assert np.allclose(fc.seeded[seen], ref.seeded[seen], rtol=1e-9, atol=0) and np.isnan(fc.seeded[~seen]).all()
