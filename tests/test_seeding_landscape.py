"""The seeding landscape: the forecast scalars of every genotype from one backward sweep (MetMHN.seeding_landscape /
seeding_landscape_at, SeedingLandscape, mmhn_seeding_landscape, regularized_optimization.seeding_risk;
metmhn_amd/csrc/landscape.h).

CPU: the host definition against MetMHN.seeding_forecast of every genotype (1e-12 relative, the bar against the dense
oracle elsewhere; exact zeros exact), its identities, the four recursions re-evaluated in long double, a mutation of rate
0, the refusals and the cohort wrapper.

GPU: the device landscape against the host definition and against the forward kernel (mmhn_seeding_forecasts, which
shares no code with the backward one) under a bound computed from the model: lattice_common's chain_bound with the
primary tumour's eps (pt_eps, obs1 without the clock's entry).  A state's numerator and den add at most 2 n + 8 roundings,
both sides together; the chain behind a value is at most n + 1 states deep; no value is a sum over tiles, so there is no
reduction term.  Every value agrees within relative bound(n) = (n + 1) (4 eps + (2 n + 8) u).  Against the forward kernel
the bar is bound(n) + the forecast bound of the row (tests/test_seeding_forecasts.py: f + 1 steps of 2 f + 6, and
S_FORECAST u for the final sums).

Measured on an MI355X, worst error / bound per test: device against host 1.7e-2 (n = 1, until the seeding; 2.4e-3 at
n = c + 3), against the forward kernel 5.4e-4 (n = c + 6) and 2.1e-4 (n = 22), statuses 2.5e-3, seeding_risk against
seeding_forecast 1.4e-3.  The host definition against seeding_forecast of every genotype (CPU): 3.6e-15 relative at the worst.
"""
import re

import numpy as np
import pytest

import metmhn_amd.model as model_mod
from metmhn_amd import regularized_optimization as ro
from metmhn_amd.model import MetMHN, SeedingLandscape
from lattice_common import C, U, bits, check_same_bytes, forecast_bound, genotype, host_once, note
from lattice_common import landscape_bound as bound
from lattice_common import rel_nan as rel
from order_common import mixed_cohort, model

UNTIL = ("seeding", "observation")
FIELDS = SeedingLandscape.FIELDS


@host_once
def host(n, seed, until):
    """The host landscape [4, 2^n] of order_common.model(n, seed)."""
    return model(n, seed=seed)._landscape_host(until)


def forecast_scalars(r):
    """(p_seed, time, new_events, seed_events) [R, 4] of a SeedingForecast(s)."""
    return np.stack([np.atleast_1d(np.asarray(r.p_seed, dtype=np.float64)), np.atleast_1d(np.asarray(r.time, dtype=np.float64)),
                     np.nansum(np.atleast_2d(r.before), axis=1), np.nansum(np.atleast_2d(r.with_seed), axis=1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("until", UNTIL)
def test_host_definition_against_the_forecast_of_every_genotype(until):
    worst = 0.0
    for n in range(1, 9):
        mod = model(n, seed=n)
        got = mod.seeding_landscape(until, backend="host")
        assert isinstance(got, SeedingLandscape) and np.array_equal(got.codes, np.arange(1 << n))
        whole = np.stack([getattr(got, name) for name in FIELDS])
        assert whole.shape == (4, 1 << n) and np.array_equal(whole, host(n, n, until))
        for x in range(1 << n):
            ref = forecast_scalars(mod.seeding_forecast(bits(n, [x])[0], until))[0]
            worst = max(worst, rel(whole[:, x], ref))
        assert whole[2, -1] == 0.0 and whole[3, -1] == 0.0           # the full genotype: no new event, exactly
    print(f"host landscape against seeding_forecast of every genotype, n = 1 .. 8, until {until}: worst relative {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("until", UNTIL)
def test_identities(until):
    for n, seed in ((1, 31), (5, 32), (9, 33)):
        mod = model(n, seed=seed)
        p, t, e, s = host(n, seed, until)
        th = mod._pt_log_theta
        sig = np.exp(th[n, n] + th[n, :n].sum())
        kap = np.exp(mod.obs1[:n].sum()) if until == "observation" else 0.0
        close = lambda a, b: abs(a - b) <= 1e-12 * max(abs(a), abs(b))
        assert close(p[-1], sig / (sig + kap)) and close(t[-1], 1.0 / (sig + kap))
        if until == "seeding":
            # exactly 1 in exact arithmetic: the host's own share of the device bound (module docstring) is the bar
            assert np.abs(p - 1.0).max() <= bound(mod)
        # (until the seeding the two are equal in exact arithmetic: the comparison allows for the rounding of both)
        assert (s >= 0).all() and (s <= e * (1 + bound(mod))).all() and (t > 0).all() and (p > 0).all() and (p <= 1 + bound(mod)).all()


@pytest.mark.parametrize("until", UNTIL)
def test_recursions_in_long_double(until):
    """Every state of one n = 10 model: the right-hand sides of the four recursions from the host's own fp64 rates and its
    values at the successors, evaluated in np.longdouble, against the host's value at the state.  The fp64 evaluation of one
    state rounds at most 2 n + 8 times along any path of a non-negative sum-product (n products and n additions of the
    numerator or of den, the seeding and the clock, the inner sum, the division), so the residual is within (2 n + 8) u
    relative; the long double side adds 2^-64 terms, below the 1 % allowed on top."""
    n, seed, ld = 10, 34, np.longdouble
    mod = model(n, seed=seed)
    th = mod._pt_log_theta
    V = host(n, seed, until)
    sums = model_mod._subset_sums
    lam = [np.exp(th[j, j] + sums(np.where(np.arange(n) == j, 0.0, th[j, :n]))) for j in range(n)]
    sig = np.exp(th[n, n] + sums(th[n, :n]))
    kap = np.exp(sums(mod.obs1[:n])) if until == "observation" else np.zeros(1 << n)
    worst = 0.0
    for x in range(1 << n):
        num = [ld(sig[x]), ld(1), ld(0), ld(0)]
        den = ld(sig[x]) + ld(kap[x])
        for j in range(n):
            if not x >> j & 1:
                y, r = x | 1 << j, ld(lam[j][x])
                num[0] += r * ld(V[0, y])
                num[1] += r * ld(V[1, y])
                num[2] += r * (1 + ld(V[2, y]))
                num[3] += r * (ld(V[0, y]) + ld(V[3, y]))
                den += r
        for k in range(4):
            ref = num[k] / den
            if ref == 0:
                assert V[k, x] == 0.0
            else:
                worst = max(worst, float(abs(ld(V[k, x]) - ref) / ref))
    print(f"residual of the four recursions in long double, n = {n}, until {until}: {worst / U:.2f} u, bar {2 * n + 8} u")
    assert worst <= 1.01 * (2 * n + 8) * U


def test_a_mutation_of_rate_zero():
    n, j = 6, 2
    mod = model(n, seed=35)
    th = mod.log_theta.copy()
    th[j, j] = -1e10
    dead = MetMHN(th, mod.obs1, mod.obs2)
    keep = [i for i in range(n + 1) if i != j]
    less = MetMHN(th[np.ix_(keep, keep)], mod.obs1[keep], mod.obs2[keep])
    codes = np.array([x for x in range(1 << n) if not x >> j & 1])
    small = (codes & ((1 << j) - 1)) | (codes >> (j + 1) << j)       # the code without bit j
    assert np.array_equal(np.sort(small), np.arange(1 << (n - 1)))
    for until in UNTIL:
        a, b = dead.seeding_landscape(until, backend="host"), less.seeding_landscape(until, backend="host")
        for name in FIELDS:
            assert np.isfinite(getattr(a, name)).all(), name
            assert rel(getattr(a, name)[codes], getattr(b, name)[small]) <= 1e-12, name


def test_refusals():
    n = 5
    mod = model(n, seed=36)
    G = np.array([genotype(n, [0]), genotype(n, [1, 3]), genotype(n, [])])
    for call in (lambda: mod.seeding_landscape("never", backend="host"),
                 lambda: mod.seeding_landscape_at(G, "never", backend="host")):
        with pytest.raises(ValueError, match="until must be 'seeding' or 'observation'"):
            call()
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.seeding_landscape(backend="cpu")
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.seeding_landscape_at(G, backend="cpu")
    for bad in (G[0], G[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=rf"genotypes must have shape \[R, {n}\]") as e1:
            mod.seeding_landscape_at(bad, backend="host")
        with pytest.raises(ValueError) as e2:
            mod.seeding_forecasts(bad, backend="host")
        assert str(e1.value) == str(e2.value)
    H = G.copy()
    H[1, 4] = 2
    with pytest.raises(ValueError, match=r"^row 1: ") as e1:
        mod.seeding_landscape_at(H, backend="host")
    with pytest.raises(ValueError) as e2:
        mod.seeding_forecasts(H, backend="host")
    assert str(e1.value) == str(e2.value)
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    unseen = MetMHN(th, mod.obs1, mod.obs2)
    with pytest.raises(ValueError, match="no exit"):
        unseen.seeding_landscape("seeding", backend="host")
    with pytest.raises(ValueError, match="no exit"):
        unseen.seeding_landscape_at(G, "seeding", backend="host")
    assert (unseen.seeding_landscape("observation", backend="host").p_seed == 0.0).all()
    wide = model(25, seed=1)
    with pytest.raises(ValueError, match="host landscape stops at 24.*backend='device'"):
        wide.seeding_landscape(backend="host")
    with pytest.raises(ValueError, match="host landscape stops at 24.*backend='device'"):
        wide.seeding_landscape_at(np.zeros((1, 25), dtype=np.int8), backend="host")
    with pytest.raises(ValueError, match=rf"needs {32 << n} bytes, more than max_bytes = 1000"):
        mod.seeding_landscape(backend="host", max_bytes=1000)
    with pytest.raises(ValueError, match=rf"needs {32 << 30} bytes"):       # before any library is reached
        model(30, seed=1).seeding_landscape()
    assert mod.seeding_landscape(backend="host", max_bytes=32 << n).p_seed.shape == (1 << n,)
    # neighbours: a lookup on a full landscape only
    whole = mod.seeding_landscape("observation", backend="host")
    nb = whole.neighbours(G[1])
    assert nb.shape == (n + 1, 4) and (np.isnan(nb[1:]).all(axis=1) == (G[1] == 1)).all()
    assert np.array_equal(nb[0], [getattr(whole, name)[0b01010] for name in FIELDS])
    assert np.array_equal(nb[1 + 2], [getattr(whole, name)[0b01110] for name in FIELDS])
    some = mod.seeding_landscape_at(G, "observation", backend="host")
    assert some.codes.tolist() == [1, 10, 0]
    for name in FIELDS:
        assert np.array_equal(getattr(some, name), getattr(whole, name)[[1, 10, 0]]), name
    with pytest.raises(ValueError, match="full landscape"):
        some.neighbours(G[1])
    empty = mod.seeding_landscape_at(np.zeros((0, n), dtype=np.int8), backend="host")
    assert empty.p_seed.shape == (0,) and empty.codes.shape == (0,)


def test_seeding_risk_scatters_over_a_mixed_cohort(monkeypatch):
    """Types 0 / 1 / 4 get the values of their PT genotype, 2 and 3 NaN; next to it met_status_posterior's column."""
    import unknown_common as UC
    from metmhn_amd import synthetic
    n = 6
    lt, dp, dm = UC.params(n)
    x = UC.unknown_row(n, [0, 3, 4])
    paired = synthetic.full_k_cohort(n, 2, k=4, seed=1)
    mt_only = UC.relabel(x, 1); mt_only[0:2 * n:2] = 0; mt_only[1] = 1; mt_only[-1] = 2
    dat = np.vstack((UC.relabel(x, 0), UC.relabel(x, 1), x, paired, mt_only, UC.unknown_row(n, [])))

    def host_status(lt_, dp_, dm_, rows):                          # the one device call, from the oracle
        rows = np.asarray(rows)
        return np.array([UC.mixture_lp(lt_, dp_, dm_, r)[1] if r[-1] in (0, 1, 4) else np.nan for r in rows])
    monkeypatch.setattr(ro, "met_status_posterior", host_status)
    got, seeded = ro.seeding_risk(lt, dp, dm, dat, backend="host")
    assert isinstance(got, SeedingLandscape) and got.p_seed.shape == (7,)
    assert np.array_equal(seeded, host_status(lt, dp, dm, dat), equal_nan=True)
    mod = MetMHN(lt, dp, dm)
    for i in (0, 1, 2, 6):
        ref = forecast_scalars(mod.seeding_forecast(dat[i, 0:2 * n:2], "observation"))[0]
        assert rel([getattr(got, name)[i] for name in FIELDS], ref) <= 1e-12
    assert got.codes.tolist() == [25, 25, 25, -1, -1, -1, 0]
    for name in FIELDS:
        assert np.isnan(getattr(got, name)[3:6]).all(), name
    assert np.isnan(seeded[3:6]).all() and np.isfinite(seeded[[0, 1, 2, 6]]).all()
    only, _ = ro.seeding_risk(lt, dp, dm, paired, backend="host")
    assert np.isnan(only.p_seed).all()


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("until", UNTIL)
@pytest.mark.parametrize("n", (1, 3, C, C + 1, C + 3))
def test_device_landscape_against_the_host_definition(n, until):
    """One partial tile (n = 1, 3), exactly one tile (n = c), two tiles and one high bit (c + 1), several tiles on a level
    (c + 3).  Bound: module docstring."""
    from metmhn_amd.jx import engine
    seed = 40 + n
    mod = model(n, seed=seed)
    values, status, whole = engine(n).seeding_landscape(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8), until, full=True)
    assert values.shape == (0, 4) and status.shape == (0,) and whole.shape == (4, 1 << n)
    note(f"device against host, n = {n}, until {until}", rel(whole, host(n, seed, until)) / bound(mod))
    got = mod.seeding_landscape(until)
    assert np.stack([getattr(got, name) for name in FIELDS]).tobytes() == whole.tobytes()


def fullest_rows(n, seed, count=24, fmax=17):
    """The `count` genotypes with the fewest free mutations among those a fixed seed draws, at most fmax of them free."""
    rng = np.random.default_rng(seed)
    G = np.unique((rng.random((400, n)) < 0.3).astype(np.int8), axis=0)
    f = n - G.sum(axis=1)
    G, f = G[f <= fmax], f[f <= fmax]
    pick = np.argsort(f, kind="stable")[:count]
    assert len(pick) == count
    return G[pick]


@pytest.mark.gpu
@pytest.mark.parametrize("until", UNTIL)
@pytest.mark.parametrize("n", (C + 6, 22))
def test_device_landscape_against_the_forward_kernel(n, until):
    """n = c + 6: levels of up to 20 tiles of 64; n = 22: 128 MiB, 4 096 tiles.  The forward kernel (forecast.h) shares
    no code with the backward one; the bar is the sum of both bounds."""
    from metmhn_amd.jx import engine
    mod = model(n, seed=50 + n)
    G = fullest_rows(n, 60 + n)
    values, status, _ = engine(n).seeding_landscape(mod.log_theta, mod.obs1, G, until)
    assert (status == 0).all() and np.isfinite(values).all()
    p_seed, time, before, with_seed, _, st = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, G, until)
    assert (st == 0).all()
    ref = np.stack([p_seed, time, np.nansum(before, axis=1), np.nansum(with_seed, axis=1)], axis=1)
    worst = 0.0
    for i, g in enumerate(G):
        worst = max(worst, rel(values[i], ref[i]) / (bound(mod) + forecast_bound(mod, int((g == 0).sum()))))
    note(f"landscape against the forward kernel, n = {n}, until {until}", worst)
    at = mod.seeding_landscape_at(G, until)
    assert np.stack([getattr(at, name) for name in FIELDS], axis=1).tobytes() == values.tobytes()


@pytest.mark.gpu
def test_a_landscape_that_does_not_fit_is_refused_with_its_bytes():
    from metmhn_amd.engine import Engine
    n = 31
    mod = model(n, seed=3)
    row = genotype(n, [0, 30])[None, :]
    with Engine(n, workspace_bytes=1 << 30) as small:
        with pytest.raises(RuntimeError, match=r"31 mutations need (\d+) bytes.*limit is 1073741824 bytes") as err:
            small.seeding_landscape(mod.log_theta, mod.obs1, row, "observation")
        need = int(re.search(r"need (\d+) bytes", str(err.value)).group(1))
        assert (32 << n) + (4 << (n - C)) <= need <= (32 << n) + (4 << (n - C)) + (1 << 16)
        with pytest.raises(RuntimeError, match=r"need \d+ bytes"):
            small.seeding_landscape(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8), "seeding")
    with pytest.raises(ValueError, match=rf"needs {32 << n} bytes"):
        mod.seeding_landscape("observation")


@pytest.mark.gpu
def test_same_bytes_whatever_the_queries():
    from metmhn_amd.jx import engine
    n = C + 1
    mod = model(n, seed=41 + C)
    for until in UNTIL:
        def call(G, **kw):
            values, status, whole = engine(n).seeding_landscape(mod.log_theta, mod.obs1, G, until, **kw)
            return values, status, None, whole
        check_same_bytes(call, 4, n)


@pytest.mark.gpu
def test_statuses_layout_and_the_cohort_wrapper():
    from metmhn_amd.jx import engine
    n, seed = 7, 47
    mod = model(n, seed=seed)
    G = bits(n, [0, 5, 127, 64, 33, 90])
    G[1, 0] = 2
    G[4, 6] = -1
    good = np.array([True, False, True, True, False, True])
    th = mod.log_theta.copy()
    th[3, 3] = -1e10                                               # a mutation that never arises: exact zeros, nothing NaN
    for until in UNTIL:
        values, status, whole = engine(n).seeding_landscape(mod.log_theta, mod.obs1, G, until, full=True)
        assert (status[good] == 0).all() and (status[~good] == (2 | 8 << 16)).all()
        assert np.isnan(values[~good]).all() and np.isfinite(values[good]).all() and np.isfinite(whole).all()
        assert values[good].tobytes() == np.ascontiguousarray(whole[:, [0, 127, 64, 90]].T).tobytes()
        assert whole[2, -1] == 0.0 and whole[3, -1] == 0.0
        note(f"statuses, n = {n}, until {until}", rel(whole, host(n, seed, until)) / bound(mod))
        _, _, dead = engine(n).seeding_landscape(th, mod.obs1, G[:0], until, full=True)
        assert np.isfinite(dead).all()
        ref = MetMHN(th, mod.obs1, mod.obs2)._landscape_host(until)
        assert rel(dead, ref) <= bound(mod)
    with pytest.raises(ValueError, match=r"^row 1: "):
        mod.seeding_landscape_at(G)
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    with pytest.raises(RuntimeError, match="without exit"):
        engine(n).seeding_landscape(th, mod.obs1, G[:1], "seeding")
    # the cohort wrapper on the device against seeding_forecast's fields, row by row
    m5 = model(5, seed=48)
    dat = mixed_cohort(5)
    for until in UNTIL:
        risk, seeded = ro.seeding_risk(m5.log_theta, m5.obs1, m5.obs2, dat, until)
        fc, seeded_fc = ro.seeding_forecast(m5.log_theta, m5.obs1, m5.obs2, dat, until)
        assert np.array_equal(seeded, seeded_fc, equal_nan=True)
        own = np.isin(dat[:, -1], (0, 1, 4))
        assert own.any() and not own.all() and (risk.codes[~own] == -1).all()
        assert np.array_equal(risk.codes[own], dat[own][:, 0:10:2].astype(np.int64) @ (1 << np.arange(5)))
        got = np.stack([getattr(risk, name) for name in FIELDS], axis=1)
        assert np.isnan(got[~own]).all()
        f = 5 - dat[own][:, 0:10:2].sum(axis=1)
        worst = max(rel(a, b) / (bound(m5) + forecast_bound(m5, int(fi))) for a, b, fi in zip(got[own], forecast_scalars(fc)[own], f))
        note(f"seeding_risk against seeding_forecast, until {until}", worst)
