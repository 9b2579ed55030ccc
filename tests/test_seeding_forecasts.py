"""Seeding forecasts from a tumour's genotype (MetMHN.seeding_forecast / seeding_forecasts, mmhn_seeding_forecasts,
regularized_optimization.seeding_forecast; metmhn_amd/csrc/forecast.h).

CPU: the host definition against a dense absorbing-chain solve built entry by entry here and a long-double recursion state
by state (1e-12 relative, the bar against the dense oracle elsewhere), its identities, the link to the likelihood side
(1 - the summed type-0 likelihoods of every PT genotype), zero rates and refusals, the cohort wrapper.

GPU: the device against the host definition under a bound computed from the row (lattice_common.forecast_bound): chain_bound with the
primary tumour's eps (pt_eps, obs1 without the clock's entry).  A state's den and pull add at most 2 f + 6 roundings, f + 1
levels deep; the final sums add S u, S the longest chain of additions of either side - S_FORECAST = 655 for the device's
reduction (forecast.h), NumPy's pairwise sums are shorter.  Every output agrees within relative
(f + 1) (4 eps + (2 f + 6) u) + S u.

Measured on an MI355X, worst error / bound per test: shapes 5.1e-3 (n_mut = 31, until the observation), mixed widths 6.9e-3,
LUAD-28's 20 fullest genotypes (f = 13 .. 18) 1.6e-3; until the seeding every figure is below 1.1e-3.  The host definition
against the dense solve and the long-double recursion (CPU): 5.3e-15 relative at the worst.
"""
import functools

import numpy as np
import pytest

from metmhn_amd import regularized_optimization as ro
from metmhn_amd.model import MetMHN, SeedingForecasts
from lattice_common import forecast_bound, frozen, genotype, note
from lattice_common import rel_nan as rel
from order_common import model

UNTIL = ("seeding", "observation")
FIELDS = ("p_seed", "time", "before", "with_seed", "n_before")


def rates(mod, held_set, until):
    """(lam(j, y), sig(y), kap(y)) of the definition, y a frozenset of mutations: plain Python, one term at a time."""
    th, n = mod._pt_log_theta, mod.n

    def expo(row, y, dtype):
        s = dtype(row[0])
        for i in sorted(y):
            s = s + dtype(row[1][i])
        return np.exp(s)
    lam = lambda j, y, dtype=np.float64: expo((th[j, j], th[j]), y, dtype)
    sig = lambda y, dtype=np.float64: expo((th[n, n], th[n]), y, dtype)
    kap = lambda y, dtype=np.float64: expo((0.0, mod.obs1), y, dtype) if until == "observation" else dtype(0.0)
    return lam, sig, kap


def outputs(mod, g, occ, until, dtype=np.float64):
    """The outputs of the definition from the occupancies occ[idx] (expected time in the state of index idx)."""
    n = mod.n
    free = [j for j in range(n) if not g[j]]
    held = frozenset(j for j in range(n) if g[j])
    f = len(free)
    lam, sig, kap = rates(mod, held, until)
    state = lambda idx: held | {free[b] for b in range(f) if idx >> b & 1}
    out = dict(p_seed=dtype(0), time=dtype(0), before=np.full(n, np.nan, dtype=dtype), with_seed=np.full(n, np.nan, dtype=dtype),
               n_before=np.zeros(n + 1, dtype=dtype))
    for j in free:
        out["before"][j] = out["with_seed"][j] = 0
    for idx in range(1 << f):
        y = state(idx)
        s = occ[idx] * sig(y, dtype)
        out["p_seed"] += s
        out["time"] += occ[idx]
        out["n_before"][bin(idx).count("1")] += s
        for j in free:
            if j in y:
                out["with_seed"][j] += s
            else:
                out["before"][j] += occ[idx] * lam(j, y, dtype)
    x = state(0)
    d0 = sum(lam(j, x) for j in free) + sig(x) + kap(x)
    nxt = np.full(n + 1, np.nan)
    for j in free:
        nxt[j] = lam(j, x) / d0
    nxt[n] = sig(x) / d0
    out["next"] = nxt
    return out


def dense(mod, g, until):
    """The generator over the 2^f supersets entry by entry, the occupancies by a dense solve."""
    n = mod.n
    free = [j for j in range(n) if not g[j]]
    held = frozenset(j for j in range(n) if g[j])
    f = len(free)
    lam, sig, kap = rates(mod, held, until)
    Q = np.zeros((1 << f, 1 << f))                                  # Q[to, from] over the transient states
    for idx in range(1 << f):
        y = held | {free[b] for b in range(f) if idx >> b & 1}
        Q[idx, idx] = -(sig(y) + kap(y))
        for b in range(f):
            if not idx >> b & 1:
                Q[idx | 1 << b, idx] = lam(free[b], y)
                Q[idx, idx] -= lam(free[b], y)
    e0 = np.zeros(1 << f)
    e0[0] = 1.0
    return outputs(mod, g, np.linalg.solve(-Q, e0), until)


def recursion(mod, g, until):
    """F and G state by state in np.longdouble."""
    n, ld = mod.n, np.longdouble
    free = [j for j in range(n) if not g[j]]
    held = frozenset(j for j in range(n) if g[j])
    f = len(free)
    lam, sig, kap = rates(mod, held, until)
    state = lambda idx: held | {free[b] for b in range(f) if idx >> b & 1}
    G = np.zeros(1 << f, dtype=ld)
    for idx in sorted(range(1 << f), key=lambda i: bin(i).count("1")):
        y = state(idx)
        F = ld(1) if idx == 0 else sum(G[idx ^ 1 << b] * lam(free[b], state(idx ^ 1 << b), ld) for b in range(f) if idx >> b & 1)
        G[idx] = F / (sum(lam(j, y, ld) for j in free if j not in y) + sig(y, ld) + kap(y, ld))
    return outputs(mod, g, G, until, ld)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("until", UNTIL)
def test_host_definition_against_dense_solve_and_long_double(until):
    worst = 0.0
    for n in range(1, 10):
        mod = model(n, seed=n)
        rng = np.random.default_rng(100 + n)
        some = genotype(n, rng.choice(n, size=n // 2, replace=False))
        for g in (genotype(n, []), some, genotype(n, range(n))):
            got = mod.seeding_forecast(g, until)
            for ref in (dense(mod, g, until), recursion(mod, g, until)):
                for name in FIELDS + ("next",):
                    worst = max(worst, rel(getattr(got, name), ref[name]))
    print(f"host definition against the dense solve and the long-double recursion, until {until}: worst relative {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("until", UNTIL)
def test_identities_of_the_host_definition(until):
    for n, held in ((6, []), (7, [1, 4]), (5, range(5)), (8, [0, 2, 7])):
        mod = model(n, seed=20 + n)
        g = genotype(n, held)
        r = mod.seeding_forecast(g, until)
        check_identities(mod, g[None, :], until, SimpleFields(r), 1e-12)


class SimpleFields:
    """One SeedingForecast with a leading axis, as SeedingForecasts has it."""

    def __init__(self, r):
        for name in FIELDS + ("next",):
            setattr(self, name, np.asarray(getattr(r, name))[None, ...])


def check_identities(mod, G, until, r, tol):
    """The identities of the definition on the rows G [R, n] of a result r, each within relative tol[row]."""
    n = mod.n
    tol = np.broadcast_to(tol, (G.shape[0],))
    for i, g in enumerate(G):
        free = g == 0
        m = np.arange(n + 1)
        close = lambda a, b: abs(a - b) <= tol[i] * max(abs(a), abs(b))
        assert close(r.n_before[i].sum(), r.p_seed[i])
        assert (r.n_before[i, int(free.sum()) + 1:] == 0).all()
        if until == "seeding":
            assert close(r.p_seed[i], 1.0)
            assert np.all(np.abs(r.with_seed[i, free] - r.before[i, free]) <= tol[i] * r.before[i, free])
            assert close(r.before[i, free].sum(), (m * r.n_before[i]).sum())
        th = mod._pt_log_theta
        x = np.flatnonzero(g)
        kap = np.exp(mod.obs1[x].sum()) if until == "observation" else 0.0
        sig = np.exp(th[n, n] + th[n, x].sum())
        leave = sig + sum(np.exp(th[j, j] + th[j, x].sum()) for j in np.flatnonzero(free))
        assert close(np.nansum(r.next[i]), leave / (leave + kap))        # 1 - kap / den, without the cancellation
        if not free.any():
            assert close(r.p_seed[i], sig / (sig + kap)) and close(r.time[i], 1.0 / (sig + kap))


@pytest.mark.parametrize("n", (4, 6))
def test_link_to_the_likelihood_side(n):
    """From the empty genotype, until the observation with obs1 = log_d_p: 1 - the summed likelihoods of every PT genotype
    observed unseeded."""
    from oracle import dense as D
    mod = model(n, seed=3)
    total = 0.0
    for x in range(1 << n):
        row = np.zeros(2 * n + 3, dtype=np.int8)
        row[0:2 * n:2] = [x >> b & 1 for b in range(n)]
        total += np.exp(D.patient_lp(mod.log_theta, mod.obs1, mod.obs2, row))
    got = mod.seeding_forecast(np.zeros(n, dtype=np.int8), "observation").p_seed
    print(f"n = {n}: p_seed {got:.15f}, 1 - the summed likelihoods {1 - total:.15f}")
    assert abs(got - (1.0 - total)) <= 1e-12


def test_zero_rates_and_refusals():
    n = 5
    mod = model(n, seed=5)
    th = mod.log_theta.copy()
    th[2, 2] = -1e10
    dead = MetMHN(th, mod.obs1, mod.obs2)
    for until in UNTIL:
        r = dead.seeding_forecast(genotype(n, [0]), until)
        assert r.before[2] == 0.0 and r.with_seed[2] == 0.0
        for name in FIELDS:
            v = np.asarray(getattr(r, name), dtype=np.float64)
            held = np.zeros(v.shape, dtype=bool)
            if name in ("before", "with_seed"):
                held[0] = True
            assert (np.isnan(v) == held).all(), name
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    unseen = MetMHN(th, mod.obs1, mod.obs2)
    with pytest.raises(ValueError, match="no exit"):
        unseen.seeding_forecast(genotype(n, [0]), "seeding")
    with pytest.raises(ValueError, match="no exit"):
        unseen.seeding_forecasts(genotype(n, [0])[None, :], "seeding", backend="host")
    assert unseen.seeding_forecast(genotype(n, [0]), "observation").p_seed == 0.0
    G = np.array([genotype(n, [0]), genotype(n, [1, 3]), genotype(n, [])])
    G[1, 4] = 2
    for backend in ("host",):
        with pytest.raises(ValueError, match=r"^row 1: "):
            mod.seeding_forecasts(G, backend=backend)
    with pytest.raises(ValueError, match="until"):
        mod.seeding_forecast(genotype(n, []), "never")
    # the primary tumour does not feel the seeding: theta[:n, n] has no effect
    th = mod.log_theta.copy()
    th[:n, n] += 3.0
    other = MetMHN(th, mod.obs1, mod.obs2)
    for until in UNTIL:
        a, b = mod.seeding_forecast(genotype(n, [1]), until), other.seeding_forecast(genotype(n, [1]), until)
        for name in FIELDS + ("next",):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name


def test_host_cohort_solves_duplicates_once_and_scatters(monkeypatch):
    n = 6
    mod = model(n, seed=6)
    G = np.array([genotype(n, [0, 1]), genotype(n, []), genotype(n, [0, 1]), genotype(n, range(n)), genotype(n, [])])
    calls = []
    one = MetMHN.seeding_forecast
    monkeypatch.setattr(MetMHN, "seeding_forecast", lambda self, g, until="seeding": calls.append(1) or one(self, g, until))
    got = mod.seeding_forecasts(G, "observation", backend="host")
    assert len(calls) == 3 and isinstance(got, SeedingForecasts)
    for i, g in enumerate(G):
        ref = one(mod, g, "observation")
        for name in FIELDS + ("next",):
            assert np.array_equal(getattr(got, name)[i], getattr(ref, name), equal_nan=True), (i, name)
    assert np.array_equal(got.expected_new_events(), np.nansum(got.before, axis=1))
    assert got.expected_new_events()[3] == 0.0
    empty = mod.seeding_forecasts(np.zeros((0, n), dtype=np.int8), backend="host")
    assert empty.p_seed.shape == (0,) and empty.before.shape == (0, n) and empty.next.shape == (0, n + 1)


def test_cohort_wrapper(monkeypatch):
    """Types 0 / 1 / 4 get the forecast of their PT genotype, 2 and 3 NaN; next to it met_status_posterior's column."""
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
    got, seeded = ro.seeding_forecast(lt, dp, dm, dat, backend="host")
    assert isinstance(got, SeedingForecasts) and got.p_seed.shape == (7,) and got.before.shape == (7, n)
    assert np.array_equal(seeded, host_status(lt, dp, dm, dat), equal_nan=True)
    mod = MetMHN(lt, dp, dm)
    for i in (0, 1, 2, 6):
        ref = mod.seeding_forecast(dat[i, 0:2 * n:2], "observation")
        for name in FIELDS + ("next",):
            assert np.array_equal(getattr(got, name)[i], getattr(ref, name), equal_nan=True), (i, name)
    for name in FIELDS + ("next",):
        assert np.isnan(getattr(got, name)[3:6]).all(), name
    assert np.isnan(seeded[3:6]).all() and np.isfinite(seeded[[0, 1, 2, 6]]).all()
    only, _ = ro.seeding_forecast(lt, dp, dm, paired, backend="host")
    assert np.isnan(only.p_seed).all()


# ------------------------------------------------------------------------------------------------------------------ GPU
@functools.lru_cache(maxsize=None)
def _host(n, seed, key, until):
    return frozen(model(n, seed=seed).seeding_forecast(np.frombuffer(key, dtype=np.int8), until))


def host(n, seed, g, until):
    return _host(n, seed, np.ascontiguousarray(g, dtype=np.int8).tobytes(), until)


def against_host(tag, n, seed, G, until, dev, mod=None, ref=None):
    """dev = (p_seed, time, before, with_seed, n_before) arrays over the rows G against the host definition."""
    mod = mod or model(n, seed=seed)
    worst = 0.0
    for i, g in enumerate(G):
        f = int((g == 0).sum())
        r = ref[i] if ref is not None else host(n, seed, g, until)
        b = forecast_bound(mod, f)
        for name, a in zip(FIELDS, dev):
            worst = max(worst, rel(a[i], getattr(r, name)) / b)
    note(f"{tag}, until {until}, {len(G)} rows", worst)


def shape_rows():
    """(n, seed, genotypes): f = 0, 1, 5, 6, 7 (a chunk below, at and above a wave), 10, 11 (one chunk, two), 13, 15, 17
    (several workgroups per row, chunks idle on a level) with held events, the whole model free at n = 7, 11, 17, and
    n_mut = 31 with 14, 17 and 20 events held, event 30 among them."""
    rng = np.random.default_rng(17)
    out = []
    n = 17
    out.append((n, 1, np.array([genotype(n, rng.choice(n, size=n - f, replace=False)) for f in (0, 1, 5, 6, 7, 10, 11, 13, 15, 17)])))
    for n in (7, 11):
        out.append((n, 2, genotype(n, [])[None, :]))
    n = 31
    out.append((n, 3, np.array([genotype(n, list(rng.choice(n - 1, size=h - 1, replace=False)) + [30]) for h in (14, 17, 20)])))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("until", UNTIL)
def test_shapes(until):
    from metmhn_amd.jx import engine
    for n, seed, G in shape_rows():
        mod = model(n, seed=seed)
        *dev, status = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, G, until)
        assert (status == 0).all(), status
        against_host(f"shapes n = {n}", n, seed, G, until, dev)


def mixed_rows(n=16):
    rng = np.random.default_rng(5)
    fs = (12, 3, 14, 0, 11, 14, 7, 13, 10, 1)                      # not sorted by f
    G = [genotype(n, rng.choice(n, size=n - f, replace=False)) for f in fs]
    G += [G[2], G[0], G[2]]                                        # duplicates in the call
    return np.array(G)


@pytest.mark.gpu
def test_mixed_widths_duplicates_one_row_and_none():
    from metmhn_amd.jx import engine
    n, seed = 16, 4
    mod, G = model(n, seed=seed), mixed_rows()
    eng = engine(n)
    for until in UNTIL:
        *dev, status = eng.seeding_forecasts(mod.log_theta, mod.obs1, G, until)
        assert (status == 0).all()
        against_host("mixed widths", n, seed, G, until, dev)
        for a in dev:
            assert a[10].tobytes() == a[2].tobytes() == a[12].tobytes() and a[11].tobytes() == a[0].tobytes()
        *one, st1 = eng.seeding_forecasts(mod.log_theta, mod.obs1, G[2:3], until)
        assert st1.tolist() == [0] and all(a[0].tobytes() == b[2].tobytes() for a, b in zip(one, dev))
    *none, st0 = eng.seeding_forecasts(mod.log_theta, mod.obs1, np.zeros((0, n), dtype=np.int8), "seeding")
    assert st0.shape == (0,) and none[2].shape == (0, n) and none[4].shape == (0, n + 1)
    # the Python layer: duplicates solved once, scattered back, the host's `next`
    got = mod.seeding_forecasts(G, "observation")
    ref = mod.seeding_forecasts(G, "observation", backend="host")
    *dev, _ = eng.seeding_forecasts(mod.log_theta, mod.obs1, G, "observation")
    for name, a in zip(FIELDS, dev):
        assert getattr(got, name).tobytes() == a.tobytes(), name
    assert np.array_equal(got.next, ref.next, equal_nan=True)
    assert mod.seeding_forecasts(np.zeros((0, n), dtype=np.int8)).p_seed.shape == (0,)


@pytest.mark.gpu
def test_batching_keeps_every_bit(monkeypatch):
    from metmhn_amd import jx
    from metmhn_amd.engine import Engine
    n, seed = 17, 1
    mod = model(n, seed=seed)
    rng = np.random.default_rng(8)
    fs = (15, 13, 15, 14, 15, 12, 15, 15, 6, 14, 15, 15, 15)       # 8 B x 2^15 = 256 KiB a row: three to a MiB
    G = np.array([genotype(n, rng.choice(n, size=n - f, replace=False)) for f in fs])
    need = sum(8 << f for f in fs)
    assert need > 2 * (1 << 20)                                    # the lattices alone: three batches or more under 1 MiB
    args = (mod.log_theta, mod.obs1)
    *whole, status = jx.engine(n).seeding_forecasts(*args, G, "observation")
    assert (status == 0).all()
    with Engine(n, workspace_bytes=1 << 20) as small:
        *cut, st = small.seeding_forecasts(*args, G, "observation")
        assert (st == 0).all()
        for a, b in zip(cut, whole):
            assert a.tobytes() == b.tobytes()
        perm = np.random.default_rng(9).permutation(len(G))
        *mixed, st = small.seeding_forecasts(*args, G[perm], "observation")
        for a, b in zip(mixed, whole):
            assert a.tobytes() == b[perm].tobytes()
        # a row that does not fit on its own: its status, the others finished
        big = np.vstack((G[:3], genotype(n, [])[None, :], G[3:5]))          # f = 17: 1 MiB of lattice and its partials
        *out, st = small.seeding_forecasts(*args, big, "observation")
        assert st.tolist() == [0, 0, 0, 3, 0, 0]
        for a, b in zip(out, whole):
            assert np.isnan(a[3]).all() and a[[0, 1, 2, 4, 5]].tobytes() == b[:5].tobytes()
        monkeypatch.setattr(jx, "engine", lambda n_mut, dtype="f64": small)
        with pytest.raises(ValueError, match=r"^row 3: 17 free mutations.*1048576 bytes"):
            mod.seeding_forecasts(big, "observation")


@pytest.mark.gpu
def test_two_calls_same_bytes():
    from metmhn_amd.jx import engine
    n, seed = 16, 4
    mod, G = model(n, seed=seed), mixed_rows()
    for until in UNTIL:
        a = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, G, until)
        b = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, G, until)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.gpu
def test_output_layout_statuses_and_identities():
    from metmhn_amd.jx import engine
    n, seed = 16, 4
    mod, G = model(n, seed=seed), mixed_rows().copy()
    G[4, 3] = 2                                                    # an entry other than 0 / 1
    G[7, 0] = -1
    good = np.ones(len(G), dtype=bool)
    good[[4, 7]] = False
    for until in UNTIL:
        p_seed, time, before, with_seed, n_before, status = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, G, until)
        assert (status[good] == 0).all() and (status[~good] == (2 | 8 << 16)).all()
        for a in (p_seed, time, before, with_seed, n_before):
            assert np.isnan(a[~good]).all()
        held = G[good] == 1
        assert (np.isnan(before[good]) == held).all() and (np.isnan(with_seed[good]) == held).all()
        assert np.isfinite(p_seed[good]).all() and np.isfinite(time[good]).all() and np.isfinite(n_before[good]).all()
        r = SeedingForecasts(p_seed[good], time[good], before[good], with_seed[good], n_before[good],
                             mod._forecast_next(G[good].astype(np.int64), until))
        f = (G[good] == 0).sum(axis=1)
        for i, fi in enumerate(f):
            assert (n_before[good][i, fi + 1:] == 0.0).all()
        # each side of an identity is one output within its bound of the exact value (twice for a sum of f of them)
        check_identities(mod, G[good], until, r, np.array([4 * forecast_bound(mod, int(fi)) for fi in f]))
    with pytest.raises(ValueError, match=r"^row 4: "):
        mod.seeding_forecasts(G)
    th = mod.log_theta.copy()
    th[n, n] = -1e10
    with pytest.raises(RuntimeError, match="without exit"):
        engine(n).seeding_forecasts(th, mod.obs1, G[:1], "seeding")
    th = mod.log_theta.copy()
    th[5, 5] = -1e10                                               # a mutation that never arises
    dead = MetMHN(th, mod.obs1, mod.obs2)
    rows = G[good][G[good][:, 5] == 0]
    got = dead.seeding_forecasts(rows, "observation")
    assert (got.before[:, 5] == 0.0).all() and (got.with_seed[:, 5] == 0.0).all()
    assert (np.isnan(got.before) == (rows == 1)).all() and np.isfinite(got.p_seed).all() and np.isfinite(got.time).all()


@pytest.mark.gpu
def test_luad_fullest_genotypes(golden):
    """The 20 distinct primary-tumour genotypes of LUAD-28 with the most events, at the fixture's fitted parameters."""
    from metmhn_amd.jx import engine
    d = golden("luad28")
    mod = MetMHN(d["fit_theta"], d["fit_dp"], d["fit_dm"])
    n = mod.n
    pts = np.unique(d["dat"][np.isin(d["dat"][:, -1], (0, 1, 3, 4))][:, 0:2 * n:2], axis=0)
    pts = pts[np.argsort(-pts.sum(axis=1), kind="stable")][:20]
    pts = pts[n - pts.sum(axis=1) <= 18].astype(np.int8)
    f = n - pts.sum(axis=1)
    print(f"{len(pts)} genotypes, f = {f.min()} .. {f.max()}")
    assert len(pts) > 0
    for until in UNTIL:
        ref = [mod.seeding_forecast(g, until) for g in pts]
        *dev, status = engine(n).seeding_forecasts(mod.log_theta, mod.obs1, pts, until)
        assert (status == 0).all()
        against_host("LUAD-28", n, None, pts, until, dev, mod=mod, ref=ref)
