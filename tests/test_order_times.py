"""Posterior event and observation times (MetMHN.order_time / order_times, mmhn_order_times, OrderTimes.relative /
cohort_mean).

Anchors:
  * the host sums over the lattice against an explicit enumeration of every path - an order together with the point at
    which the first observation falls -, walked with a clock that adds 1 / den of every state held.  The enumerators take
    their factors from the tables alone (_single_tables, _paired_tables), and the summed path probability of every order is
    MetMHN.likelihood of that order (pinned to the reference by tests/golden/orders.npz);
  * identities: an "unknown" diagnosis order is the mixture of "PT" and "Met" with the weight pt_first; the seeding precedes
    the first observation, that the second, and every event the last observation;
  * the device kernel against the host code; on rows too slow for a live comparison with it (k >= 15) against the host
    values of tests/golden/orders_big.npz on a selection of them, and on all of them the identities and order_posteriors'
    evidence.
What order_times shares with the other cohort entry points: order_common.check_*.

Bars: those of tests/test_order_posteriors.py, where they are derived.  1e-12 relative on exp(log_evidence); times and
observation times 1e-12 relative to the row's last observation time (every time is a sum of non-negative terms that the
last observation time bounds); pt_first 1e-12 absolute; NaN patterns equal.  The orderings are sums of the same non-negative
terms taken over nested sets of states, but by trees of different shapes: they hold up to the same 1e-12 of the last
observation time.  Every test prints the worst value it saw before it asserts.
"""
import functools
import itertools
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from metmhn_amd import _lib
from metmhn_amd.model import OrderTimes
from metmhn_amd.state import MetState
from order_common import (BAR, Row, big_models, check_arguments_before_the_library, check_big_rows, check_errors_name_the_row,
                          check_too_large_rows_get_the_host_value, error_rows, host_only, large_rows, luad, luad_selection,
                          last_observation, model, random_paired_states, small_shapes_n8, times_diff, times_orderings, too_large_cohort_k14)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = SimpleNamespace(cohort="order_times", single="order_time", engine="order_times",
                        symbol="mmhn_order_times", n_args=12, fallback="times_fallback_rows",
                        fields=("time", "obs", "pt_first"), extra=lambda *a: (),
                        error_good=lambda n: error_rows(n)[0], too_large=too_large_cohort_k14,
                        workspace=1 << 20, luad=("fit", luad_selection))
FIRST_OBS = ("PT", "Met", "unknown", "sync")


# ---------------------------------------------------------------------------------------------------- enumeration
def _single_paths(mod, state, status):
    """(evidence, OrderTime-like, summed likelihood) of a one-tumour observation by a walk of every permutation with a
    clock: 1 / den of the state held is added, a slot's time is the clock when it enters; probabilities as _single_walk."""
    n = mod.n
    chain, st = mod._route(state, status, None)
    mt = chain == "mt"
    T = mod._single_tables(mod.log_theta if mt else mod._pt_log_theta, st, mod.obs2 if mt else mod.obs1)
    codes = [2 * n if e == n else 2 * e + mt for e in T.ev]
    Z, Zl, obs, when = 0.0, 0.0, 0.0, np.zeros(T.k)
    for perm in itertools.permutations(range(T.k)):
        x, p, t = 0, 1.0 / T.den[0], 1.0 / T.den[0]
        enter = np.zeros(T.k)
        for b in perm:
            enter[b] = t
            x |= 1 << b
            p *= T.num[b][x] / T.den[x]
            t += 1.0 / T.den[x]
        p *= T.final
        Z, obs, when = Z + p, obs + p * t, when + p * enter
        Zl += mod.likelihood([codes[b] for b in perm], status)
    time = np.full(2 * n + 1, np.nan)
    time[codes] = when / Z
    return SimpleNamespace(log_evidence=np.log(Z), time=time, obs=np.array([obs / Z, np.nan]), pt_first=np.nan), Zl


def _paired_paths(T):
    """Every path of a paired row from the tables of _paired_tables alone: joint moves, the seeding, seeded moves with no
    observation made, the first observation at an admissible state, moves of the remaining tumour under its own den, the
    last observation.  Yields (order, probability, slot -> time it entered, first observation time, second, "P" / "M" /
    "S": the primary tumour or the metastasis observed first, or both at once)."""
    k = T.k
    top, full = 1 << (k - 1), (1 << k) - 1
    out, when, order = [], {}, []

    def alone(x, p, t, t1, den, kind, fin, tag):
        if x == full:
            out.append((tuple(order), p * fin[full], dict(when), t1, t, tag))
            return
        for b in range(k - 1):
            if not x >> b & 1 and T.kind[b] == kind:
                y = x | 1 << b
                when[b] = t
                order.append(T.slots[b])
                alone(y, p * T.num[b][y] / den[y], t + 1.0 / den[y], t1, den, kind, fin, tag)
                order.pop()

    def seeded(x, p, t):
        if T.pt_first and x & T.pt_mask == T.pt_mask:
            alone(x, p * T.o1[x] / T.den_mt[x], t + 1.0 / T.den_mt[x], t, T.den_mt, 1, T.o2, "P")
        if T.mt_first and x & T.mt_mask == T.mt_mask:
            alone(x, p * T.o2[x] / T.den_pt[x], t + 1.0 / T.den_pt[x], t, T.den_pt, 0, T.o1, "M")
        if T.sync and x == full:
            out.append((tuple(order), p * (T.o1[full] + T.o2[full]), dict(when), t, t, "S"))
        for b in range(k - 1):
            if not x >> b & 1:
                y = x | 1 << b
                when[b] = t
                order.append(T.slots[b])
                seeded(y, p * T.num[b][y] / T.den[y], t + 1.0 / T.den[y])
                order.pop()

    def unseeded(x, p, t):
        for b in range(k - 1):
            if T.joint >> b & 1 and not x >> b & 1:
                y = x | 3 << b
                when[b] = when[b + 1] = t
                order.extend((T.slots[b], T.slots[b + 1]))
                unseeded(y, p * T.num[b][y] / T.den[y], t + 1.0 / T.den[y])
                del order[-2:]
        y = x | top
        when[k - 1] = t
        order.append(T.slots[k - 1])
        seeded(y, p * T.num[k - 1][y] / T.den[y], t + 1.0 / T.den[y])
        order.pop()

    unseeded(0, 1.0 / T.den[0], 1.0 / T.den[0])
    return out


def _paired_enumeration(mod, state, first):
    """(OrderTime-like, worst relative difference of an order's summed path probability to MetMHN.likelihood)."""
    n = mod.n
    T = mod._paired_tables(state, first)
    paths = _paired_paths(T)
    Z = sum(p for _, p, *_ in paths)
    slot, t1, t2, pt, per_order = np.zeros(T.k), 0.0, 0.0, 0.0, {}
    for order, p, when, a, b, tag in paths:
        slot += p * np.array([when[d] for d in range(T.k)])
        t1, t2, pt = t1 + p * a, t2 + p * b, pt + p * (tag == "P")
        per_order[order] = per_order.get(order, 0.0) + p
    # (likelihood builds the tables of the order's state anew for every order: the orders of one state share them here)
    tables, build = {}, mod._paired_tables
    mod._paired_tables = lambda st, fo: tables[tuple(st), fo] if (tuple(st), fo) in tables else tables.setdefault(
        (tuple(st), fo), build(st, fo))
    worst = 0.0
    try:
        for order, p in per_order.items():
            lik = mod.likelihood(order, "isPaired", first)
            worst = max(worst, abs(p - lik) / lik)
    finally:
        del mod._paired_tables
    assert len(tables) == 1
    time = np.full(2 * n + 1, np.nan)
    time[T.slots] = slot / Z
    want = SimpleNamespace(log_evidence=np.log(Z), time=time, obs=np.array([t1 / Z, t2 / Z]),
                           pt_first=np.nan if first == "sync" else pt / Z)
    return want, worst


@functools.lru_cache(maxsize=None)
def _paired_cases(n):
    """The random paired states of the CPU tests with their host results under every first_obs, computed once:
    [(model, slots with the seeding, {first_obs: OrderTime})], and the events seen.  Called under host_only."""
    cases = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for mod, slots, seen in random_paired_states(n, 40 + n, (200 + 10 * n, 201 + 10 * n), 8):
            state = MetState(slots + [2 * n], size=2 * n + 1)
            cases.append((mod, slots + [2 * n], {f: mod.order_time(state, "isPaired", f) for f in FIRST_OBS}))
    return cases, dict(seen)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [4, 5])
def test_one_tumour_rows_against_enumeration(n, host_only):
    """order_time of "isMetastasis", "present" and "absent" states, k <= 6, against every permutation walked with a clock."""
    rng = np.random.default_rng(70 + n)
    S, results = 2 * n, []
    for seed in range(2):
        mod = model(n, seed=300 + 10 * n + seed)
        todo = [([S], "isMetastasis"), ([S], "present"), ([], "absent"), (list(range(0, 2 * n, 2))[:5] + [S], "present"),
                (list(range(0, 2 * n, 2))[:5] + [S], "isMetastasis"), (list(range(0, 2 * n, 2)), "absent")]
        for _ in range(4):
            ev = [2 * i for i in range(n) if rng.random() < 0.6]
            todo += [(ev + [S], "isMetastasis"), (ev + [S], "present"), (ev, "absent")]
        for sl, status in todo:
            assert len(sl) <= 6
            state = MetState([s + 1 if status == "isMetastasis" and s != S else s for s in sl], size=2 * n + 1)
            got = mod.order_time(state, status)
            want, Zl = _single_paths(mod, state, status)
            results.append((got, want, abs(np.exp(want.log_evidence) - Zl) / Zl, (sl, status)))
    worst = np.max([times_diff(got, want) + (dl,) for got, want, dl, _ in results], axis=0)
    print(f"one-tumour rows against enumeration, n = {n}: {len(results)} cases, worst evidence {worst[0]:.2e}, times "
          f"{worst[1]:.2e}, enumerated evidence against the summed likelihood {worst[3]:.2e}")
    for got, want, dl, tag in results:
        assert got.time.shape == (2 * n + 1,) and got.obs.shape == (2,), tag
        assert np.isnan(got.obs[1]) and np.isnan(got.pt_first), tag
        assert dl <= BAR, tag
        d = times_diff(got, want)
        assert d[0] <= BAR and d[1] <= BAR, (tag, d)
    assert len(results) == 2 * 18


@pytest.mark.parametrize("n", [4, 5])
def test_paired_rows_against_enumeration(n, host_only):
    """Random paired states with k <= 7, all four first_obs values, against the explicit paths; every order's summed path
    probability is MetMHN.likelihood's; events only in the PT, only in the MT and in both must all occur."""
    cases, seen = _paired_cases(n)
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for mod, slots, got in cases:
            for first in FIRST_OBS:
                want, dl = _paired_enumeration(mod, MetState(slots, size=2 * n + 1), first)
                results.append((got[first], want, dl, (slots, first)))
    worst = np.max([times_diff(got, want) + (dl,) for got, want, dl, _ in results], axis=0)
    print(f"paired rows against enumeration, n = {n}: {len(results)} cases, events {seen}, worst evidence {worst[0]:.2e}, "
          f"times {worst[1]:.2e}, pt_first {worst[2]:.2e}, an order's paths against its likelihood {worst[3]:.2e}")
    for got, want, dl, tag in results:
        assert got.time.shape == (2 * n + 1,) and got.obs.shape == (2,), tag
        assert dl <= BAR, tag
        d = times_diff(got, want)
        assert d[0] <= BAR and d[1] <= BAR and d[2] <= BAR, (tag, d)
    assert len(results) == 2 * 8 * 4
    assert min(seen.values()) > 0


def _mixture(pt, met, unk):
    """Residuals of the mixture identity of one row's results under "PT", "Met" and "unknown": (evidence, relative;
    pt_first, absolute; time and obs, over the last observation time)."""
    zp, zm, zu = (np.exp(r.log_evidence) for r in (pt, met, unk))
    p = zp / zu
    last = last_observation(unk.obs)
    d_time = np.abs(p * pt.time + (1.0 - p) * met.time - unk.time)
    d = max(d_time[~np.isnan(d_time)].max(), np.abs(p * pt.obs + (1.0 - p) * met.obs - unk.obs).max()) / last
    return abs(zp + zm - zu) / zu, abs(unk.pt_first - p), d


@pytest.mark.parametrize("n", [4, 5])
def test_unknown_is_the_mixture_of_pt_and_met(n, host_only):
    cases, _ = _paired_cases(n)
    res = [_mixture(got["PT"], got["Met"], got["unknown"]) for _, _, got in cases]
    print(f"mixture identity, n = {n}: {len(res)} states, worst (evidence, pt_first, times) {np.max(res, axis=0)}")
    for (_, slots, got), r in zip(cases, res):
        assert got["PT"].pt_first == 1.0 and got["Met"].pt_first == 0.0, slots
        assert np.isnan(got["sync"].pt_first), slots
        assert got["sync"].obs[0] == got["sync"].obs[1], slots
        assert max(r) <= BAR, (slots, r)


@pytest.mark.parametrize("n", [4, 5])
def test_orderings(n, host_only):
    """The seeding before the first observation, that before the second, a code of one tumour alone after the seeding,
    every event before the last observation."""
    cases, _ = _paired_cases(n)
    worst = 0.0
    for _, slots, got in cases:
        r = np.zeros(2 * n + 3, dtype=np.int8)
        r[slots], r[-1] = 1, 3
        for first in FIRST_OBS:
            g = got[first]
            worst = max(worst, times_orderings(g.time[None], g.obs[None], r[None], n))
    print(f"orderings, n = {n}: {4 * len(cases)} cases, worst violation over the last observation time {worst:.2e}")
    assert worst <= BAR


def test_relative_and_cohort_mean():
    nan = np.nan
    time = np.array([[1.0, nan, 2.0, nan, 0.5], [nan, nan, 3.0, nan, nan], [2.0, nan, nan, nan, 1.0]])
    obs = np.array([[2.0, 4.0], [6.0, nan], [4.0, 8.0]])
    run = OrderTimes(np.zeros(3), time, obs, np.array([0.25, nan, 1.0]))
    want_last = time / np.array([4.0, 6.0, 8.0])[:, None]
    want_first = time / np.array([2.0, 6.0, 4.0])[:, None]
    print(f"summaries: relative {run.relative().tolist()}, cohort mean {run.cohort_mean().tolist()}")
    np.testing.assert_array_equal(run.relative(), want_last)
    np.testing.assert_array_equal(run.relative("last"), want_last)
    np.testing.assert_array_equal(run.relative("first"), want_first)
    np.testing.assert_array_equal(run.cohort_mean(), [(0.25 + 0.25) / 2, nan, (0.5 + 0.5) / 2, nan, (0.125 + 0.125) / 2])
    np.testing.assert_array_equal(run.cohort_mean("first"), [0.5, nan, (1.0 + 0.5) / 2, nan, 0.25])
    for call in (run.relative, run.cohort_mean):
        with pytest.raises(ValueError, match="^to must be 'first' or 'last'$"):
            call("second")
    assert "ratio of two expectations" in " ".join(OrderTimes.relative.__doc__.split())


def test_arguments_are_checked_before_the_library(monkeypatch):
    mod = check_arguments_before_the_library(ENTRY, monkeypatch)
    assert mod.times_fallback_rows == 0                            # the counter is there before the first call


def test_abi_carries_the_symbol_and_version_8():
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert ENTRY.symbol in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[ENTRY.symbol]) == ENTRY.n_args == 12
    assert re.search(r"\bint %s\s*\(" % ENTRY.symbol, hdr)
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define MMHN_ABI_VERSION (\d+)", hdr).group(1))


# ---------------------------------------------------------------------------------------------------- GPU
def _host(mod, dat):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return mod.order_times(dat, backend="host")


@pytest.mark.gpu
def test_device_against_host_small_shapes():
    mod, dat = small_shapes_n8()
    n = mod.n
    k = dat[:, :-2].astype(int).sum(1)
    ks = set(int(v) for v in k)
    dev = mod.order_times(dat)
    assert mod.times_fallback_rows == 0
    host = _host(mod, dat)
    assert dev.time.shape == host.time.shape == (len(dat), 2 * n + 1)
    assert dev.obs.shape == host.obs.shape == (len(dat), 2) and dev.pt_first.shape == host.pt_first.shape == (len(dat),)
    carried = np.zeros(dev.time.shape, dtype=bool)
    for i, r in enumerate(dat):
        carried[i, Row(r, n).codes] = True
    paired = dat[:, -1] == 3
    d = times_diff(dev, host)
    print(f"device against host, small shapes: {len(dat)} rows, k in {sorted(ks)}, worst rel. evidence {d[0]:.2e}, times "
          f"{d[1]:.2e}, pt_first {d[2]:.2e}, orderings {times_orderings(dev.time, dev.obs, dat, n):.2e}")
    assert ks >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11}
    np.testing.assert_array_equal(~np.isnan(dev.time), carried)
    np.testing.assert_array_equal(~np.isnan(dev.obs), np.stack((np.ones(len(dat), dtype=bool), paired), axis=1))
    np.testing.assert_array_equal(~np.isnan(dev.pt_first), paired)
    assert np.all(dev.pt_first[paired & (dat[:, -2] == 1)] == 1.0)
    assert np.all(dev.pt_first[paired & (dat[:, -2] != 0) & (dat[:, -2] != 1)] == 0.0)
    assert max(d) <= BAR
    assert times_orderings(dev.time, dev.obs, dat, n) <= BAR


def _three_orders(dat):
    """Every paired row of dat with the diagnosis orders 0, 1 and 2 one behind the other, then the other rows."""
    rows = []
    for r in dat[dat[:, -1] == 3]:
        for d in (0, 1, 2):
            rows.append(r.copy())
            rows[-1][-2] = d
    return np.array(rows + list(dat[dat[:, -1] != 3])), len(rows) // 3


@pytest.mark.gpu
def test_large_synthetic_rows():
    """Paired rows with k = 14 ... 17 (n = 9) under all three diagnosis orders and one-tumour rows with k = 14 ... 17
    (n = 16), both sides of the 1024-thread switch at 15 slots: the mixture identity, the orderings, order_posteriors'
    evidence; the rows with k = 14 against the host code."""
    for n, seed, tag in ((9, 31, "synthetic n = 9"), (16, 32, "one tumour n = 16")):
        mod = model(n, seed=seed)
        dat, triples = _three_orders(large_rows(n))
        k = dat[:, :-2].astype(int).sum(1)
        got = mod.order_times(dat)
        assert mod.times_fallback_rows == 0
        post = mod.order_posteriors(dat)
        row = lambda i: SimpleNamespace(log_evidence=got.log_evidence[i], time=got.time[i], obs=got.obs[i],
                                        pt_first=got.pt_first[i])
        mix = [_mixture(row(3 * j + 1), row(3 * j + 2), row(3 * j)) for j in range(triples)]
        d_le = np.abs(np.expm1(got.log_evidence - post.log_evidence)).max()
        order = times_orderings(got.time, got.obs, dat, n)
        k14 = np.flatnonzero(k == 14)
        host = _host(mod, dat[k14])
        d = times_diff(OrderTimes(got.log_evidence[k14], got.time[k14], got.obs[k14], got.pt_first[k14]), host)
        print(f"large rows, {tag}: {len(dat)} rows, k = {sorted(set(k.tolist()))}, mixture (evidence, pt_first, times) "
              f"{np.max(mix, axis=0) if mix else None}, orderings {order:.2e}, evidence against order_posteriors "
              f"{d_le:.2e}, {len(k14)} rows with k = 14 against the host {d}")
        assert (k >= 15).any() and len(k14) >= 3
        for j in range(triples):
            assert got.pt_first[3 * j + 1] == 1.0 and got.pt_first[3 * j + 2] == 0.0
        assert triples == (6 if n == 9 else 0)
        assert max((max(m) for m in mix), default=0.0) <= BAR
        assert order <= BAR and d_le <= BAR and max(d) <= BAR


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The rows of tests/golden/orders_big.npz, k = 15 ... 21: every one on the device (the 1 024-thread instantiation),
    every field at BAR against the host values the fixture holds, times over the row's last observation time as in _diff."""
    device = {}
    for name, m in big_models():
        device[name] = m.mod.order_times(m.dat)
        assert m.mod.times_fallback_rows == 0
    check_big_rows("order_times", device, BAR)


@pytest.mark.gpu
def test_luad_rows(golden):
    """LUAD-28 at the fit point: the 71 rows with k >= 15 (k = 21 among them), 300 rows with k <= 12 and up to 200 with
    k = 13, 14: the orderings, and order_posteriors' evidence."""
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    le, time, obs, pt_first, status = engine(mod.n).order_times(mod.log_theta, mod.obs1, mod.obs2, dat)
    assert np.all(status == 0)
    assert (k >= 15).sum() == 71 and k.max() == 21
    post = mod.order_posteriors(dat)
    assert mod.posteriors_fallback_rows == 0
    d_le = np.abs(np.expm1(le - post.log_evidence)).max()
    order = times_orderings(time, obs, dat, mod.n)
    paired = dat[:, -1] == 3
    print(f"LUAD-28 fit: {len(dat)} rows, k up to {k.max()}, evidence against order_posteriors {d_le:.2e}, orderings "
          f"{order:.2e}, pt_first in [{np.nanmin(pt_first):.3f}, {np.nanmax(pt_first):.3f}]")
    for i, r in enumerate(dat):
        have = np.zeros(2 * mod.n + 1, dtype=bool)
        have[Row(r, mod.n).codes] = True
        assert np.array_equal(~np.isnan(time[i]), have), i
    np.testing.assert_array_equal(~np.isnan(pt_first), paired)
    assert np.all((pt_first[paired] >= 0.0) & (pt_first[paired] <= 1.0))
    assert np.all(time[~np.isnan(time)] > 0.0)
    assert d_le <= BAR and order <= BAR


@pytest.mark.gpu
def test_bitwise_reproducible_and_batching(golden):
    """The rows of LUAD-28 twice, then in another order through a small workspace, then with a row turned away."""
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    first = engine(mod.n).order_times(*args, dat)
    again = engine(mod.n).order_times(*args, dat)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
    keep = np.flatnonzero(k <= 16)
    assert k[keep].max() == 16 and (k[keep] >= 15).any()
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.8 MiB: many batches
        b = small.order_times(*args, dat[perm])
        for x, y in zip(first, b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        assert len(big) == 1
        *out, status = small.order_times(*args, np.vstack((dat[big], dat[keep[:5]])))
        assert status[0] == 3 and np.all(status[1:] == 0)
        for x, y in zip(first, out):
            assert np.all(np.isnan(y[0]))
            np.testing.assert_array_equal(y[1:], x[keep[:5]])
    print(f"bitwise: {len(dat)} rows twice, {len(perm)} permuted rows in batches of 8 MiB, one row turned away")


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """... with order_time: the k = 14 row (1.2 MiB, over the 1 MiB workspace), its host value against the device's."""
    mod, dat, ref, raw, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    for a in raw[:-1]:
        assert np.all(np.isnan(a[0]))
    d = times_diff(OrderTimes(ref.log_evidence[0], ref.time[0], ref.obs[0], ref.pt_first[0]), host)
    print(f"host fallback, k = 14: rel. evidence {d[0]:.2e}, times {d[1]:.2e}, pt_first {d[2]:.2e} against the device")
    assert max(d) <= BAR


@pytest.mark.gpu
def test_errors_name_the_row():
    check_errors_name_the_row(ENTRY)
