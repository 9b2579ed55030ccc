"""Posterior genotypes at the first observation (MetMHN.order_snapshot / order_snapshots, mmhn_order_snapshots,
OrderSnapshots.cohort_late).

Anchors:
  * the host sums over the lattice against an explicit enumeration of every path - an order together with the point at which
    the first observation falls -, walked with a clock; the state at the first observation of a path is the set of slots
    that entered before it.  The enumerator takes its factors from the tables alone (_paired_tables);
  * identities: the late block sums to 1; its rows sum to held[r, seeding], and held[0, seeding] is order_time's pt_first;
    the mean number of late events equals the summed deficits of the other tumour's codes (two different reductions); an
    "unknown" diagnosis order is the mixture of "PT" and "Met"; the regime a diagnosis order excludes is exactly 0;
  * the device kernel against the host code; on rows too slow for a live comparison with it (k >= 15) against the host
    values of tests/golden/orders_big.npz on a selection of them, and on all of them the identities, order_posteriors'
    evidence and order_times' pt_first.
What order_snapshots shares with the other cohort entry points: order_common.check_*.

Bars: those of tests/test_order_posteriors.py, where they are derived.  1e-12 relative on exp(log_evidence); 1e-12 absolute
on held, late and map_prob - probabilities, sums of non-negative terms over the evidence; NaN / -1 patterns, map_first and
map_state equal.  Every test prints the worst value it saw before it asserts.
"""
import functools
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

from metmhn_amd import _lib
from metmhn_amd.model import OrderSnapshot, OrderSnapshots
from metmhn_amd.state import MetState
from order_common import (big_models, check_arguments_before_the_library, check_big_rows, check_errors_name_the_row,
                          check_too_large_rows_get_the_host_value, error_rows, host_only, large_rows, luad, luad_selection,
                          model, random_paired_states, small_shapes_n8, snapshots_diff, snapshots_patterns, too_large_cohort_k14, worst_entry)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = SimpleNamespace(cohort="order_snapshots", single="order_snapshot", engine="order_snapshots",
                        symbol="mmhn_order_snapshots", n_args=14, fallback="snapshots_fallback_rows",
                        fields=("held", "late", "map_state", "map_first", "map_prob"), extra=lambda *a: (),
                        error_good=lambda n: error_rows(n)[0], too_large=too_large_cohort_k14,
                        workspace=1 << 20, luad=("fit", luad_selection))
FIRST_OBS = ("PT", "Met", "unknown")
BAR = 1e-12


def _rows_of(run, idx):
    return OrderSnapshots(*(getattr(run, name)[idx] for name in ("log_evidence",) + ENTRY.fields))


def _one(run, i):
    return OrderSnapshot(*(getattr(run, name)[i] for name in ("log_evidence",) + ENTRY.fields))


def _others(dat_row, n):
    """Of a paired dat row: (the MT codes, the PT codes) - the codes of the OTHER tumour of regime 0 and of regime 1."""
    return ([2 * i + 1 for i in range(n) if dat_row[2 * i + 1]], [2 * i for i in range(n) if dat_row[2 * i]])


def _identities(s, others, n):
    """Residuals of one paired row's identities: (the late block sums to 1; late's rows sum to held[r, seeding]; the mean
    number of late events against the summed deficits of the other tumour's codes; held[r, c] = held[r, seeding] for the
    codes of tumour r; late past the other tumour's events, which must be exactly 0)."""
    S = 2 * n
    rows = max(abs(s.late[r].sum() - s.held[r, S]) for r in (0, 1))
    mean = max(abs(np.dot(np.arange(n + 1), s.late[r]) - sum(s.held[r, S] - s.held[r, c] for c in others[r])) for r in (0, 1))
    own = max([abs(s.held[r, c] - s.held[r, S]) for r in (0, 1) for c in others[1 - r]], default=0.0)
    past = max(np.abs(s.late[r, len(others[r]) + 1:]).max(initial=0.0) for r in (0, 1))
    return abs(s.late.sum() - 1.0), rows, mean, own, past


def _mixture(pt, met, unk):
    """Residuals of the mixture identity of one row's results under "PT", "Met" and "unknown": (evidence, relative; held;
    late; map_prob against the larger of the two weighted ones)."""
    zp, zm, zu = (np.exp(r.log_evidence) for r in (pt, met, unk))
    p = zp / zu
    d_held = max(worst_entry(np.abs(unk.held[0] - p * pt.held[0])), worst_entry(np.abs(unk.held[1] - (1.0 - p) * met.held[1])))
    d_late = max(np.abs(unk.late[0] - p * pt.late[0]).max(), np.abs(unk.late[1] - (1.0 - p) * met.late[1]).max())
    return abs(zp + zm - zu) / zu, d_held, d_late, abs(unk.map_prob - max(p * pt.map_prob, (1.0 - p) * met.map_prob))


def _excluded_is_zero(s, first):
    """The regime a diagnosis order excludes is exactly 0 (NaN where the code is not carried)."""
    out = {"PT": (1,), "Met": (0,), "unknown": ()}[first]
    return all(np.all(s.held[r][~np.isnan(s.held[r])] == 0.0) and np.all(s.late[r] == 0.0) for r in out) and \
        s.map_first not in out


# ---------------------------------------------------------------------------------------------------- enumeration
def _paired_paths(T):
    """Every path of a paired row from the tables of _paired_tables alone: joint moves, the seeding, seeded moves with no
    observation made, the first observation at an admissible state, moves of the remaining tumour under its own den, the
    last observation.  Yields (probability, slot -> time it entered, first observation time, 0 / 1: the primary tumour or
    the metastasis observed first)."""
    k = T.k
    top, full = 1 << (k - 1), (1 << k) - 1
    out, when = [], {}

    def alone(x, p, t, t1, den, kind, fin, r):
        if x == full:
            out.append((p * fin[full], dict(when), t1, r))
            return
        for b in range(k - 1):
            if not x >> b & 1 and T.kind[b] == kind:
                y = x | 1 << b
                when[b] = t
                alone(y, p * T.num[b][y] / den[y], t + 1.0 / den[y], t1, den, kind, fin, r)

    def seeded(x, p, t):
        if T.pt_first and x & T.pt_mask == T.pt_mask:
            alone(x, p * T.o1[x] / T.den_mt[x], t + 1.0 / T.den_mt[x], t, T.den_mt, 1, T.o2, 0)
        if T.mt_first and x & T.mt_mask == T.mt_mask:
            alone(x, p * T.o2[x] / T.den_pt[x], t + 1.0 / T.den_pt[x], t, T.den_pt, 0, T.o1, 1)
        for b in range(k - 1):
            if not x >> b & 1:
                y = x | 1 << b
                when[b] = t
                seeded(y, p * T.num[b][y] / T.den[y], t + 1.0 / T.den[y])

    def unseeded(x, p, t):
        for b in range(k - 1):
            if T.joint >> b & 1 and not x >> b & 1:
                y = x | 3 << b
                when[b] = when[b + 1] = t
                unseeded(y, p * T.num[b][y] / T.den[y], t + 1.0 / T.den[y])
        y = x | top
        when[k - 1] = t
        seeded(y, p * T.num[k - 1][y] / T.den[y], t + 1.0 / T.den[y])

    unseeded(0, 1.0 / T.den[0], 1.0 / T.den[0])
    return out


def _paired_enumeration(mod, state, first):
    """OrderSnapshot of a paired state from its paths: the state at the first observation of a path is the set of slots
    that entered before it."""
    n = mod.n
    T = mod._paired_tables(state, first)
    k, full = T.k, (1 << T.k) - 1
    masses = {}
    for p, when, t1, r in _paired_paths(T):
        x = sum(1 << d for d in range(k) if when[d] < t1)
        masses[r, x] = masses.get((r, x), 0.0) + p
    Z = sum(masses.values())
    slot, late = np.zeros((2, k)), np.zeros((2, n + 1))
    for (r, x), s in masses.items():
        slot[r, [d for d in range(k) if x >> d & 1]] += s
        late[r, bin(full ^ x).count("1")] += s
    (r, x), s = min(masses.items(), key=lambda kv: (-kv[1], kv[0]))
    held = np.full((2, 2 * n + 1), np.nan)
    held[:, T.slots] = slot / Z
    map_state = np.full(2 * n + 1, -1, dtype=np.int8)
    map_state[T.slots] = [x >> d & 1 for d in range(k)]
    return OrderSnapshot(np.log(Z), held, late / Z, map_state, r, s / Z)


@functools.lru_cache(maxsize=None)
def _paired_cases(n):
    """The random paired states of the CPU tests with their host results under every first_obs, computed once:
    [(model, slots with the seeding, {first_obs: OrderSnapshot})], and the events seen.  Called under host_only."""
    cases = []
    for mod, slots, seen in random_paired_states(n, 40 + n, (200 + 10 * n, 201 + 10 * n), 8):
        state = MetState(slots + [2 * n], size=2 * n + 1)
        cases.append((mod, slots + [2 * n], {f: mod.order_snapshot(state, "isPaired", f) for f in FIRST_OBS}))
    return cases, dict(seen)


def _dat_row(slots, n):
    r = np.zeros(2 * n + 3, dtype=np.int8)
    r[slots], r[-1] = 1, 3
    return r


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [4, 5])
def test_paired_rows_against_enumeration(n, host_only):
    """Random paired states with k <= 7 under "PT", "Met" and "unknown" against the explicit paths: per code, per late
    count and the most probable snapshot; events only in the PT, only in the MT and in both must all occur."""
    cases, seen = _paired_cases(n)
    results = []
    for mod, slots, got in cases:
        for first in FIRST_OBS:
            want = _paired_enumeration(mod, MetState(slots, size=2 * n + 1), first)
            results.append((got[first], want, (slots, first)))
    worst = np.max([snapshots_diff(got, want) for got, want, _ in results], axis=0)
    print(f"paired rows against enumeration, n = {n}: {len(results)} cases, events {seen}, worst evidence {worst[0]:.2e}, "
          f"held {worst[1]:.2e}, late {worst[2]:.2e}, map_prob {worst[3]:.2e}")
    for got, want, tag in results:
        assert got.held.shape == (2, 2 * n + 1) and got.late.shape == (2, n + 1) and got.map_state.shape == (2 * n + 1,), tag
        assert got.map_state.dtype == np.int8, tag
        assert max(snapshots_diff(got, want)) <= BAR, (tag, snapshots_diff(got, want))
    assert len(results) == 2 * 8 * 3
    assert min(seen.values()) > 0


@pytest.mark.parametrize("n", [4, 5])
def test_identities(n, host_only):
    """On the same states: the late block sums to 1, its rows to held[r, seeding], held[0, seeding] is order_time's
    pt_first, the mean number of late events is the summed deficit of the other tumour's codes, the codes of the observed
    tumour are held whenever it is observed, and the excluded regime is exactly 0."""
    cases, _ = _paired_cases(n)
    res, d_pt = [], 0.0
    for mod, slots, got in cases:
        state = MetState(slots, size=2 * n + 1)
        for first in FIRST_OBS:
            s = got[first]
            res.append(_identities(s, _others(_dat_row(slots, n), n), n))
            d_pt = max(d_pt, abs(s.held[0, 2 * n] - mod.order_time(state, "isPaired", first).pt_first))
            assert _excluded_is_zero(s, first), (slots, first)
            assert s.map_state[2 * n] == 1 and 0.0 < s.map_prob <= s.held[s.map_first, 2 * n], (slots, first)
    worst = np.max(res, axis=0)
    print(f"identities, n = {n}: {len(res)} cases, worst (block sum, row sums, mean late count, own codes, past the other "
          f"tumour) {worst}, held[0, seeding] against order_time's pt_first {d_pt:.2e}")
    assert worst[:4].max() <= BAR and worst[4] == 0.0 and d_pt <= BAR


@pytest.mark.parametrize("n", [4, 5])
def test_unknown_is_the_mixture_of_pt_and_met(n, host_only):
    cases, _ = _paired_cases(n)
    res = [_mixture(got["PT"], got["Met"], got["unknown"]) for _, _, got in cases]
    print(f"mixture identity, n = {n}: {len(res)} states, worst (evidence, held, late, map_prob) {np.max(res, axis=0)}")
    for (_, slots, got), r in zip(cases, res):
        assert got["PT"].map_first == 0 and got["Met"].map_first == 1, slots
        assert max(r) <= BAR, (slots, r)


def test_rows_without_a_first_observation(host_only):
    """"sync" and the one-tumour states: a valid evidence (order_posterior's), NaN / -1 everywhere else."""
    mod = model(5, seed=3)
    n = mod.n
    S = 2 * n
    todo = [(MetState([0, 1, 2, 5, S], size=S + 1), "isPaired", "sync"), (MetState([0, 4, 6], size=S + 1), "absent", None),
            (MetState([], size=S + 1), "absent", None), (MetState([2, 4, S], size=S + 1), "present", None),
            (MetState([1, 5, 9, S], size=S + 1), "isMetastasis", None), (MetState([S], size=S + 1), "isMetastasis", None)]
    worst = 0.0
    for args in todo:
        s = mod.order_snapshot(*args)
        worst = max(worst, abs(np.expm1(s.log_evidence - mod.order_posterior(*args).log_evidence)))
        assert np.all(np.isnan(s.held)) and s.held.shape == (2, S + 1), args[1:]
        assert np.all(np.isnan(s.late)) and s.late.shape == (2, n + 1), args[1:]
        assert np.all(s.map_state == -1) and s.map_state.shape == (S + 1,) and s.map_first == -1, args[1:]
        assert np.isnan(s.map_prob) and np.isfinite(s.log_evidence), args[1:]
    print(f"rows without a first observation: {len(todo)} states, worst evidence against order_posterior {worst:.2e}")
    assert worst <= BAR
    run = mod.order_snapshots(np.array([_dat_row([0, 1, 2, 5, S], n)] + [np.r_[np.zeros(S + 1), -99, 0].astype(np.int8)]),
                              backend="host")
    assert mod.snapshots_fallback_rows == 0
    assert run.map_state.dtype == np.int8 and run.map_first.dtype == np.int32
    assert run.map_first.tolist()[1] == -1 and run.map_first[0] in (0, 1) and np.all(np.isnan(run.held[1]))


def test_cohort_late():
    nan = np.nan
    # n = 2: codes 0 (PT of 0), 1 (MT of 0), 2 (PT of 1), 3 (MT of 1), 4 (the seeding)
    held = np.array([
        [[0.75, 0.5, nan, 0.25, 0.75], [0.125, 0.25, nan, 0.25, 0.25]],      # "unknown": 0 joint, 1 in the MT only
        [[nan, 0.5, 1.0, nan, 1.0], [nan, 0.0, 0.0, nan, 0.0]],              # "PT": 0 in the MT only, 1 in the PT only
        [[0.0, nan, 0.0, 0.0, 0.0], [0.25, nan, 1.0, 1.0, 1.0]],             # "Met": 0 in the PT only, 1 joint
        [[nan, nan, nan, nan, nan], [nan, nan, nan, nan, nan]],              # one tumour
        [[nan, 0.0, nan, nan, 0.0], [nan, 1.0, nan, nan, 1.0]]])             # "Met": 0 in the MT only - the first-observed one
    run = OrderSnapshots(np.zeros(5), held, np.zeros((5, 2, 3)), np.zeros((5, 5), dtype=np.int8),
                         np.zeros(5, dtype=np.int32), np.zeros(5))
    got = run.cohort_late()
    print(f"cohort_late: {got.tolist()}")
    # mutation 0: row 1 (1.0 - 0.5) and row 2 (1.0 - 0.25); mutation 1: row 0 (0.75 - 0.25); row 1 carries it in the
    # first-observed tumour only
    np.testing.assert_array_equal(got, [(0.5 + 0.75) / 2, 0.5])
    none = OrderSnapshots(np.zeros(1), held[3:4], np.zeros((1, 2, 3)), np.zeros((1, 5), dtype=np.int8),
                          np.zeros(1, dtype=np.int32), np.zeros(1))
    assert np.all(np.isnan(none.cohort_late()))
    doc = " ".join(OrderSnapshots.cohort_late.__doc__.split())
    assert "divided by nothing" in doc and "later-observed tumour only" in doc


def test_arguments_are_checked_before_the_library(monkeypatch):
    mod = check_arguments_before_the_library(ENTRY, monkeypatch)
    assert mod.snapshots_fallback_rows == 0                        # the counter is there before the first call


def test_abi_carries_the_symbol_and_version_8():
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert ENTRY.symbol in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[ENTRY.symbol]) == ENTRY.n_args == 14
    assert re.search(r"\bint %s\s*\(" % ENTRY.symbol, hdr)
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define MMHN_ABI_VERSION (\d+)", hdr).group(1))


# ---------------------------------------------------------------------------------------------------- GPU
def _host(mod, dat):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return mod.order_snapshots(dat, backend="host")


def _first_name(dat_row):
    return {0: "unknown", 1: "PT"}.get(int(dat_row[-2]), "Met")


def _paired_identities(run, dat, n):
    """Worst residuals of _identities over the paired rows of a cohort, the excluded regimes and the consistency of the
    chosen snapshot asserted row by row."""
    res = []
    for i in np.flatnonzero(dat[:, -1] == 3):
        s, others = _one(run, i), _others(dat[i], n)
        res.append(_identities(s, others, n))
        assert _excluded_is_zero(s, _first_name(dat[i])), i
        own = others[1 - s.map_first]
        assert s.map_state[2 * n] == 1 and np.all(s.map_state[own] == 1), i
        assert 0.0 < s.map_prob <= s.held[s.map_first, 2 * n], i
    return np.max(res, axis=0)


@pytest.mark.gpu
def test_device_against_host_small_shapes():
    """k = 0 ... 11, every diagnosis order, no joint event, only joint events, the three one-tumour types: every field at
    the bars, the patterns and the most probable snapshot equal on every row."""
    mod, dat = small_shapes_n8()
    n = mod.n
    k = dat[:, :-2].astype(int).sum(1)
    dev = mod.order_snapshots(dat)
    assert mod.snapshots_fallback_rows == 0
    host = _host(mod, dat)
    for name, shape in zip(ENTRY.fields, ((2, 2 * n + 1), (2, n + 1), (2 * n + 1,), (), ())):
        assert getattr(dev, name).shape == getattr(host, name).shape == (len(dat),) + shape, name
        assert getattr(dev, name).dtype == getattr(host, name).dtype, name
    d = snapshots_diff(dev, host)
    ident = _paired_identities(dev, dat, n)
    print(f"device against host, small shapes: {len(dat)} rows, k in {sorted(set(k.tolist()))}, worst rel. evidence "
          f"{d[0]:.2e}, held {d[1]:.2e}, late {d[2]:.2e}, map_prob {d[3]:.2e}, identities {ident}")
    assert set(k.tolist()) >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11}
    snapshots_patterns(dev, dat, n)
    assert (dat[:, -1] == 3).sum() == 52 and set(dev.map_first[dat[:, -1] == 3].tolist()) == {0, 1}
    assert max(d) <= BAR
    assert ident[:4].max() <= BAR and ident[4] == 0.0


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
    (n = 16), both sides of the 1024-thread switch at 15 slots: the mixture identity and the others, order_posteriors'
    evidence, order_times' pt_first; the rows with k = 14 against the host code."""
    for n, seed, tag in ((9, 31, "synthetic n = 9"), (16, 32, "one tumour n = 16")):
        mod = model(n, seed=seed)
        dat, triples = _three_orders(large_rows(n))
        k = dat[:, :-2].astype(int).sum(1)
        paired = dat[:, -1] == 3
        got = mod.order_snapshots(dat)
        assert mod.snapshots_fallback_rows == 0
        post = mod.order_posteriors(dat)
        times = mod.order_times(dat)
        assert mod.posteriors_fallback_rows == 0 and mod.times_fallback_rows == 0
        snapshots_patterns(got, dat, n)
        mix = [_mixture(_one(got, 3 * j + 1), _one(got, 3 * j + 2), _one(got, 3 * j)) for j in range(triples)]
        ident = _paired_identities(got, dat, n) if paired.any() else np.zeros(5)
        d_le = np.abs(np.expm1(got.log_evidence - post.log_evidence)).max()
        d_pt = worst_entry(np.abs(got.held[:, 0, 2 * n] - times.pt_first))
        np.testing.assert_array_equal(np.isnan(got.held[:, 0, 2 * n]), np.isnan(times.pt_first))
        k14 = np.flatnonzero(k == 14)
        d = snapshots_diff(_rows_of(got, k14), _host(mod, dat[k14]))
        print(f"large rows, {tag}: {len(dat)} rows, k = {sorted(set(k.tolist()))}, mixture (evidence, held, late, map_prob) "
              f"{np.max(mix, axis=0) if mix else None}, identities {ident}, evidence against order_posteriors {d_le:.2e}, "
              f"held[0, seeding] against order_times' pt_first {d_pt:.2e}, {len(k14)} rows with k = 14 against the host {d}")
        assert (k >= 15).any() and len(k14) >= 3
        assert triples == (6 if n == 9 else 0)
        assert max((max(m) for m in mix), default=0.0) <= BAR
        assert ident[:4].max() <= BAR and ident[4] == 0.0
        assert d_le <= BAR and d_pt <= BAR and max(d) <= BAR


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The rows of tests/golden/orders_big.npz, k = 15 ... 21: every one on the device (the 1 024-thread instantiation),
    held, late and map_prob at BAR against the host values the fixture holds; map_first and map_state equal, except on a
    row (one at the most) whose two best snapshots the host has within 1e-12 relative of each other."""
    device = {}
    for name, m in big_models():
        device[name] = m.mod.order_snapshots(m.dat)
        assert m.mod.snapshots_fallback_rows == 0
    check_big_rows("order_snapshots", device, BAR)


@pytest.mark.gpu
def test_luad_rows(golden):
    """LUAD-28 at the fit point: the 71 rows with k >= 15 (k = 21 among them), 300 rows with k <= 12 and up to 200 with
    k = 13, 14: all status 0, the identities, order_posteriors' evidence."""
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    n = mod.n
    k = dat[:, :-2].astype(int).sum(1)
    *out, status = engine(n).order_snapshots(mod.log_theta, mod.obs1, mod.obs2, dat)
    assert np.all(status == 0)
    assert (k >= 15).sum() == 71 and k.max() == 21
    run = OrderSnapshots(*out)
    post = mod.order_posteriors(dat)
    assert mod.posteriors_fallback_rows == 0
    d_le = np.abs(np.expm1(run.log_evidence - post.log_evidence)).max()
    ident = _paired_identities(run, dat, n)
    paired = dat[:, -1] == 3
    print(f"LUAD-28 fit: {len(dat)} rows ({paired.sum()} paired), k up to {k.max()}, evidence against order_posteriors "
          f"{d_le:.2e}, identities {ident}, map_prob in [{np.nanmin(run.map_prob):.3f}, {np.nanmax(run.map_prob):.3f}]")
    snapshots_patterns(run, dat, n)
    assert paired[k == 21].all()
    assert d_le <= BAR and ident[:4].max() <= BAR and ident[4] == 0.0


@pytest.mark.gpu
def test_bitwise_reproducible_and_batching(golden):
    """The rows of LUAD-28 twice, then in another order through a small workspace, then with a row turned away."""
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    first = engine(mod.n).order_snapshots(*args, dat)
    again = engine(mod.n).order_snapshots(*args, dat)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
    keep = np.flatnonzero(k <= 16)
    assert k[keep].max() == 16 and (k[keep] >= 15).any()
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.8 MiB: many batches
        b = small.order_snapshots(*args, dat[perm])
        for x, y in zip(first, b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        assert len(big) == 1
        *out, status = small.order_snapshots(*args, np.vstack((dat[big], dat[keep[:5]])))
        assert status[0] == 3 and np.all(status[1:] == 0)
        for x, y in zip(first, out):
            assert np.all(np.isnan(y[0])) if y.dtype == np.float64 else np.all(y[0] == -1)
            np.testing.assert_array_equal(y[1:], x[keep[:5]])
    print(f"bitwise: {len(dat)} rows twice, {len(perm)} permuted rows in batches of 8 MiB, one row turned away")


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """... with order_snapshot: the k = 14 row (1.2 MiB, over the 1 MiB workspace), its host value against the device's."""
    mod, dat, ref, raw, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    for a in raw[:-1]:
        assert np.all(np.isnan(a[0])) if a.dtype == np.float64 else np.all(a[0] == -1)
    d = snapshots_diff(_one(ref, 0), host)
    print(f"host fallback, k = 14: rel. evidence {d[0]:.2e}, held {d[1]:.2e}, late {d[2]:.2e}, map_prob {d[3]:.2e} "
          f"against the device")
    assert max(d) <= BAR


@pytest.mark.gpu
def test_errors_name_the_row():
    check_errors_name_the_row(ENTRY)
