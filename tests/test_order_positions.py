"""Posterior event positions (MetMHN.order_position / order_positions, mmhn_order_positions, OrderPositions.relative_profile).

Anchors:
  * the host sum-product against brute force over MetMHN.likelihood (pinned to the reference by tests/golden/orders.npz)
    for every admissible order: pos[e, j] = the likelihood-weighted share of the orders whose lineage has e at index j.  The
    MT lineage of an order is the order without its even codes other than the seeding, the PT lineage the order without its
    odd codes;
  * the device kernel against the host code;
  * on rows too slow for a live comparison with the host code (k >= 15), the host values of tests/golden/orders_big.npz
    on a selection of them, and on all of them identities that tie the positions to themselves, to order_posteriors and
    to order_precedences.
What order_positions shares with the other cohort entry points: order_common.check_* and tests/test_order_contract.py.

Bars: those of tests/test_order_posteriors.py, where they are derived.  Device against host 1e-12 absolute on the positions
and 1e-12 relative on exp(log_evidence); host against enumeration 1e-12 relative; the identities 1e-12 absolute.  Every
test prints the worst value it saw before it asserts.
"""
import itertools
import warnings

import numpy as np
import pytest

from metmhn_amd.state import MetState
from order_common import (ENTRIES, Row, all_orders, big_models, check_arguments_before_the_library, check_big_rows,
                          check_errors_name_the_row, check_too_large_rows_get_the_host_value, large_rows, luad,
                          luad_selection, model, random_paired_states, small_shapes_n8, split)

ENTRY = ENTRIES["order_positions"]


def _enumerate(mod, slots, status, first):
    """(evidence, pos_pt, pos_mt) by brute force over MetMHN.likelihood."""
    n = mod.n
    if status == "isPaired":
        orders = all_orders(MetState(slots, size=2 * n + 1))
    else:
        orders = itertools.permutations(sorted(slots))
    Z = 0.0
    pos = {"pt": np.full((n + 1, n + 1), np.nan), "mt": np.full((n + 1, n + 1), np.nan)}
    has = {"isPaired": ("pt", "mt"), "isMetastasis": ("mt",)}.get(status, ("pt",))
    for name, codes in zip(("pt", "mt"), split(slots, n)):
        if name in has:
            pos[name][[c // 2 for c in codes]] = 0.0
    for o in orders:
        p = mod.likelihood(o, status, first)
        Z += p
        for name, lin in zip(("pt", "mt"), split(o, n)):
            if name in has:
                for j, c in enumerate(lin):
                    pos[name][c // 2, j] += p
    return Z, pos["pt"] / Z, pos["mt"] / Z


def _assert_enum(got, Z, ppt, pmt, tag):
    assert abs(np.exp(got.log_evidence) - Z) <= 1e-12 * Z, tag
    for mine, ref in ((got.pos_pt, ppt), (got.pos_mt, pmt)):
        assert mine.shape == ref.shape
        np.testing.assert_array_equal(np.isnan(mine), np.isnan(ref), err_msg=str(tag))
        np.testing.assert_allclose(mine, ref, rtol=1e-12, atol=1e-15, err_msg=str(tag))
        carried = ~np.isnan(ref[:, 0])
        assert np.all(mine[carried][:, carried.sum():] == 0.0), tag                # zeros past the lineage's length


def _worst(worst, got, Z, ppt, pmt):
    worst["Z"] = max(worst["Z"], abs(np.exp(got.log_evidence) - Z) / Z)
    for mine, ref in ((got.pos_pt, ppt), (got.pos_mt, pmt)):
        have = ~np.isnan(ref) & ~np.isnan(mine)
        if have.any():
            worst["pos"] = max(worst["pos"], np.abs(mine[have] - ref[have]).max())


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [4, 5])
def test_one_tumour_rows_against_enumeration(n):
    """order_position of "isMetastasis", "present" and "absent" states, k <= 6, against every permutation."""
    rng = np.random.default_rng(70 + n)
    worst = {"Z": 0.0, "pos": 0.0}
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
            # the state of a one-tumour row holds its events in the tumour the status names
            state = [s + 1 if status == "isMetastasis" and s != S else s for s in sl]
            got = mod.order_position(MetState(state, size=2 * n + 1), status)
            Z, ppt, pmt = _enumerate(mod, state, status, None)
            _worst(worst, got, Z, ppt, pmt)
            results.append((got, Z, ppt, pmt, (sl, status)))
    print(f"one-tumour rows against enumeration, n = {n}: {len(results)} cases, worst {worst}")
    for got, Z, ppt, pmt, tag in results:
        _assert_enum(got, Z, ppt, pmt, tag)
        # one lineage: "isMetastasis" the metastasis', the others the primary tumour's ("absent" without the seeding)
        other = got.pos_pt if tag[1] == "isMetastasis" else got.pos_mt
        assert np.all(np.isnan(other)), tag
        if tag[1] == "absent":
            assert np.all(np.isnan(got.pos_pt[n])), tag
    assert len(results) == 2 * 18


def test_relative_profile_is_the_notebooks_histogram():
    """On 0/1 positions (one order per row) relative_profile is the loop of post_training_analyses.ipynb, "Finding relative
    event positions": x[e, unit * i // L : unit * (i + 1) // L] += L for the i-th entry e of a row's order of length L."""
    from metmhn_amd.model import OrderPositions
    n = 5
    orders = [[3, 5, 0], [5], [1, 0, 2, 5, 4], None, [2, 5], [0, 1, 2, 3, 4, 5]]          # events of the MT lineage, 5 the seeding
    pos = np.full((len(orders), n + 1, n + 1), np.nan)
    for i, o in enumerate(orders):
        if o is not None:
            pos[i, o] = 0.0
            pos[i, o, range(len(o))] = 1.0
    unit = int(np.lcm.reduce(np.arange(1, 7)))
    want = np.zeros((n + 1, unit))
    for o in orders:
        if o is not None:
            L = len(o)
            for i, e in enumerate(o):
                want[e, unit * i // L:unit * (i + 1) // L] += L
    run = OrderPositions(np.zeros(len(orders)), np.full_like(pos, np.nan), pos)
    got = run.relative_profile()
    print(f"relative profile: {len(orders)} rows, {unit} bins, largest difference {np.abs(got - want).max():.1e}")
    assert got.shape == (n + 1, unit) == (6, 60)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(run.relative_profile("mt", bins=120)[:, ::2], want)
    np.testing.assert_array_equal(OrderPositions(np.zeros(6), pos, pos).relative_profile("pt"), want)
    # a cohort without the lineage: nothing to add
    assert not run.relative_profile("pt").any()
    with pytest.raises(ValueError, match="lineage must be 'mt' or 'pt'"):
        run.relative_profile("met")


def test_arguments_are_checked_before_the_library(monkeypatch):
    check_arguments_before_the_library(ENTRY, monkeypatch)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration_paired(n):
    """Random paired states with k <= 7, all four first_obs values; events only in PT, only in MT and in both must all
    occur."""
    worst = {"Z": 0.0, "pos": 0.0}
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for mod, slots, seen in random_paired_states(n, 40 + n, (200 + 10 * n, 201 + 10 * n), 8):
            for first in ("PT", "Met", "unknown", "sync"):
                got = mod.order_position(MetState(slots + [2 * n], size=2 * n + 1), "isPaired", first)
                Z, ppt, pmt = _enumerate(mod, slots + [2 * n], "isPaired", first)
                _worst(worst, got, Z, ppt, pmt)
                results.append((got, Z, ppt, pmt, (slots, first)))
    print(f"paired host against enumeration, n = {n}: {len(results)} cases, events {seen}, worst {worst}")
    for got, Z, ppt, pmt, tag in results:
        _assert_enum(got, Z, ppt, pmt, tag)
    assert len(results) == 2 * 8 * 4
    assert min(seen.values()) > 0


@pytest.mark.gpu
def test_device_against_host_small_shapes():
    mod, dat = small_shapes_n8()
    k = dat[:, :-2].astype(int).sum(1)
    ks = set(int(v) for v in k)
    assert k.max() <= 11
    dev = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        host = mod.order_positions(dat, backend="host")
    N = mod.n + 1
    assert dev.pos_pt.shape == dev.pos_mt.shape == host.pos_pt.shape == host.pos_mt.shape == (len(dat), N, N)
    rel = np.abs(np.exp(dev.log_evidence) - np.exp(host.log_evidence)) / np.exp(host.log_evidence)
    worst_abs = 0.0
    for a, b in ((dev.pos_pt, host.pos_pt), (dev.pos_mt, host.pos_mt)):
        have = ~np.isnan(a) & ~np.isnan(b)
        worst_abs = max(worst_abs, np.abs(a[have] - b[have]).max())
    print(f"device against host, small shapes: {len(dat)} rows, k in {sorted(ks)}, worst rel. evidence {rel.max():.2e}, "
          f"positions {worst_abs:.2e}")
    assert ks >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11}
    for i, r in enumerate(dat):
        lin = Row(r, mod.n).lineages
        for name, pos in (("pt", host.pos_pt[i]), ("mt", host.pos_mt[i])):
            carried = np.zeros(N, dtype=bool)
            carried[[c // 2 for c in lin.get(name, [])]] = True
            np.testing.assert_array_equal(~np.isnan(pos), np.repeat(carried[:, None], N, axis=1))
    np.testing.assert_array_equal(np.isnan(dev.pos_pt), np.isnan(host.pos_pt))
    np.testing.assert_array_equal(np.isnan(dev.pos_mt), np.isnan(host.pos_mt))
    assert rel.max() <= 1e-12
    assert worst_abs <= 1e-12


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The rows of tests/golden/orders_big.npz, k = 15 ... 21: every one on the device (the 1 024-thread instantiation),
    evidence and positions at the bars of test_device_against_host_small_shapes against the host values the fixture holds."""
    device = {}
    for name, m in big_models():
        device[name] = m.mod.order_positions(m.dat)
        assert m.mod.positions_fallback_rows == 0
    check_big_rows("order_positions", device, 1e-12)


def _check_identities(mod, dat, le, pos_pt, pos_mt, post, prec, tag):
    """The identities of the positions with themselves, with order_posteriors (post) and order_precedences (prec)."""
    n = mod.n
    N, S = n + 1, 2 * n
    worst = {"event": 0.0, "position": 0.0, "tail": 0.0, "seed": 0.0, "mean": 0.0, "lo": 0.0, "hi": 0.0}
    for i, r in enumerate(dat):
        lin = Row(r, n).lineages
        for name, pos in (("pt", pos_pt[i]), ("mt", pos_mt[i])):
            codes = lin.get(name)
            if codes is None:
                assert np.all(np.isnan(pos)), (tag, i, name)                        # a lineage the row does not have
                continue
            ev = [c // 2 for c in codes]
            L = len(ev)
            carried = np.zeros(N, dtype=bool)
            carried[ev] = True
            assert np.array_equal(~np.isnan(pos), np.repeat(carried[:, None], N, axis=1)), (tag, i, name)
            if L == 0:
                continue
            p = pos[ev]
            worst["lo"], worst["hi"] = min(worst["lo"], p.min()), max(worst["hi"], p.max() - 1.0)
            worst["event"] = max(worst["event"], np.abs(p.sum(axis=1) - 1.0).max())
            worst["position"] = max(worst["position"], np.abs(p[:, :L].sum(axis=0) - 1.0).max())
            worst["tail"] = max(worst["tail"], np.abs(p[:, L:]).max(initial=0.0))
            if r[S]:
                worst["seed"] = max(worst["seed"], np.abs(pos[n] - post.seed_pos[i]).max())
            mean = p @ np.arange(N)
            for a, d in enumerate(codes):
                before = sum(prec[i, c, d] for c in codes if c != d)
                worst["mean"] = max(worst["mean"], abs(mean[a] - before))
    worst["le"] = np.abs(le - post.log_evidence).max()
    print(f"identities, {tag}: {len(dat)} rows, worst {worst}")
    for key in ("event", "position", "seed", "mean", "le"):
        assert worst[key] <= 1e-12, key
    assert worst["tail"] == 0.0
    assert worst["lo"] >= 0.0 and worst["hi"] <= 0.0                                       # every entry in [0, 1]


def _check_likeliest_orders(mod, dat, pos_pt, pos_mt, tag):
    """The position the likeliest order gives every event has a positive posterior (rows with k <= 12)."""
    n = mod.n
    least = np.inf
    for i, (order, _) in enumerate(mod.likeliest_orders(dat)):
        has = Row(dat[i], n).lineages
        for name, lin, pos in zip(("pt", "mt"), split(order, n), (pos_pt[i], pos_mt[i])):
            if name in has:
                for j, c in enumerate(lin):
                    least = min(least, pos[c // 2, j])
                    assert pos[c // 2, j] > 0.0, (tag, i, order, name, c, j)
    print(f"likeliest orders, {tag}: {len(dat)} rows, smallest posterior of a position the likeliest order takes {least:.3e}")


@pytest.mark.gpu
def test_large_synthetic_rows_by_identities():
    """Paired rows with k = 14 ... 17 (n = 9) and one-tumour rows with k = 14 ... 17 (n = 16): both sides of the
    1024-thread switch at 15 slots."""
    dat = large_rows(9)
    mod = model(9, seed=31)
    got = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.pos_pt, got.pos_mt, mod.order_posteriors(dat),
                      mod.order_precedences(dat).prec, "synthetic n = 9")
    small = np.flatnonzero(dat[:, :-2].astype(int).sum(1) <= 12)
    assert len(small) == 5
    _check_likeliest_orders(mod, dat[small], got.pos_pt[small], got.pos_mt[small], "synthetic n = 9")
    dat = large_rows(16)
    mod = model(16, seed=32)
    got = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.pos_pt, got.pos_mt, mod.order_posteriors(dat),
                      mod.order_precedences(dat).prec, "one tumour n = 16")


@pytest.mark.gpu
def test_luad_rows_by_identities(golden):
    """LUAD-28 at the fit point: the 71 rows with k >= 15 (k = 21 among them), 300 rows with k <= 12 and up to 200 with
    k = 13, 14."""
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    le, pos_pt, pos_mt, status = engine(mod.n).order_positions(mod.log_theta, mod.obs1, mod.obs2, dat)
    assert np.all(status == 0)
    assert (k >= 15).sum() == 71 and k.max() == 21
    post = mod.order_posteriors(dat)
    prec = mod.order_precedences(dat).prec
    assert mod.posteriors_fallback_rows == 0 and mod.precedences_fallback_rows == 0
    for sel, tag in ((k >= 15, "LUAD-28 fit, k >= 15"), (k <= 14, "LUAD-28 fit, k <= 14")):
        _check_identities(mod, dat[sel], le[sel], pos_pt[sel], pos_mt[sel],
                          type(post)(post.log_evidence[sel], post.pre[sel], post.seed_pos[sel]), prec[sel], tag)
    small = np.flatnonzero(k <= 12)
    assert len(small) == 300
    _check_likeliest_orders(mod, dat[small], pos_pt[small], pos_mt[small], "LUAD-28 fit, k <= 12")


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """... with order_position: the k = 14 row (1.2 MiB, over the 1 MiB workspace), its host value against the device's."""
    mod, dat, ref, raw, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    d_z = abs(np.exp(host.log_evidence) - np.exp(ref.log_evidence[0])) / np.exp(ref.log_evidence[0])
    d_p = 0.0
    for a, b in ((host.pos_pt, ref.pos_pt[0]), (host.pos_mt, ref.pos_mt[0])):
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        d_p = max(d_p, np.abs(a[~np.isnan(a)] - b[~np.isnan(a)]).max())
    print(f"host fallback, k = 14: rel. evidence {d_z:.2e}, positions {d_p:.2e} against the device")
    assert d_z <= 1e-12 and d_p <= 1e-12


@pytest.mark.gpu
def test_errors_name_the_row():
    check_errors_name_the_row(ENTRY)
