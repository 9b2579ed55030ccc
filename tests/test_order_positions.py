"""Posterior event positions (MetMHN.order_position / order_positions, mmhn_order_positions, OrderPositions.relative_profile).

Anchors:
  * the host sum-product against brute force over MetMHN.likelihood (pinned to the reference by tests/golden/orders.npz)
    for every admissible order: pos[e, j] = the likelihood-weighted share of the orders whose lineage has e at index j.  The
    MT lineage of an order is the order without its even codes other than the seeding, the PT lineage the order without its
    odd codes;
  * the device kernel against the host code;
  * on rows too large for the host code, identities that tie the positions to themselves, to order_posteriors and to
    order_precedences.

Bars: those of tests/test_order_posteriors.py, where they are derived - every sum runs over non-negative terms, so the
relative error of an output is a small multiple of (k + depth of the sums) x 2^-52.  Device against host 1e-12 absolute on
the positions and 1e-12 relative on exp(log_evidence); host against enumeration 1e-12 relative; the identities 1e-12
absolute.  Every test prints the worst value it saw before it asserts.
"""
import itertools
import os
import re
import warnings

import numpy as np
import pytest

from metmhn_amd import _lib
from metmhn_amd.model import MetMHN, _ROW_ERRORS
from metmhn_amd.state import MetState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n=5, seed=0):
    rng = np.random.default_rng(seed)
    th = rng.normal(0.0, 0.5, (n + 1, n + 1))
    th[np.diag_indices(n + 1)] = rng.normal(-1.0, 0.5, n + 1)
    return MetMHN(th, 2 * rng.random(n + 1) + 1, 2 * rng.random(n + 1) + 1)


def _row(n, slots, typ, diag_order=-99):
    r = np.zeros(2 * n + 3, dtype=np.int8)
    r[list(slots)] = 1
    r[-2], r[-1] = diag_order, typ
    return r


def _paired(n, pt, mt, diag_order):
    return _row(n, [2 * i for i in pt] + [2 * i + 1 for i in mt] + [2 * n], 3, diag_order)


def _lineages(row, n):
    """{"pt" / "mt": the event codes of that lineage} for the lineages a dat row has."""
    typ = int(row[-1])
    pt = [2 * i for i in range(n) if row[2 * i]]
    mt = [2 * i + 1 for i in range(n) if row[2 * i + 1]]
    seed = [2 * n] if row[2 * n] else []
    return {0: {"pt": pt}, 1: {"pt": pt + seed}, 2: {"mt": mt + seed}, 3: {"pt": pt + seed, "mt": mt + seed}}[typ]


def _luad(golden, prefix):
    d = golden("luad28")
    return MetMHN(d[prefix + "_theta"], d[prefix + "_dp"], d[prefix + "_dm"]), d["dat"]


def _paired_orders(state: MetState):
    """Every order the chain can take to a seeded paired `state`."""
    n = state.n
    both = [i for i in state.PT_events if i in state.MT_events]
    for r in range(len(both) + 1):
        for pre in itertools.permutations(both, r):
            head = [c for i in pre for c in (2 * i, 2 * i + 1)] + [2 * n]
            rest = [2 * i for i in state.PT_events if i not in pre] + [2 * i + 1 for i in state.MT_events if i not in pre]
            for tail in itertools.permutations(rest):
                yield tuple(head) + tail


def _split(order, n):
    """(PT lineage, MT lineage) of an order of event codes."""
    return [c for c in order if c % 2 == 0], [c for c in order if c % 2 == 1 or c == 2 * n]


def _enumerate(mod, slots, status, first):
    """(evidence, pos_pt, pos_mt) by brute force over MetMHN.likelihood."""
    n = mod.n
    if status == "isPaired":
        orders = _paired_orders(MetState(slots, size=2 * n + 1))
    else:
        orders = itertools.permutations(sorted(slots))
    Z = 0.0
    pos = {"pt": np.full((n + 1, n + 1), np.nan), "mt": np.full((n + 1, n + 1), np.nan)}
    has = {"isPaired": ("pt", "mt"), "isMetastasis": ("mt",)}.get(status, ("pt",))
    for name, codes in zip(("pt", "mt"), _split(slots, n)):
        if name in has:
            pos[name][[c // 2 for c in codes]] = 0.0
    for o in orders:
        p = mod.likelihood(o, status, first)
        Z += p
        for name, lin in zip(("pt", "mt"), _split(o, n)):
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
        mod = _model(n, seed=300 + 10 * n + seed)
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


def test_abi_carries_the_symbol_and_version_8():
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert "mmhn_order_positions" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mmhn_order_positions"]) == 11
    assert re.search(r"\bint mmhn_order_positions\s*\(", hdr)
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define MMHN_ABI_VERSION (\d+)", hdr).group(1))


def test_arguments_are_checked_before_the_library(monkeypatch):
    import metmhn_amd.jx as jx

    def no_engine(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(jx, "engine", no_engine)
    mod = _model()
    dat = np.array([_row(5, [0, 4, 6], 0), _row(5, [0, 1, 10], 3, 1)])
    for bad in (dat[0], dat[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=r"dat must have shape \[n_pat, 13\]") as e1:
            mod.order_positions(bad)
        with pytest.raises(ValueError) as e2:
            mod.order_precedences(bad)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'") as e1:
        mod.order_positions(dat, backend="cpu")
    with pytest.raises(ValueError) as e2:
        mod.order_precedences(dat, backend="cpu")
    assert str(e1.value) == str(e2.value)
    state = MetState([0, 1, 10], size=11)
    for args in ((state, "paired"), (state, "isPaired", "first"), (MetState([0, 10], size=11), "absent")):
        with pytest.raises(ValueError) as e1:
            mod.order_position(*args)
        with pytest.raises(ValueError) as e2:
            mod.order_precedence(*args)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="met_status must be one of"):
        mod.order_position(state, "paired")
    with pytest.raises(ValueError, match="first_obs must be one of"):
        mod.order_position(state, "isPaired", "first")


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration_paired(n):
    """Random paired states with k <= 7, all four first_obs values; events only in PT, only in MT and in both must all
    occur."""
    rng = np.random.default_rng(40 + n)
    worst = {"Z": 0.0, "pos": 0.0}
    seen = {"pt_only": 0, "mt_only": 0, "joint": 0}
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for seed in range(2):
            mod = _model(n, seed=200 + 10 * n + seed)
            drawn = 0
            while drawn < 8:
                slots = [s for s in range(2 * n) if rng.random() < 0.45]
                if len(slots) > 6:
                    continue                                   # k <= 7: under 6! x 2^3 orders per state
                drawn += 1
                pt, mt = {s // 2 for s in slots if s % 2 == 0}, {s // 2 for s in slots if s % 2 == 1}
                seen["pt_only"] += len(pt - mt); seen["mt_only"] += len(mt - pt); seen["joint"] += len(pt & mt)
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


def _small_shapes():
    """(model, dat): the smallest rows at which the kernel takes another path.  Index bits of a target's move vector:
    k - 1 for one tumour, k - 2 paired; chunks of 6 bits below 8 index bits (256 threads), so k = 9 paired is the first row
    whose classes split between a chunk's number and its low bits."""
    n = 8
    S = 2 * n
    rows = []
    for d in (0, 1, 2, -99):
        rows += [_paired(n, [], [], d),                                   # k = 1: the seeding alone
                 _paired(n, [2], [3], d),                                 # k = 3: one PT-only and one MT-only event
                 _paired(n, [2], [], d), _paired(n, [], [3], d),          # k = 2
                 _paired(n, [0], [0], d),                                 # k = 3: the smallest joint row
                 _paired(n, [0, 1, 3], [0, 2], d),                        # k = 6: a chunk narrower than a wave
                 _paired(n, [0, 2, 4], [0, 2, 5], d),                     # k = 7
                 _paired(n, [0, 1, 2, 3], [0, 1, 4], d),                  # k = 8: one chunk
                 _paired(n, [0, 1, 2, 3, 4], [0, 5, 6], d),               # k = 9: two chunks
                 _paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 3], d),            # k = 10
                 _paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], d),         # k = 11
                 _paired(n, [0, 1, 2], [3, 4, 5], d),     # k = 7, no joint event, PT slots low and MT slots high: the
                                                          # MT mask has no low bit, the PT mask no high one
                 _paired(n, [0, 1, 2, 3], [0, 1, 2, 3], d)]               # k = 9, only joint events
    ev = lambda k, odd: [2 * i + odd for i in range(k)]
    rows += [_row(n, ev(k, 0), 0) for k in (0, 1, 6, 7, 8)]               # "absent"
    rows += [_row(n, ev(k - 1, 0) + [S], 1) for k in (1, 6, 7, 8)]        # "present"
    rows += [_row(n, ev(k - 1, 1) + [S], 2) for k in (1, 6, 7, 8)]        # "isMetastasis"
    return _model(n, seed=21), np.array(rows)


@pytest.mark.gpu
def test_device_against_host_small_shapes():
    mod, dat = _small_shapes()
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
    for i, row in enumerate(dat):
        lin = _lineages(row, mod.n)
        for name, pos in (("pt", host.pos_pt[i]), ("mt", host.pos_mt[i])):
            carried = np.zeros(N, dtype=bool)
            carried[[c // 2 for c in lin.get(name, [])]] = True
            np.testing.assert_array_equal(~np.isnan(pos), np.repeat(carried[:, None], N, axis=1))
    np.testing.assert_array_equal(np.isnan(dev.pos_pt), np.isnan(host.pos_pt))
    np.testing.assert_array_equal(np.isnan(dev.pos_mt), np.isnan(host.pos_mt))
    assert rel.max() <= 1e-12
    assert worst_abs <= 1e-12


def _check_identities(mod, dat, le, pos_pt, pos_mt, post, prec, tag):
    """The identities of the positions with themselves, with order_posteriors (post) and order_precedences (prec)."""
    n = mod.n
    N, S = n + 1, 2 * n
    worst = {"event": 0.0, "position": 0.0, "tail": 0.0, "seed": 0.0, "mean": 0.0, "lo": 0.0, "hi": 0.0}
    for i, row in enumerate(dat):
        lin = _lineages(row, n)
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
            if row[S]:
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
        has = _lineages(dat[i], n)
        for name, lin, pos in zip(("pt", "mt"), _split(order, n), (pos_pt[i], pos_mt[i])):
            if name in has:
                for j, c in enumerate(lin):
                    least = min(least, pos[c // 2, j])
                    assert pos[c // 2, j] > 0.0, (tag, i, order, name, c, j)
    print(f"likeliest orders, {tag}: {len(dat)} rows, smallest posterior of a position the likeliest order takes {least:.3e}")


@pytest.mark.gpu
def test_large_synthetic_rows_by_identities():
    """Paired rows with k = 14 ... 17 (n = 9) and one-tumour rows with k = 14 ... 17 (n = 16): both sides of the
    1024-thread switch at 15 slots."""
    n = 9
    rows = []
    for j, k in enumerate((14, 15, 16, 17)):
        # k - 1 = 2 joint + PT-only + MT-only
        nj = (5, 5, 6, 7)[j]
        rest = k - 1 - 2 * nj
        pt_only = list(range(nj, nj + (rest + 1) // 2))
        mt_only = list(range(nj + (rest + 1) // 2, nj + rest))
        assert nj + rest <= n
        rows.append(_paired(n, list(range(nj)) + pt_only, list(range(nj)) + mt_only, (0, 1, 2, -99)[j]))
    rows += [_paired(n, range(8), range(8), 0),                                  # k = 17, only joint events
             _paired(n, [0, 1, 2, 3, 4, 5, 6], [7, 8, 0, 1, 2, 3, 4], 1),        # k = 15
             _row(n, list(range(0, 18, 2)) + [18], 1), _row(n, list(range(1, 18, 2)) + [18], 2), _row(n, list(range(0, 18, 2)), 0),
             _row(n, [0, 4, 18], 1), _row(n, [18], 2)]
    dat = np.array(rows)
    mod = _model(n, seed=31)
    got = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.pos_pt, got.pos_mt, mod.order_posteriors(dat),
                      mod.order_precedences(dat).prec, "synthetic n = 9")
    small = np.flatnonzero(dat[:, :-2].astype(int).sum(1) <= 12)
    assert len(small) == 5
    _check_likeliest_orders(mod, dat[small], got.pos_pt[small], got.pos_mt[small], "synthetic n = 9")
    n = 16
    rows = []
    for k in (14, 15, 16, 17):
        rows += [_row(n, [2 * i for i in range(k - 1)] + [2 * n], 1), _row(n, [2 * i + 1 for i in range(k - 1)] + [2 * n], 2)]
        if k <= n:
            rows.append(_row(n, [2 * i for i in range(k)], 0))
    dat = np.array(rows)
    mod = _model(n, seed=32)
    got = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.pos_pt, got.pos_mt, mod.order_posteriors(dat),
                      mod.order_precedences(dat).prec, "one tumour n = 16")


@pytest.fixture(scope="module")
def luad_run(golden):
    """order_positions of the LUAD-28 rows these tests use (fit point): the 71 rows with k >= 15, 300 rows with k <= 12
    and up to 200 with k = 13, 14; the raw device outputs."""
    from metmhn_amd.jx import engine
    mod, dat = _luad(golden, "fit")
    k = dat[:, :-2].astype(int).sum(1)
    small = np.flatnonzero(k <= 12)
    sel = np.concatenate((np.flatnonzero(k >= 15), small[np.linspace(0, len(small) - 1, 300).astype(int)], np.flatnonzero((k >= 13) & (k <= 14))[:200]))
    sub = dat[sel]
    le, pos_pt, pos_mt, status = engine(mod.n).order_positions(mod.log_theta, mod.obs1, mod.obs2, sub)
    return mod, sub, k[sel], le, pos_pt, pos_mt, status


@pytest.mark.gpu
def test_luad_rows_by_identities(luad_run):
    """The 71 LUAD-28 rows with k >= 15 (k = 21 among them) and the smaller rows of the fixture."""
    mod, dat, k, le, pos_pt, pos_mt, status = luad_run
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
def test_bitwise_reproducible_and_batching(luad_run):
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat, k, le, pos_pt, pos_mt, status = luad_run
    first = (le, pos_pt, pos_mt, status)
    args = (mod.log_theta, mod.obs1, mod.obs2)
    again = engine(mod.n).order_positions(*args, dat)
    for x, y in zip(first, again):
        np.testing.assert_array_equal(x, y)
    keep = np.flatnonzero(k <= 16)
    assert k[keep].max() == 16 and (k[keep] >= 15).any()
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.8 MiB: many batches
        b = small.order_positions(*args, dat[perm])
        for x, y in zip(first, b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        assert len(big) == 1
        rows = np.vstack((dat[big], dat[keep[:5]]))
        ble, bpt, bmt, bst = small.order_positions(*args, rows)
        assert bst[0] == 3 and np.all(bst[1:] == 0)
        assert np.isnan(ble[0]) and np.all(np.isnan(bpt[0])) and np.all(np.isnan(bmt[0]))
        np.testing.assert_array_equal(ble[1:], le[keep[:5]])
        np.testing.assert_array_equal(bpt[1:], pos_pt[keep[:5]])
        np.testing.assert_array_equal(bmt[1:], pos_mt[keep[:5]])
    print(f"bitwise: {len(dat)} rows twice, {len(perm)} permuted rows in batches of 8 MiB, one row turned away")


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """The Python layer recomputes MMHN_ORD_TOO_LARGE rows with order_position and counts them."""
    import metmhn_amd.jx as jx
    from metmhn_amd.engine import Engine
    n = 9
    mod = _model(n, seed=11)
    S = 2 * n
    wide = _paired(n, [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 7, 8], 0)         # k = 14: 1.2 MiB, over the 1 MiB limit below
    dat = np.vstack((wide[None], [_row(n, [0, 1, 2, 3, 6, S], 3, 1), _row(n, [0, 2, S], 1), _row(n, [0, 2], 0)]))
    ref = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 0
    with Engine(n, workspace_bytes=1 << 20) as small:
        assert small.order_positions(mod.log_theta, mod.obs1, mod.obs2, dat)[3].tolist() == [3, 0, 0, 0]
        monkeypatch.setattr(jx, "engine", lambda n_mut: small)
        got = mod.order_positions(dat)
    assert mod.positions_fallback_rows == 1
    host = mod.order_position(MetState.from_seq(wide[:S + 1]), "isPaired", "unknown")
    assert got.log_evidence[0] == host.log_evidence
    np.testing.assert_array_equal(got.pos_pt[0], host.pos_pt)
    np.testing.assert_array_equal(got.pos_mt[0], host.pos_mt)
    for name in ("log_evidence", "pos_pt", "pos_mt"):
        np.testing.assert_array_equal(getattr(got, name)[1:], getattr(ref, name)[1:])
    d_z = abs(np.exp(got.log_evidence[0]) - np.exp(ref.log_evidence[0])) / np.exp(ref.log_evidence[0])
    d_p = 0.0
    for a, b in ((host.pos_pt, ref.pos_pt[0]), (host.pos_mt, ref.pos_mt[0])):
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        d_p = max(d_p, np.abs(a[~np.isnan(a)] - b[~np.isnan(a)]).max())
    print(f"host fallback, k = 14: rel. evidence {d_z:.2e}, positions {d_p:.2e} against the device")
    assert d_z <= 1e-12 and d_p <= 1e-12


@pytest.mark.gpu
def test_errors_name_the_row():
    from metmhn_amd.engine import Engine
    mod = _model()
    n = mod.n
    S = 2 * n
    good = np.array([_row(n, [0, 4, 6], 0), _row(n, [], 0), _row(n, [2, 4, 8, S], 1), _row(n, [1, 5, 9, S], 2),
                     _row(n, [0, 1, 2, 5, 6, 7, S], 3, 0), _row(n, [0, 1, 4, 5, 3, S], 3, 1), _row(n, [1, S], 3, 2)])
    # one row per MMHN_ORD_* reason, in the order of the enum (1 ... 7)
    bad = [_row(n, [0], 5), _row(n, [0, 3], 3, 1), _row(n, [0, 1], 3, 0), _row(n, [0, 1, 2 * n], 2), _row(n, [1, 3], 2),
           _row(n, [1], 0), _row(n, [0, 1, 2 * n], 1)]
    for reason, b in enumerate(bad, start=1):
        dat = np.vstack((good[:3], b[None], good[3:]))
        with pytest.raises(ValueError) as lo_err:
            mod.likeliest_orders(dat)
        with pytest.raises(ValueError) as dev_err:
            mod.order_positions(dat)
        assert str(dev_err.value) == str(lo_err.value) == f"row 3: {_ROW_ERRORS[reason]}"
        with pytest.raises(ValueError, match=r"^row 3: "):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                mod.order_positions(dat, backend="host")
    with Engine(n, dtype="f32") as e32:
        with pytest.raises(RuntimeError, match="fp64"):
            e32.order_positions(mod.log_theta, mod.obs1, mod.obs2, good)
