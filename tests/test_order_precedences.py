"""Pairwise event-precedence posteriors (MetMHN.order_precedence / order_precedences, mmhn_order_precedences).

Anchors:
  * the host sum-product against brute force over MetMHN.likelihood (pinned to the reference by tests/golden/orders.npz)
    for every admissible order: prec[c, d] = the likelihood-weighted share of the orders with c strictly before d;
  * the device kernel against the host code;
  * on rows too large for the host code, identities that tie prec to itself and to order_posteriors.

Bars: those of tests/test_order_posteriors.py, where they are derived - every sum runs over non-negative terms, so the
relative error of an output is a small multiple of (k + depth of the sums) x 2^-52.  Device against host 1e-12 absolute on
prec and 1e-12 relative on exp(log_evidence); host against enumeration 1e-12 relative; the identities 1e-12 absolute.
Every test prints the worst value it saw before it asserts.
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


def _codes(row, n):
    """The event codes a row carries, as likeliest_order writes them."""
    typ = int(row[-1])
    pt = [2 * i for i in range(n) if row[2 * i]]
    mt = [2 * i + 1 for i in range(n) if row[2 * i + 1]]
    seed = [2 * n] if row[2 * n] else []
    return {0: pt, 1: pt + seed, 2: mt + seed, 3: sorted(pt + mt) + seed}[typ]


def _luad(golden, prefix):
    d = golden("luad28")
    return MetMHN(d[prefix + "_theta"], d[prefix + "_dp"], d[prefix + "_dm"]), d["dat"]


def _paired_orders(state: MetState):
    """Every order the chain can take to a seeded paired `state`, with the number of joint events before the seeding."""
    n = state.n
    both = [i for i in state.PT_events if i in state.MT_events]
    for r in range(len(both) + 1):
        for pre in itertools.permutations(both, r):
            head = [c for i in pre for c in (2 * i, 2 * i + 1)] + [2 * n]
            rest = [2 * i for i in state.PT_events if i not in pre] + [2 * i + 1 for i in state.MT_events if i not in pre]
            for tail in itertools.permutations(rest):
                yield tuple(head) + tail, r


def _moments(order, joint_before):
    """code -> the moment it happened: the two codes of a joint event before the seeding share one."""
    t = {}
    for j, c in enumerate(order):
        t[c] = j // 2 if j < 2 * joint_before else j - joint_before
    return t


def _enumerate(mod, slots, status, first):
    """(evidence, prec [2n+1, 2n+1]) by brute force over MetMHN.likelihood."""
    L = 2 * mod.n + 1
    if status == "isPaired":
        orders = _paired_orders(MetState(slots, size=L))
    else:
        orders = ((o, 0) for o in itertools.permutations(sorted(slots)))
    Z, P = 0.0, np.full((L, L), np.nan)
    P[np.ix_(slots, slots)] = 0.0
    for o, r in orders:
        p = mod.likelihood(o, status, first)
        Z += p
        t = _moments(o, r)
        for c in o:
            for d in o:
                if t[c] < t[d]:
                    P[c, d] += p
    return Z, P / Z


def _compare_enum(mod, slots, status, first, worst):
    L = 2 * mod.n + 1
    got = mod.order_precedence(MetState(slots, size=L), status, first)
    codes = list(slots)
    Z, P = _enumerate(mod, codes, status, first)
    worst["Z"] = max(worst["Z"], abs(np.exp(got.log_evidence) - Z) / Z)
    assert got.prec.shape == (L, L)
    np.testing.assert_array_equal(np.isnan(got.prec), np.isnan(P))
    if codes:
        have = ~np.isnan(P)
        worst["prec"] = max(worst["prec"], np.abs(got.prec[have] - P[have]).max())
    return got, Z, P


def _assert_enum(got, Z, P, tag):
    assert abs(np.exp(got.log_evidence) - Z) <= 1e-12 * Z, tag
    np.testing.assert_allclose(got.prec, P, rtol=1e-12, atol=1e-15, err_msg=str(tag))
    assert np.all(np.diag(got.prec)[~np.isnan(np.diag(got.prec))] == 0.0)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n", [4, 5])
def test_one_tumour_rows_against_enumeration(n):
    """order_precedence of "isMetastasis", "present" and "absent" states, k <= 6, against every permutation."""
    rng = np.random.default_rng(70 + n)
    worst = {"Z": 0.0, "prec": 0.0}
    S, cases, results = 2 * n, 0, []
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
            L = 2 * n + 1
            got = mod.order_precedence(MetState(state, size=L), status)
            Z, P = _enumerate(mod, state, status, None)
            worst["Z"] = max(worst["Z"], abs(np.exp(got.log_evidence) - Z) / Z)
            if state:
                have = ~np.isnan(P)
                worst["prec"] = max(worst["prec"], np.abs(got.prec[have] - P[have]).max())
            results.append((got, Z, P, (sl, status)))
            cases += 1
    print(f"one-tumour rows against enumeration, n = {n}: {cases} cases, worst {worst}")
    for got, Z, P, tag in results:
        np.testing.assert_array_equal(np.isnan(got.prec), np.isnan(P))
        _assert_enum(got, Z, P, tag)
    assert cases == 2 * 18


def test_cohort_mean_averages_over_the_rows_that_carry_both_codes():
    from metmhn_amd.model import OrderPrecedences
    nan = np.nan
    prec = np.array([[[0.0, 0.2], [0.8, 0.0]], [[0.0, nan], [nan, nan]], [[0.0, 0.6], [0.4, 0.0]]])
    mean = OrderPrecedences(np.zeros(3), prec).cohort_mean()
    np.testing.assert_allclose(mean, [[0.0, 0.4], [0.6, 0.0]], rtol=0, atol=1e-15)
    assert np.isnan(OrderPrecedences(np.zeros(1), prec[1:2]).cohort_mean()[1, 1])


def test_abi_carries_the_symbol_and_version_8():
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert "mmhn_order_precedences" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mmhn_order_precedences"]) == 10
    assert re.search(r"\bint mmhn_order_precedences\s*\(", hdr)
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
            mod.order_precedences(bad)
        with pytest.raises(ValueError) as e2:
            mod.order_posteriors(bad)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'") as e1:
        mod.order_precedences(dat, backend="cpu")
    with pytest.raises(ValueError) as e2:
        mod.order_posteriors(dat, backend="cpu")
    assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="met_status must be one of"):
        mod.order_precedence(MetState([0, 1, 10], size=11), "paired")
    with pytest.raises(ValueError, match="first_obs must be one of"):
        mod.order_precedence(MetState([0, 1, 10], size=11), "isPaired", "first")
    with pytest.raises(ValueError, match="Met part of the state was not empty, but met_status is 'absent'"):
        mod.order_precedence(MetState([0, 10], size=11), "absent")


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration_paired(n):
    """The scheme of test_order_posteriors.test_host_against_enumeration: random paired states with k <= 7, all four
    first_obs values; events only in PT, only in MT and in both must all occur."""
    rng = np.random.default_rng(40 + n)
    worst = {"Z": 0.0, "prec": 0.0}
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
                    got, Z, P = _compare_enum(mod, slots + [2 * n], "isPaired", first, worst)
                    results.append((got, Z, P, (slots, first)))
    print(f"paired host against enumeration, n = {n}: {len(results)} cases, events {seen}, worst {worst}")
    for got, Z, P, tag in results:
        _assert_enum(got, Z, P, tag)
    assert len(results) == 2 * 8 * 4
    assert min(seen.values()) > 0


def _small_shapes():
    """(model, dat) pairs: the smallest rows at which the kernel takes another path.  Index bits of a target's move vector:
    k - 1 for one tumour, k - 2 paired; chunks of 6 bits below 8 index bits (256 threads)."""
    out = []
    n = 7
    S = 2 * n
    rows = []
    orders = (0, 1, 2, -99)
    for d in orders:
        rows += [_paired(n, [], [], d),                                   # k = 1: the seeding alone
                 _paired(n, [0], [0], d),                                 # k = 3: the smallest joint row
                 _paired(n, [0, 1, 3], [0, 2], d),                        # k = 6: a chunk narrower than a wave
                 _paired(n, [0, 2, 4], [0, 2, 5], d),                     # k = 7
                 _paired(n, [0, 1, 2, 3], [0, 1, 4], d),                  # k = 8: one chunk
                 _paired(n, [0, 1, 2, 3, 4], [0, 5, 6], d)]               # k = 9: two chunks
    rows += [_paired(n, [0, 1, 2], [3, 4, 5], 0), _paired(n, [0, 1, 2], [3, 4, 5], 1),      # zero joint events, k = 7
             _paired(n, [1, 3, 5, 6], [0, 2, 4, 5], 2),                                       # one joint event, k = 9
             _paired(n, [0, 1, 2, 3], [0, 1, 2, 3], 0), _paired(n, [0, 1, 2, 3], [0, 1, 2, 3], -99),   # only joint, k = 9
             _paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], 0), _paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], 1),   # k = 11
             _paired(n, [2], [], 2), _paired(n, [], [3], 1)]                                  # k = 2
    ev = lambda k, odd: [2 * i + odd for i in range(k)]
    rows += [_row(n, [], 0), _row(n, [4], 0), _row(n, ev(6, 0), 0), _row(n, ev(7, 0), 0),                 # absent k = 0, 1, 6, 7
             _row(n, [S], 1), _row(n, ev(5, 0) + [S], 1), _row(n, ev(6, 0) + [S], 1), _row(n, ev(7, 0) + [S], 1),   # k = 1, 6, 7, 8
             _row(n, [S], 2), _row(n, ev(5, 1) + [S], 2), _row(n, ev(6, 1) + [S], 2), _row(n, ev(7, 1) + [S], 2)]
    out.append((_model(n, seed=21), np.array(rows)))
    n = 5
    out.append((_model(n, seed=22), np.array([_paired(n, range(5), range(5), d) for d in (1, 2)]      # only joint, k = 11
                                             + [_paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 3], -99),          # k = 10
                                                _row(n, [0, 2, 4, 6, 8, 10], 1), _row(n, [1, 5, 10], 2), _row(n, [2, 6], 0)])))
    n = 6
    out.append((_model(n, seed=23), np.array([_paired(n, [0, 1, 2, 3, 4, 5], [1, 3, 4, 5], 0),           # k = 11
                                             _paired(n, [0, 2], [0, 1, 2, 3, 4, 5], 2),                   # k = 9
                                             _row(n, [0, 2, 4, 6, 8, 10, 12], 1), _row(n, [1, 3, 5, 7, 9, 11, 12], 2)])))
    return out


@pytest.mark.gpu
def test_device_against_host_small_shapes():
    worst_rel, worst_abs, total, ks = 0.0, 0.0, 0, set()
    for mod, dat in _small_shapes():
        k = dat[:, :-2].astype(int).sum(1)
        assert k.max() <= 11
        ks |= set(int(v) for v in k)
        dev = mod.order_precedences(dat)
        assert mod.precedences_fallback_rows == 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", DeprecationWarning)
            host = mod.order_precedences(dat, backend="host")
        assert dev.prec.shape == host.prec.shape == (len(dat), 2 * mod.n + 1, 2 * mod.n + 1)
        np.testing.assert_array_equal(np.isnan(dev.prec), np.isnan(host.prec))
        for i, row in enumerate(dat):
            present = np.zeros(2 * mod.n + 1, dtype=bool)
            present[_codes(row, mod.n)] = True
            np.testing.assert_array_equal(~np.isnan(host.prec[i]), np.outer(present, present))
        rel = np.abs(np.exp(dev.log_evidence) - np.exp(host.log_evidence)) / np.exp(host.log_evidence)
        have = ~np.isnan(host.prec)
        worst_rel = max(worst_rel, rel.max())
        if have.any():
            worst_abs = max(worst_abs, np.abs(dev.prec[have] - host.prec[have]).max())
        total += len(dat)
    print(f"device against host, small shapes: {total} rows, k in {sorted(ks)}, worst rel. evidence {worst_rel:.2e}, "
          f"prec {worst_abs:.2e}")
    assert ks >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11}
    assert worst_rel <= 1e-12
    assert worst_abs <= 1e-12


def _check_identities(mod, dat, le, prec, post, tag):
    """The identities of prec with itself and with order_posteriors (le, pre) on the rows of dat."""
    n = mod.n
    S = 2 * n
    worst = {"sum": 0.0, "joint": 0.0, "seed": 0.0, "le": 0.0, "lo": 0.0, "hi": 0.0}
    for i, row in enumerate(dat):
        typ = int(row[-1])
        codes = _codes(row, n)
        present = np.zeros(S + 1, dtype=bool)
        present[codes] = True
        p = prec[i]
        assert np.array_equal(~np.isnan(p), np.outer(present, present)), (tag, i)          # NaN exactly where a code is absent
        sub = p[np.ix_(codes, codes)]
        if codes:
            worst["lo"], worst["hi"] = min(worst["lo"], sub.min()), max(worst["hi"], sub.max() - 1.0)
            assert np.all(np.diag(sub) == 0.0)
        pre = post.pre[i]
        for a, c in enumerate(codes):
            for d in codes[a + 1:]:
                both = p[c, d] + p[d, c]
                if typ == 3 and c % 2 == 0 and d == c + 1 and c != S:
                    worst["joint"] = max(worst["joint"], abs(both - (1.0 - pre[c // 2])))
                else:
                    worst["sum"] = max(worst["sum"], abs(both - 1.0))
        if row[S]:
            for c in codes[:-1]:
                e = c // 2
                joint = typ != 3 or (row[2 * e] and row[2 * e + 1])
                worst["seed"] = max(worst["seed"], abs(p[c, S] - (pre[e] if joint else 0.0)))
    worst["le"] = np.abs(le - post.log_evidence).max()
    print(f"identities, {tag}: {len(dat)} rows, worst {worst}")
    assert worst["sum"] <= 1e-12 and worst["joint"] <= 1e-12 and worst["seed"] <= 1e-12 and worst["le"] <= 1e-12
    assert worst["lo"] >= 0.0 and worst["hi"] <= 0.0                                       # every entry in [0, 1]


def _check_likeliest_orders(mod, dat, prec, tag):
    """Every pair the likeliest order places c before d has a positive posterior (rows with k <= 12)."""
    n = mod.n
    least = np.inf
    for i, (order, _) in enumerate(mod.likeliest_orders(dat)):
        s = order.index(2 * n) if 2 * n in order else len(order)
        joint_before = s // 2 if dat[i, -1] == 3 else 0
        t = _moments(order, joint_before)
        for c in order:
            for d in order:
                if t[c] < t[d]:
                    least = min(least, prec[i, c, d])
                    assert prec[i, c, d] > 0.0, (tag, i, order, c, d)
    print(f"likeliest orders, {tag}: {len(dat)} rows, smallest posterior of a pair the likeliest order decides {least:.3e}")


@pytest.mark.gpu
def test_large_synthetic_rows_by_identities():
    """Paired rows with k = 14 ... 17 (n = 9) and one-tumour rows with k = 14 ... 17 (n = 16; n = 9 has room for 10 slots,
    those rows are here too): both sides of the 1024-thread switch at 15 slots."""
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
    got = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 0
    post = mod.order_posteriors(dat)
    _check_identities(mod, dat, got.log_evidence, got.prec, post, "synthetic n = 9")
    small = np.flatnonzero(dat[:, :-2].astype(int).sum(1) <= 12)
    assert len(small) == 5
    _check_likeliest_orders(mod, dat[small], got.prec[small], "synthetic n = 9")
    n = 16
    rows = []
    for k in (14, 15, 16, 17):
        rows += [_row(n, [2 * i for i in range(k - 1)] + [2 * n], 1), _row(n, [2 * i + 1 for i in range(k - 1)] + [2 * n], 2)]
        if k <= n:
            rows.append(_row(n, [2 * i for i in range(k)], 0))
    dat = np.array(rows)
    mod = _model(n, seed=32)
    got = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.prec, mod.order_posteriors(dat), "one tumour n = 16")


@pytest.fixture(scope="module")
def luad_run(golden):
    """order_precedences and order_posteriors of the LUAD-28 rows these tests use (fit point): the 71 rows with k >= 15,
    300 rows with k <= 12 and up to 200 with k = 13, 14; the raw device outputs."""
    from metmhn_amd.jx import engine
    mod, dat = _luad(golden, "fit")
    k = dat[:, :-2].astype(int).sum(1)
    small = np.flatnonzero(k <= 12)
    sel = np.concatenate((np.flatnonzero(k >= 15), small[np.linspace(0, len(small) - 1, 300).astype(int)], np.flatnonzero((k >= 13) & (k <= 14))[:200]))
    sub = dat[sel]
    le, prec, status = engine(mod.n).order_precedences(mod.log_theta, mod.obs1, mod.obs2, sub)
    return mod, sub, k[sel], le, prec, status


@pytest.mark.gpu
def test_luad_rows_by_identities(luad_run):
    """The 71 LUAD-28 rows with k >= 15 (k = 21 among them) and the smaller rows of the fixture."""
    mod, dat, k, le, prec, status = luad_run
    assert np.all(status == 0)
    assert (k >= 15).sum() == 71 and k.max() == 21
    post = mod.order_posteriors(dat)
    assert mod.posteriors_fallback_rows == 0
    big = k >= 15
    _check_identities(mod, dat[big], le[big], prec[big], type(post)(post.log_evidence[big], post.pre[big], post.seed_pos[big]),
                      "LUAD-28 fit, k >= 15")
    _check_identities(mod, dat[~big], le[~big], prec[~big],
                      type(post)(post.log_evidence[~big], post.pre[~big], post.seed_pos[~big]), "LUAD-28 fit, k <= 14")
    small = np.flatnonzero(k <= 12)
    assert len(small) == 300
    _check_likeliest_orders(mod, dat[small], prec[small], "LUAD-28 fit, k <= 12")


@pytest.mark.gpu
def test_bitwise_reproducible_and_batching(luad_run):
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat, k, le, prec, status = luad_run
    args = (mod.log_theta, mod.obs1, mod.obs2)
    again = engine(mod.n).order_precedences(*args, dat)
    for x, y in zip((le, prec, status), again):
        np.testing.assert_array_equal(x, y)
    keep = np.flatnonzero(k <= 16)
    assert k[keep].max() == 16 and (k[keep] >= 15).any()
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.8 MiB: many batches
        b = small.order_precedences(*args, dat[perm])
        for x, y in zip((le, prec, status), b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        assert len(big) == 1
        rows = np.vstack((dat[big], dat[keep[:5]]))
        ble, bprec, bst = small.order_precedences(*args, rows)
        assert bst[0] == 3 and np.all(bst[1:] == 0)
        assert np.isnan(ble[0]) and np.all(np.isnan(bprec[0]))
        np.testing.assert_array_equal(ble[1:], le[keep[:5]])
        np.testing.assert_array_equal(bprec[1:], prec[keep[:5]])


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """The Python layer recomputes MMHN_ORD_TOO_LARGE rows with order_precedence and counts them."""
    import metmhn_amd.jx as jx
    from metmhn_amd.engine import Engine
    n = 9
    mod = _model(n, seed=11)
    S = 2 * n
    wide = _paired(n, [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 7, 8], 0)         # k = 14: 1.2 MiB, over the 1 MiB limit below
    dat = np.vstack((wide[None], [_row(n, [0, 1, 2, 3, 6, S], 3, 1), _row(n, [0, 2, S], 1), _row(n, [0, 2], 0)]))
    ref = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 0
    with Engine(n, workspace_bytes=1 << 20) as small:
        assert small.order_precedences(mod.log_theta, mod.obs1, mod.obs2, dat)[2].tolist() == [3, 0, 0, 0]
        monkeypatch.setattr(jx, "engine", lambda n_mut: small)
        got = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 1
    host = mod.order_precedence(MetState.from_seq(wide[:S + 1]), "isPaired", "unknown")
    assert got.log_evidence[0] == host.log_evidence
    np.testing.assert_array_equal(got.prec[0], host.prec)
    np.testing.assert_array_equal(got.log_evidence[1:], ref.log_evidence[1:])
    np.testing.assert_array_equal(got.prec[1:], ref.prec[1:])
    have = ~np.isnan(host.prec)
    np.testing.assert_array_equal(have, ~np.isnan(ref.prec[0]))
    d_z = abs(np.exp(got.log_evidence[0]) - np.exp(ref.log_evidence[0])) / np.exp(ref.log_evidence[0])
    d_p = np.abs(got.prec[0][have] - ref.prec[0][have]).max()
    print(f"host fallback, k = 14: rel. evidence {d_z:.2e}, prec {d_p:.2e} against the device")
    assert d_z <= 1e-12 and d_p <= 1e-12
    # cohort_mean: entry by entry over the rows that carry both codes
    mean = ref.cohort_mean()
    np.testing.assert_allclose(mean[0, 2], np.mean(ref.prec[:, 0, 2]), rtol=1e-15)            # every row carries 0 and 2
    np.testing.assert_allclose(mean[0, S], np.mean(ref.prec[:3, 0, S]), rtol=1e-15)           # the "absent" row has no seeding
    assert np.isnan(mean[9, 9]) and np.isnan(mean[0, 9]) and mean[0, 0] == 0.0                # no row carries code 9


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
            mod.order_precedences(dat)
        assert str(dev_err.value) == str(lo_err.value) == f"row 3: {_ROW_ERRORS[reason]}"
        with pytest.raises(ValueError, match=r"^row 3: "):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                mod.order_precedences(dat, backend="host")
    with Engine(n, dtype="f32") as e32:
        with pytest.raises(RuntimeError, match="fp64"):
            e32.order_precedences(mod.log_theta, mod.obs1, mod.obs2, good)
