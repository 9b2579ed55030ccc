"""Pairwise event-precedence posteriors (MetMHN.order_precedence / order_precedences, mmhn_order_precedences).

Anchors:
  * the host sum-product against brute force over MetMHN.likelihood (pinned to the reference by tests/golden/orders.npz)
    for every admissible order: prec[c, d] = the likelihood-weighted share of the orders with c strictly before d;
  * the device kernel against the host code;
  * on rows too slow for a live comparison with the host code (k >= 15), the host values of tests/golden/orders_big.npz
    on a selection of them, and on all of them identities that tie prec to itself and to order_posteriors.
What order_precedences shares with the other cohort entry points: order_common.check_* and tests/test_order_contract.py.

Bars: those of tests/test_order_posteriors.py, where they are derived.  Device against host 1e-12 absolute on prec and
1e-12 relative on exp(log_evidence); host against enumeration 1e-12 relative; the identities 1e-12 absolute.  Every test
prints the worst value it saw before it asserts.
"""
import itertools
import warnings

import numpy as np
import pytest

from metmhn_amd.state import MetState
from order_common import (ENTRIES, Row, big_models, check_arguments_before_the_library, check_big_rows,
                          check_errors_name_the_row, check_too_large_rows_get_the_host_value, large_rows, luad,
                          luad_selection, model, moments, paired, paired_orders, random_paired_states, row)

ENTRY = ENTRIES["order_precedences"]


def _enumerate(mod, slots, status, first):
    """(evidence, prec [2n+1, 2n+1]) by brute force over MetMHN.likelihood."""
    L = 2 * mod.n + 1
    if status == "isPaired":
        orders = paired_orders(MetState(slots, size=L))
    else:
        orders = ((o, 0) for o in itertools.permutations(sorted(slots)))
    Z, P = 0.0, np.full((L, L), np.nan)
    P[np.ix_(slots, slots)] = 0.0
    for o, r in orders:
        p = mod.likelihood(o, status, first)
        Z += p
        t = moments(o, r)
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


def test_arguments_are_checked_before_the_library(monkeypatch):
    check_arguments_before_the_library(ENTRY, monkeypatch)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration_paired(n):
    """The scheme of test_order_posteriors.test_host_against_enumeration: random paired states with k <= 7, all four
    first_obs values; events only in PT, only in MT and in both must all occur."""
    worst = {"Z": 0.0, "prec": 0.0}
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for mod, slots, seen in random_paired_states(n, 40 + n, (200 + 10 * n, 201 + 10 * n), 8):
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
        rows += [paired(n, [], [], d),                                   # k = 1: the seeding alone
                 paired(n, [0], [0], d),                                 # k = 3: the smallest joint row
                 paired(n, [0, 1, 3], [0, 2], d),                        # k = 6: a chunk narrower than a wave
                 paired(n, [0, 2, 4], [0, 2, 5], d),                     # k = 7
                 paired(n, [0, 1, 2, 3], [0, 1, 4], d),                  # k = 8: one chunk
                 paired(n, [0, 1, 2, 3, 4], [0, 5, 6], d)]               # k = 9: two chunks
    rows += [paired(n, [0, 1, 2], [3, 4, 5], 0), paired(n, [0, 1, 2], [3, 4, 5], 1),      # zero joint events, k = 7
             paired(n, [1, 3, 5, 6], [0, 2, 4, 5], 2),                                      # one joint event, k = 9
             paired(n, [0, 1, 2, 3], [0, 1, 2, 3], 0), paired(n, [0, 1, 2, 3], [0, 1, 2, 3], -99),   # only joint, k = 9
             paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], 0), paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], 1),   # k = 11
             paired(n, [2], [], 2), paired(n, [], [3], 1)]                                  # k = 2
    ev = lambda k, odd: [2 * i + odd for i in range(k)]
    rows += [row(n, [], 0), row(n, [4], 0), row(n, ev(6, 0), 0), row(n, ev(7, 0), 0),                 # absent k = 0, 1, 6, 7
             row(n, [S], 1), row(n, ev(5, 0) + [S], 1), row(n, ev(6, 0) + [S], 1), row(n, ev(7, 0) + [S], 1),   # k = 1, 6, 7, 8
             row(n, [S], 2), row(n, ev(5, 1) + [S], 2), row(n, ev(6, 1) + [S], 2), row(n, ev(7, 1) + [S], 2)]
    out.append((model(n, seed=21), np.array(rows)))
    n = 5
    out.append((model(n, seed=22), np.array([paired(n, range(5), range(5), d) for d in (1, 2)]      # only joint, k = 11
                                            + [paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 3], -99),          # k = 10
                                               row(n, [0, 2, 4, 6, 8, 10], 1), row(n, [1, 5, 10], 2), row(n, [2, 6], 0)])))
    n = 6
    out.append((model(n, seed=23), np.array([paired(n, [0, 1, 2, 3, 4, 5], [1, 3, 4, 5], 0),           # k = 11
                                            paired(n, [0, 2], [0, 1, 2, 3, 4, 5], 2),                   # k = 9
                                            row(n, [0, 2, 4, 6, 8, 10, 12], 1), row(n, [1, 3, 5, 7, 9, 11, 12], 2)])))
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
        for i, r in enumerate(dat):
            present = np.zeros(2 * mod.n + 1, dtype=bool)
            present[Row(r, mod.n).codes] = True
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


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The rows of tests/golden/orders_big.npz, k = 15 ... 21: every one on the device (the 1 024-thread instantiation),
    evidence and prec at the bars of test_device_against_host_small_shapes against the host values the fixture holds."""
    device = {}
    for name, m in big_models():
        device[name] = m.mod.order_precedences(m.dat)
        assert m.mod.precedences_fallback_rows == 0
    check_big_rows("order_precedences", device, 1e-12)


def _check_identities(mod, dat, le, prec, post, tag):
    """The identities of prec with itself and with order_posteriors (le, pre) on the rows of dat."""
    n = mod.n
    S = 2 * n
    worst = {"sum": 0.0, "joint": 0.0, "seed": 0.0, "le": 0.0, "lo": 0.0, "hi": 0.0}
    for i, r in enumerate(dat):
        typ = int(r[-1])
        codes = Row(r, n).codes
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
        if r[S]:
            for c in codes[:-1]:
                e = c // 2
                joint = typ != 3 or (r[2 * e] and r[2 * e + 1])
                worst["seed"] = max(worst["seed"], abs(p[c, S] - (pre[e] if joint else 0.0)))
    worst["le"] = np.abs(le - post.log_evidence).max()
    print(f"identities, {tag}: {len(dat)} rows, worst {worst}")
    assert worst["sum"] <= 1e-12 and worst["joint"] <= 1e-12 and worst["seed"] <= 1e-12 and worst["le"] <= 1e-12
    assert worst["lo"] >= 0.0 and worst["hi"] <= 0.0                                       # every entry in [0, 1]


def _check_likeliest_orders(mod, dat, prec, tag):
    """Every pair the likeliest order places c before d has a positive posterior (rows with k <= 12)."""
    least = np.inf
    for i, (order, _) in enumerate(mod.likeliest_orders(dat)):
        t = Row(dat[i], mod.n).moments(order)
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
    dat = large_rows(9)
    mod = model(9, seed=31)
    got = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 0
    post = mod.order_posteriors(dat)
    _check_identities(mod, dat, got.log_evidence, got.prec, post, "synthetic n = 9")
    small = np.flatnonzero(dat[:, :-2].astype(int).sum(1) <= 12)
    assert len(small) == 5
    _check_likeliest_orders(mod, dat[small], got.prec[small], "synthetic n = 9")
    dat = large_rows(16)
    mod = model(16, seed=32)
    got = mod.order_precedences(dat)
    assert mod.precedences_fallback_rows == 0
    _check_identities(mod, dat, got.log_evidence, got.prec, mod.order_posteriors(dat), "one tumour n = 16")


@pytest.mark.gpu
def test_luad_rows_by_identities(golden):
    """LUAD-28 at the fit point: the 71 rows with k >= 15 (k = 21 among them), 300 rows with k <= 12 and up to 200 with
    k = 13, 14."""
    from metmhn_amd.jx import engine
    mod, dat = luad(golden, "fit")
    dat = dat[luad_selection(dat)]
    k = dat[:, :-2].astype(int).sum(1)
    le, prec, status = engine(mod.n).order_precedences(mod.log_theta, mod.obs1, mod.obs2, dat)
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
def test_too_large_rows_get_the_host_value(monkeypatch):
    """... with order_precedence: the k = 14 row (1.2 MiB, over the 1 MiB workspace), its host value against the device's."""
    mod, dat, ref, raw, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    S = 2 * mod.n
    have = ~np.isnan(host.prec)
    np.testing.assert_array_equal(have, ~np.isnan(ref.prec[0]))
    d_z = abs(np.exp(host.log_evidence) - np.exp(ref.log_evidence[0])) / np.exp(ref.log_evidence[0])
    d_p = np.abs(host.prec[have] - ref.prec[0][have]).max()
    print(f"host fallback, k = 14: rel. evidence {d_z:.2e}, prec {d_p:.2e} against the device")
    assert d_z <= 1e-12 and d_p <= 1e-12
    # cohort_mean: entry by entry over the rows that carry both codes
    mean = ref.cohort_mean()
    np.testing.assert_allclose(mean[0, 2], np.mean(ref.prec[:, 0, 2]), rtol=1e-15)            # every row carries 0 and 2
    np.testing.assert_allclose(mean[0, S], np.mean(ref.prec[:3, 0, S]), rtol=1e-15)           # the "absent" row has no seeding
    assert np.isnan(mean[9, 9]) and np.isnan(mean[0, 9]) and mean[0, 0] == 0.0                # no row carries code 9


@pytest.mark.gpu
def test_errors_name_the_row():
    check_errors_name_the_row(ENTRY)
