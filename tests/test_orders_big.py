"""tests/golden/orders_big.npz (tests/tools/make_golden_orders_big.py): the host values of rows with k = 15 ... 21 that the
GPU tests test_big_rows_against_host_values of the order family's files compare the 1 024-thread kernels with.  Here, without
a GPU: the fixture still is what the host code computes, and the comparator those tests share would notice an error.

Bars.  The drift guard recomputes with the code and the inputs that wrote the fixture, so it expects the same bits; it
allows 1e-13 (absolute on probabilities and times, which are O(1); relative on exp(log_evidence)) for a NumPy whose sums
or exp round differently.  The comparator is handed an error of 1e-9, a thousand bars.
"""
import numpy as np
import pytest

from order_common import (BIG_ENTRIES, BIG_MODELS, BIG_SAMPLES, FIRST, KEY, Row, big_host, big_host_samples, big_rows,
                          check_big_rows, host_only)

BARS = {"order_posteriors": 1e-12, "order_precedences": 1e-12, "order_positions": 1e-12, "order_times": 1e-12,
        "order_snapshots": 1e-12}                 # the device-against-host bars of the entry points' own files


def test_fixture_covers_the_rows_it_is_for():
    """k = 15 ... 21 and nothing below, all four row types, every diagnosis order, paired rows without a joint event and
    of joint events only, the k = 21 row of LUAD-28."""
    big = big_rows()
    ks, types, orders, joint = set(), set(), set(), set()
    for name, n, _ in BIG_MODELS:
        dat = big[name].dat
        k = dat[:, :-2].astype(int).sum(1)
        ks |= set(k.tolist())
        types |= set(dat[:, -1].tolist())
        for r in dat[dat[:, -1] == 3]:
            orders.add(int(r[-2]))
            w = Row(r, n)
            kj = len(set(w.lineages["pt"][:-1]) & {c - 1 for c in w.lineages["mt"][:-1]})
            joint.add("none" if kj == 0 else "all" if 2 * kj + 1 == len(w.codes) else "some")
    print(f"orders_big: {big['rows']} rows, k in {sorted(ks)}, types {sorted(types)}, diagnosis orders {sorted(orders)}")
    assert ks == set(range(15, 22)) and types == {0, 1, 2, 3} and orders == {0, 1, 2, -99}
    assert joint == {"none", "some", "all"}
    assert big["rows"] < 60


def test_host_code_still_gives_the_fixture(host_only):
    """Drift guard: the cheapest row of the fixture, the first paired row with k = 15, once more through every
    one-observation method of the host code.  An edit of model.py that moves the host values fails here, not as a device
    error on the GPU."""
    m = big_rows()["n9"]
    i = 0
    assert m.dat[i, -1] == 3 and m.dat[i, :-2].sum() == 15
    args = m.mod._row_args(m.dat, i)
    worst = {}
    for entry, (_, single, _, fields) in BIG_ENTRIES.items():
        got, want = getattr(m.mod, single)(*args), big_host(entry, "n9", rows=[i])
        zg, zw = np.exp(got.log_evidence), np.exp(want.log_evidence[0])
        worst[entry] = abs(zg - zw) / zw
        for f in fields:
            g, w = np.asarray(getattr(got, f)), getattr(want, f)[0]
            assert g.shape == w.shape, (entry, f)
            if f in ("map_state", "map_first"):
                np.testing.assert_array_equal(g, w, err_msg=f"{entry}: {f}")
                continue
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{entry}: {f}")
            worst[entry] = max(worst[entry], float(np.nanmax(np.abs(g - w), initial=0.0)))
    le, orders, log_prob, margin = big_host_samples("n9")
    s = m.mod.sample_order(*args, n_samples=BIG_SAMPLES, key=KEY + m.n, first=FIRST, row=i)
    np.testing.assert_array_equal(s.orders, orders[i])
    worst["sample_orders"] = max(float(np.abs(s.log_prob - log_prob[i]).max()), float(np.abs(s.margin - margin[i]).max()),
                                 abs(s.log_evidence - le[i]))
    print(f"host code against the fixture, row {i} of n9 (paired, k = 15): worst difference {worst}")
    assert max(worst.values()) <= 1e-13


def _moved(entry, name, change):
    """The fixture's own values as a device result, those of model `name` copied and handed to `change`."""
    device = {n: big_host(entry, n) for n, _, _ in BIG_MODELS}
    _, _, cls, fields = BIG_ENTRIES[entry]
    device[name] = cls(*(getattr(device[name], f).copy() for f in ("log_evidence",) + fields))
    change(device[name])
    return device


def test_comparator_notices_an_error():
    """check_big_rows passes the fixture's own values; with one entry of one row moved by 1e-9, and with one NaN where a
    value belongs, it fails - for every entry point and in every model."""
    cases = 0
    for entry, (_, _, _, fields) in BIG_ENTRIES.items():
        worst = check_big_rows(entry, {n: big_host(entry, n) for n, _, _ in BIG_MODELS}, BARS[entry])
        assert max(worst.values()) == 0.0
        field = fields[0]
        for name, _, _ in BIG_MODELS:
            have = np.argwhere(~np.isnan(getattr(big_host(entry, name), field)))
            at = tuple(have[len(have) // 2])                          # a value in the middle of the model's rows

            def shift(res):
                getattr(res, field)[at] += 1e-9

            def lose(res):
                getattr(res, field)[at] = np.nan

            def evidence(res):
                res.log_evidence[at[0]] += 1e-9

            def fewer(res):
                for f in ("log_evidence",) + fields:
                    setattr(res, f, getattr(res, f)[:-1])
            for change in (shift, lose, evidence, fewer):
                with pytest.raises(AssertionError):
                    check_big_rows(entry, _moved(entry, name, change), BARS[entry])
                cases += 1
    # the chosen snapshot: one held / still-to-come flag of one row
    def flip(res):
        i = int(np.flatnonzero(res.map_first >= 0)[0])
        c = int(np.flatnonzero(res.map_state[i] >= 0)[0])
        res.map_state[i, c] ^= 1
    with pytest.raises(AssertionError):
        check_big_rows("order_snapshots", _moved("order_snapshots", "luad", flip), BARS["order_snapshots"])
    print(f"comparator: the fixture passes for {len(BIG_ENTRIES)} entry points, {cases + 1} altered results fail")
