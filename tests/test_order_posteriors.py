"""Exact pre-seeding posteriors (MetMHN.order_posterior / order_posteriors, mmhn_order_posteriors).

Three independent anchors:
  * the host sum-product against the brute-force sum of MetMHN.likelihood (pinned to the reference by
    tests/golden/orders.npz) over every admissible order;
  * the device kernel against the host code, same summation order;
  * the device evidence against the likelihood engine (Engine.patient_grads), a second implementation of the model;
  * on rows of 15 - 21 slots (the 1 024-thread kernel), too slow for a live comparison, the device against the host values
    of tests/golden/orders_big.npz.
What order_posteriors shares with the other cohort entry points: order_common.check_* and tests/test_order_contract.py.

Bars (none taken from the code under test).  Every sum in both passes runs over non-negative terms, so nothing cancels:
the relative error of an output is a small multiple of (k + depth of the sums) x 2^-52, about 1e-14 at k = 21.  Device
against host 1e-12 relative on exp(log_evidence) and 1e-12 absolute on pre / seed_pos; host against enumeration 1e-12
relative; against patient_grads the project's bar for fp64 log-probs, 1e-9 relative on lp.  Every test prints the worst
value it saw before it asserts.  (The count holds for sums formed by trees, as the kernels form them.  The host code of
order_precedence, order_position and order_time adds the 2^(k-1) masses of a paired row one after the other: on the rows
with k = 19 ... 21 of tests/golden/orders_big.npz its own rounding, measured against math.fsum of the same terms, is a few
1e-13, and that is what the comparison with the device then shows - up to 0.69 of the 1e-12 bar)
"""
import itertools
import warnings

import numpy as np
import pytest

from metmhn_amd.state import MetState
from order_common import (ENTRIES, all_orders, big_models, check_arguments_before_the_library, check_big_rows,
                          check_errors_name_the_row, check_too_large_rows_get_the_host_value, luad, mixed_cohort, model,
                          random_paired_states, row)

ENTRY = ENTRIES["order_posteriors"]


def _enumerate(mod, slots, status, first):
    """(evidence, pre [n], seed_pos [n+1]) by brute force over MetMHN.likelihood."""
    n = mod.n
    if status == "isPaired":
        orders = all_orders(MetState(slots, size=2 * n + 1))
    else:
        orders = itertools.permutations(sorted(slots))
    Z, pre, pos = 0.0, np.zeros(n), np.zeros(n + 1)
    for o in orders:
        p = mod.likelihood(o, status, first)
        Z += p
        if 2 * n in o:
            before = {e // 2 for e in o[:o.index(2 * n)]}
            pos[len(before)] += p
            for m in before:
                pre[m] += p
    return Z, pre / Z, pos / Z


def test_arguments_are_checked_before_the_library(monkeypatch):
    check_arguments_before_the_library(ENTRY, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration(n):
    """exp(log_evidence) = the sum of MetMHN.likelihood over every admissible order, pre[m] = the likelihood-weighted
    share of the orders with m before the seeding; the edge masses sum to the evidence (seed_pos sums to 1)."""
    worst = {"Z": 0.0, "pre": 0.0, "pos": 0.0, "edges": 0.0}
    cases = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for mod, slots, _ in random_paired_states(n, 40 + n, (200 + 10 * n, 201 + 10 * n), 8):
            S = 2 * n
            todo = [(slots + [S], "isPaired", f) for f in ("PT", "Met", "unknown", "sync")]
            todo += [([s for s in slots if s % 2 == 1] + [S], "isMetastasis", None),
                     ([s for s in slots if s % 2 == 0] + [S], "present", None),
                     ([s for s in slots if s % 2 == 0], "absent", None)]
            for sl, status, first in todo:
                got = mod.order_posterior(MetState(sl, size=2 * n + 1), status, first)
                Z, pre, pos = _enumerate(mod, sl, status, first)
                cases += 1
                worst["Z"] = max(worst["Z"], abs(np.exp(got.log_evidence) - Z) / Z)
                assert abs(np.exp(got.log_evidence) - Z) <= 1e-12 * Z, (sl, status, first)
                if status == "absent":
                    assert np.all(np.isnan(got.pre)) and np.all(np.isnan(got.seed_pos))
                    continue
                worst["pre"] = max(worst["pre"], np.abs(got.pre - pre).max())
                worst["pos"] = max(worst["pos"], np.abs(got.seed_pos - pos).max())
                worst["edges"] = max(worst["edges"], abs(got.seed_pos.sum() - 1.0))
                np.testing.assert_allclose(got.pre, pre, rtol=1e-12, atol=1e-15)
                np.testing.assert_allclose(got.seed_pos, pos, rtol=1e-12, atol=1e-15)
                assert abs(got.seed_pos.sum() - 1.0) <= 1e-12          # sum of the seeding-edge masses = Z
    print(f"host against enumeration, n = {n}: {cases} cases, worst {worst}")
    assert cases == 2 * 8 * 7


def _check_device_host(mod, dat, sel, tag):
    dev = mod.order_posteriors(dat[sel])
    assert mod.posteriors_fallback_rows == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        host = mod.order_posteriors(dat[sel], backend="host")
    rel = np.abs(np.exp(dev.log_evidence) - np.exp(host.log_evidence)) / np.exp(host.log_evidence)
    seeded = dat[sel][:, -1] != 0
    assert np.all(np.isnan(dev.pre[~seeded])) and np.all(np.isnan(dev.seed_pos[~seeded]))
    assert np.all(np.isnan(host.pre[~seeded])) and np.all(np.isnan(host.seed_pos[~seeded]))
    d_pre = np.abs(dev.pre[seeded] - host.pre[seeded]).max()
    d_pos = np.abs(dev.seed_pos[seeded] - host.seed_pos[seeded]).max()
    print(f"device against host, {tag}: {len(sel)} rows, worst rel. evidence {rel.max():.2e}, pre {d_pre:.2e}, "
          f"seed_pos {d_pos:.2e}")
    assert rel.max() <= 1e-12
    assert d_pre <= 1e-12 and d_pos <= 1e-12


@pytest.mark.gpu
def test_device_against_host_luad28(golden):
    """The 4 781 rows of LUAD-28 with k <= 14: every type and every first observation."""
    mod, dat = luad(golden, "fit")
    k = dat[:, :-2].astype(int).sum(1)
    sel = np.flatnonzero(k <= 14)
    assert len(sel) == 4781
    assert set(np.unique(dat[sel][:, -1])) == {0, 1, 2, 3}
    assert set(np.unique(dat[sel][dat[sel][:, -1] == 3][:, -2])) >= {0, 1, 2}
    _check_device_host(mod, dat, sel, "LUAD-28 fit, k <= 14")


@pytest.mark.gpu
def test_device_against_host_mixed_cohorts():
    for n, seed in ((4, 3), (5, 4)):
        mod = model(n, seed)
        dat = mixed_cohort(n) if n == 5 else np.array(
            [row(4, [0, 1, 2, 3, 8], 3, d) for d in (0, 1, 2)] + [row(4, [8], 3, 0), row(4, [0, 2, 6, 8], 1),
                                                                 row(4, [1, 3, 5, 7, 8], 2), row(4, [0, 2, 4, 6], 0)])
        _check_device_host(mod, dat, np.arange(len(dat)), f"mixed cohort n = {n}")


@pytest.mark.gpu
def test_big_rows_against_host_values():
    """The rows of tests/golden/orders_big.npz, k = 15 ... 21: every one on the device (the 1 024-thread instantiation),
    evidence, pre and seed_pos at the bars of _check_device_host against the host values the fixture holds."""
    device = {}
    for name, m in big_models():
        device[name] = m.mod.order_posteriors(m.dat)
        assert m.mod.posteriors_fallback_rows == 0
    check_big_rows("order_posteriors", device, 1e-12)


@pytest.fixture(scope="module")
def luad_runs(golden):
    """order_posteriors of the whole LUAD-28 cohort at both parameter points, with the raw device outputs."""
    from metmhn_amd.jx import engine
    out = {}
    for prefix in ("fit", "indep"):
        mod, dat = luad(golden, prefix)
        le, pre, sp, status = engine(mod.n).order_posteriors(mod.log_theta, mod.obs1, mod.obs2, dat)
        out[prefix] = (mod, dat, le, pre, sp, status)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", ["fit", "indep"])
def test_evidence_against_the_likelihood_engine(luad_runs, prefix):
    """All 4 852 rows (k up to 21): log_evidence[i] is lp[i] of Engine.patient_grads, an independent implementation."""
    from metmhn_amd.engine import Engine
    mod, dat, le, pre, sp, status = luad_runs[prefix]
    assert len(dat) == 4852 and dat[:, :-2].astype(int).sum(1).max() == 21
    assert np.all(status == 0)
    with Engine(mod.n) as eng:
        eng.set_cohort(dat)
        lp = eng.patient_grads(mod.log_theta, mod.obs1, mod.obs2, with_grad=False)
    rel = np.abs(le - lp) / np.abs(lp)
    print(f"evidence against patient_grads, {prefix}: worst rel. difference of lp {rel.max():.2e} (row {rel.argmax()})")
    assert rel.max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", ["fit", "indep"])
def test_invariants(luad_runs, prefix):
    mod, dat, le, pre, sp, status = luad_runs[prefix]
    n = mod.n
    seeded = dat[:, -1] != 0
    assert np.all(np.isnan(pre[~seeded])) and np.all(np.isnan(sp[~seeded])) and np.all(np.isfinite(le))
    pre, sp, rows = pre[seeded], sp[seeded], dat[seeded]
    print(f"invariants, {prefix}: |sum seed_pos - 1| {np.abs(sp.sum(1) - 1).max():.2e}, "
          f"|mean - sum pre| {np.abs(sp @ np.arange(n + 1) - pre.sum(1)).max():.2e}")
    assert np.abs(sp.sum(1) - 1.0).max() <= 1e-12
    assert np.abs(sp @ np.arange(n + 1) - pre.sum(1)).max() <= 1e-12 * n
    print(f"invariants, {prefix}: pre in [{pre.min():.3e}, 1 - {1.0 - pre.max():.3e}], seed_pos >= {sp.min():.3e}")
    assert pre.min() >= 0.0 and pre.max() <= 1.0 and sp.min() >= 0.0
    pt, mt = rows[:, 0:2 * n:2] != 0, rows[:, 1:2 * n:2] != 0
    typ = rows[:, -1][:, None]
    carried = np.where(typ == 3, pt & mt, np.where(typ == 2, mt, pt))
    assert np.all(pre[~carried] == 0.0)
    # what the likeliest order puts before the seeding has a positive posterior
    k = dat[:, :-2].astype(int).sum(1)
    sub = np.flatnonzero(seeded & (k <= 12))[:400]
    orders = mod.likeliest_orders(dat[sub])
    pre_all = luad_runs[prefix][3]
    for i, (order, _) in zip(sub, orders):
        for e in order[:order.index(2 * n)]:
            assert pre_all[i, e // 2] > 0.0, (i, order)


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """... with order_posterior: the k = 17 row (9.5 MiB, over the 8 MiB workspace), its host value against the device's."""
    mod, dat, ref, raw, host = check_too_large_rows_get_the_host_value(ENTRY, monkeypatch)
    assert abs(np.exp(host.log_evidence) - np.exp(ref.log_evidence[0])) <= 1e-12 * np.exp(ref.log_evidence[0])
    assert np.abs(host.pre - ref.pre[0]).max() <= 1e-12 and np.abs(host.seed_pos - ref.seed_pos[0]).max() <= 1e-12
    seeded = dat[:, -1] != 0
    np.testing.assert_allclose(ref.cohort_preseeding(), ref.pre[seeded].mean(0), rtol=0, atol=0)


@pytest.mark.gpu
def test_errors_name_the_row():
    check_errors_name_the_row(ENTRY)
