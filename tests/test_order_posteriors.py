"""Exact pre-seeding posteriors (MetMHN.order_posterior / order_posteriors, mmhn_order_posteriors).

Three independent anchors:
  * the host sum-product against the brute-force sum of MetMHN.likelihood (pinned to the reference by
    tests/golden/orders.npz) over every admissible order;
  * the device kernel against the host code, same summation order;
  * the device evidence against the likelihood engine (Engine.patient_grads), a second implementation of the model.

Bars (none taken from the code under test).  Every sum in both passes runs over non-negative terms, so nothing cancels:
the relative error of an output is a small multiple of (k + depth of the sums) x 2^-52, about 1e-14 at k = 21.  Device
against host 1e-12 relative on exp(log_evidence) and 1e-12 absolute on pre / seed_pos; host against enumeration 1e-12
relative; against patient_grads the project's bar for fp64 log-probs, 1e-9 relative on lp.  Every test prints the worst
value it saw before it asserts.
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
DIAG_ORDER = {"unknown": 0, "PT": 1, "Met": 2}


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


def _mixed_cohort(n=5):
    S = 2 * n
    rows = [_row(n, [0, 4, 6], 0), _row(n, [], 0), _row(n, [2, 4, 8, S], 1), _row(n, [S], 1),
            _row(n, [1, 5, 9, S], 2), _row(n, [S], 2)]
    for d in (0, 1, 2, -99):
        rows += [_row(n, [0, 1, 2, 5, 6, 7, S], 3, d), _row(n, [0, 1, 4, 5, 3, S], 3, d), _row(n, [1, S], 3, d)]
    return np.array(rows)


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


def _enumerate(mod, slots, status, first):
    """(evidence, pre [n], seed_pos [n+1]) by brute force over MetMHN.likelihood."""
    n = mod.n
    if status == "isPaired":
        orders = _paired_orders(MetState(slots, size=2 * n + 1))
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


# ---------------------------------------------------------------------------------------------------- CPU
def test_abi_carries_the_symbol_and_version_8():
    hdr = open(os.path.join(ROOT, "include", "metmhn_amd.h")).read()
    assert "mmhn_order_posteriors" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["mmhn_order_posteriors"]) == 11
    assert re.search(r"\bint mmhn_order_posteriors\s*\(", hdr)
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define MMHN_ABI_VERSION (\d+)", hdr).group(1))


def test_arguments_are_checked_before_the_library(monkeypatch):
    import metmhn_amd.jx as jx

    def no_engine(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(jx, "engine", no_engine)
    mod = _model()
    dat = _mixed_cohort(mod.n)
    for bad in (dat[0], dat[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=r"dat must have shape \[n_pat, 13\]"):
            mod.order_posteriors(bad)
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'"):
        mod.order_posteriors(dat, backend="cpu")
    with pytest.raises(ValueError, match="met_status must be one of"):
        mod.order_posterior(MetState([0, 1, 10], size=11), "paired")
    with pytest.raises(ValueError, match="first_obs must be one of"):
        mod.order_posterior(MetState([0, 1, 10], size=11), "isPaired", "first")


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_host_against_enumeration(n):
    """exp(log_evidence) = the sum of MetMHN.likelihood over every admissible order, pre[m] = the likelihood-weighted
    share of the orders with m before the seeding; the edge masses sum to the evidence (seed_pos sums to 1)."""
    rng = np.random.default_rng(40 + n)
    worst = {"Z": 0.0, "pre": 0.0, "pos": 0.0, "edges": 0.0}
    cases = 0
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
    mod, dat = _luad(golden, "fit")
    k = dat[:, :-2].astype(int).sum(1)
    sel = np.flatnonzero(k <= 14)
    assert len(sel) == 4781
    assert set(np.unique(dat[sel][:, -1])) == {0, 1, 2, 3}
    assert set(np.unique(dat[sel][dat[sel][:, -1] == 3][:, -2])) >= {0, 1, 2}
    _check_device_host(mod, dat, sel, "LUAD-28 fit, k <= 14")


@pytest.mark.gpu
def test_device_against_host_mixed_cohorts():
    for n, seed in ((4, 3), (5, 4)):
        mod = _model(n, seed)
        dat = _mixed_cohort(n) if n == 5 else np.array(
            [_row(4, [0, 1, 2, 3, 8], 3, d) for d in (0, 1, 2)] + [_row(4, [8], 3, 0), _row(4, [0, 2, 6, 8], 1),
                                                                  _row(4, [1, 3, 5, 7, 8], 2), _row(4, [0, 2, 4, 6], 0)])
        _check_device_host(mod, dat, np.arange(len(dat)), f"mixed cohort n = {n}")


@pytest.fixture(scope="module")
def luad_runs(golden):
    """order_posteriors of the whole LUAD-28 cohort at both parameter points, with the raw device outputs."""
    from metmhn_amd.jx import engine
    out = {}
    for prefix in ("fit", "indep"):
        mod, dat = _luad(golden, prefix)
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
def test_bitwise_reproducible_and_batching(luad_runs):
    from metmhn_amd.engine import Engine
    from metmhn_amd.jx import engine
    mod, dat, le, pre, sp, status = luad_runs["indep"]
    args = (mod.log_theta, mod.obs1, mod.obs2)
    again = engine(mod.n).order_posteriors(*args, dat)
    for x, y in zip((le, pre, sp, status), again):
        np.testing.assert_array_equal(x, y)
    k = dat[:, :-2].astype(int).sum(1)
    keep = np.flatnonzero(k <= 16)
    perm = np.random.default_rng(5).permutation(keep)
    with Engine(mod.n, workspace_bytes=8 << 20) as small:          # a k = 16 paired row needs 4.75 MiB: many batches
        b = small.order_posteriors(*args, dat[perm])
        for x, y in zip((le, pre, sp, status), b):
            np.testing.assert_array_equal(x[perm], y)
        # a lattice larger than the whole workspace is turned away per row, the rest of the call goes on
        big = np.flatnonzero((dat[:, -1] == 3) & (k == 18))[:1]
        rows = np.vstack((dat[big], dat[keep[:5]]))
        ble, bpre, bsp, bst = small.order_posteriors(*args, rows)
        assert bst[0] == 3 and np.all(bst[1:] == 0)
        assert np.isnan(ble[0]) and np.all(np.isnan(bpre[0])) and np.all(np.isnan(bsp[0]))
        np.testing.assert_array_equal(ble[1:], le[keep[:5]])


@pytest.mark.gpu
def test_too_large_rows_get_the_host_value(monkeypatch):
    """The Python layer recomputes MMHN_ORD_TOO_LARGE rows with order_posterior and counts them."""
    import metmhn_amd.jx as jx
    from metmhn_amd.engine import Engine
    n = 9
    mod = _model(n, seed=11)
    S = 2 * n
    wide = _row(n, list(range(16)) + [S], 3, 0)                    # k = 17: 9.5 MiB, over the 8 MiB limit below
    dat = np.vstack((wide[None], [_row(n, [0, 1, 2, 3, 6, S], 3, 1), _row(n, [0, 2, S], 1), _row(n, [0, 2], 0)]))
    ref = mod.order_posteriors(dat)
    assert mod.posteriors_fallback_rows == 0
    with Engine(n, workspace_bytes=8 << 20) as small:
        assert small.order_posteriors(mod.log_theta, mod.obs1, mod.obs2, dat)[3].tolist() == [3, 0, 0, 0]
        monkeypatch.setattr(jx, "engine", lambda n_mut: small)
        got = mod.order_posteriors(dat)
    assert mod.posteriors_fallback_rows == 1
    host = mod.order_posterior(MetState.from_seq(wide[:S + 1]), "isPaired", "unknown")
    assert got.log_evidence[0] == host.log_evidence
    np.testing.assert_array_equal(got.pre[0], host.pre)
    np.testing.assert_array_equal(got.seed_pos[0], host.seed_pos)
    np.testing.assert_array_equal(got.log_evidence[1:], ref.log_evidence[1:])
    np.testing.assert_array_equal(got.pre[1:], ref.pre[1:])
    assert abs(np.exp(got.log_evidence[0]) - np.exp(ref.log_evidence[0])) <= 1e-12 * np.exp(ref.log_evidence[0])
    assert np.abs(got.pre[0] - ref.pre[0]).max() <= 1e-12 and np.abs(got.seed_pos[0] - ref.seed_pos[0]).max() <= 1e-12
    seeded = dat[:, -1] != 0
    np.testing.assert_allclose(ref.cohort_preseeding(), ref.pre[seeded].mean(0), rtol=0, atol=0)


@pytest.mark.gpu
def test_errors_name_the_row():
    from metmhn_amd.engine import Engine
    mod = _model()
    n = mod.n
    good = _mixed_cohort(n)
    # one row per MMHN_ORD_* reason, in the order of the enum (1 ... 7)
    bad = [_row(n, [0], 5), _row(n, [0, 3], 3, 1), _row(n, [0, 1], 3, 0), _row(n, [0, 1, 2 * n], 2), _row(n, [1, 3], 2),
           _row(n, [1], 0), _row(n, [0, 1, 2 * n], 1)]
    for reason, b in enumerate(bad, start=1):
        dat = np.vstack((good[:3], b[None], good[3:]))
        with pytest.raises(ValueError) as lo_err:
            mod.likeliest_orders(dat)
        with pytest.raises(ValueError) as dev_err:
            mod.order_posteriors(dat)
        assert str(dev_err.value) == str(lo_err.value) == f"row 3: {_ROW_ERRORS[reason]}"
        with pytest.raises(ValueError, match=r"^row 3: "):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                mod.order_posteriors(dat, backend="host")
    with Engine(n, dtype="f32") as e32:
        with pytest.raises(RuntimeError, match="fp64"):
            e32.order_posteriors(mod.log_theta, mod.obs1, mod.obs2, good)
