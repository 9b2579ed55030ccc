"""The engine at its size limits: n_mut = 31 (MAXN = 32 events with the seeding, dat of 65 columns, event codes up to 62)
through every entry-point family, the rows the planner refuses, and the largest shape of each route of the joint solves
up to k = 27.  Spaces of 28 - 30 bits are accepted by the planner (tests/host/plan_check.hip checks their sizes) and are
not compared with a reference anywhere: the C port needs tens of seconds and tens of GB for one of them.

The references are the C ports (oracle/metmhn_ref.c, oracle/metmhn_fast.c); the first test, on the CPU, pins both to the
Python oracle at n = 31, where their fixed arrays are full to the last element.  Every bar is the bar of the existing test
of the same route and dtype, named where it is used; every comparison prints its worst ratio to its bar."""
import re
import time
import warnings

import numpy as np
import pytest

from eval_common import FP32_BAR, WINDOW_TOL, close, close_grads, close_to_largest, fp32_grads, paired, patient_grads, row, shape_rows, top_rows
from order_common import BAR, MARGIN, MAX_EXCLUDED, same_or_tie, snapshots_diff, snapshots_patterns, times_diff, times_orderings

N31 = 31
BAD_N = "n_mut must be in [1, 31]"
TOO_MANY = "too many active events for one patient"
TOO_MANY_SIM = "too many events for the sampler (n_mut <= 30: event and diagnosis flags share one 32-bit set)"


# ---------------------------------------------------------------------------------------------------- helpers
def _fails_with(text):
    """the call raises with exactly this text of mmhn_last_error (the bindings put the package's name in front)"""
    return pytest.raises(RuntimeError, match="^" + re.escape("metmhn_amd: " + text) + "$")


def _refused_rows():
    """(n, row, what): single-tumour spaces of more than MAXK = 30 bits, and a joint one"""
    return [(31, row(31, range(31), [], 0, -99, 0), "type 0, 31 PT events (k = 31)"),
            (31, row(31, range(31), [], 1, -99, 1), "type 1, 31 PT events and the seeding (k = 32)"),
            (30, row(30, [], range(30), 1, -99, 2), "type 2, 30 MT events and the seeding (k = 31)"),
            (31, paired(31, range(16), range(16, 31), 0), "paired, 16 PT and 15 MT events and the seeding (k = 32)")]


def _fixed_rows():
    n = N31
    rows = [row(n, [], [], 0, -99, 0), row(n, [], [], 1, -99, 1), row(n, [], [], 1, -99, 2)]
    for order in (0, 1, 2):
        rows += [paired(n, [], [], order), paired(n, [30], [], order), paired(n, [], [30], order), paired(n, [30], [30], order)]
    return rows


# ---------------------------------------------------------------------------------------------------- CPU: the C ports
def test_c_ports_at_n31_against_the_python_oracle():
    """oracle/metmhn_ref.c (cref.patients, every row type) and oracle/metmhn_fast.c (cref.fast_patients, paired rows) against
    oracle/metmhn_oracle.py's score_and_grad of each row alone (one row: weight 1, the score is the row's log-probability)
    at n = 31, N = 32: rows with k <= 8 that carry the events 29 and 30 and the seeding, log-probabilities and every
    gradient entry to 1e-10 (relative, and absolute for the entries that are zero)."""
    from oracle import cref, metmhn_oracle as O
    from metmhn_amd import synthetic
    n = N31
    lt, dp, dm = synthetic.random_params(n, seed=3131)
    rng = np.random.default_rng(31)
    rows = []
    for i in range(16):
        low = [int(e) for e in rng.choice(29, size=int(rng.integers(0, 3)), replace=False)]
        typ = i % 4
        if typ == 3:
            pt, mt = low[:1] + [29, 30][:1 + i // 4 % 2], low[1:] + [30, 29][:1 + i // 8]
            rows.append(paired(n, pt, mt, [0, 1, 2, -99][i // 4]))
        elif typ == 2:
            rows.append(row(n, [], low + [29, 30], 1, -99, 2))
        else:
            rows.append(row(n, low + [29, 30], [], typ, -99, typ))
    rows += [paired(n, [0, 29, 30], [29, 30], 0), paired(n, [29, 30], [1, 29, 30], 1), paired(n, [28, 29, 30], [30], 2),
             paired(n, [30], [28, 29], 2), row(n, [], [], 0, -99, 0), paired(n, [], [], 0)]
    dat = np.array(rows, dtype=np.int8)
    k = dat[:, :2 * n + 1].astype(int).sum(1)
    assert len(dat) >= 20 and k.max() <= 8
    carry = (dat[:, 58] | dat[:, 59]) & (dat[:, 60] | dat[:, 61]) & dat[:, 62]
    assert carry.sum() >= 16
    t0 = time.perf_counter()
    ref = [O.score_and_grad(lt, dp, dm, dat[i:i + 1], 0.5) for i in range(len(dat))]
    ref = [np.array([np.asarray(r[j], dtype=np.float64) for r in ref]) for j in range(4)]
    print(f"[limits] Python oracle, {len(dat)} rows at n = 31: {time.perf_counter() - t0:.1f} s")
    assert ref[1].shape == (len(dat), n + 1, n + 1) and ref[2].shape == ref[3].shape == (len(dat), n + 1)
    bar = (1e-10, 1e-10)
    close_grads("metmhn_ref.c at n = 31", cref.patients(lt, dp, dm, dat, with_grad=True), ref, bar, bar)
    both = dat[:, -1] == 3
    close_grads("metmhn_fast.c at n = 31", cref.fast_patients(lt, dp, dm, dat[both]), [r[both] for r in ref], bar, bar)


# ---------------------------------------------------------------------------------------------------- GPU: n_mut = 31
@pytest.mark.gpu
def test_limits_are_refused_before_any_launch():
    """The event count, the rows of more than MAXK = 30 slots in one space (refused by the planner on the host, with the
    message of the joint case) and the sampler's own limit, each with its whole message.  The engine that refused a cohort
    has none, although it held one before: it evaluates zero rows and counts zero patients (include/metmhn_amd.h: "leaves the
    engine without a cohort"), and evaluates the next valid one."""
    from oracle import cref
    from metmhn_amd import Engine, synthetic
    with _fails_with(BAD_N):
        Engine(32)
    valid = {n: np.array([paired(n, [0, n - 1], [n - 1], 0), row(n, [n - 1], [], 1, -99, 1)], dtype=np.int8) for n in (30, 31)}
    for n, bad, what in _refused_rows():
        lt, dp, dm = synthetic.random_params(n, seed=n)
        want = cref.patients(lt, dp, dm, valid[n], with_grad=False)[0]
        with Engine(n) as e:
            for dat in (bad[None], np.vstack((valid[n], bad[None])), np.vstack((valid[n][:1], bad[None], valid[n][1:]))):
                e.set_cohort(valid[n])
                with _fails_with(TOO_MANY):
                    e.set_cohort(dat)
                assert e.patient_grads(lt, dp, dm, with_grad=False).shape == (0,), what
                sums = e.cohort_sums(lt, dp, dm, with_grad=False)     # (score of the EM rows, of the NM rows, n_em, n_pat, ...)
                assert sums[2] == 0 and sums[3] == 0 and sums[0] == 0 and sums[1] == 0, (what, sums[:4])
            e.set_cohort(valid[n])
            close(f"after refusing {what}: lp", e.patient_grads(lt, dp, dm, with_grad=False), want, 1e-9, 1e-12)
    lt, dp, dm = synthetic.random_params(N31, seed=1)
    with Engine(N31) as e:
        for call in (lambda: e.simulate(lt, dp, dm, 16, seed=1), lambda: e.simulate_summary(lt, dp, dm, 16, seed=1),
                     lambda: e.simulate_pairs(lt, dp, dm, 16, seed=1)):
            with _fails_with(TOO_MANY_SIM):
                call()
    with Engine(30) as e:                                                          # the largest event count it takes
        lt, dp, dm = synthetic.random_params(30, seed=2)
        counts = e.simulate_summary(lt, dp, dm, 64, seed=1)
        assert counts[0] == 64 and counts.shape == (4 + 5 * 30,)


@pytest.fixture(scope="module")
def top_cohort():
    """(lt, dp, dm, dat, reference): 60 generated rows and the fixed ones at n = 31 with metmhn_ref.c's results"""
    from oracle import cref
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(N31, seed=131)
    dat = np.array(top_rows(np.random.default_rng(20240831), 60) + _fixed_rows(), dtype=np.int8)
    k = dat[:, :2 * N31 + 1].astype(int).sum(1)
    assert k.max() <= 12 and k.max() >= 9 and set(dat[:, -1]) == {0, 1, 2, 3} and set(dat[dat[:, -1] == 3, -2]) == {0, 1, 2, 3, -99}
    assert dat[:, 54:62].sum() > 8 * dat[:, :54].sum() / 54                       # the slots of the events 27 .. 30 carry the weight
    return lt, dp, dm, dat, cref.patients(lt, dp, dm, dat, with_grad=True)


@pytest.mark.gpu
@pytest.mark.parametrize("pmin", ["1", "1000000"])
def test_cohort_at_n31_against_c_port(monkeypatch, top_cohort, pmin):
    """Every row type and order code (-99 and an invalid one among them) at n = 31, the fixed rows (all-zero, seeding only,
    event 30 alone in either tumour and in both), both kernel schedules, buffers NaN-poisoned; per-patient results against
    oracle/metmhn_ref.c at the bars of test_random_patients_against_c_oracle (lp 1e-9 / 1e-12, gradients 1e-8 / 1e-10).
    Row and column 31 of d_theta and the entries of events no row carries are compared like every other entry."""
    lt, dp, dm, dat, ref = top_cohort
    got = patient_grads(monkeypatch, N31, dat, (lt, dp, dm), MMHN_PSOLVE_MIN=pmin, MMHN_POISON="1")
    assert got[1].shape == (len(dat), 32, 32) and np.abs(ref[1][:, 31, :]).max() > 0 and np.abs(ref[1][:, :, 31]).max() > 0
    close_grads(f"n = 31 cohort, MMHN_PSOLVE_MIN={pmin}", got, ref, (1e-9, 1e-12), (1e-8, 1e-10))


@pytest.mark.gpu
def test_cohort_at_n31_fp32_against_fp64(top_cohort):
    """The same cohort on an fp32 engine against the fp64 engine: the weighted sums at the bar of
    test_fp32_engine_close_to_fp64 (score 2e-5, gradients 2e-3 / 2e-5)."""
    from metmhn_amd import Engine, distributed as D
    lt, dp, dm, dat, _ = top_cohort
    res = {}
    for dt in ("f64", "f32"):
        with Engine(N31, dtype=dt) as e:
            e.set_cohort(dat)
            res[dt] = D.combine_sums(e.cohort_sums(lt, dp, dm), N31 + 1, 0.5)
    close_grads("n = 31 cohort fp32", res["f32"], res["f64"], (2e-5, 0.0), FP32_BAR)


def _k20_chain_top(kr, kc, rows_p, seed):
    """tests/test_window_rows_gpu.py's k = 20 chains at n = 31 with the events 28 .. 30 in every row: three rows of one shape
    (kr row-class bits, kc column-class bits), orders 0 / 1 / 2; the row class carries 28 and 30, the column class 29 and 30"""
    return shape_rows(N31, kr, kc, rows_p, 3, seed, fixed=((28, 30), (29, 30)))


@pytest.mark.gpu
def test_window_route_at_n31(monkeypatch):
    """Two chains of three k = 20 rows of shape (12, 7), either class as rows, on the window route (MMHN_WSOLVE=1) and on the
    tile kernels (0), poisoned, against oracle/metmhn_fast.c at the bars of
    test_full_size_patients_against_optimised_cpu_variant (lp 1e-10, gradients 1e-7 / 1e-10)."""
    from oracle import cref
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(N31, seed=231)
    dat = np.array(_k20_chain_top(12, 7, True, 71) + _k20_chain_top(12, 7, False, 72), dtype=np.int8)
    assert (dat[:, :63].sum(1) == 20).all() and (dat[:, 56:62:2] | dat[:, 57:62:2]).all() and dat[:, [60, 61]].all()
    ref = cref.fast_patients(lt, dp, dm, dat)
    monkeypatch.setenv("MMHN_POISON", "1")
    monkeypatch.setenv("MMHN_TIME_KERNELS", "1")        # (6 * 2^20 states: launches are counted only when asked for)
    for ms in ("1", "0"):
        # window route: its own minimum lowered, so that a row it turned away would show on the tile route; without it: the
        # per-patient kernel from one problem on, as in tests/test_window_rows_gpu.py
        got, counters = patient_grads(monkeypatch, N31, dat, (lt, dp, dm), counters=True, MMHN_WSOLVE=ms, **_ROUTE_MIN[ms])
        if ms == "1":
            _assert_window_route("n = 31 window chains", counters)
        close_grads(f"n = 31 window chains, MMHN_WSOLVE={ms}", got, ref, (1e-10, 0.0), (1e-7, 1e-10))


# ---------------------------------------------------------------------------------------------------- GPU: the largest shapes
def _timed_reference(tag, lt, dp, dm, dat):
    from oracle import cref
    t0 = time.perf_counter()
    ref = cref.fast_patients(lt, dp, dm, dat)
    print(f"[limits] {tag}: metmhn_fast.c took {time.perf_counter() - t0:.1f} s for {len(dat)} rows on {cref.num_threads()} threads")
    return ref


# the minimum of the route under test at 1 and the other one at its default, by MMHN_WSOLVE
_ROUTE_MIN = {"1": {"MMHN_WSOLVE_MIN": "1", "MMHN_PSOLVE_MIN": None}, "0": {"MMHN_PSOLVE_MIN": "1", "MMHN_WSOLVE_MIN": None}}


def _joint_launches(counters):
    """timed launches of the joint solves by counter class (include/metmhn_amd.h, MMHN_K_*): (window and per-patient
    kernels forward, adjoint; tile route forward, adjoint).  They are counted in batches whose launches are timed: 2^26
    states or more, or MMHN_TIME_KERNELS=1."""
    return tuple(counters[c]["launches"] for c in ("psolve_fwd", "psolve_adj", "csolve_fwd", "csolve_adj"))


def _assert_window_route(tag, counters):
    """Every joint problem took the window route.  The caller leaves MMHN_PSOLVE_MIN at its default (384 multi-tile problems:
    no row of these cohorts takes the per-patient kernel, which counts in the same class), so a row that window_ok turned away
    would be on the tile route and show as a csolve launch."""
    pf, pa, cf, ca = _joint_launches(counters)
    print(f"[limits] {tag}: joint solve launches psolve {pf} / {pa}, csolve {cf} / {ca}, evals {counters['evals']}")
    assert counters["evals"] == 1 and pf >= 1 and pa == pf and cf == 0 and ca == 0, (tag, counters)


@pytest.mark.gpu
def test_largest_fp64_window_shape(monkeypatch):
    """(kR, kC) = (15, 9), k = 25: WCfg<double>::KR and KC both at their maximum, one row per class orientation, orders 0
    and 2.  The window layout read in place (MMHN_WSOLVE=1) against the same solves converted to index order (2) as in
    tests/test_wclass_external_rows.py's _check (WINDOW_TOL: 1e-12 of the largest entry), and against oracle/metmhn_fast.c at the fp64
    bars of test_window_layout_solves_match_cpu_port (lp 1e-10, gradients 1e-7 / 1e-10).  Measured: metmhn_fast.c takes
    1.5 s for the two rows on 16 threads (0.75 s per k = 25 row)."""
    from metmhn_amd import synthetic
    n = 25
    lt, dp, dm = synthetic.random_params(n)
    dat = np.array([paired(n, range(15), range(12, 21), 0), paired(n, range(2, 11), range(8, 23), 2)], dtype=np.int8)
    assert (dat[:, :2 * n + 1].sum(1) == 25).all()
    ref = _timed_reference("fp64 window corner, k = 25", lt, dp, dm, dat)
    monkeypatch.delenv("MMHN_PSOLVE_MIN", raising=False)
    monkeypatch.setenv("MMHN_WSOLVE_MIN", "1")          # (two window-shaped rows take the window route)
    monkeypatch.setenv("MMHN_POISON", "1")
    win, cw = patient_grads(monkeypatch, n, dat, (lt, dp, dm), counters=True, MMHN_WSOLVE="1")
    idx, ci = patient_grads(monkeypatch, n, dat, (lt, dp, dm), counters=True, MMHN_WSOLVE="2")
    _assert_window_route("(15, 9) fp64, MMHN_WSOLVE=1", cw)      # (2 * 2^25 states: the batch is timed)
    _assert_window_route("(15, 9) fp64, MMHN_WSOLVE=2", ci)
    close_to_largest("(15, 9) fp64 window layout against index order,", win, idx, WINDOW_TOL["f64"])
    close_grads("(15, 9) fp64 window layout against metmhn_fast.c", win, ref, (1e-10, 0.0), (1e-7, 1e-10))


@pytest.mark.gpu
def test_largest_fp32_window_shapes(monkeypatch):
    """n = k = 27 on the fp32 window route: (18, 8), WCfg<float>::KR at its maximum, and (14, 12), KC at its maximum (both
    pass wtab_fits), against oracle/metmhn_fast.c (fp64) at the bars of test_window_path_fp32_k25_shapes (lp 1e-4, gradients
    2e-3 |x| + 2e-5 componentwise), and again on the tile kernels (MMHN_WSOLVE=0).  Measured: metmhn_fast.c takes 6.7 s for
    the two rows on 16 threads (3.4 s per k = 27 row), most of this test's time."""
    from metmhn_amd import synthetic
    n = 27
    lt, dp, dm = synthetic.random_params(n)
    dat = np.array([paired(n, range(18), range(16, 24), 1), paired(n, range(3, 15), range(10, 24), 0)], dtype=np.int8)
    assert (dat[:, :2 * n + 1].sum(1) == 27).all()
    ref = _timed_reference("fp32 window corners, k = 27", lt, dp, dm, dat)
    monkeypatch.setenv("MMHN_POISON", "1")
    for ms in ("1", "0"):
        # (the window route's own minimum, so that a row it turned away would show on the tile route; MMHN_WSOLVE=0: the
        # per-patient kernel from one problem on)
        got, counters = patient_grads(monkeypatch, n, dat, (lt, dp, dm), dtype="f32", counters=True, MMHN_WSOLVE=ms, **_ROUTE_MIN[ms])
        if ms == "1":
            _assert_window_route("k = 27 fp32, (18, 8) and (14, 12)", counters)      # (2 * 2^27 states: the batch is timed)
        fp32_grads(f"k = 27 MMHN_WSOLVE={ms}", got, ref)


@pytest.mark.gpu
def test_largest_tile_route_problem(monkeypatch):
    """One paired row with k = 26 at n = 13 (every slot but one), order 0: the 16 384 tiles of one fp64 problem in one
    cooperative launch, and level by level (MMHN_COOP=0), against oracle/metmhn_fast.c at the bars of
    test_full_size_patients_against_optimised_cpu_variant (lp 1e-10, gradients 1e-7 / 1e-10).

    A cooperative launch whose wait timed out fails the call (the counters hold no abort word), so the call returning is
    the first half of "no abort"; the counters then show that the cooperative launch was what ran: one evaluation, one
    csolve launch forward and one adjoint, none of the window / per-patient class, and level by level one launch per
    popcount of the 14 tile-index bits, 15 each way.  The launches are counted because the batch has 2^26 states.  Their
    algorithmic bytes are one tile written per live tile: the 8 192 seeded tiles, and of the others those whose tile bits
    (the slots 12 .. 24: six PT / MT pairs and the PT-only event 12) have the pairs equal and event 12 unset, 2^6 = 64.

    Measured: metmhn_fast.c takes 1.9 s for the row on 16 threads, the engine 3.4 ms per evaluation."""
    from metmhn_amd import synthetic
    n = 13
    lt, dp, dm = synthetic.random_params(n)
    dat = np.array([paired(n, range(13), range(12), 0)], dtype=np.int8)
    assert dat[0, :2 * n + 1].sum() == 26
    ref = _timed_reference("tile route, k = 26", lt, dp, dm, dat)
    monkeypatch.setenv("MMHN_POISON", "1")
    monkeypatch.delenv("MMHN_COOP", raising=False)
    for coop in (None, "0"):
        got, counters = patient_grads(monkeypatch, n, dat, (lt, dp, dm), counters=True, MMHN_COOP=coop)
        print(f"[limits] k = 26 tile route, MMHN_COOP={coop}: counters {counters}")
        levels = 1 if coop is None else 15
        assert counters["evals"] == 1, counters
        assert _joint_launches(counters) == (0, 0, levels, levels), (coop, counters)
        live = (8192 + 64) * 4096 * 8.0
        assert counters["csolve_fwd"]["alg_bytes"] == live and counters["csolve_adj"]["alg_bytes"] == live, (coop, counters)
        close_grads(f"k = 26 tile route, MMHN_COOP={coop}", got, ref, (1e-10, 0.0), (1e-7, 1e-10))


# ---------------------------------------------------------------------------------------------------- GPU: the order family
@pytest.fixture(scope="module")
def order_cohort():
    """(model, dat) at n = 31: order_common.small_shapes_n8() with every event shifted up by 23 (events 23 .. 30, the seeding
    is code 62), then rows of 15 and 16 slots - the first sizes on the 1 024-thread side of the switch -, paired and of one
    tumour."""
    from order_common import model, paired, row, small_shapes_n8
    n = N31
    _, dat8 = small_shapes_n8()
    dat = np.zeros((len(dat8), 2 * n + 3), dtype=np.int8)
    dat[:, 46:62], dat[:, 62:] = dat8[:, :16], dat8[:, 16:]
    big = [paired(n, range(23, 30), range(24, 31), 0), paired(n, range(23, 31), range(24, 31), 2),
           row(n, [2 * i for i in range(17, 31)] + [2 * n], 1), row(n, [2 * i + 1 for i in range(16, 31)] + [2 * n], 2)]
    assert not dat[:, :46].any()
    dat = np.vstack((dat, big))
    k = dat[:, :-2].astype(int).sum(1)
    assert set(k.tolist()) >= {0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 15, 16}
    return model(n, seed=21), dat


def _host_run(mod, name, dat):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        return getattr(mod, name)(dat, backend="host")


def _bar(tag, **worst):
    """every figure against the order tests' bar, the worst ratio printed first"""
    bar = BAR
    print(f"[limits] {tag}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"; worst error / bar = {max(worst.values()) / bar:.3g}")
    for name, v in worst.items():
        assert v <= bar, (tag, name, v)


def _rel_evidence(dev, host):
    zd, zh = np.exp(np.asarray(dev.log_evidence)), np.exp(np.asarray(host.log_evidence))
    return float(np.max(np.abs(zd - zh) / zh))


def _worst_abs(a, b):
    """largest |a - b| where both hold a value; the NaN patterns must be the same"""
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    have = ~np.isnan(b)
    return float(np.abs(a[have] - b[have]).max(initial=0.0))


def _carried(dat, n):
    from order_common import Row
    out = np.zeros((len(dat), 2 * n + 1), dtype=bool)
    for i, r in enumerate(dat):
        out[i, Row(r, n).codes] = True
    return out


@pytest.mark.gpu
def test_likeliest_orders_at_n31(order_cohort):
    """orders of width 63 with codes up to 62: the device's order and probability of every row against the host's (a tie:
    an order as likely as the host's), every order holds the row's slots once."""
    from order_common import Row
    mod, dat = order_cohort
    got = mod.likeliest_orders(dat)
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        for i, r in enumerate(dat):
            want = mod._row_order(dat, i)
            same_or_tie(mod, r, got[i], want, rel=BAR)
            worst = max(worst, abs(got[i][1] - want[1]) / want[1])
            assert set(got[i][0]) == Row(r, mod.n).slots and len(got[i][0]) == len(set(got[i][0])), i
    assert max(max(o, default=0) for o, _ in got) == 62
    print(f"[limits] likeliest_orders at n = 31: {len(dat)} rows, {mod.orders_fallback_rows} recomputed on the host")
    _bar("likeliest_orders at n = 31", probability=worst)


@pytest.mark.gpu
def test_order_posteriors_at_n31(order_cohort):
    mod, dat = order_cohort
    dev, host = mod.order_posteriors(dat), _host_run(mod, "order_posteriors", dat)
    assert mod.posteriors_fallback_rows == 0
    assert dev.pre.shape == (len(dat), 31) and dev.seed_pos.shape == (len(dat), 32)
    seeded = dat[:, -1] != 0
    assert np.all(np.isnan(dev.pre[~seeded])) and np.all(np.isnan(dev.seed_pos[~seeded])) and np.all(np.isfinite(dev.pre[seeded]))
    small = np.arange(len(dat)) < len(dat) - 4           # (the shifted rows: no event below 23)
    # include/metmhn_amd.h, mmhn_order_posteriors: pre is "0 for mutations the row does not carry"
    assert np.all(dev.pre[seeded & small][:, :23] == 0.0)
    _bar("order_posteriors at n = 31", evidence=_rel_evidence(dev, host), pre=_worst_abs(dev.pre, host.pre),
         seed_pos=_worst_abs(dev.seed_pos, host.seed_pos))


@pytest.mark.gpu
def test_order_precedences_at_n31(order_cohort):
    mod, dat = order_cohort
    dev, host = mod.order_precedences(dat), _host_run(mod, "order_precedences", dat)
    assert mod.precedences_fallback_rows == 0
    assert dev.prec.shape == (len(dat), 63, 63)
    carried = _carried(dat, mod.n)
    np.testing.assert_array_equal(~np.isnan(dev.prec), carried[:, :, None] & carried[:, None, :])   # NaN where a code is absent
    _bar("order_precedences at n = 31", evidence=_rel_evidence(dev, host), prec=_worst_abs(dev.prec, host.prec))


@pytest.mark.gpu
def test_order_positions_at_n31(order_cohort):
    from order_common import Row
    mod, dat = order_cohort
    dev, host = mod.order_positions(dat), _host_run(mod, "order_positions", dat)
    assert mod.positions_fallback_rows == 0
    assert dev.pos_pt.shape == dev.pos_mt.shape == (len(dat), 32, 32)
    for i, r in enumerate(dat):
        lin = Row(r, mod.n).lineages
        for name, pos in (("pt", dev.pos_pt[i]), ("mt", dev.pos_mt[i])):
            carried = np.zeros(32, dtype=bool)
            carried[[c // 2 for c in lin.get(name, [])]] = True
            np.testing.assert_array_equal(~np.isnan(pos), np.repeat(carried[:, None], 32, axis=1))
    _bar("order_positions at n = 31", evidence=_rel_evidence(dev, host), pos_pt=_worst_abs(dev.pos_pt, host.pos_pt),
         pos_mt=_worst_abs(dev.pos_mt, host.pos_mt))


@pytest.mark.gpu
def test_order_times_at_n31(order_cohort):
    mod, dat = order_cohort
    dev, host = mod.order_times(dat), _host_run(mod, "order_times", dat)
    assert mod.times_fallback_rows == 0
    assert dev.time.shape == (len(dat), 63) and dev.obs.shape == (len(dat), 2)
    paired = dat[:, -1] == 3
    np.testing.assert_array_equal(~np.isnan(dev.time), _carried(dat, mod.n))
    np.testing.assert_array_equal(~np.isnan(dev.obs), np.stack((np.ones(len(dat), dtype=bool), paired), axis=1))
    np.testing.assert_array_equal(~np.isnan(dev.pt_first), paired)
    d = times_diff(dev, host)
    _bar("order_times at n = 31", evidence=d[0], times=d[1], pt_first=d[2], orderings=max(0.0, times_orderings(dev.time, dev.obs, dat, mod.n)))


@pytest.mark.gpu
def test_order_snapshots_at_n31(order_cohort):
    mod, dat = order_cohort
    dev, host = mod.order_snapshots(dat), _host_run(mod, "order_snapshots", dat)
    assert mod.snapshots_fallback_rows == 0
    assert dev.held.shape == (len(dat), 2, 63) and dev.late.shape == (len(dat), 2, 32) and dev.map_state.shape == (len(dat), 63)
    snapshots_patterns(dev, dat, mod.n)                           # NaN / -1 wherever the row does not carry the code
    d = snapshots_diff(dev, host)                        # (map_state and map_first equal on every row)
    _bar("order_snapshots at n = 31", evidence=d[0], held=d[1], late=d[2], map_prob=d[3])


@pytest.mark.gpu
def test_sample_orders_at_n31(order_cohort):
    """64 samples per row, sample indices across the low counter word, a seed with a high word: every device sample equals
    MetMHN.sample_order's (a sample whose closest draw lies within 1e-9 of a boundary is set aside, as in
    tests/test_order_samples.py), log_prob to 1e-10."""
    from order_common import FIRST, KEY
    mod, dat = order_cohort
    M = 64
    dev = mod.sample_orders(dat, M, key=KEY, first=FIRST)
    assert mod.samples_fallback_rows == 0
    assert dev.orders.shape == (len(dat), M, 63) and dev.orders.dtype == np.int8 and dev.orders.max() == 62
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        host = [mod.sample_order(*mod._row_args(dat, i), n_samples=M, key=KEY, first=FIRST, row=i) for i in range(len(dat))]
    safe = np.array([h.margin for h in host]) >= MARGIN
    same = np.array([(h.orders == dev.orders[i]).all(axis=1) for i, h in enumerate(host)])
    d_lp = np.abs(np.array([h.log_prob for h in host]) - dev.log_prob)
    print(f"[limits] sample_orders at n = 31: {len(dat)} rows x {M} samples, {int((~safe).sum())} set aside, "
          f"{int((~same & safe).sum())} of the others differ")
    assert (~safe).sum() <= max(1, MAX_EXCLUDED * safe.size)
    assert np.all(same[safe])
    for i, r in enumerate(dat):                          # every order holds the row's codes once, padded with -1
        codes = np.flatnonzero(r[:63])
        o = np.sort(dev.orders[i].astype(int), axis=1)
        assert np.all(o[:, 63 - len(codes):] == codes) and np.all(o[:, :63 - len(codes)] == -1), i
    le = np.array([h.log_evidence for h in host])
    print(f"[limits] sample_orders at n = 31: worst |log_prob| difference {d_lp[safe].max():.2e} (bar 1e-10: {d_lp[safe].max() / 1e-10:.3g})")
    assert d_lp[safe].max() <= 1e-10
    _bar("sample_orders at n = 31", evidence=float(np.max(np.abs(np.exp(dev.log_evidence) - np.exp(le)) / np.exp(le))))
