"""k_wclass sums the neighbours along the external row bits in phase C (csrc/wclass.h): a chunk holds every setting of
the lowest m external row bits, the row sums are reduced over the threads that share a row (DPP segment sums, across
waves through LDS) and written once.  Single-shape cohorts of every window shape class are checked against the
index-order class marginals (MMHN_WSOLVE=2: the same solves, converted to index order, k_pclass), with the class-table
range that no memset clears NaN-poisoned (MMHN_POISON=1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _row(n, pt, mt, order):
    r = np.zeros(2 * n + 3, dtype=np.int8)
    for j in pt:
        r[2 * j] = 1
    for j in mt:
        r[2 * j + 1] = 1
    r[2 * n], r[2 * n + 1], r[2 * n + 2] = 1, order, 3
    return r


def _shape_rows(n, kr, kc, rows_p, count, seed):
    """`count` patients whose joint space has kr row-class and kc column-class bits (rows_p: the PT class is the rows)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        a = rng.choice(n, size=kr, replace=False)
        b = rng.choice(n, size=kc, replace=False)
        pt, mt = (a, b) if rows_p else (b, a)
        out.append(_row(n, pt, mt, i % 3))
    return out


def _grads(monkeypatch, n, dat, mode, dtype):
    from metmhn_amd import Engine, synthetic
    lt, dp, dm = synthetic.random_params(n)
    monkeypatch.setenv("MMHN_WSOLVE", mode)
    with Engine(n, dtype=dtype) as e:
        e.set_cohort(dat)
        return e.patient_grads(lt, dp, dm)


def _check(monkeypatch, n, cohort, dtype="f64", rtol=1e-12):
    monkeypatch.setenv("MMHN_PSOLVE_MIN", "1")          # (also the window route's minimum: a few patients take it)
    monkeypatch.setenv("MMHN_POISON", "1")
    dat = np.array(cohort, dtype=np.int8)
    win = _grads(monkeypatch, n, dat, "1", dtype)
    idx = _grads(monkeypatch, n, dat, "2", dtype)
    for x, y, nm in zip(win, idx, ("lp", "d_theta", "d_dp", "d_dm")):
        assert np.isfinite(x).all(), nm
        np.testing.assert_allclose(x, y, rtol=rtol, atol=rtol * np.abs(y).max(), err_msg=nm)


# fp64, k = 20: kR + kC = 19, every external row bit in phase C; chains of three patients, either class as rows
@pytest.mark.parametrize("kr", [10, 11, 12, 13, 14, 15])
def test_wclass_fp64_k20_shapes(monkeypatch, kr):
    n = 20
    cohort = _shape_rows(n, kr, 19 - kr, kr % 2 == 0, 3, 100 + kr) + _shape_rows(n, kr, 19 - kr, kr % 2 == 1, 2, 200 + kr)
    _check(monkeypatch, n, cohort)


def test_wclass_fp64_k20_mixed_with_index_order_problems(monkeypatch):
    """every k = 20 shape in one batch next to a problem the window route leaves to the index-order kernels: the
    cleared class-table range and the uncleared one side by side"""
    n = 20
    cohort = []
    for kr in range(10, 16):
        cohort += _shape_rows(n, kr, 19 - kr, kr % 2 == 0, 2, 300 + kr)
    cohort.append(_row(n, range(16), [16, 17, 18], 1))   # 16 row bits: beyond the window path
    _check(monkeypatch, n, cohort)


def test_wclass_fp64_partial_external_bits(monkeypatch):
    """k > 20: only the lowest m external row bits fit a chunk (kC + nXr > 10), phase R reads q again for the rest"""
    n = 25
    cohort = []
    for i, (kr, kc) in enumerate(((12, 9), (13, 8), (15, 6), (14, 9))):
        cohort += _shape_rows(n, kr, kc, i % 2 == 0, 2, 400 + i)
    _check(monkeypatch, n, cohort)


def test_wclass_fp32_extremes(monkeypatch):
    """fp32, k = 25 (kC + nXr = 14): five of eight external bits in phase C (18, 6), four of seven (17, 7), two with a
    row over two waves (15, 9), one with a row over four waves (14, 10), none (12, 12); fp32 summation-order bar"""
    n = 25
    cohort = []
    for i, (kr, kc) in enumerate(((18, 6), (17, 7), (15, 9), (14, 10), (12, 12))):
        cohort += _shape_rows(n, kr, kc, i % 2 == 0, 2, 500 + i)
    _check(monkeypatch, n, cohort, dtype="f32", rtol=2e-4)
