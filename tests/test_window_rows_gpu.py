"""The window layout's storage-row order (csrc/wlayout.h: wrho) is private to the window route: every producer and consumer
of a seeded half goes through wrho / wrho_inv / wpos*, the tile route (MMHN_WSOLVE=0) never sees it.  Per-patient gradients
of the window route are compared with the tile route's on the window shapes of synthetic.WINDOW_PATTERNS (k = 16 - 18,
either class as rows, one to three external bits, orders 0 / 1 / 2) and on chains of three k = 20 rows per class
orientation, in fp64 and fp32, buffers NaN-poisoned.  The marginal problems of these rows read the solution through both
branches of wpos_marg (free class = rows / columns), the eq-block flows through wpos_nat."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-12, "f32": 2e-4}        # (tests/test_wclass_external_rows.py)


def _k20_chain(n, kr, kc, rows_p, seed):
    """three rows of one shape (kr row-class bits, kc column-class bits; rows_p: the PT class is the rows), orders 0 / 1 / 2"""
    rng = np.random.default_rng(seed)
    out = []
    for order in range(3):
        a, b = rng.choice(n, size=kr, replace=False), rng.choice(n, size=kc, replace=False)
        pt, mt = (a, b) if rows_p else (b, a)
        r = np.zeros(2 * n + 3, dtype=np.int8)
        r[2 * pt] = 1
        r[2 * mt + 1] = 1
        r[2 * n], r[2 * n + 1], r[2 * n + 2] = 1, order, 3
        out.append(r)
    return out


def _cohorts():
    from metmhn_amd import synthetic
    pat = np.array([synthetic.pattern_row(12, p, o) for p in synthetic.WINDOW_PATTERNS for o in (0, 1, 2)], dtype=np.int8)
    k20 = np.array(_k20_chain(20, 12, 7, True, 71) + _k20_chain(20, 12, 7, False, 72), dtype=np.int8)
    return {"patterns": (12, pat), "k20_chains": (20, k20)}


def _grads(monkeypatch, n, dat, mode, dtype):
    from metmhn_amd import Engine, synthetic
    lt, dp, dm = synthetic.random_params(n)
    monkeypatch.setenv("MMHN_WSOLVE", mode)
    with Engine(n, dtype=dtype) as e:
        e.set_cohort(dat)
        return e.patient_grads(lt, dp, dm)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["patterns", "k20_chains"])
def test_window_route_against_tile_route(monkeypatch, name, dtype):
    n, dat = _cohorts()[name]
    monkeypatch.setenv("MMHN_PSOLVE_MIN", "1")          # (also the window route's minimum: a few patients take it)
    monkeypatch.setenv("MMHN_POISON", "1")
    win = _grads(monkeypatch, n, dat, "1", dtype)
    tile = _grads(monkeypatch, n, dat, "0", dtype)
    rtol = TOL[dtype]
    for x, y, nm in zip(win, tile, ("lp", "d_theta", "d_dp", "d_dm")):
        assert np.isfinite(x).all(), nm
        err = np.abs(x - y).max() / np.abs(y).max()
        print(f"{name} {dtype} {nm}: max |window - tile| / max |tile| = {err:.3e}")
        np.testing.assert_allclose(x, y, rtol=rtol, atol=rtol * np.abs(y).max(), err_msg=nm)
