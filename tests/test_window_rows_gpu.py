"""The window layout's storage-row order (csrc/wlayout.h: wrho) is private to the window route: every producer and consumer
of a seeded half goes through wrho / wrho_inv / wpos*, the tile route (MMHN_WSOLVE=0) never sees it.  Per-patient gradients
of the window route are compared with the tile route's on the window shapes of synthetic.WINDOW_PATTERNS (k = 16 - 18,
either class as rows, one to three external bits, orders 0 / 1 / 2) and on chains of three k = 20 rows per class
orientation, in fp64 and fp32, buffers NaN-poisoned.  The marginal problems of these rows read the solution through both
branches of wpos_marg (free class = rows / columns), the eq-block flows through wpos_nat."""
import numpy as np
import pytest

from eval_common import NAMES, shape_rows, window_against

pytestmark = pytest.mark.gpu


def _cohorts():
    from metmhn_amd import synthetic
    pat = np.array([synthetic.pattern_row(12, p, o) for p in synthetic.WINDOW_PATTERNS for o in (0, 1, 2)], dtype=np.int8)
    k20 = np.array(shape_rows(20, 12, 7, True, 3, 71) + shape_rows(20, 12, 7, False, 3, 72), dtype=np.int8)
    return {"patterns": (12, pat), "k20_chains": (20, k20)}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", ["patterns", "k20_chains"])
def test_window_route_against_tile_route(monkeypatch, name, dtype):
    n, dat = _cohorts()[name]
    win, tile = window_against(monkeypatch, n, dat, "0", dtype, f"{name} {dtype} window against tile")
    for x, y, nm in zip(win, tile, NAMES):
        print(f"{name} {dtype} {nm}: max |window - tile| / max |tile| = {np.abs(x - y).max() / np.abs(y).max():.3e}")
