"""k_wclass sums the neighbours along the external row bits in phase C (csrc/wclass.h): a chunk holds every setting of
the lowest m external row bits, the row sums are reduced over the threads that share a row (DPP segment sums, across
waves through LDS) and written once.  Single-shape cohorts of every window shape class are checked against the
index-order class marginals (MMHN_WSOLVE=2: the same solves, converted to index order, k_pclass), with the class-table
range that no memset clears NaN-poisoned (MMHN_POISON=1)."""
import numpy as np
import pytest

from eval_common import paired, shape_rows, window_against

pytestmark = pytest.mark.gpu


def _check(monkeypatch, n, cohort, dtype="f64"):
    window_against(monkeypatch, n, np.array(cohort, dtype=np.int8), "2", dtype, f"{dtype} window against index order")


# fp64, k = 20: kR + kC = 19, every external row bit in phase C; chains of three patients, either class as rows
@pytest.mark.parametrize("kr", [10, 11, 12, 13, 14, 15])
def test_wclass_fp64_k20_shapes(monkeypatch, kr):
    n = 20
    cohort = shape_rows(n, kr, 19 - kr, kr % 2 == 0, 3, 100 + kr) + shape_rows(n, kr, 19 - kr, kr % 2 == 1, 2, 200 + kr)
    _check(monkeypatch, n, cohort)


def test_wclass_fp64_k20_mixed_with_index_order_problems(monkeypatch):
    """every k = 20 shape in one batch next to a problem the window route leaves to the index-order kernels: the
    cleared class-table range and the uncleared one side by side"""
    n = 20
    cohort = []
    for kr in range(10, 16):
        cohort += shape_rows(n, kr, 19 - kr, kr % 2 == 0, 2, 300 + kr)
    cohort.append(paired(n, range(16), [16, 17, 18], 1))   # 16 row bits: beyond the window path
    _check(monkeypatch, n, cohort)


def test_wclass_fp64_partial_external_bits(monkeypatch):
    """k > 20: only the lowest m external row bits fit a chunk (kC + nXr > 10), phase R reads q again for the rest"""
    n = 25
    cohort = []
    for i, (kr, kc) in enumerate(((12, 9), (13, 8), (15, 6), (14, 9))):
        cohort += shape_rows(n, kr, kc, i % 2 == 0, 2, 400 + i)
    _check(monkeypatch, n, cohort)


def test_wclass_fp32_extremes(monkeypatch):
    """fp32, k = 25 (kC + nXr = 14): five of eight external bits in phase C (18, 6), four of seven (17, 7), two with a
    row over two waves (15, 9), one with a row over four waves (14, 10), none (12, 12); fp32 summation-order bar"""
    n = 25
    cohort = []
    for i, (kr, kc) in enumerate(((18, 6), (17, 7), (15, 9), (14, 10), (12, 12))):
        cohort += shape_rows(n, kr, kc, i % 2 == 0, 2, 500 + i)
    _check(monkeypatch, n, cohort, dtype="f32")
