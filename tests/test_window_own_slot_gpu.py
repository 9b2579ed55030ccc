"""k_wsolve takes the move along external bit 0 from the thread's own window slot and requests only the nX - 1 bits above it
(csrc/wsolve.h: own_take).  The smallest shapes at which that can go wrong, window route against the tile route
(MMHN_WSOLVE=0) and once against the same solves converted to index order (MMHN_WSOLVE=2), buffers NaN-poisoned, at WINDOW_TOL:
  nX = 1   no global read of earlier output left; bit 0 a column bit (nXc = 1) or the lowest external row bit (nXc = 0)
  nX = 2   the first shapes that mix the register term with real requests
  nX = 3   chains of three rows solved by ONE workgroup (MMHN_WSOLVE_WGS=1): lanes of odd lane-level cross a patient boundary
           between an even and an odd pass; (13, 4) has external row bits only
  k = 20   the compile-time instantiation of five external bits, shapes beside the (12, 7) of test_window_rows_gpu.py
  fp32     15 on-chip bits: single rows with nX = 1, chains with nX = 3
A shape is (row-class bits, column-class bits); fp64 keeps 14 bits of a seeded state on the chip, fp32 15."""
import numpy as np
import pytest

from eval_common import shape_rows, window_against

pytestmark = pytest.mark.gpu


def _rows(n, kr, kc, rows_p, count, seed):
    return np.array(shape_rows(n, kr, kc, rows_p, count, seed), dtype=np.int8)


@pytest.mark.parametrize("rows_p", [True, False], ids=["rows_P", "rows_M"])
def test_one_external_column_bit(monkeypatch, rows_p):
    window_against(monkeypatch, 16, _rows(16, 10, 5, rows_p, 1, 11 + rows_p), "0", "f64", f"(10, 5) rows_p={rows_p}")


def test_one_external_row_bit(monkeypatch):
    window_against(monkeypatch, 16, _rows(16, 11, 4, True, 1, 13), "0", "f64", "(11, 4)")


@pytest.mark.parametrize("shape", [(11, 5), (10, 6), (12, 4)], ids=str)
def test_two_external_bits(monkeypatch, shape):
    window_against(monkeypatch, 16, _rows(16, *shape, shape[0] % 2 == 0, 1, 20 + shape[0]), "0", "f64", str(shape))


@pytest.mark.parametrize("shape", [(11, 6), (13, 4), (10, 7)], ids=str)
def test_three_external_bits_chain_in_one_workgroup(monkeypatch, shape):
    monkeypatch.setenv("MMHN_WSOLVE_WGS", "1")
    window_against(monkeypatch, 16, _rows(16, *shape, shape[0] % 2 == 1, 3, 30 + shape[0]), "0", "f64", f"{shape} chain")


def test_chain_against_index_order(monkeypatch):
    monkeypatch.setenv("MMHN_WSOLVE_WGS", "1")
    window_against(monkeypatch, 16, _rows(16, 11, 6, False, 3, 41), "2", "f64", "(11, 6) chain against index order")


@pytest.mark.parametrize("shape", [(15, 4), (10, 9)], ids=str)
def test_k20_chains(monkeypatch, shape):
    monkeypatch.setenv("MMHN_WSOLVE_WGS", "1")
    window_against(monkeypatch, 20, _rows(20, *shape, shape[0] % 2 == 1, 3, 50 + shape[0]), "0", "f64", f"k = 20 {shape} chain")


@pytest.mark.parametrize("shape", [(10, 6), (11, 5)], ids=str)
def test_fp32_one_external_bit(monkeypatch, shape):
    window_against(monkeypatch, 16, _rows(16, *shape, True, 1, 60 + shape[0]), "0", "f32", f"fp32 {shape}")


@pytest.mark.parametrize("shape", [(11, 7), (13, 5)], ids=str)
def test_fp32_chains(monkeypatch, shape):
    monkeypatch.setenv("MMHN_WSOLVE_WGS", "1")
    window_against(monkeypatch, 20, _rows(20, *shape, shape[0] % 2 == 1, 3, 70 + shape[0]), "0", "f32", f"fp32 {shape} chain")
