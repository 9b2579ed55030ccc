"""Synthetic parameters and cohorts of BASELINE.md section 3 (seeded NumPy generators)."""
from __future__ import annotations

import numpy as np


def random_params(n: int, seed: int | None = None):
    """log_theta (diag ~ N(0,1), off-diagonals non-zero w.p. 0.5 ~ N(0,1)), log_d_p, log_d_m ~ N(0, 0.25)."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    N = n + 1
    lt = np.diag(rng.normal(size=N))
    mask = rng.random((N, N)) < 0.5
    np.fill_diagonal(mask, False)
    lt = lt + mask * rng.normal(size=(N, N))
    return lt, rng.normal(size=N) * 0.5, rng.normal(size=N) * 0.5


def full_k_cohort(n: int, n_pat: int, k: int | None = None, seed: int | None = None) -> np.ndarray:
    """Every row type 3, seeding = 1, k-1 ones uniformly without replacement over the 2n PT/MT slots,
    order ~ U{0,1,2}; int8 [n_pat, 2n+3]."""
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    k = n if k is None else k
    dat = np.zeros((n_pat, 2 * n + 3), dtype=np.int8)
    for r in range(n_pat):
        dat[r, rng.choice(2 * n, size=k - 1, replace=False)] = 1
    dat[:, 2 * n] = 1
    dat[:, 2 * n + 1] = rng.integers(0, 3, size=n_pat)
    dat[:, 2 * n + 2] = 3
    return dat


def mixed_cohort(n: int, n_pat: int, seed: int = 0, p_event: float = 0.3) -> np.ndarray:
    """Mixed types with the fractions of examples/recall_study.py:120-125
    (11.5 % never-metastasising; of the rest 10.7 % paired, 38.6 % PT-only, remainder MT-only)."""
    rng = np.random.default_rng(seed)
    dat = np.zeros((n_pat, 2 * n + 3), dtype=np.int8)
    for r in range(n_pat):
        bits = (rng.random(2 * n) < p_event).astype(np.int8)
        u = rng.random()
        if u < 0.115:
            bits[1::2] = 0
            dat[r] = np.concatenate((bits, [0, -99, 0]))
        else:
            v = rng.random()
            if v < 0.107:
                dat[r] = np.concatenate((bits, [1, rng.integers(0, 3), 3]))
            elif v < 0.107 + 0.386:
                bits[1::2] = 0
                dat[r] = np.concatenate((bits, [1, -99, 1]))
            else:
                bits[0::2] = 0
                dat[r] = np.concatenate((bits, [1, -99, 2]))
    return dat


def pattern_row(n: int, events: str, order: int) -> np.ndarray:
    """One paired row from a string of events: J = in both tumours, P = PT only, M = MT only, - = in neither.
    The index bits of its joint space follow the string: two per J (PT bit, then MT bit), one per P / M, seeding last."""
    assert len(events) <= n
    r = np.zeros(2 * n + 3, dtype=np.int8)
    for j, ch in enumerate(events):
        r[2 * j] = ch in "JP"
        r[2 * j + 1] = ch in "JM"
    r[2 * n], r[2 * n + 1], r[2 * n + 2] = 1, order, 3
    return r


# joint spaces around the 2^12 tile boundary: a pair on bits 11 / 12 (seeding on 13, k = 14; behind an MT-only event; with
# events above it), the seeding on bit 11 (k = 12), on bit 12 (k = 13) and on bit 13, pairs wholly above the tile
TILE_EDGE_PATTERNS = ("JJJJJPJ", "JJJJJMJ", "JJJJJPJP", "JJJJJPJJ", "JJJJJP", "JJJJJJ", "JJJJJPM", "JJJJJJP", "JJJJJJM",
                      "JJJJJJJ", "JJJJJJJJ")
# window shapes of the fp64 engine (10 .. 12 bits in one class, 4 .. 6 in the other, k = 16 .. 18); the last one has the three
# external bits from which same-shape rows form a chain.  Twelve events each.
WINDOW_PATTERNS = ("JJJPPPPPPPMM", "JJJPPPPPPPPM", "JJJMMMMMMMMP", "JJJJPPPPPPPP", "JJJMMMMMMMPP", "JJJJPPPPPPMM", "JJJJJPPPPPPP")


def tile_edge_cohort(n: int, per_k: int = 8, seed: int = 412) -> np.ndarray:
    """Paired rows whose joint spaces sit on the tile boundary (TILE_EDGE_PATTERNS at orders 0 / 1 / 2 / -99), for n >= 12
    the window shapes as well, between per_k rows each of full_k_cohort(n, k = 13 .. 16); shuffled.  n >= 8."""
    rows = [pattern_row(n, p, o) for p in TILE_EDGE_PATTERNS for o in (0, 1, 2, -99)]
    if n >= 12:
        rows += [pattern_row(n, p, o) for p in WINDOW_PATTERNS for o in (0, 1, 2, -99)]
    dat = np.vstack([np.array(rows, dtype=np.int8)] + [full_k_cohort(n, per_k, k=kk, seed=seed + kk) for kk in (13, 14, 15, 16)])
    np.random.default_rng(seed).shuffle(dat, axis=0)
    return dat
