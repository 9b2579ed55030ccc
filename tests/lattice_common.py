"""What the tests of the sweeps over all 2^n genotypes share (test_seeding_landscape.py, test_genotype_distribution.py,
test_metastasis_distribution.py): the tile size read from the header, the error measures, the device's reduction and
the brute-force summary it is held against, the models with a dead mutation, the cohort of the fit tests and the body
of the three test_same_bytes_whatever_the_queries.  Imported by name (`from lattice_common import ...`); tests/ is on
sys.path.  The bars are derived in the three files' docstrings: each keeps its own eps_of, bound and summary_bound."""
import os
import re

import numpy as np
import pytest

from metmhn_amd.model import GenotypeSummary, MetMHN
from order_common import mixed_cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
C = int(re.search(r"constexpr int LS_TILE_BITS = (\d+);",
                  open(os.path.join(ROOT, "metmhn_amd", "csrc", "lattice.h")).read()).group(1))
WORST = {}                         # test -> worst error / bound seen (printed)


def bits(n, codes):
    """[R, n] int8 genotypes of the codes."""
    return (np.asarray(codes, dtype=np.int64)[:, None] >> np.arange(n) & 1).astype(np.int8)


def rel(got, ref, nan=False):
    """Worst |got - ref| / |ref| over the entries; an exact 0 must be met exactly; nothing may be NaN or infinite - with
    `nan`, NaN must sit where NaN sits instead."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if nan:
        assert (np.isnan(got) == np.isnan(ref)).all(), "NaN pattern"
    else:
        assert np.isfinite(got).all() and np.isfinite(ref).all(), "not finite"
    ok = ~np.isnan(ref)
    zero = ok & (ref == 0)
    assert (got[zero] == 0).all(), "an exact zero of the reference is not met"
    live = ok & ~zero
    return float(np.max(np.abs(got[live] - ref[live]) / np.abs(ref[live]), initial=0.0))


def ld_rel(got, ref):
    """Worst relative difference of fp64 `got` against long double `ref`; exact zeros exact."""
    got, ref = np.asarray(got), np.asarray(ref)
    zero = ref == 0
    assert (got[zero] == 0).all()
    return float(np.max(np.abs(got[~zero].astype(np.longdouble) - ref[~zero]) / ref[~zero], initial=0.0))


def note(tag, worst):
    WORST[tag] = max(WORST.get(tag, 0.0), worst)
    print(f"{tag}: worst error / bound {worst:.3e}")
    assert worst <= 1.0, (tag, worst)


def red(n):
    """Longest chain of additions of the device's reduction."""
    return 52 + -(-(1 << max(n - C, 0)) // 256)


def summary_rel(got, ref):
    """Worst relative difference of the three arrays of two summaries (mass, pairs, burden as tuples or GenotypeSummary)."""
    a = (got.mass, got.pairs, got.burden) if isinstance(got, GenotypeSummary) else got
    b = (ref.mass, ref.pairs, ref.burden) if isinstance(ref, GenotypeSummary) else ref
    return max(rel(x, y) for x, y in zip(a, b))


def brute_summary(P):
    """(mass, pairs, burden) of the planes P [2, 2^n] in long double, over the bits of every code."""
    ld = np.longdouble
    n = P.shape[1].bit_length() - 1
    g = bits(n, np.arange(1 << n)).astype(ld)
    level = g.sum(axis=1).astype(np.int64)
    mass, pairs, burden = np.zeros(2, dtype=ld), np.zeros((2, n, n), dtype=ld), np.zeros((2, n + 1), dtype=ld)
    for s in range(2):
        p = P[s].astype(ld)
        mass[s] = p.sum()
        for i in range(n):
            for j in range(n):
                pairs[s, i, j] = (p * g[:, i] * g[:, j]).sum()
        for m in range(n + 1):
            burden[s, m] = p[level == m].sum()
    return mass, pairs, burden


def without(mod, j):
    """(the model with theta_jj = -1e10, the model without mutation j, the codes without bit j, the same codes in the smaller
    model)."""
    n = mod.n
    th = mod.log_theta.copy()
    th[j, j] = -1e10
    keep = [i for i in range(n + 1) if i != j]
    codes = np.array([x for x in range(1 << n) if not x >> j & 1])
    small = (codes & ((1 << j) - 1)) | (codes >> (j + 1) << j)
    return MetMHN(th, mod.obs1, mod.obs2), MetMHN(th[np.ix_(keep, keep)], mod.obs1[keep], mod.obs2[keep]), codes, small


def fit_cohort(n=5):
    """The cohort of test_genotype_distribution.py's fit tests: the mixed cohort, repeats and rows of unknown status."""
    import unknown_common as UC
    extra = [UC.unknown_row(n, e) for e in ([0, 3], [], [1, 2, 4], [0, 3])]
    return np.vstack((mixed_cohort(n), mixed_cohort(n)[:3], extra)).astype(np.int8)


def check_same_bytes(call, planes, n, at=None):
    """The body of the three test_same_bytes_whatever_the_queries.  call(G, **kw) -> values, status, sums, whole of a sweep
    of `planes` values over n = c + 1 mutations, sums None throughout for the sweep without a summary; at: the model's _at
    method of a sweep with one."""
    G = bits(n, np.arange(1 << n))
    same = lambda a, b: (a is None and b is None) or all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    values, status, sums, whole = call(G, full=True)
    assert (sums is None) == (at is None)
    assert (status == 0).all() and values.tobytes() == np.ascontiguousarray(whole.T).tobytes()
    again = call(G, full=True)
    assert again[0].tobytes() == values.tobytes() and again[3].tobytes() == whole.tobytes() and same(again[2], sums)
    perm = np.random.default_rng(7).permutation(len(G))[:300]
    mixed, st, s2, none = call(G[perm])
    assert none is None and (st == 0).all() and mixed.tobytes() == values[perm].tobytes() and same(s2, sums)
    for x in (0, 1, (1 << C) - 1, 1 << C, (1 << n) - 1):
        one, st, s2, _ = call(G[x:x + 1])
        assert st.tolist() == [0] and one[0].tobytes() == values[x].tobytes() and same(s2, sums)
    bad = np.vstack((G[5], G[6], G[(1 << n) - 7]))
    bad[1, 2] = 3
    out, st, s2, _ = call(bad)
    assert st.tolist() == [0, 2 | 8 << 16, 0] and np.isnan(out[1]).all() and same(s2, sums)
    assert out[[0, 2]].tobytes() == values[[5, (1 << n) - 7]].tobytes()
    v0, s0, s2, only = call(np.zeros((0, n), dtype=np.int8), full=True)
    assert v0.shape == (0, planes) and s0.shape == (0,) and only.tobytes() == whole.tobytes() and same(s2, sums)
    if at is not None:
        v1, _, s3, o3 = call(G[:9], summary=False, full=True)
        assert s3 is None and o3.tobytes() == whole.tobytes() and v1.tobytes() == values[:9].tobytes()
        with pytest.raises(ValueError, match=r"^row 1: "):
            at(bad)
