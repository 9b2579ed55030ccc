"""What the tests of the seeding forecasts and of the sweeps over all 2^n genotypes share (test_seeding_forecasts.py,
test_seeding_landscape.py, test_genotype_distribution.py, test_metastasis_distribution.py, test_partner_distribution.py,
test_cross_table.py): the tile size read from the header, the error measures, the bars of the device against the host,
the device's reduction and the brute-force summary it is held against, the models with a dead mutation, the cohort of the
fit tests, the host results computed once, the library kept out of reach and the body of the three
test_same_bytes_whatever_the_queries.  Imported by name (`from lattice_common import ...`); tests/ is on sys.path.

The bars of the device against the host definition, derived once.  Both sides are fp64 evaluations of non-negative
sum-products, so relative errors add along a path and a sum takes the worst of its terms plus its additions; u = 2^-53.
  The rates.  The primary tumour's (pt_eps): A = max_j (|theta_jj| + sum_i |theta_ji|) (the seeding included), B = sum
|obs1_i| - with the entry n where the clock exp(obs1_n) is a factor of a value (the distributions), without it where it is
not (the forecasts and the landscape) -: an exponential of a sum of at most n + 2 terms, and the device's product of three
of them, is within eps = 2 (n + 2) u max(A, B) + 4 u of the exact rate.  The pair's (pair_eps): A = max_j (|theta_jj| +
|theta_jn| + sum_i |theta_ji|), B = max(sum |obs1_i|, sum |obs2_i|) (the n-th entries included): a rate or a clock is an
exponential of a sum of at most n + 3 terms and on the device a product of FOUR exponentials (the tile's factor, the two
tables, exp(theta_jn) or exp(obs_n)), within eps = 2 (n + 3) u max(A, B) + 5 u.
  The chain (chain_bound).  One step of a chain takes its rates from both sides, once in the numerator and once in den
(4 eps), and `per_step` roundings: the products, the additions of the numerator and of den and the division, on both
sides.  A value sits behind at most `steps` steps: steps (4 eps + per_step u).  Where a value leaves as a clock or a rate
times G (`out`): 2 eps + 8 u for both sides.  Where it is summed over the genotypes (`summed`): RED(n) = 52 +
ceil(2^(n - c) / 256) additions on the device (genodist.h: 8 + 4 + 32 in the fold of a tile, ceil(tiles / 256) + 8 across the
tiles), at most n + 19 for NumPy's pairwise sum of 2^n contiguous entries on the host (blocks of 128 on 8 accumulators,
16 + 3 additions, and a tree above them): (RED(n) + n + 19) u.  Each file states its own `steps` and `per_step` and what it
measured; the counts that more than one file needs stand here once (forecast_bound, landscape_bound, genodist_bound,
genodist_summary_bound); every bar is asserted to stay below 1e-9.
  Two host evaluations of one quantity (identity_bar, the CPU identities of the partner distribution and the cross table)
share their fp64 rates: a step costs a product, at most n + 1 additions of the numerator, n + 2 of den and the division,
2 n + 5 u; a path has at most 2 n + 4 steps and 3 u on the way out; two paths and the additions of the sums."""
import functools
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
S_FORECAST = 655                   # forecast.h: the longest chain of additions behind an output of the forward kernel
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


def rel_nan(got, ref):
    """rel where NaN must sit where NaN sits."""
    return rel(got, ref, nan=True)


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


def pt_eps(mod, clock=True):
    """The rate error of the primary tumour's chain (module docstring); clock: obs1 with its entry n."""
    th, n = mod._pt_log_theta, mod.n
    A = max(abs(th[j, j]) + np.abs(np.delete(th[j, :n], j) if j < n else th[j, :n]).sum() for j in range(n + 1))
    B = np.abs(mod.obs1 if clock else mod.obs1[:n]).sum()
    return 2 * (n + 2) * U * max(A, B) + 4 * U


def pair_eps(mod):
    """The rate error of the pair's chains (module docstring)."""
    th, n = mod.log_theta, mod.n
    A = max(np.abs(th[j, :n]).sum() + (abs(th[j, n]) if j < n else abs(th[n, n])) for j in range(n + 1))
    B = max(np.abs(mod.obs1).sum(), np.abs(mod.obs2).sum())
    return 2 * (n + 3) * U * max(A, B) + 5 * U


def chain_bound(eps, steps, per_step, out=False, summed=None):
    """steps (4 eps + per_step u) [+ 2 eps + 8 u with `out`] [+ (RED(n) + n + 19) u with summed = n] (module docstring)."""
    b = steps * (4 * eps + per_step * U)
    if out:
        b = b + 2 * eps + 8 * U
    if summed is not None:
        b = b + (red(summed) + summed + 19) * U
    assert b < 1e-9, (steps, per_step, summed, b)
    return b


def forecast_bound(mod, f):
    """A row of f free mutations of the forward kernel against its host definition (tests/test_seeding_forecasts.py): f + 1
    levels of 2 f + 6 roundings and the final sums."""
    b = chain_bound(pt_eps(mod, clock=False), f + 1, 2 * f + 6) + S_FORECAST * U
    assert b < 1e-9, (f, b)
    return b


def landscape_bound(mod, clock=False):
    """The device landscape against its host definition (tests/test_seeding_landscape.py): n + 1 states of 2 n + 8 roundings;
    clock: with the eps of the distributions that are held against it."""
    return chain_bound(pt_eps(mod, clock), mod.n + 1, 2 * mod.n + 8)


def genodist_bound(mod):
    """Either plane of the primary tumour's distribution on the device against its host definition
    (tests/test_genotype_distribution.py): n + 2 steps of 4 n + 14 roundings and the way out."""
    return chain_bound(pt_eps(mod), mod.n + 2, 4 * mod.n + 14, out=True)


def genodist_summary_bound(mod):
    """genodist_bound with the reductions of a summary entry."""
    return chain_bound(pt_eps(mod), mod.n + 2, 4 * mod.n + 14, out=True, summed=mod.n)


def identity_bar(n, additions):
    """Two host evaluations of one quantity, in u (module docstring): two paths and the additions of the sum."""
    return 2 * ((2 * n + 4) * (2 * n + 5) + 3) + additions


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


def genotype(n, held):
    """The int8 genotype [n] that holds the mutations `held`."""
    g = np.zeros(n, dtype=np.int8)
    g[list(held)] = 1
    return g


def frozen(got):
    """`got` - an array, or a tuple or an object of arrays - with every array read-only: what a cached host(...) returns."""
    parts = got if isinstance(got, tuple) else (got,) if isinstance(got, np.ndarray) else vars(got).values()
    for a in parts:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return got


def host_once(compute):
    """Decorator of a host(*key) that returns the host definition's result: computed once per key, never written to."""
    @functools.lru_cache(maxsize=None)
    @functools.wraps(compute)
    def cached(*key):
        return frozen(compute(*key))
    return cached


def no_library(monkeypatch):
    """From here on the test fails if it reaches the library."""
    import metmhn_amd.jx as jx

    def no_engine(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(jx, "engine", no_engine)


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
