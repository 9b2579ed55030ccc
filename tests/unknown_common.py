"""Helpers of tests/test_unknown_status.py: cohort rows of type 4 (primary tumour sequenced, metastatic status unknown), their
NumPy reference and the bars.

Reference of a type-4 row with PT genotype x: oracle.metmhn_oracle.patient_lp / patient_grad on the row relabelled as type 0
(lp0) and as type 1 with seeding = 1 (lp1), combined here:
    lp = logaddexp(lp0, lp1),  r1 = exp(lp1 - lp) = P(seeded | x),  grad = (1 - r1) grad0 + r1 grad1,  d_dm = 0.
Bars: the per-patient bars of tests/test_gpu_parity.py and tests/test_parity_fp32.py (fp64: lp rtol 1e-9 atol 1e-12, gradients
rtol 1e-8 atol 1e-10; fp32: lp rtol 1e-4, gradients 2e-3 |ref| + 2e-5).  For p_seeded, r1 = 1 / (1 + exp(lp0 - lp1)) has |dr1 / d(lp0 - lp1)| = r1 (1 - r1) <= 1 / 4,
so with each of lp0, lp1 inside the lp bar: |dr1| <= 0.25 (rtol (|lp0| + |lp1|) + 2 atol)."""
import functools

import numpy as np

TB = 12                                                       # tile bits (csrc/common.h)
N_SHAPES = 13                                                 # n of the shape rows: |x| reaches TB
SHAPE_SIZES = (0, 1, 5, 6, 8, 9, TB - 1, TB)                  # the larger part, |x| + 1, sits at and just past 6, 9, TB

LP_BAR = {"f64": (1e-9, 1e-12), "f32": (1e-4, 0.0)}
GRAD_BAR = {"f64": (1e-8, 1e-10), "f32": (2e-3, 2e-5)}


def params(n):
    from metmhn_amd import synthetic
    return synthetic.random_params(n)


def unknown_row(n, events):
    """Type-4 row with the PT events `events`; order column -99 (ignored)."""
    r = np.zeros(2 * n + 3, dtype=np.int8)
    r[[2 * j for j in events]] = 1
    r[-2], r[-1] = -99, 4
    return r


def relabel(row, typ):
    """The PT genotype of `row` as a row of type 0 (seeding 0) or type 1 (seeding 1) or type 4 (seeding 0)."""
    r = np.array(row, dtype=np.int8, copy=True)
    n = (r.shape[0] - 3) // 2
    r[1:2 * n:2] = 0
    r[-3], r[-2], r[-1] = (1 if typ == 1 else 0), -99, typ
    return r


def shape_rows(n=N_SHAPES, sizes=SHAPE_SIZES, seed=4):
    rng = np.random.default_rng(seed)
    return np.array([unknown_row(n, rng.choice(n, size=k, replace=False)) for k in sizes], dtype=np.int8)


def combine(lp0, lp1, rows0=None, rows1=None):
    """(lp, r1[, rows]) of the mixture from the two statuses' log-probabilities (and per-patient rows [.., st])."""
    lp0, lp1 = np.asarray(lp0, dtype=np.float64), np.asarray(lp1, dtype=np.float64)
    lp = np.logaddexp(lp0, lp1)
    r1 = np.exp(lp1 - lp)
    if rows0 is None:
        return lp, r1
    r1c = r1.reshape(r1.shape + (1,) * (np.ndim(rows0) - np.ndim(r1)))
    return lp, r1, (1.0 - r1c) * rows0 + r1c * rows1


def mixture_lp(lt, dp, dm, row):
    """(lp, r1, lp0, lp1) of one type-4 row through the oracle."""
    from oracle import metmhn_oracle as O
    lp0 = float(O.patient_lp(lt, dp, dm, relabel(row, 0))[0])
    lp1 = float(O.patient_lp(lt, dp, dm, relabel(row, 1))[0])
    lp, r1 = combine(lp0, lp1)
    return float(lp), float(r1), lp0, lp1


def mixture(lt, dp, dm, row):
    """dict(lp, r1, lp0, lp1, g [N, N], a [N], b [N]) of one type-4 row through the oracle."""
    from oracle import metmhn_oracle as O
    lp0, g0, a0, b0, _ = O.patient_grad(lt, dp, dm, relabel(row, 0))
    lp1, g1, a1, b1, _ = O.patient_grad(lt, dp, dm, relabel(row, 1))
    lp, r1 = combine(float(lp0), float(lp1))
    f = lambda x0, x1: (1.0 - r1) * np.asarray(x0, dtype=np.float64) + r1 * np.asarray(x1, dtype=np.float64)
    return dict(lp=float(lp), r1=float(r1), lp0=float(lp0), lp1=float(lp1), g=f(g0, g1), a=f(a0, a1), b=f(b0, b1))


def reference(lt, dp, dm, rows):
    """The oracle's mixture of every row: dict of arrays lp, r1, lp0, lp1 [P], g [P, N, N], a, b [P, N]."""
    out = [mixture(lt, dp, dm, r) for r in rows]
    return {k: np.array([o[k] for o in out]) for k in out[0]}


@functools.lru_cache(maxsize=None)
def shape_reference():
    """(lt, dp, dm, rows, reference) of the shape rows: computed once, shared by the tests, never written to."""
    lt, dp, dm = params(N_SHAPES)
    rows = shape_rows()
    ref = reference(lt, dp, dm, rows)
    for v in (lt, dp, dm, rows, *ref.values()):
        v.setflags(write=False)
    return lt, dp, dm, rows, ref


def ratio(got, ref, rtol, atol, what):
    """Worst |got - ref| / (rtol |ref| + atol), printed; NaN or inf never passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, expected {ref.shape}"
    assert np.isfinite(got).all(), f"{what}: not finite"
    bar = rtol * np.abs(ref) + atol
    err = np.abs(got - ref)
    exact = bar == 0
    assert (err[exact] == 0).all(), f"{what}: differs where the bar is 0"
    worst = float((err[~exact] / bar[~exact]).max()) if (~exact).any() else 0.0
    print(f"{what}: worst error / bar {worst:.3e} (max abs error {err.max() if err.size else 0.0:.3e})")
    return worst


def p_bar(ref_lp0, ref_lp1, dtype):
    rtol, atol = LP_BAR[dtype]
    return 0.25 * (rtol * (np.abs(ref_lp0) + np.abs(ref_lp1)) + 2 * atol)


def check_rows(got, ps, ref, dtype, tag):
    """patient_grads output `got` = (lp, g, a, b) and p_seeded `ps` of type-4 rows against `ref` (reference()'s dict)."""
    lp, g, a, b = got
    worst = [ratio(lp, ref["lp"], *LP_BAR[dtype], f"{tag} lp"),
             ratio(g, ref["g"], *GRAD_BAR[dtype], f"{tag} d_theta"),
             ratio(a, ref["a"], *GRAD_BAR[dtype], f"{tag} d_dp")]
    assert not np.asarray(b).any(), f"{tag}: a type-4 row has a d_dm entry"
    bar = p_bar(ref["lp0"], ref["lp1"], dtype)
    err = np.abs(np.asarray(ps) - ref["r1"])
    assert np.isfinite(ps).all(), f"{tag} p_seeded: not finite"
    worst.append(float((err / bar).max()))
    print(f"{tag} p_seeded: worst error / bar {worst[-1]:.3e} (max abs error {err.max():.3e})")
    assert max(worst) <= 1.0, f"{tag}: worst error / bar {max(worst):.3e}"
    return max(worst)


def objective(rows, dat, perc_met):
    """(score, d_theta, d_dp, d_dm) by the definition: rows [P, st] = [lp, G, d_dp, d_dm] per patient, the counts from `dat`.
    n_em = sum of the seeding column, n_nm = n_pat - n_em - n_unknown (the type-0 rows of a cohort whose rows of types 1 - 3 all
    carry the seeding), w from those two, type-4 rows weight 1; also (w, n_full)."""
    import math
    dat = np.asarray(dat)
    N = (dat.shape[1] - 3) // 2 + 1
    typ = dat[:, -1]
    n_em, n_unknown = float(dat[:, -3].sum()), float((typ == 4).sum())
    n_nm = float(dat.shape[0]) - n_em - n_unknown
    w = perc_met * n_nm / ((1 - perc_met) * n_em) if n_em * n_nm != 0 else 1.0
    n_full = w * n_em + n_nm + n_unknown
    col = lambda sel: np.array([math.fsum(c) for c in rows[sel].T])
    tot = (w * col((typ != 0) & (typ != 4)) + col(typ == 0) + col(typ == 4)) / n_full
    return tot[0], tot[1:1 + N * N].reshape(N, N), tot[1 + N * N:1 + N * N + N], tot[1 + N * N + N:], (w, n_full)
