#!/usr/bin/env python3
"""Row weights on the 28-event LUAD cohort (tests/golden/luad28.npz; perc_met and lambda of the LUAD fixtures): one JSON line,
every time the best of 3.
  * ms per score_and_grad_reg evaluation at the published parameters: the 4 852 rows as they are and as their distinct rows
    with the counts as weights (Utilityfunctions.collapse_rows); the same for the cohort bootstrapped x20 (97 040 rows drawn
    with replacement, seed 20) - the registry-scale cohort of VERDICT.md;
  * seconds for Utilityfunctions.bootstrap_fits with 20 replicates (key 0, started at the published parameters, SciPy's
    L-BFGS-B at the reference's default ftol 1e-4);
  * the largest relative difference between the collapsed and the plain objective and gradient (gradient: largest absolute
    difference over the largest absolute entry).
    python scripts/luad28_weighted.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metmhn_amd.regularized_optimization as ro
from metmhn_amd import Utilityfunctions as UF

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
pm, lam = float(g["perc_met"]), float(g["lam"])
pub = np.concatenate((g["fit_theta"].flatten(), g["fit_dp"], g["fit_dm"]))
REPS = {4852: 50, 97040: 10}


def eval_ms(dat, weights, reps):
    """Best of 3 of the mean time of `reps` evaluations, in ms; the last value and gradient."""
    for _ in range(3):
        out = ro.score_and_grad_reg(pub, dat, pm, ro.symmetric_penal, lam, weights=weights)
    best = np.inf
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            out = ro.score_and_grad_reg(pub, dat, pm, ro.symmetric_penal, lam, weights=weights)
        best = min(best, (time.perf_counter() - t0) / reps * 1e3)
    return best, out


def pair(dat):
    rows, counts, _ = UF.collapse_rows(dat)
    reps = REPS[dat.shape[0]]
    t0 = time.perf_counter()
    ms_plain, (v0, g0) = eval_ms(dat, None, reps)
    ms_coll, (v1, g1) = eval_ms(rows, counts, reps)
    res = {"rows": int(dat.shape[0]), "distinct_rows": int(rows.shape[0]), "ms_plain": round(ms_plain, 3), "ms_collapsed": round(ms_coll, 3),
           "rel_diff_objective": float(abs(v1 - v0) / abs(v0)), "rel_diff_gradient": float(np.abs(g1 - g0).max() / np.abs(g0).max()),
           "seconds_total": round(time.perf_counter() - t0, 1)}
    ro.invalidate()
    return res


dat = np.ascontiguousarray(g["dat"])
big = np.ascontiguousarray(dat[np.random.default_rng(20).integers(0, dat.shape[0], size=20 * dat.shape[0])])
out = {"luad28": pair(dat), "luad28_x20": pair(big)}
start = (g["fit_theta"], g["fit_dp"], g["fit_dm"])
best = np.inf
for _ in range(3):
    t0 = time.perf_counter()
    fits = UF.bootstrap_fits(dat, 20, pm, ro.symmetric_penal, lam, key=0, start=start)
    best = min(best, time.perf_counter() - t0)
    ro.invalidate()
stab = fits.sign_stability()["theta"]
off = ~np.eye(stab.shape[0], dtype=bool)
out["bootstrap_fits_20_seconds"] = round(best, 2)
out["bootstrap_distinct_rows"] = int(fits.rows.shape[0])
out["theta_offdiag_sign_stability_min_median"] = [round(float(stab[off].min()), 2), round(float(np.median(stab[off])), 2)]
out["rel_diff_max"] = max(out[k][m] for k in ("luad28", "luad28_x20") for m in ("rel_diff_objective", "rel_diff_gradient"))
print(json.dumps(out))
