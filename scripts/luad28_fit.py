#!/usr/bin/env python3
"""examples/analysis.py:104-113 of the reference on the engine: learn_mhn of the 28-event LUAD cohort from indep(dat)
(tests/golden/luad28.npz; perc_met 0.2, lambda 1e-3 as in the LUAD fixtures, SciPy L-BFGS-B with the reference's default
ftol 1e-4 and with 1e-8) - wall time, evaluations, objective, and the objective at the reference's published parameters.
    python scripts/luad28_fit.py [--unknown]
--unknown: the same run a second time with the 1 227 primary tumours of unknown metastatic status appended as rows of type 4
(tests/golden/luad28_unknown_rows.npy): evaluation time, fit time and evaluation count of both cohorts, taken in this run."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import metmhn_amd.regularized_optimization as ro
from metmhn_amd.Utilityfunctions import indep

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
pm, lam = float(g["perc_met"]), float(g["lam"])
pub = np.concatenate((g["fit_theta"].flatten(), g["fit_dp"], g["fit_dm"]))
calls = [0]
orig = ro.score_and_grad_reg


def counted(*a, **k):
    calls[0] += 1
    return orig(*a, **k)


ro.score_and_grad_reg = counted


def run(dat, tag, start):
    v_pub = float(ro.score_reg(pub, dat, pm, ro.symmetric_penal, lam))
    print(f"[{tag}] {dat.shape[0]} rows; objective at the published parameters: {v_pub:.10f}"
          + (f" (fixture {float(g['fit_reg_value']):.10f})" if tag == "known" else ""))
    reps = 50
    for _ in range(5):
        orig(pub, dat, pm, ro.symmetric_penal, lam)
    t0 = time.perf_counter()
    for _ in range(reps):
        orig(pub, dat, pm, ro.symmetric_penal, lam)
    print(f"[{tag}] score_and_grad_reg at the published parameters: {(time.perf_counter() - t0) / reps * 1e3:.3f} ms per evaluation ({reps} calls)")
    for ftol in (1e-4, 1e-8):
        calls[0] = 0
        t0 = time.perf_counter()
        th, dp, dm = ro.learn_mhn(*start, dat, pm, ro.symmetric_penal, lam, opt_ftol=ftol, opt_v=False)
        dt = time.perf_counter() - t0
        v = float(ro.score_reg(np.concatenate((th.flatten(), dp, dm)), dat, pm, ro.symmetric_penal, lam))
        print(f"[{tag}] learn_mhn ftol {ftol:g}: {dt:.2f} s, {calls[0]} evaluations ({dt / max(calls[0], 1) * 1e3:.2f} ms each incl. SciPy), objective {v:.10f}")
    return th, dp, dm


dat = g["dat"]
run(dat, "known", (g["indep_theta"], g["indep_dp"], g["indep_dm"]))
if "--unknown" in sys.argv[1:]:
    both = np.ascontiguousarray(np.vstack((dat, np.load(os.path.join(ROOT, "tests", "golden", "luad28_unknown_rows.npy")))))
    th, dp, dm = run(both, "known + unknown", indep(both))
    ps = ro.met_status_posterior(th, dp, dm, both[dat.shape[0]:])
    print(f"[known + unknown] P(seeded | genotype) of the {ps.size} primaries of unknown status at the fit: "
          f"min {ps.min():.3f}, median {np.median(ps):.3f}, mean {ps.mean():.3f}, max {ps.max():.3f}")
