#!/usr/bin/env python3
"""Posterior order samples of the whole 28-event LUAD cohort (tests/golden/luad28.npz, its fit point) on the device, 1 000
samples per row, next to the pairwise precedences of the same cohort, same process, best of 3 each; prints one JSON line
with the times per call - also of a call without samples (the passes alone) and of 100 samples per row, which separate the
passes from the walk and the download of the orders -, the rows the device turned away and the worst distance of the
sample means from the exact marginals in units of the statistical bar 5 sqrt(p (1 - p) / M) + 1 / M.
    python scripts/order_samples.py [reps=3] [samples=1000] [point=fit|indep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN, OrderSamples

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
M = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
pt = sys.argv[3] if len(sys.argv) > 3 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
n = mod.n
k = dat[:, :-2].astype(int).sum(1)
eng = engine(n)
args = (mod.log_theta, mod.obs1, mod.obs2)
eng.order_precedences(*args, dat[:8])                          # warm-up: runtime and module load
eng.order_samples(*args, dat[:8], 8)


def best(fn):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


(le_pr, prec, st_pr), t_pr = best(lambda: eng.order_precedences(*args, dat))
(le, orders, log_prob, st), t_sm = best(lambda: eng.order_samples(*args, dat, M, 1))
_, t_none = best(lambda: eng.order_samples(*args, dat, 0, 1))
_, t_tenth = best(lambda: eng.order_samples(*args, dat, M // 10, 1))
_, t_sm14 = best(lambda: eng.order_samples(*args, dat[k <= 14], M, 1))
_, t_pr14 = best(lambda: eng.order_precedences(*args, dat[k <= 14]))

ok = (st == 0) & (st_pr == 0)
run = OrderSamples(le[ok], orders[ok], log_prob[ok])
t0 = time.perf_counter()
est = run.precedence()
t_mean = time.perf_counter() - t0
exact = prec[ok]
have = ~np.isnan(exact)
p = np.clip(exact[have], 0.0, 1.0)
units = np.abs(est[have] - p) / (5.0 * np.sqrt(p * (1.0 - p) / M) + 1.0 / M)
print(json.dumps({
    "cohort": "luad28", "point": pt, "rows": int(len(dat)), "k_max": int(k.max()), "reps": reps, "samples_per_row": M,
    "orders_bytes": int(orders.nbytes + log_prob.nbytes),
    "order_samples_s": round(min(t_sm), 4), "order_samples_all_s": [round(t, 4) for t in t_sm],
    "order_samples_no_samples_s": round(min(t_none), 4), "order_samples_tenth_s": round(min(t_tenth), 4),
    "order_precedences_s": round(min(t_pr), 4),
    "order_samples_k14_s": round(min(t_sm14), 4), "order_precedences_k14_s": round(min(t_pr14), 4),
    "fallback_rows": int((st != 0).sum()), "status_samples": np.bincount(st & 0xFFFF, minlength=4).tolist(),
    "max_abs_log_evidence_vs_precedences": float(np.max(np.abs(le[ok] - le_pr[ok]))),
    "precedence_entries": int(have.sum()), "worst_mean_in_units_of_the_bar": float(units.max()),
    "host_precedence_means_s": round(t_mean, 3),
}))
