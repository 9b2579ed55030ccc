#!/usr/bin/env python3
"""Likeliest orders and pre-seeding posteriors of the whole 28-event LUAD cohort (tests/golden/luad28.npz, its
published-parameter point) on the device, same process, best of 3 each; prints one JSON line.
    python scripts/order_posteriors.py [reps=3] [point=fit|indep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN, OrderPosteriors

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
pt = sys.argv[2] if len(sys.argv) > 2 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
k = dat[:, :-2].astype(int).sum(1)
eng = engine(mod.n)
args = (mod.log_theta, mod.obs1, mod.obs2)
eng.likeliest_orders(*args, dat[:8])                           # warm-up: runtime and module load
eng.order_posteriors(*args, dat[:8])


def best(fn):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


(orders, prob, st_lo), t_lo = best(lambda: eng.likeliest_orders(*args, dat))
(le, pre, sp, st_po), t_po = best(lambda: eng.order_posteriors(*args, dat))
(_, t_14) = best(lambda: eng.order_posteriors(*args, dat[k <= 14]))
eng.set_cohort(dat)
lp = eng.patient_grads(*args, with_grad=False)
print(json.dumps({
    "cohort": "luad28", "point": pt, "rows": int(len(dat)), "k_max": int(k.max()), "reps": reps,
    "likeliest_orders_s": round(min(t_lo), 4), "likeliest_orders_all_s": [round(t, 4) for t in t_lo],
    "order_posteriors_s": round(min(t_po), 4), "order_posteriors_all_s": [round(t, 4) for t in t_po],
    "order_posteriors_k14_s": round(min(t_14), 4),
    "status_orders": np.bincount(st_lo, minlength=4).tolist(), "status_posteriors": np.bincount(st_po, minlength=4).tolist(),
    "max_rel_lp_vs_patient_grads": float(np.max(np.abs(le - lp) / np.abs(lp))),
    "cohort_preseeding_max": float(np.max(OrderPosteriors(le, pre, sp).cohort_preseeding())),
}))
