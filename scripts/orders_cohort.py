#!/usr/bin/env python3
"""Likeliest orders of the whole 28-event LUAD cohort (tests/golden/luad28.npz, fitted parameters) on the device in one
call, against the host loop (MetMHN.likeliest_order per row) on the rows with at most 14 occupied slots.
    python scripts/orders_cohort.py [reps=3] [point=fit|indep]"""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
pt = sys.argv[2] if len(sys.argv) > 2 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
k = dat[:, :-2].astype(int).sum(1)
paired = dat[:, -1] == 3
eng = engine(mod.n)
args = (mod.log_theta, mod.obs1, mod.obs2)
eng.likeliest_orders(*args, dat[:8])                           # warm-up: runtime and module load
times = []
for _ in range(reps):
    t0 = time.perf_counter()
    orders, prob, status = eng.likeliest_orders(*args, dat)
    times.append(time.perf_counter() - t0)
print(f"device, whole cohort: {len(dat)} rows ({paired.sum()} paired, k <= {k.max()}), "
      f"{min(times):.3f} s per call (best of {reps}; all: {', '.join(f'{t:.3f}' for t in times)}); "
      f"status counts {np.bincount(status, minlength=4).tolist()}", flush=True)
t0 = time.perf_counter()
eng.likeliest_orders(*args, dat[k <= 14])
t_dev14 = time.perf_counter() - t0
sub = np.flatnonzero(k <= 14)
with warnings.catch_warnings():
    warnings.simplefilter("ignore", DeprecationWarning)
    t0 = time.perf_counter()
    host = mod.likeliest_orders(dat[sub], backend="host")
    t_host = time.perf_counter() - t0
worst = max(abs(p - prob[i]) / p for i, (_, p) in zip(sub, host))
same = sum(tuple(int(e) for e in orders[i] if e >= 0) == o for i, (o, _) in zip(sub, host))
print(f"k <= 14 subset: {len(sub)} rows ({paired[sub].sum()} paired); device {t_dev14:.3f} s, host loop {t_host:.1f} s "
      f"({t_host / t_dev14:.0f}x); same order {same}/{len(sub)}, max rel. prob difference {worst:.1e}", flush=True)
