#!/usr/bin/env python3
"""Pairwise precedence posteriors of the whole 28-event LUAD cohort (tests/golden/luad28.npz, its published-parameter
point) on the device next to the pre-seeding posteriors, same process, best of 3 each; prints one JSON line, then the ten
most and the ten least decided pairs of the cohort mean.
    python scripts/order_precedences.py [reps=3] [point=fit|indep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN, OrderPrecedences

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
pt = sys.argv[2] if len(sys.argv) > 2 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
n = mod.n
k = dat[:, :-2].astype(int).sum(1)
eng = engine(n)
args = (mod.log_theta, mod.obs1, mod.obs2)
eng.order_posteriors(*args, dat[:8])                           # warm-up: runtime and module load
eng.order_precedences(*args, dat[:8])


def best(fn):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


(le_po, pre, _, st_po), t_po = best(lambda: eng.order_posteriors(*args, dat))
(le, prec, st_pr), t_pr = best(lambda: eng.order_precedences(*args, dat))
(_, t_14) = best(lambda: eng.order_precedences(*args, dat[k <= 14]))
(_, t_po14) = best(lambda: eng.order_posteriors(*args, dat[k <= 14]))
mean = OrderPrecedences(le, prec).cohort_mean()
print(json.dumps({
    "cohort": "luad28", "point": pt, "rows": int(len(dat)), "k_max": int(k.max()), "reps": reps,
    "order_posteriors_s": round(min(t_po), 4), "order_posteriors_k14_s": round(min(t_po14), 4),
    "order_precedences_s": round(min(t_pr), 4), "order_precedences_all_s": [round(t, 4) for t in t_pr],
    "order_precedences_k14_s": round(min(t_14), 4),
    "status_posteriors": np.bincount(st_po, minlength=4).tolist(), "status_precedences": np.bincount(st_pr, minlength=4).tolist(),
    "max_abs_log_evidence_vs_posteriors": float(np.max(np.abs(le - le_po))),
}))

names = [str(e) for e in g["events"]] if "events" in g.files else [f"e{i}" for i in range(n)] + ["seeding"]


def label(c):
    return "seeding" if c == 2 * n else f"{names[c // 2]}({'MT' if c % 2 else 'PT'})"


# every unordered pair once, as (c, d) with c the likelier first; a pair no row carries is left out
pairs = [(max(mean[c, d], mean[d, c]), (c, d) if mean[c, d] >= mean[d, c] else (d, c))
         for c in range(2 * n + 1) for d in range(c + 1, 2 * n + 1) if not np.isnan(mean[c, d])]
pairs.sort(key=lambda p: -p[0])
for title, part in (("most decided", pairs[:10]), ("least decided", pairs[-10:])):
    print(title + " pairs of the cohort mean:")
    for p, (c, d) in part:
        print(f"  P({label(c)} before {label(d)}) = {p:.4f}   (the reverse {mean[d, c]:.4f})")
