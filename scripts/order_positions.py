#!/usr/bin/env python3
"""Posterior event positions of the whole 28-event LUAD cohort (tests/golden/luad28.npz, its published-parameter point)
on the device next to the pairwise precedences and the pre-seeding posteriors, same process, best of 3 each; prints one
JSON line with the times, the rows the device turned away and the worst residuals of the identities that tie the positions
to themselves and to the other two calls, then the events of the metastasis' lineage by their mean relative position.
    python scripts/order_positions.py [reps=3] [point=fit|indep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN, OrderPositions

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
pt = sys.argv[2] if len(sys.argv) > 2 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
n = mod.n
k = dat[:, :-2].astype(int).sum(1)
eng = engine(n)
args = (mod.log_theta, mod.obs1, mod.obs2)
for call in (eng.order_posteriors, eng.order_precedences, eng.order_positions):
    call(*args, dat[:8])                                       # warm-up: runtime and module load


def best(fn):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


(le_po, _, seed_pos, st_po), t_po = best(lambda: eng.order_posteriors(*args, dat))
(_, prec, st_pr), t_pr = best(lambda: eng.order_precedences(*args, dat))
(le, pos_pt, pos_mt, st), t_ps = best(lambda: eng.order_positions(*args, dat))
(_, t_ps14) = best(lambda: eng.order_positions(*args, dat[k <= 14]))
(_, t_pr14) = best(lambda: eng.order_precedences(*args, dat[k <= 14]))
(_, t_po14) = best(lambda: eng.order_posteriors(*args, dat[k <= 14]))

# the identities, per lineage: every carried event's positions sum to 1; every position below the lineage's length sums to
# 1 over the events, the others to 0; the seeding's row is seed_pos; the mean position of an event is the summed
# precedence of the lineage's other codes over it
res = {"event_sum": 0.0, "position_sum": 0.0, "seed_pos": 0.0, "mean_vs_precedences": 0.0}
ok = st == 0
for pos, codes in ((pos_pt[ok], [2 * e for e in range(n + 1)]), (pos_mt[ok], [2 * e + 1 for e in range(n)] + [2 * n])):
    carried = ~np.isnan(pos[:, :, 0])
    length = carried.sum(axis=1)
    res["event_sum"] = max(res["event_sum"], np.abs(np.nansum(pos, axis=2) - 1.0)[carried].max())
    want = (np.arange(n + 1)[None, :] < length[:, None]).astype(float)
    res["position_sum"] = max(res["position_sum"], np.abs(np.nansum(pos, axis=1) - want).max())
    seeded = carried[:, n]
    res["seed_pos"] = max(res["seed_pos"], np.abs(pos[seeded, n] - seed_pos[ok][seeded]).max())
    before = np.nansum(prec[ok][:, codes][:, :, codes], axis=1)
    mean = np.nansum(pos * np.arange(n + 1), axis=2)
    res["mean_vs_precedences"] = max(res["mean_vs_precedences"], np.abs(mean - before)[carried].max())
print(json.dumps({
    "cohort": "luad28", "point": pt, "rows": int(len(dat)), "k_max": int(k.max()), "reps": reps,
    "order_positions_s": round(min(t_ps), 4), "order_positions_all_s": [round(t, 4) for t in t_ps],
    "order_precedences_s": round(min(t_pr), 4), "order_posteriors_s": round(min(t_po), 4),
    "order_positions_k14_s": round(min(t_ps14), 4), "order_precedences_k14_s": round(min(t_pr14), 4),
    "order_posteriors_k14_s": round(min(t_po14), 4),
    "fallback_rows": int((st != 0).sum()), "status_positions": np.bincount(st & 0xFFFF, minlength=4).tolist(),
    "max_abs_log_evidence_vs_posteriors": float(np.max(np.abs(le - le_po))),
    "worst_identity_residuals": {key: float(v) for key, v in res.items()},
}))

names = [str(e) for e in g["events"]] if "events" in g.files else [f"e{i}" for i in range(n)]
names = (names + ["seeding"])[:n] + ["seeding"]
profile = OrderPositions(le[ok], pos_pt[ok], pos_mt[ok]).relative_profile("mt", bins=120)
weight = profile.sum(axis=1)
centre = (profile * (np.arange(profile.shape[1]) + 0.5)).sum(axis=1) / np.maximum(weight, 1e-300) / profile.shape[1]
print("events of the metastasis' lineage by their mean relative position (0 first, 1 last):")
for e in np.argsort(centre):
    if weight[e] > 0:
        print(f"  {names[e]:>12s}  {centre[e]:.3f}")
