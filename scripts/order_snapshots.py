#!/usr/bin/env python3
"""Posterior genotypes at the first observation of the whole 28-event LUAD cohort (tests/golden/luad28.npz, its
published-parameter point) on the device next to the event times and the pre-seeding posteriors, same process, best of 3
each; prints one JSON line with the times, the rows the device turned away and the worst residuals of the snapshots'
identities over the paired rows - the late block sums to 1, its rows to held[r, seeding], held[0, seeding] is order_times'
pt_first, the mean number of late events is the summed deficit of the other tumour's codes, the codes of the observed tumour
are held, the evidence is order_posteriors', and "unknown" is the mixture of "PT" and "Met" -, then the ten mutations with the
largest cohort_late().
    python scripts/order_snapshots.py [reps=3] [point=fit|indep]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.jx import engine
from metmhn_amd.model import MetMHN, OrderSnapshots

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
pt = sys.argv[2] if len(sys.argv) > 2 else "fit"
dat = g["dat"]
mod = MetMHN(g[pt + "_theta"], g[pt + "_dp"], g[pt + "_dm"])
n = mod.n
S = 2 * n
k = dat[:, :-2].astype(int).sum(1)
eng = engine(n)
args = (mod.log_theta, mod.obs1, mod.obs2)
for call in (eng.order_posteriors, eng.order_times, eng.order_snapshots):
    call(*args, dat[:8])                                       # warm-up: runtime and module load


def best(fn):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return out, times


(le_po, _, _, st_po), t_po = best(lambda: eng.order_posteriors(*args, dat))
(_, _, _, ptf, st_tm), t_tm = best(lambda: eng.order_times(*args, dat))
(le, held, late, mstate, mfirst, mprob, st), t_sn = best(lambda: eng.order_snapshots(*args, dat))
(_, t_sn14) = best(lambda: eng.order_snapshots(*args, dat[k <= 14]))
(_, t_tm14) = best(lambda: eng.order_times(*args, dat[k <= 14]))
(_, t_po14) = best(lambda: eng.order_posteriors(*args, dat[k <= 14]))

nz = lambda d: np.where(np.isnan(d), 0.0, d)
pr = np.flatnonzero((st == 0) & (dat[:, -1] == 3))
H, La = held[pr], late[pr]
has = ~np.isnan(H[:, 0, :S])                                   # [rows, 2n]: the codes below the seeding a row carries
other = (has[:, 1::2], has[:, 0::2])                           # regime 0: the MT codes are the other tumour's; 1: the PT's
deficit = [nz(H[:, r, S, None] - H[:, r, r ^ 1:S:2]) * other[r] for r in (0, 1)]
own = [nz(np.abs(H[:, r, S, None] - H[:, r, r:S:2])) * other[r ^ 1] for r in (0, 1)]
res = {"late_block_sum": float(np.abs(La.sum(axis=(1, 2)) - 1.0).max()),
       "late_rows_vs_held_seeding": float(np.abs(La.sum(axis=2) - H[:, :, S]).max()),
       "held_seeding_sum": float(np.abs(H[:, 0, S] + H[:, 1, S] - 1.0).max()),
       "pt_first_vs_order_times": float(np.abs(H[:, 0, S] - ptf[pr]).max()),
       "mean_late_count_vs_deficits": float(max(np.abs(La[:, r] @ np.arange(n + 1) - deficit[r].sum(axis=1)).max()
                                                for r in (0, 1))),
       "own_codes_vs_held_seeding": float(max(o.max() for o in own)),
       "map_prob_over_held_seeding": float((mprob[pr] - H[np.arange(len(pr)), mfirst[pr], S]).max())}
# the paired rows under the three diagnosis orders: "unknown" is the mixture of "PT" and "Met"
runs = []
for d in (0, 1, 2):
    rows = dat[pr].copy()
    rows[:, -2] = d
    runs.append(eng.order_snapshots(*args, rows))
(le_u, h_u, l_u, *_), (le_p, h_p, l_p, *_), (le_m, h_m, l_m, *_) = runs
p = np.exp(le_p - le_u)
res["mixture_evidence"] = float(np.abs(np.exp(le_p - le_u) + np.exp(le_m - le_u) - 1.0).max())
res["mixture_held"] = float(max(nz(np.abs(h_u[:, 0] - p[:, None] * h_p[:, 0])).max(),
                                nz(np.abs(h_u[:, 1] - (1 - p)[:, None] * h_m[:, 1])).max()))
res["mixture_late"] = float(max(np.abs(l_u[:, 0] - p[:, None] * l_p[:, 0]).max(),
                                np.abs(l_u[:, 1] - (1 - p)[:, None] * l_m[:, 1]).max()))
res["excluded_regime_exact_zero"] = bool(np.all(nz(h_p[:, 1]) == 0.0) and np.all(nz(h_m[:, 0]) == 0.0)
                                         and np.all(l_p[:, 1] == 0.0) and np.all(l_m[:, 0] == 0.0))
print(json.dumps({
    "cohort": "luad28", "point": pt, "rows": int(len(dat)), "k_max": int(k.max()), "reps": reps,
    "order_snapshots_s": round(min(t_sn), 4), "order_snapshots_all_s": [round(t, 4) for t in t_sn],
    "order_times_s": round(min(t_tm), 4), "order_posteriors_s": round(min(t_po), 4),
    "order_snapshots_k14_s": round(min(t_sn14), 4), "order_times_k14_s": round(min(t_tm14), 4),
    "order_posteriors_k14_s": round(min(t_po14), 4),
    "fallback_rows": int((st != 0).sum()), "status_snapshots": np.bincount(st & 0xFFFF, minlength=4).tolist(),
    "max_abs_log_evidence_vs_posteriors": float(np.max(np.abs(le - le_po)[st == 0])),
    "paired_rows": int(len(pr)), "worst_identity_residuals": res,
}))

names = [str(e) for e in g["events"]] if "events" in g.files else [f"e{i}" for i in range(n)]
ok = st == 0
run = OrderSnapshots(le[ok], held[ok], late[ok], mstate[ok], mfirst[ok], mprob[ok])
cl = run.cohort_late()
print("mutations by cohort_late() (mean over the paired rows that carry the mutation in the later-observed tumour only of "
      "P(that tumour was observed second and the mutation arose after the first observation)):")
for i in sorted((i for i in range(n) if not np.isnan(cl[i])), key=lambda i: -cl[i])[:10]:
    print(f"  {names[i]:>12s}  {cl[i]:.3f}")
