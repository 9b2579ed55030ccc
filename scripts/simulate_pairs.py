#!/usr/bin/env python3
"""Throughput of the pair sampler (mmhn_simulate_pairs) next to the summary sampler (mmhn_simulate_summary) in one process,
then the posterior-predictive check the pair tables exist for: the ten largest standardised residuals of the 28-event LUAD
cohort's observed co-occurrence counts (tests/golden/luad28.npz) against the model at its fit point.
    python scripts/simulate_pairs.py [n_mut=20] [n_sim=1e7] [long n_sim=1e8] [luad n_sim=1e8]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd import Engine, synthetic
from metmhn_amd import simulations as S
from metmhn_amd.Utilityfunctions import pair_counts

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sizes = [int(float(sys.argv[i])) if len(sys.argv) > i else d for i, d in ((2, 10_000_000), (3, 100_000_000))]
n_luad = int(float(sys.argv[4])) if len(sys.argv) > 4 else 100_000_000
lt, dp, dm = synthetic.random_params(n)
e = Engine(n)
e.simulate_summary(lt, dp, dm, 100_000, 1)                         # warm-up: runtime and module load
e.simulate_pairs(lt, dp, dm, 100_000, 1)


def rates(fn, ns, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return [ns / t / 1e6 for t in sorted(ts)]                      # M samples/s, best first


for ns in sizes:
    # alternate the two so that both see the same state of the machine
    rs, rp = [], []
    for _ in range(3):
        rs += rates(lambda: e.simulate_summary(lt, dp, dm, ns, 2), ns, 1)
        rp += rates(lambda: e.simulate_pairs(lt, dp, dm, ns, 2), ns, 1)
    print(json.dumps({"n_mut": n, "n_sim": ns, "unit": "M samples/s",
                      "simulate_summary": {"best": round(max(rs), 1), "all": [round(r, 1) for r in rs]},
                      "simulate_pairs": {"best": round(max(rp), 1), "all": [round(r, 1) for r in rp]},
                      "pairs_over_summary": round(max(rp) / max(rs), 3)}), flush=True)

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
dat = g["dat"]
n28 = g["fit_theta"].shape[0] - 1
names = [str(x) for x in g["events"]] if "events" in g.files else [f"e{i}" for i in range(n28)]
t0 = time.perf_counter()
s = S.simulate_pairs(g["fit_theta"], g["fit_dp"], g["fit_dm"], n_luad, original_key=28)
print(f"luad28 fit point: {n_luad} samples in {time.perf_counter() - t0:.2f} s, classes {s.n_class.tolist()}", flush=True)
label = lambda c: f"{names[c // 2]}({'MT' if c % 2 else 'PT'})"
rows = []
obs = pair_counts(dat)[1]
for stratum, r in s.compare(dat).items():
    p = s.frequencies(stratum)
    t = S.STRATA.index(stratum)
    n_t = int(np.count_nonzero(dat[:, -1] == t))
    for a, b in zip(*np.triu_indices(2 * n28)):
        if not np.isnan(r[a, b]):
            rows.append((abs(r[a, b]), stratum, n_t, a, b, r[a, b], p[a, b], int(obs[t][a, b])))
rows.sort(key=lambda x: -x[0])
print(f"ten largest residuals of {len(rows)} observed (stratum, pair) cells [(obs - n p) / sqrt(n p (1 - p))]:")
for _, stratum, n_t, a, b, r, p, o in rows[:10]:
    what = label(a) if a == b else f"{label(a)} & {label(b)}"
    print(f"  {stratum:7s} n={n_t:5d}  {what:32s} model p = {p:.5f}  expected {n_t * p:8.2f}  observed {o:5d}  residual {r:+7.2f}")
