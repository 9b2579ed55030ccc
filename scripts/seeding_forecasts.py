#!/usr/bin/env python3
"""Seeding forecasts of every distinct primary-tumour genotype of the 28-event LUAD cohort (tests/golden/luad28.npz, its
fitted parameters) on the device: best-of-`reps` seconds per call of mmhn_seeding_forecasts until the seeding and until the
observation, the batches a call takes under the workspace limit, the host definition's time on a sample of the rows with at
most 20 free mutations next to the device's time on the same rows, their worst relative difference, and the distribution of
p_seed.  One JSON line, progress on stderr.
    python scripts/seeding_forecasts.py [reps=3] [workspace GiB=128] [host rows=12]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.engine import Engine
from metmhn_amd.model import MetMHN

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ws_gib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
host_rows = int(sys.argv[3]) if len(sys.argv) > 3 else 12
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n = mod.n
pts = np.unique(dat[np.isin(dat[:, -1], (0, 1, 3, 4))][:, 0:2 * n:2], axis=0).astype(np.int8)
f = n - pts.sum(axis=1)
limit = ws_gib << 30


def row_bytes(fr):
    """forecast.h fc_doubles: the lattice and, per tile of 2^(c + tb) states, 3 f + 3 doubles of partials."""
    c = min(fr, 10)
    tb = min(fr - c, 4)
    return 8 * ((1 << fr) + (1 << (fr - c - tb)) * (3 * fr + 3))


def batches(fs):
    """forecast_host.h's cut: rows in call order while they fit."""
    count, used = 1, 0
    for fr in fs:
        b = row_bytes(int(fr))
        if used and used + b > limit:
            count, used = count + 1, 0
        used += b
    return count


def best(fn, what):
    times = []
    for i in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
        print(f"{what}: call {i + 1} of {reps} took {times[-1]:.3f} s", file=sys.stderr, flush=True)
    return out, times


with Engine(n, workspace_bytes=limit) as eng:
    args = (mod.log_theta, mod.obs1)
    eng.seeding_forecasts(*args, pts[np.argsort(f)[:8]], "observation")         # warm-up: runtime and module load
    out, secs = {}, {}
    for until in ("seeding", "observation"):
        out[until], secs[until] = best(lambda: eng.seeding_forecasts(*args, pts, until), until)
    status = out["observation"][-1]
    ok = status == 0
    small = np.flatnonzero(ok & (f <= 20))
    pick = small[np.linspace(0, len(small) - 1, min(host_rows, len(small))).astype(int)] if len(small) else small
    t0 = time.perf_counter()
    ref = [mod.seeding_forecast(pts[i], "observation") for i in pick]
    t_host = time.perf_counter() - t0
    (dev, t_dev) = best(lambda: eng.seeding_forecasts(*args, pts[pick], "observation"), "host sample on the device")

worst = 0.0
for j, r in enumerate(ref):
    for name, a in zip(("p_seed", "time", "before", "with_seed", "n_before"), dev):
        x, y = np.asarray(a[j], dtype=float), np.asarray(getattr(r, name), dtype=float)
        live = ~np.isnan(y) & (y != 0)
        worst = max(worst, float(np.max(np.abs(x[live] - y[live]) / y[live], initial=0.0)))
p = out["observation"][0][ok]
new = np.nansum(out["observation"][2][ok], axis=1)
print(json.dumps({
    "cohort": "luad28", "point": "fit", "distinct_pt_genotypes": int(len(pts)), "f_min": int(f.min()), "f_max": int(f.max()),
    "states": int(sum(1 << int(x) for x in f)), "moves": int(sum(int(x) << int(x) for x in f)),
    "workspace_limit_gib": ws_gib, "lattice_gib": round(sum(row_bytes(int(x)) for x in f) / 2 ** 30, 1),
    "batches": batches(f), "status": np.bincount(status & 0xFFFF, minlength=4).tolist(), "reps": reps,
    "until_seeding_s": round(min(secs["seeding"]), 3), "until_seeding_all_s": [round(t, 3) for t in secs["seeding"]],
    "until_observation_s": round(min(secs["observation"]), 3),
    "until_observation_all_s": [round(t, 3) for t in secs["observation"]],
    "host_sample_rows": int(len(pick)), "host_sample_f": [int(x) for x in f[pick]], "host_sample_s": round(t_host, 3),
    "device_on_host_sample_s": round(min(t_dev), 4), "worst_relative_difference_on_sample": worst,
    "p_seed_quantiles_0_5_25_50_75_95_100": [float(q) for q in np.quantile(p, (0, .05, .25, .5, .75, .95, 1))],
    "p_seed_until_seeding_max_abs_deviation_from_1": float(np.abs(out["seeding"][0][ok] - 1.0).max()),
    "expected_new_events_quantiles_0_50_100": [float(q) for q in np.quantile(new, (0, .5, 1))],
    "expected_time_until_seeding_quantiles_0_50_100": [float(q) for q in np.quantile(out["seeding"][1][ok], (0, .5, 1))],
}))
