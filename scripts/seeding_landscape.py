#!/usr/bin/env python3
"""The seeding landscape of the 28-event LUAD model (tests/golden/luad28.npz, its fitted parameters) on the device: best-of-
`reps` seconds per call of mmhn_seeding_landscape until the seeding and until the observation, queried at every distinct
primary-tumour genotype of the cohort (a call allocates its workspace, sweeps all 2^28 genotypes, gathers the queries and
frees the workspace: the seconds are the call's), moves per second, the bytes the sweep must move over the time next to
Engine.bench_stream's copy rate, the time of mmhn_seeding_forecasts on the same genotypes and the worst relative difference
of the four values between the two, and the distribution of p_seed over ALL genotypes against the cohort's.  One JSON line,
progress on stderr.
    python scripts/seeding_landscape.py [reps=3] [workspace GiB=128] [forecasts=1] [full=1]"""
import json
import os
import re
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
with_forecasts = bool(int(sys.argv[3])) if len(sys.argv) > 3 else True
with_full = bool(int(sys.argv[4])) if len(sys.argv) > 4 else True
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n = mod.n
pts = np.unique(dat[np.isin(dat[:, -1], (0, 1, 3, 4))][:, 0:2 * n:2], axis=0).astype(np.int8)
c = min(n, int(re.search(r"LS_TILE_BITS = (\d+);", open(os.path.join(ROOT, "metmhn_amd", "csrc", "lattice.h")).read()).group(1)))
moves = n << (n - 1)                                   # pairs (x, j not in x)
sweep_bytes = ((n - c) / 2 + 1) * 32 * 2 ** n          # a tile reads (n - c) / 2 finished tiles on average and is written once
QS = (0, .05, .25, .5, .75, .95, 1)


def say(text):
    print(text, file=sys.stderr, flush=True)


def best(fn, what):
    times = []
    for i in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
        say(f"{what}: call {i + 1} of {reps} took {times[-1]:.4f} s")
    return out, times


def worst_rel(a, b):
    live = b != 0
    return float(np.max(np.abs(a[live] - b[live]) / np.abs(b[live]), initial=0.0))


res = {"cohort": "luad28", "point": "fit", "n_mut": n, "tile_bits": c, "genotypes": 1 << n, "moves": moves,
       "distinct_pt_genotypes": int(len(pts)), "workspace_limit_gib": ws_gib, "landscape_gib": round(32 * 2 ** n / 2 ** 30, 2),
       "sweep_gib": round(sweep_bytes / 2 ** 30, 1), "reps": reps}
with Engine(n, workspace_bytes=ws_gib << 30) as eng:
    args = (mod.log_theta, mod.obs1)
    t0 = time.perf_counter()
    eng.seeding_landscape(*args, pts[:1], "observation")                         # warm-up: runtime and module load
    say(f"first call took {time.perf_counter() - t0:.3f} s")
    out = {}
    for until in ("seeding", "observation"):
        (out[until], status, _), secs = best(lambda: eng.seeding_landscape(*args, pts, until), until)
        assert (status == 0).all()
        res[f"until_{until}_s"] = round(min(secs), 4)
        res[f"until_{until}_all_s"] = [round(t, 4) for t in secs]
        res[f"until_{until}_moves_per_s"] = float(f"{moves / min(secs):.4g}")
        res[f"until_{until}_sweep_gb_per_s"] = round(sweep_bytes / min(secs) / 1e9, 1)
    res["bench_stream_copy_gb_per_s"] = round(eng.bench_stream(), 1)
    if with_forecasts:
        for until in ("seeding", "observation"):
            t0 = time.perf_counter()
            p_seed, tm, before, with_seed, _, st = eng.seeding_forecasts(*args, pts, until)
            res[f"forecasts_until_{until}_s"] = round(time.perf_counter() - t0, 3)
            say(f"seeding_forecasts until {until}: {res[f'forecasts_until_{until}_s']} s")
            ok = st == 0
            ref = np.stack([p_seed, tm, np.nansum(before, axis=1), np.nansum(with_seed, axis=1)], axis=1)
            res[f"forecasts_until_{until}_rows"] = int(ok.sum())
            res[f"worst_relative_difference_until_{until}"] = [worst_rel(out[until][ok, k], ref[ok, k]) for k in range(4)]
    v = out["observation"]
    res["cohort_p_seed_quantiles_0_5_25_50_75_95_100"] = [float(q) for q in np.quantile(v[:, 0], QS)]
    res["cohort_new_events_quantiles_0_50_100"] = [float(q) for q in np.quantile(v[:, 2], (0, .5, 1))]
    res["p_seed_until_seeding_max_abs_deviation_from_1"] = float(np.abs(out["seeding"][:, 0] - 1.0).max())
    if with_full:
        t0 = time.perf_counter()
        _, _, whole = eng.seeding_landscape(*args, pts[:0], "observation", full=True)
        res["full_copy_call_s"] = round(time.perf_counter() - t0, 2)
        say(f"call with the full landscape copied out: {res['full_copy_call_s']} s")
        codes = pts.astype(np.int64) @ (1 << np.arange(n, dtype=np.int64))
        assert np.ascontiguousarray(whole[:, codes].T).tobytes() == v.tobytes()
        res["all_p_seed_quantiles_0_5_25_50_75_95_100"] = [float(q) for q in np.quantile(whole[0], QS)]
        res["all_new_events_quantiles_0_50_100"] = [float(q) for q in np.quantile(whole[2], (0, .5, 1))]
print(json.dumps(res))
