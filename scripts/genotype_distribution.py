#!/usr/bin/env python3
"""The genotype distribution of the primary tumour of the 28-event LUAD model (tests/golden/luad28.npz, its fitted
parameters) on the device: best-of-`reps` seconds per call of mmhn_genotype_distribution with and without the summary,
queried at every distinct primary-tumour genotype of the cohort (a call allocates its workspace, sweeps all 2^28
genotypes, folds the summary, gathers the queries and frees the workspace: the seconds are the call's), next to
mmhn_seeding_landscape until the observation in the same run; the two masses; mass[1] against the landscape's p_seed of
the empty genotype; the share of the NM mass that lies on the genotypes the cohort observed; the ten largest residuals of
GenotypeSummary.compare; the exact NM and EM-PT frequencies next to simulate_pairs' estimates.  One JSON line, progress
on stderr.
    python scripts/genotype_distribution.py [reps=3] [workspace GiB=128] [samples=1000000]"""
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.engine import Engine
from metmhn_amd.model import GENOTYPE_STRATA, GenotypeSummary, MetMHN
from metmhn_amd.simulations import simulate_pairs

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ws_gib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
n_sim = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n = mod.n
pts = np.unique(dat[np.isin(dat[:, -1], (0, 1, 3, 4))][:, 0:2 * n:2], axis=0).astype(np.int8)
c = min(n, int(re.search(r"LS_TILE_BITS = (\d+);", open(os.path.join(ROOT, "metmhn_amd", "csrc", "lattice.h")).read()).group(1)))
sweep_bytes = ((n - c) / 2 + 1) * 16 * 2 ** n + 32 * 2 ** n    # a tile reads (n - c) / 2 finished tiles on average and is written once; the planes are read and written once more on the way to probabilities


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


res = {"cohort": "luad28", "point": "fit", "n_mut": n, "tile_bits": c, "genotypes": 1 << n, "rate_products": n << n,
       "distinct_pt_genotypes": int(len(pts)), "workspace_limit_gib": ws_gib, "planes_gib": round(16 * 2 ** n / 2 ** 30, 2),
       "sweep_gib": round(sweep_bytes / 2 ** 30, 1), "reps": reps}
with Engine(n, workspace_bytes=ws_gib << 30) as eng:
    args = (mod.log_theta, mod.obs1)
    t0 = time.perf_counter()
    eng.genotype_distribution(*args, pts[:1])                                    # warm-up: runtime and module load
    eng.seeding_landscape(*args, pts[:1], "observation")
    say(f"first calls took {time.perf_counter() - t0:.3f} s")
    (values, status, sums, _), secs = best(lambda: eng.genotype_distribution(*args, pts, summary=True), "with the summary")
    assert (status == 0).all()
    res["with_summary_s"], res["with_summary_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    (plain, status, none, _), secs = best(lambda: eng.genotype_distribution(*args, pts, summary=False), "without the summary")
    assert (status == 0).all() and none is None and plain.tobytes() == values.tobytes()
    res["without_summary_s"], res["without_summary_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    res["without_summary_rate_products_per_s"] = float(f"{(n << n) / min(secs):.4g}")
    res["without_summary_sweep_gb_per_s"] = round(sweep_bytes / min(secs) / 1e9, 1)
    (back, status, _), secs = best(lambda: eng.seeding_landscape(*args, np.vstack((np.zeros((1, n), dtype=np.int8), pts)),
                                                                 "observation"), "seeding landscape until the observation")
    assert (status == 0).all()
    res["landscape_until_observation_s"], res["landscape_until_observation_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    res["bench_stream_copy_gb_per_s"] = round(eng.bench_stream(), 1)
summary = GenotypeSummary(*sums)
res["mass"] = [float(m) for m in summary.mass]
res["mass_sum_minus_1"] = float(summary.mass.sum() - 1.0)
res["mass1_against_landscape_p_seed_of_empty_relative"] = float(abs(summary.mass[1] - back[0, 0]) / back[0, 0])
nm = np.unique(dat[dat[:, -1] == 0][:, 0:2 * n:2], axis=0).astype(np.int8)
at = mod.genotype_distribution_at(nm)
res["nm_distinct_genotypes"] = int(len(nm))
res["nm_mass_share_on_observed_genotypes"] = float(at.unseeded.sum() / summary.mass[0])
resid = summary.compare(dat)
top = []
for stratum, r in resid.items():
    iu = np.triu_indices(n)
    for i, j, v in zip(*iu, r[iu]):
        if np.isfinite(v):
            top.append((abs(float(v)), stratum, int(i), int(j), float(v)))
top.sort(reverse=True)
res["rows_per_stratum"] = {s: int((dat[:, -1] == t).sum()) for s, t in zip(GENOTYPE_STRATA, (0, 1, 4))}
res["largest_residuals_stratum_i_j_value"] = [[s, i, j, round(v, 3)] for _, s, i, j, v in top[:10]]
t0 = time.perf_counter()
sim = simulate_pairs(mod.log_theta, mod.obs1, mod.obs2, n_sim, original_key=0)
res["simulate_pairs_s"], res["samples"] = round(time.perf_counter() - t0, 3), n_sim
for stratum in ("NM", "EM-PT"):
    exact = summary.frequencies(stratum)
    est = sim.frequencies(stratum)[0::2, 0::2]
    rows = int(sim.n_class[0]) if stratum == "NM" else int(sim.n_class[1] + sim.n_class[2])
    z = (est - exact) / np.sqrt(exact * (1.0 - exact) / rows)
    res[f"{stratum}_samples"] = rows
    res[f"{stratum}_marginals_exact"] = [round(float(v), 5) for v in np.diag(exact)]
    res[f"{stratum}_marginals_simulated"] = [round(float(v), 5) for v in np.diag(est)]
    res[f"{stratum}_largest_deviation_in_binomial_standard_errors"] = float(np.nanmax(np.abs(z)))
print(json.dumps(res))
