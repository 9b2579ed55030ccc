#!/usr/bin/env python3
"""The genotype distribution of the metastasis and of its founder of the 28-event LUAD model (tests/golden/luad28.npz, its
fitted parameters) on the device: best-of-`reps` seconds per call of mmhn_metastasis_distribution with and without the
summary, queried at every distinct metastasis genotype of the cohort (a call allocates its workspace, sweeps all 2^28
genotypes, folds the summary, gathers the queries and frees the workspace: the seconds are the call's), next to
mmhn_genotype_distribution and Engine.bench_stream in the same run; the planes' and the sweep's bytes; the masses against
genotype_distribution's mass[1]; MetastasisSummary.acquired and expected_founder_events; the ten largest residuals of
MetastasisSummary.compare; the largest deviation, in binomial standard errors, of the exact "MT" frequencies and burden
from simulate_pairs' "EM-MT" frequencies and "mt" burden.  One JSON line, progress on stderr.
    python scripts/metastasis_distribution.py [reps=3] [workspace GiB=128] [samples=1000000]"""
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.engine import Engine
from metmhn_amd.model import MetastasisSummary, MetMHN
from metmhn_amd.simulations import simulate_pairs

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ws_gib = int(sys.argv[2]) if len(sys.argv) > 2 else 128
n_sim = int(sys.argv[3]) if len(sys.argv) > 3 else 1000000
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n = mod.n
mts = np.unique(dat[np.isin(dat[:, -1], (2, 3))][:, 1:2 * n:2], axis=0).astype(np.int8)
c = min(n, int(re.search(r"LS_TILE_BITS = (\d+);", open(os.path.join(ROOT, "metmhn_amd", "csrc", "lattice.h")).read()).group(1)))
sweep_bytes = ((n - c) / 2 + 1) * 24 * 2 ** n + 48 * 2 ** n    # a tile reads (n - c) / 2 finished tiles on average and is written once; the planes are read and written once more on the way to probabilities
genodist_bytes = ((n - c) / 2 + 1) * 16 * 2 ** n + 32 * 2 ** n


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
       "distinct_mt_genotypes": int(len(mts)), "workspace_limit_gib": ws_gib, "planes_gib": round(24 * 2 ** n / 2 ** 30, 2),
       "sweep_gib": round(sweep_bytes / 2 ** 30, 1), "genotype_distribution_sweep_gib": round(genodist_bytes / 2 ** 30, 1),
       "reps": reps}
with Engine(n, workspace_bytes=ws_gib << 30) as eng:
    args = (mod.log_theta, mod.obs1, mod.obs2)
    t0 = time.perf_counter()
    eng.metastasis_distribution(*args, mts[:1])                                  # warm-up: runtime and module load
    eng.genotype_distribution(*args[:2], mts[:1])
    say(f"first calls took {time.perf_counter() - t0:.3f} s")
    (values, status, sums, _), secs = best(lambda: eng.metastasis_distribution(*args, mts, summary=True), "with the summary")
    assert (status == 0).all()
    res["with_summary_s"], res["with_summary_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    (plain, status, none, _), secs = best(lambda: eng.metastasis_distribution(*args, mts, summary=False), "without the summary")
    assert (status == 0).all() and none is None and plain.tobytes() == values.tobytes()
    res["without_summary_s"], res["without_summary_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    res["without_summary_rate_products_per_s"] = float(f"{(n << n) / min(secs):.4g}")
    res["without_summary_sweep_gb_per_s"] = round(sweep_bytes / min(secs) / 1e9, 1)
    (_, status, gsums, _), secs = best(lambda: eng.genotype_distribution(*args[:2], mts, summary=True),
                                       "genotype_distribution with the summary")
    assert (status == 0).all()
    res["genotype_distribution_with_summary_s"] = round(min(secs), 4)
    res["genotype_distribution_with_summary_all_s"] = [round(t, 4) for t in secs]
    res["with_summary_over_genotype_distribution"] = round(res["with_summary_s"] / min(secs), 3)
    res["bench_stream_copy_gb_per_s"] = round(eng.bench_stream(), 1)
summary = MetastasisSummary(*sums)
res["mass"] = [float(m) for m in summary.mass]
res["masses_against_genotype_distribution_mass1_relative"] = [float(abs(m - gsums[0][1]) / gsums[0][1]) for m in summary.mass]
res["mt_mass_share_on_observed_genotypes"] = float(values[:, 1].sum() / summary.mass[1])
res["acquired"] = [round(float(v), 5) for v in summary.acquired()]
res["expected_founder_events"] = round(summary.expected_founder_events(), 5)
res["expected_mt_events"] = round(float(np.arange(n + 1) @ summary.burden_pmf("MT")), 5)
resid = summary.compare(dat)
top = []
for stratum, r in resid.items():
    iu = np.triu_indices(n)
    for i, j, v in zip(*iu, r[iu]):
        if np.isfinite(v):
            top.append((abs(float(v)), stratum, int(i), int(j), float(v)))
top.sort(reverse=True)
res["rows_per_stratum"] = {s: int((dat[:, -1] == t).sum()) for s, t in (("EM-MT", 2), ("paired", 3))}
res["largest_residuals_stratum_i_j_value"] = [[s, i, j, round(v, 3)] for _, s, i, j, v in top[:10]]
t0 = time.perf_counter()
sim = simulate_pairs(mod.log_theta, mod.obs1, mod.obs2, n_sim, original_key=0)
res["simulate_pairs_s"], res["samples"] = round(time.perf_counter() - t0, 3), n_sim
rows = int(sim.n_class[1] + sim.n_class[2])
res["seeded_samples"] = rows
for what, exact, est in (("frequencies", summary.frequencies("MT"), sim.frequencies("EM-MT")[1::2, 1::2]),
                         ("burden", summary.burden_pmf("MT"), sim.burden_pmf("mt", "EM-MT"))):
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.abs(est - exact) / np.sqrt(exact * (1.0 - exact) / rows)
    z[~((exact > 0) & (exact < 1))] = np.nan
    res[f"MT_{what}_largest_deviation_in_binomial_standard_errors"] = float(np.nanmax(z))
res["MT_marginals_exact"] = [round(float(v), 5) for v in np.diag(summary.frequencies("MT"))]
res["MT_marginals_simulated"] = [round(float(v), 5) for v in np.diag(sim.frequencies("EM-MT")[1::2, 1::2])]
print(json.dumps(res))
