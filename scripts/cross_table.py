#!/usr/bin/env python3
"""The exact PT x MT co-occurrence and joint burden tables of the 28-event LUAD model (tests/golden/luad28.npz, its fitted
parameters) on the device: best-of-`reps` seconds per call of mmhn_cross_table with and without the burden, next to
mmhn_genotype_distribution with its summary in the same run; the sweeps of the call and the bytes they move by the
algorithm (a backward sweep writes its four planes once and pulls them along the free high bits, half of the n - c on
average; a fold reads Z and 4 + 4 planes); the ten largest standardised residuals of the 453 paired rows against the exact
table (PairedSummary.compare); the largest deviation of the PT x MT block from simulate_pairs at 10^6 samples in binomial
standard errors.  One JSON line, progress on stderr.
    python scripts/cross_table.py [reps=3] [workspace GiB=160] [samples=1000000]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from metmhn_amd.engine import Engine
from metmhn_amd.model import MetMHN
from metmhn_amd.results import CrossSummary, GenotypeSummary, MetastasisSummary, PairedSummary
from metmhn_amd.simulations import simulate_pairs

g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ws_gib = int(sys.argv[2]) if len(sys.argv) > 2 else 160
samples = int(sys.argv[3]) if len(sys.argv) > 3 else 10 ** 6
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n, c = mod.n, 10


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


def plan(features, planes_fit):
    """(PT blocks held, backward sweeps, folds) of a call whose workspace holds planes_fit planes."""
    fb = -(-features // 4)
    held = min(fb, (planes_fit - 5) // 4)
    fixed = fb if held == fb else held - 1
    return held, fb + fixed + (fb - fixed) * fb, fb * fb


res = {"cohort": "luad28", "point": "fit", "n_mut": n, "genotypes": 1 << n, "workspace_limit_gib": ws_gib, "reps": reps}
args = (mod.log_theta, mod.obs1, mod.obs2)
none = np.zeros((0, n), dtype=np.int8)
plane = 8 << n
with Engine(n, workspace_bytes=ws_gib << 30) as eng:
    t0 = time.perf_counter()
    eng.cross_table(*args, burden=False)                                           # warm-up: runtime and module load
    eng.genotype_distribution(*args[:2], none)
    say(f"first calls took {time.perf_counter() - t0:.3f} s")
    for key, burden, features in (("with_burden", True, 2 * n + 1), ("genes_only", False, n)):
        out, secs = best(lambda: eng.cross_table(*args, burden=burden), f"cross_table, burden={burden}")
        held, sweeps, folds = plan(features, (ws_gib << 30) // plane)
        moved = sweeps * 4 * plane * (1 + (n - c) / 2) + folds * 9 * plane + plane * (1 + (n - c) / 2) + 2 * plane
        res[key] = {"call_s": round(min(secs), 4), "call_all_s": [round(t, 4) for t in secs], "pt_blocks_held": held,
                    "planes": 5 + 4 * held, "backward_sweeps": sweeps, "forward_sweeps": 1, "folds": folds,
                    "algorithmic_gib_moved": round(moved / 2 ** 30, 1),
                    "algorithmic_gb_per_s": round(moved / min(secs) / 1e9, 1)}
        if burden:
            cross = CrossSummary(*out)
        else:
            res["gene_outputs_same_bytes"] = all(np.asarray(a).tobytes() == np.asarray(b).tobytes()
                                                 for a, b in zip(out[:4], (cross.mass, cross.pt, cross.mt, cross.cross)))
    (_, _, gsum, _), secs = best(lambda: eng.genotype_distribution(*args[:2], none), "genotype_distribution with its summary")
    res["genotype_distribution_s"] = round(min(secs), 4)
    _, _, msum, _ = eng.metastasis_distribution(*args, none)
    res["bench_stream_copy_gb_per_s"] = round(eng.bench_stream(), 1)
summary = PairedSummary(GenotypeSummary(*gsum), MetastasisSummary(*msum), cross)
res["p_seeded"], res["expected_shared_events"] = round(cross.mass, 6), round(cross.expected_shared(), 4)
pmf = cross.burden_pmf()
res["expected_events_pt_mt"] = [round(float(np.arange(n + 1) @ pmf.sum(axis=1)), 4), round(float(np.arange(n + 1) @ pmf.sum(axis=0)), 4)]
res["mass_against_one_tumour_sweeps_relative"] = float(max(abs(cross.mass - gsum[0][1]) / gsum[0][1], abs(cross.mass - msum[0][1]) / msum[0][1]))
r = summary.compare(dat)["paired"]
name = lambda k: ("PT" if k % 2 == 0 else "MT") + str(k // 2)
iu = np.triu_indices(2 * n)
order = np.argsort(-np.nan_to_num(np.abs(r[iu])))[:10]
res["paired_rows"] = int((dat[:, -1] == 3).sum())
res["largest_residuals"] = [[name(int(iu[0][k])), name(int(iu[1][k])), round(float(r[iu][k]), 2)] for k in order]
t0 = time.perf_counter()
sim = simulate_pairs(*args, samples, original_key=5)
rows = int(sim.n_class[1] + sim.n_class[2])
exact, est = cross.frequencies(), sim.frequencies("paired")[0::2, 1::2]
inside = (exact > 0) & (exact < 1)
z = np.abs(est - exact)[inside] / np.sqrt(exact[inside] * (1 - exact[inside]) / rows)
res["simulate_pairs"] = {"samples": samples, "seeded": rows, "s": round(time.perf_counter() - t0, 3), "entries": int(inside.sum()),
                         "worst_deviation_standard_errors": round(float(z.max()), 3)}
print(json.dumps(res))
