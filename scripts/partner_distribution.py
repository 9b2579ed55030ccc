#!/usr/bin/env python3
"""The genotype distribution of the tumour that was not sequenced, of the 28-event LUAD model (tests/golden/luad28.npz, its
fitted parameters) on the device: best-of-`reps` seconds per call and per query of mmhn_partner_distributions with
summaries, given="PT" on the distinct PT genotypes of the type-1 rows and given="MT" on the distinct MT genotypes of the
type-2 rows (a call allocates its workspace once, then runs a backward pass, a seeding pass and one full sweep of one plane
per query), next to mmhn_metastasis_distribution without summary in the same run; the worst relative difference of
at_target on the 453 paired rows, as targets of their own PT and of their own MT, against exp of the engine's own per-row
lp; the mutations the metastasis most often gained and the primary tumour most often lacks, averaged over the rows.  One
JSON line, progress on stderr.
    python scripts/partner_distribution.py [reps=3] [workspace GiB=128] [queries per given=0: all]"""
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
cap = int(sys.argv[3]) if len(sys.argv) > 3 else 0
dat = g["dat"]
mod = MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
n = mod.n
typ = dat[:, -1]


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


def distinct(rows):
    """The distinct genotypes of `rows`, most frequent first (so a capped run keeps the common ones), and their counts."""
    uniq, counts = np.unique(rows, axis=0, return_counts=True)
    order = np.argsort(-counts, kind="stable")
    return uniq[order].astype(np.int8), counts[order]


res = {"cohort": "luad28", "point": "fit", "n_mut": n, "genotypes": 1 << n, "workspace_limit_gib": ws_gib,
       "planes_gib": round(16 * 2 ** n / 2 ** 30, 2), "reps": reps}
args = (mod.log_theta, mod.obs1, mod.obs2)
with Engine(n, workspace_bytes=ws_gib << 30) as eng:
    t0 = time.perf_counter()
    eng.partner_distributions(*args, np.zeros((1, n), dtype=np.int8))            # warm-up: runtime and module load
    eng.metastasis_distribution(*args, np.zeros((1, n), dtype=np.int8), summary=False)
    say(f"first calls took {time.perf_counter() - t0:.3f} s")
    for given, rows in (("PT", dat[typ == 1][:, 0:2 * n:2]), ("MT", dat[typ == 2][:, 1:2 * n:2])):
        G, counts = distinct(rows)
        res[f"{given}_rows"], res[f"{given}_distinct_genotypes"] = int(len(rows)), int(len(G))
        if cap:
            G, counts = G[:cap], counts[:cap]
        (values, status, sums, _), secs = best(lambda: eng.partner_distributions(*args, G, given), f"given {given}, {len(G)} queries")
        assert (status == 0).all()
        res[f"{given}_queries"], res[f"{given}_rows_covered"] = int(len(G)), int(counts.sum())
        res[f"{given}_call_s"], res[f"{given}_call_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
        res[f"{given}_per_query_ms"] = round(1e3 * min(secs) / len(G), 3)
        held = G.astype(bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            freq = np.diagonal(sums[1][:, 1], axis1=1, axis2=2) / sums[0][:, 1, None]          # P(partner holds j | query)
            burden = (sums[2][:, 1] / sums[0][:, 1, None]) @ np.arange(n + 1)
            founder = (sums[2][:, 0] / sums[0][:, 0, None]) @ np.arange(n + 1)
        w = counts / counts.sum()
        gained = (w[:, None] * np.where(held, 0.0, freq)).sum(axis=0)            # per row: the partner holds j and the query does not
        lost = (w[:, None] * np.where(held, 1.0 - freq, 0.0)).sum(axis=0)
        res[f"{given}_most_gained_event_probability"] = [[int(j), round(float(gained[j]), 4)] for j in np.argsort(-gained)[:5]]
        res[f"{given}_most_lost_event_probability"] = [[int(j), round(float(lost[j]), 4)] for j in np.argsort(-lost)[:5]]
        res[f"{given}_mean_events_query_partner_founder"] = [round(float(w @ G.sum(axis=1)), 3), round(float(w @ burden), 3),
                                                             round(float(w @ founder), 3)]
        one = eng.genotype_distribution(*args[:2], G, summary=False)[0][:, 1] if given == "PT" else \
            eng.metastasis_distribution(*args, G, summary=False)[0][:, 1]
        res[f"{given}_mass_against_one_tumour_sweep_relative"] = float(np.max(np.abs(values[:, 0] - one) / one))
    some = np.zeros((1, n), dtype=np.int8)
    (_, status, _, _), secs = best(lambda: eng.metastasis_distribution(*args, some, summary=False),
                                   "metastasis_distribution without the summary")
    res["metastasis_distribution_without_summary_s"] = round(min(secs), 4)
    (_, status, _, _), secs = best(lambda: eng.partner_distributions(*args, some, summary=False), "one query without summaries")
    res["one_query_call_s"], res["one_query_call_all_s"] = round(min(secs), 4), [round(t, 4) for t in secs]
    res["bench_stream_copy_gb_per_s"] = round(eng.bench_stream(), 1)
    pairs = dat[typ == 3].astype(np.int8).copy()
    pairs[:, -2] = 0                                                             # the order of observation unknown
    PT, MT = pairs[:, 0:2 * n:2], pairs[:, 1:2 * n:2]
    t0 = time.perf_counter()
    at_pt = eng.partner_distributions(*args, PT, "PT", targets=MT, summary=False)[0][:, 2]
    at_mt = eng.partner_distributions(*args, MT, "MT", targets=PT, summary=False)[0][:, 2]
    res["paired_rows"], res["paired_rows_both_given_s"] = int(len(pairs)), round(time.perf_counter() - t0, 3)
    eng.set_cohort(pairs)
    lp = eng.patient_grads(*args, with_grad=False)
ref = np.exp(lp)
res["at_target_against_exp_lp_relative"] = {"PT": float(np.max(np.abs(at_pt - ref) / ref)), "MT": float(np.max(np.abs(at_mt - ref) / ref))}
res["at_target_PT_against_MT_relative"] = float(np.max(np.abs(at_pt - at_mt) / at_mt))
print(json.dumps(res))
