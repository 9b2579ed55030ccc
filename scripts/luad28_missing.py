#!/usr/bin/env python3
"""Unobserved entries on the 28-event LUAD cohort (tests/golden/luad28.npz; perc_met and lambda of the LUAD fixtures): one
JSON line.  Entries are masked with a seeded "panel" pattern (panel_mask): a fixed set of 3 and of 6 genes is unassayed in a
seeded 30 % of the samples, the PT and the MT sample of a paired row drawn independently.
  * the distinct completed rows (Utilityfunctions.expand_missing) against the sum of 2^m over the rows;
  * ms per score_and_grad_reg evaluation at the published parameters with groups (best of 3), and of the same expanded rows
    with weights of one on the path without groups in the same run: the difference is what the mixing costs;
  * for the 3-gene mask the fit started at indep of the unmasked data with (a) groups, (b) the masked rows dropped, (c) missing
    coded as 0: the log-likelihood of the unmasked cohort at the fit and the largest parameter difference to the fit of the
    unmasked cohort.
    python scripts/luad28_missing.py"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GENES3 = (0, 5, 11)
GENES6 = (0, 3, 5, 11, 17, 23)
MISSING = -1


def panel_mask(dat, genes, frac=0.3, seed=0, missing=MISSING):
    """(masked copy of dat, rows with a masked entry).  One uniform draw per row and sample from default_rng(seed): the PT
    sample of rows of types 0, 1, 3, 4 and the MT sample of rows of type 2 are unassayed for `genes` when the first draw is
    below frac, the MT sample of a paired row (type 3) when the second is."""
    dat = np.asarray(dat)
    out = dat.astype(np.int8, copy=True)
    rng = np.random.default_rng(seed)
    first, second = rng.random(dat.shape[0]) < frac, rng.random(dat.shape[0]) < frac
    typ = dat[:, -1]
    pt_cols, mt_cols = [2 * j for j in genes], [2 * j + 1 for j in genes]
    pt_rows = first & np.isin(typ, (0, 1, 3, 4))
    mt_rows = (first & (typ == 2)) | (second & (typ == 3))
    out[np.ix_(pt_rows, pt_cols)] = missing
    out[np.ix_(mt_rows, mt_cols)] = missing
    return out, pt_rows | mt_rows


def main():
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import Utilityfunctions as UF
    g = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))
    pm, lam = float(g["perc_met"]), float(g["lam"])
    pub = np.concatenate((g["fit_theta"].flatten(), g["fit_dp"], g["fit_dm"]))
    dat = np.ascontiguousarray(g["dat"])

    def eval_ms(rows, reps, **kw):
        for _ in range(2):
            out = ro.score_and_grad_reg(pub, rows, pm, ro.symmetric_penal, lam, **kw)
        best = np.inf
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(reps):
                out = ro.score_and_grad_reg(pub, rows, pm, ro.symmetric_penal, lam, **kw)
            best = min(best, (time.perf_counter() - t0) / reps * 1e3)
        return best, out

    out = {}
    groups3 = masked3 = hit3 = None
    for name, genes in (("mask3", GENES3), ("mask6", GENES6)):
        masked, hit = panel_mask(dat, genes)
        groups = UF.expand_missing(masked, max_alternatives=1 << (2 * len(genes)))
        total = int(groups.ptr[-1])
        reps = 20 if total < 50000 else 5
        ms_groups, (v, _) = eval_ms(groups.rows, reps, groups=groups)
        ms_rows, _ = eval_ms(groups.rows, reps, weights=np.ones(groups.rows.shape[0]))
        out[name] = {"genes": list(genes), "masked_rows": int(hit.sum()), "sum_2m": total, "distinct_rows": int(groups.rows.shape[0]),
                     "ms_groups": round(ms_groups, 3), "ms_same_rows_weights_one": round(ms_rows, 3), "objective": float(v)}
        ro.invalidate()
        if name == "mask3":
            groups3, masked3, hit3 = groups, masked, hit
    th0, dp0, dm0 = UF.indep(dat)
    fit = lambda rows, **kw: ro.learn_mhn(th0, dp0, dm0, rows, pm, ro.symmetric_penal, lam, opt_v=False, **kw)
    t0 = time.perf_counter()
    full = fit(dat)
    fits = {"groups": fit(groups3.rows, groups=groups3), "dropped": fit(np.ascontiguousarray(dat[~hit3])),
            "coded_0": fit(np.where(masked3 == MISSING, 0, masked3).astype(np.int8))}
    ll = lambda f: float(ro.score(f[0], f[1], f[2], dat, pm))
    out["fits_mask3"] = {"loglik_unmasked_fit": ll(full), "seconds": round(time.perf_counter() - t0, 1)}
    for k, f in fits.items():
        out["fits_mask3"][k] = {"loglik_on_unmasked": ll(f),
                                "max_param_diff": float(max(np.abs(a - b).max() for a, b in zip(f, full)))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
