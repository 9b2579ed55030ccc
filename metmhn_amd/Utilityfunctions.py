"""Workflow callers of the hot path: the parts of metmhn/Utilityfunctions.py and
examples/analysis.py that sit directly around score / learn_mhn.  Host-side NumPy / pandas, same
names and argument meaning as the reference; the likelihood work goes to the GPU engine through
metmhn_amd.regularized_optimization.

`marg_frequs` tabulates a cohort for comparison with `simulations.simulate_summary(...).marg_frequs`, `pair_counts` for
`simulations.simulate_pairs(...).compare`.

Not mirrored (plots, Gillespie sampling, state-space helpers): out of scope, see DESIGN.md.
"""
from __future__ import annotations

import logging
from typing import Callable

import numpy as np

from .regularized_optimization import learn_mhn, score


def indep(dat) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Initial estimate of theta, d_p, d_m from marginal event counts (Utilityfunctions.py:157-183).  Rows of type 4
    (primary tumour, status unknown) count as single PT observations in the event frequencies; the seeding's rate is
    taken from the rows of known status alone."""
    dat = np.asarray(dat)
    n_unknown = int(np.sum(dat[:, -1] == 4))
    n_coupled = int(np.sum(dat[:, -1] == 3))
    n = (dat.shape[1] - 3) // 2
    n_single = dat.shape[0] - n_coupled
    theta = np.zeros((n + 1, n + 1))
    for i in range(n):
        mut_count = np.sum(dat[:, 2 * i].astype(np.int64) + dat[:, 2 * i + 1].astype(np.int64))
        if mut_count == 0:
            theta[i, i] = -1e10
        else:
            theta[i, i] = np.log(mut_count / (2 * n_coupled + n_single - mut_count + 1e-10))
    seed_count = np.sum(dat[:, -3].astype(np.int64))
    theta[n, n] = np.log(seed_count / (n_coupled + n_single - n_unknown - seed_count + 1e-10))
    return theta, np.zeros(n + 1), np.zeros(n + 1)


def cross_val(dat, penal_fun: Callable, splits, n_folds: int, m_p_corr: float, key: int = 42,
              parallel_folds: bool = False, _learn=None, _score=None):
    """n_folds cross-validation over the penalty weights `splits` (Utilityfunctions.py:186-231).

    `key` seeds a NumPy Generator for the row permutation (the reference uses jax.random.permutation;
    the fold assignment therefore differs from the reference's for the same key, the procedure does not).
    Returns a DataFrame [n_folds x len(splits)] of held-out scores.

    `parallel_folds`: the len(splits) x n_folds fits are independent, so under torch.distributed (one process
    per GPU) rank r takes the jobs `distributed.fold_jobs` assigns to it, fits them on its own GPU with the whole
    training fold (no patient sharding inside a fit) and ONE all-reduce of the score matrix at the end gives every
    rank the full table.  Without an initialised process group it is the plain loop.
    """
    import pandas as pd
    from . import distributed as D
    from . import regularized_optimization as ro
    learn = learn_mhn if _learn is None else _learn
    score_fn = score if _score is None else _score
    dat = np.asarray(dat)
    splits = np.asarray(splits, dtype=np.float64)
    rng = np.random.default_rng(key)
    shuffled = dat[rng.permutation(dat.shape[0])]
    runs = np.zeros((n_folds, splits.shape[0]))
    batch_size = int(np.ceil(dat.shape[0] / n_folds))
    rank, world = ro._rank_world() if parallel_folds else (0, 1)
    prev_shard = ro._OPTIONS["shard"]
    if world > 1:
        ro.configure(device=ro._OPTIONS["device"], dtype=ro._OPTIONS["dtype"], shard=False)
    logging.info("Crossvalidation started")
    try:
        for i, fold in D.fold_jobs(splits.size, n_folds, rank, world):
            n_dat = shuffled.shape[0]
            start = batch_size * fold
            stop = min(batch_size * (fold + 1), n_dat)
            train = np.concatenate((shuffled[:start], shuffled[stop:]))
            th0, dp0, dm0 = indep(train)
            th, dp, dm = learn(th0, dp0, dm0, train, m_p_corr, penal_fun, splits[i], opt_v=False)
            runs[fold, i] = score_fn(th, dp, dm, shuffled[start:stop], m_p_corr)
            logging.info(f"Lambda: {splits[i]} Fold: {fold} Test Score: {runs[fold, i]}")
    finally:
        if world > 1:
            ro.configure(device=ro._OPTIONS["device"], dtype=ro._OPTIONS["dtype"], shard=prev_shard)
    if world > 1:
        runs = D.allreduce_sums(runs.ravel()).reshape(runs.shape)
    return pd.DataFrame(runs, columns=splits, index=np.arange(n_folds))


def collapse_rows(dat) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Distinct rows of a cohort with their multiplicities: (rows [U, 2n+3] in order of first occurrence, counts float64
    [U], inverse int64 [P]) with rows[inverse] == dat.  `counts` as the row weights of `rows` (learn_mhn(..., weights=counts))
    gives the objective of `dat` itself; rows of type 4 collapse like any others."""
    dat = np.asarray(dat)
    if dat.ndim != 2:
        raise ValueError(f"dat must be [n_pat, 2n+3], got shape {dat.shape}")
    if dat.shape[0] == 0:
        return dat.copy(), np.zeros(0), np.zeros(0, dtype=np.int64)
    _, first, inv, cnt = np.unique(dat, axis=0, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                  # np.unique sorts the rows: back to first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return dat[first[order]].copy(), cnt[order].astype(np.float64), rank[np.asarray(inv).reshape(-1)].astype(np.int64)


class RowGroups:
    """Result of `expand_missing`: a cohort with unobserved entries as groups of complete rows.

    rows [U, 2n+3] int8: the distinct completed rows in order of first occurrence (the cohort an engine is given);
    ptr [P+1], idx [ptr[-1]]: group g = row g of the original `dat` = rows[idx[ptr[g]:ptr[g+1]]], alternative s of a row
    with the expanded entries c_0 < c_1 < ... setting entry c_b to bit b of s;
    weights [P]: the group weights (ones);
    entries: one (row of dat, column, alts) per missing entry, alts = the positions s within the row's group whose
    alternative sets the entry to 1 (empty for an entry in a column the row's type ignores, which is written as 0)."""

    def __init__(self, rows, ptr, idx, weights, entries):
        self.rows, self.ptr, self.idx, self.weights, self.entries = rows, ptr, idx, weights, entries

    @property
    def n_groups(self) -> int:
        return self.ptr.shape[0] - 1


def expand_missing(dat, missing=-1, max_alternatives: int = 1024) -> RowGroups:
    """Rows with unobserved event entries as mixtures over their completions.  An entry equal to `missing` in an event
    column means "not assayed"; the seeding, order and type columns must be known.  A row with m such entries in the columns
    its type reads - PT columns for types 0, 1 and 4, MT columns for type 2, both (independently) for type 3 - becomes the
    group of its 2^m completions; a missing entry in a column the type ignores becomes 0.  Completions shared between
    patients appear once in `rows`.  Use as learn_mhn(..., groups.rows, ..., groups=groups).  A row with more than
    `max_alternatives` completions is refused by name (the index label of a DataFrame, else the row number)."""
    names = list(dat.index) if hasattr(dat, "index") and hasattr(dat, "columns") else None     # (a DataFrame)
    arr = np.asarray(dat)
    if arr.ndim != 2 or arr.shape[1] < 5 or arr.shape[1] % 2 == 0:
        raise ValueError(f"dat must be [n_pat, 2n+3], got shape {arr.shape}")
    P, nc = arr.shape
    n = (nc - 3) // 2
    name = (lambda r: repr(names[r])) if names is not None else (lambda r: str(r))
    miss = arr == missing
    for c, what in ((2 * n, "seeding"), (nc - 2, "order"), (nc - 1, "type")):
        if miss[:, c].any():
            raise ValueError(f"expand_missing: the {what} column of row {name(int(np.argmax(miss[:, c])))} is missing; it must be known")
    blocks, ptr, entries = [], np.zeros(P + 1, dtype=np.int64), []
    for r in range(P):
        t = int(arr[r, -1])
        read = np.zeros(nc, dtype=bool)
        if t in (0, 1, 4, 3):
            read[0:2 * n:2] = True
        if t in (2, 3):
            read[1:2 * n:2] = True
        cols = np.flatnonzero(miss[r, :2 * n] & read[:2 * n])
        m = cols.shape[0]
        if m > 62 or (1 << m) > max_alternatives:
            raise ValueError(f"expand_missing: row {name(r)} has {m} unobserved entries, 2^{m} completions: more than "
                             f"max_alternatives = {max_alternatives}")
        base = np.where(miss[r], 0, arr[r]).astype(np.int8)
        s = np.arange(1 << m, dtype=np.int64)
        block = np.repeat(base[None, :], 1 << m, axis=0)
        for b, c in enumerate(cols):
            block[:, c] = (s >> b) & 1
        blocks.append(block)
        ptr[r + 1] = ptr[r] + (1 << m)
        where = {int(c): b for b, c in enumerate(cols)}
        for c in np.flatnonzero(miss[r, :2 * n]):
            b = where.get(int(c))
            entries.append((r, int(c), np.flatnonzero((s >> b) & 1) if b is not None else np.zeros(0, dtype=np.int64)))
    allrows = np.concatenate(blocks, axis=0) if blocks else np.zeros((0, nc), dtype=np.int8)
    rows, _, inverse = collapse_rows(allrows)
    return RowGroups(rows.astype(np.int8), ptr, inverse.astype(np.int64), np.ones(P), entries)


class BootstrapFits:
    """Result of `bootstrap_fits`: theta [B, N, N], d_p [B, N], d_m [B, N] of the B replicates and weights [B, U], the
    weight of every distinct row (`rows`, from collapse_rows) in every replicate."""

    def __init__(self, theta, d_p, d_m, weights, rows):
        self.theta, self.d_p, self.d_m, self.weights, self.rows = theta, d_p, d_m, weights, rows

    def _all(self):
        return {"theta": self.theta, "d_p": self.d_p, "d_m": self.d_m}

    def interval(self, level: float = 0.95):
        """Percentile interval per entry: dict of (lower, upper) for theta, d_p, d_m."""
        if not 0.0 < level < 1.0:
            raise ValueError(f"level must be in (0, 1), got {level!r}")
        q = [50.0 * (1.0 - level), 100.0 - 50.0 * (1.0 - level)]
        return {k: tuple(np.percentile(v, q, axis=0)) for k, v in self._all().items()}

    def sign_stability(self):
        """Share of the replicates in which an entry has the sign of the replicate median: dict of arrays in [0, 1]."""
        return {k: np.mean(np.sign(v) == np.sign(np.median(v, axis=0)), axis=0) for k, v in self._all().items()}


def bootstrap_fits(dat, n_boot: int, perc_met: float, penal: Callable, w_penal: float, key: int = 0, start=None,
                   opt_iter: int = 1e5, opt_ftol: float = 1e-4) -> BootstrapFits:
    """Nonparametric bootstrap of the penalised fit: `n_boot` resamples of the P rows of `dat` with replacement, each
    fitted with learn_mhn.  `dat` is collapsed once (collapse_rows) and a replicate is a vector of weights on its distinct
    rows - row b of np.random.default_rng(key).multinomial(P, np.full(P, 1 / P), size=n_boot), the draw over the ORIGINAL P
    rows, folded with np.bincount(inverse, weights=draw) - so all replicates share one engine and one plan and cost one
    weight upload each.  `start`: (theta, d_p, d_m) every replicate starts from, e.g. the full-data fit; default: indep(dat).
    Distinct rows that a replicate does not draw have weight 0 there: they do not count, but they are still solved
    (dropping them would need a new plan per replicate)."""
    dat = np.asarray(dat)
    rows, _, inverse = collapse_rows(dat)
    P, U = dat.shape[0], rows.shape[0]
    if P == 0 or n_boot < 1:
        raise ValueError("bootstrap_fits needs at least one row and one replicate")
    draws = np.random.default_rng(key).multinomial(P, np.full(P, 1 / P), size=n_boot)
    weights = np.stack([np.bincount(inverse, weights=d, minlength=U) for d in draws]).astype(np.float64)
    th0, dp0, dm0 = indep(dat) if start is None else start
    fits = [learn_mhn(th0, dp0, dm0, rows, perc_met, penal, w_penal, opt_iter=opt_iter, opt_ftol=opt_ftol, opt_v=False,
                      weights=w) for w in weights]
    return BootstrapFits(np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]), np.stack([f[2] for f in fits]),
                         weights, rows)


def create_dat(dat_sim_full, n_em: int, n_nm: int, n_c: int, n_pm: int, n_mo: int, rng) -> np.ndarray:
    """Subsample simulated patients (rows of `simulate_dat`) to a cohort with the given composition and append
    the type column (examples/recall_study.py:32-47): `n_nm` never-metastasised PT-only rows (type 0, all-zero
    rows dropped first), and of the metastasised ones `n_c` paired (3), `n_mo` MT-only (2), `n_pm` PT-only (1).
    `rng`: NumPy Generator (the reference draws the indices with jax.random.choice)."""
    sim = np.asarray(dat_sim_full)
    po = sim[sim[:, -2] == 0]
    po = po[po.sum(axis=1) != 0]
    po = po[rng.choice(po.shape[0], size=n_nm, replace=False)]
    em = sim[sim[:, -2] != 0]
    idx = rng.choice(em.shape[0], size=n_em, replace=False)
    col = lambda rows, t: np.hstack((rows, np.full((rows.shape[0], 1), t, dtype=np.int8)))
    out = np.vstack((col(po, 0), col(em[idx[:n_c]], 3), col(em[idx[n_c:n_c + n_mo]], 2), col(em[idx[n_c + n_mo:]], 1)))
    return out.astype(np.int8)


def categorize(x) -> int:
    """Type of a datapoint from its annotation (Utilityfunctions.py:98-113)."""
    import pandas as pd
    if x["paired"] == 0:
        return {"absent": 0, "present": 1, "isMetastasis": 2}.get(x["metaStatus"], pd.NA if x["metaStatus"] == "unknown" else -1)
    if x["paired"] == 1:
        return 3
    return pd.NA


def load_cohort(events_csv: str, annot_csv: str, muts: list[str] | None = None, keep_unknown: bool = False):
    """Events CSV + annotation CSV -> (dat int8 [n_pat, 2n+3], event names); examples/analysis.py:49-83.

    `muts`: the P./M. event columns to keep (pairs, PT column first); default: every event column.
    `keep_unknown`: the unpaired primary tumours whose metaStatus is "unknown" - dropped by the reference and by default
    here - are kept as rows of type 4 (seeding 0, MT columns 0), which the objective scores as the sum over both
    statuses.  The order entry points (MetMHN.order_*, likeliest_order) do not take them: filter them out there.
    """
    import pandas as pd
    annot = pd.read_csv(annot_csv)
    mut = pd.read_csv(events_csv)
    mut.rename(columns={"Unnamed: 0": "patientID"}, inplace=True)
    d = pd.merge(mut, annot.loc[:, ["patientID", "metaStatus"]], on=["patientID", "patientID"])
    if muts is None:
        muts = list(d.columns[1:-4])
    d["type"] = d.apply(categorize, axis=1)
    if keep_unknown:
        unknown = (d["paired"] == 0) & (d["metaStatus"] == "unknown")
        d["type"] = d["type"].astype(object).where(~unknown, 4)
        d.loc[unknown, [c for c in muts if c.startswith("M.")]] = 0
    d["Seeding"] = d["type"].apply(lambda x: pd.NA if pd.isna(x) else 0 if x in (0, 4) else 1)
    d["M.AgeAtSeqRep"] = pd.to_numeric(d["M.AgeAtSeqRep"], errors="coerce")
    d["P.AgeAtSeqRep"] = pd.to_numeric(d["P.AgeAtSeqRep"], errors="coerce")
    d["diag_order"] = d["M.AgeAtSeqRep"] - d["P.AgeAtSeqRep"]
    d["diag_order"] = d["diag_order"].apply(lambda x: pd.NA if pd.isna(x) else 2 if x < 0 else 1 if x > 0 else 0)
    d["diag_order"] = d["diag_order"].astype(pd.Int64Dtype())
    cleaned = d.loc[~pd.isna(d["type"]), muts + ["Seeding", "diag_order", "type"]]
    dat = cleaned.to_numpy(dtype=np.int8, na_value=-99)
    events = [c.split(".")[1] for c in muts[::2]] + ["Seeding"]
    return dat, events


def marg_frequs(dat, events: list):
    """Marginal frequencies of every event per stratum of a cohort `dat` [n_pat, 2n+3] (Utilityfunctions.py:116-155):
    coupled rows (type 3) split into PT-private / MT-private / shared, NM (type 0) and EM-PT (type 1) PT bits,
    EM-MT (type 2) MT bits; the seeding column from the seeding flag.  DataFrame [n+1 events x 6], rounded to two
    decimals, columns labelled with the stratum sizes.  The reference reads the sizes by position from np.unique
    and is right only when all four types occur; a cohort without one of them raises ValueError here.  Rows of type 4
    (status unknown) belong to none of these strata and are ignored, here and in `pair_counts`."""
    import pandas as pd
    dat = np.asarray(dat)
    dat = dat[dat[:, -1] != 4]
    n_mut = (dat.shape[1] - 3) // 2
    types = dat[:, -1]
    if set(np.unique(types).tolist()) != {0, 1, 2, 3}:
        raise ValueError(f"marg_frequs needs rows of all four types 0-3, got types {sorted(set(np.unique(types).tolist()))}")
    sizes = [int(np.count_nonzero(types == t)) for t in range(4)]
    coupled = dat[types == 3].astype(np.int64)
    code = np.hstack((coupled[:, 0:2 * n_mut:2] + 2 * coupled[:, 1:2 * n_mut:2], coupled[:, 2 * n_mut:2 * n_mut + 1]))
    counts = np.zeros((6, n_mut + 1))
    for j in range(1, 4):                                   # 1 PT-private, 2 MT-private, 3 shared
        counts[j - 1] = np.count_nonzero(code == j, axis=0) / sizes[3]
    col = lambda t, c: np.sum(dat[types == t][:, c], axis=0)
    counts[3] = col(0, np.arange(0, 2 * n_mut + 1, 2)) / sizes[0]
    counts[4] = col(1, np.arange(0, 2 * n_mut + 1, 2)) / sizes[1]
    counts[5] = np.append(col(2, np.arange(1, 2 * n_mut, 2)), col(2, 2 * n_mut)) / sizes[2]
    labels = [[f"Coupled ({sizes[3]})"] * 3 + [f"NM ({sizes[0]})", f"EM-PT ({sizes[1]})", f"EM-MT ({sizes[2]})"],
              ["PT-Private", "MT-Private", "Shared"] + ["Present"] * 3]
    inds = pd.MultiIndex.from_tuples(list(zip(*labels)))
    return pd.DataFrame(np.around(counts, 2), columns=events, index=inds).T


def pair_counts(dat) -> tuple[np.ndarray, np.ndarray]:
    """Observed co-occurrence counts of a cohort `dat` [n_pat, 2n+3] per row type 0 - 3 (NM, EM-PT, EM-MT, paired):
    (n_type int64 [4], pairs int64 [4, 2n, 2n]) with pairs[t] = G.T @ G over the genotype columns [PT_0, MT_0, ...] of
    the rows of type t - the observed side of `simulations.PairSummary.compare`.  Rows of type 4 are ignored."""
    dat = np.asarray(dat)
    B = dat.shape[1] - 3
    n_type = np.zeros(4, dtype=np.int64)
    pairs = np.zeros((4, B, B), dtype=np.int64)
    for t in range(4):
        g = dat[dat[:, -1] == t][:, :B].astype(np.int64)
        n_type[t] = g.shape[0]
        pairs[t] = g.T @ g
    return n_type, pairs


def save_params(path: str, theta, d_p, d_m, events: list[str]):
    """Parameter CSV with rows d_p, d_m, theta (examples/analysis.py:115-119)."""
    import pandas as pd
    tab = np.vstack((np.asarray(d_p).reshape(1, -1), np.asarray(d_m).reshape(1, -1), np.asarray(theta)))
    pd.DataFrame(tab, columns=events).to_csv(path)
