#!/usr/bin/env python3
"""Host values of the order family on rows of 15 - 21 slots, the rows of the 1 024-thread kernels:

    python tests/tools/make_golden_orders_big.py [--workers 8]

CPU only: the project's own host code (metmhn_amd/model.py) with the one device call, the restricted joint diagonal,
taken from the oracle (order_common.OracleDiag, as the `host_only` fixture of the tests does).  Needs no GPU and nothing
outside this repository.  The host code takes seconds to minutes per row at these sizes, too slow for a live test; its
values are the definition the kernels follow (pinned to brute-force enumeration at k <= 7 by the CPU tests).

Rows.
  n9   (order_common.model(9, seed=31)): the paired rows of order_common.large_rows(9) with k >= 15 - k = 15, 16, 17, the
       k = 17 row of joint events only, the k = 15 row with two events in neither class's low bits -, each under the
       diagnosis orders 0, 1, 2 and -99.
  n16  (model(16, seed=32)): the one-tumour rows of large_rows(16) with k >= 15 (all three types), a paired row without a
       joint event (k = 15, PT and MT slots interleaved) and one whose PT slots all lie below its MT slots (k = 16, one
       joint event: the highest PT slot and the lowest MT slot), each under the four diagnosis orders.
  luad (tests/golden/luad28.npz at its "fit" point): the one type-1 row with k >= 15, the first two of the six type-2 rows
       with k >= 15, per k = 18, 19, 20 the first two paired rows in cohort order, the k = 21 row; luad_index holds their
       indices in the cohort.

Written to tests/golden/orders_big.npz - or, if that file would be larger than the largest fixture there is
(primitives.npz), to orders_big.npz (rows and models) and one orders_big_<entry>.npz per entry point; order_common.big_rows
reads either.  Per model name m (order_common.BIG_MODELS):
  m_n, m_seed (n9, n16) or m_prefix, m_index (luad), m_dat [R, 2n+3]
  per entry e of post, prec, pos, time, snap: m_e_le [R] (log_evidence), m_e_val (the rows' blocks of doubles over their own
      codes, one behind the other: order_common.big_pack), m_e_off [R+1]
  m_snap_state (the chosen snapshot over the codes of every paired row, int8), m_snap_first [R] (-1: no first observation),
      m_snap_gap [R] ((best - second best mass) / best of the snapshots; NaN: no first observation)
  n9, n16 only, sample_order with n_samples = 64, key = KEY + n, first = FIRST, row = the row's index in m_dat:
      m_samp_le [R], m_samp_orders (int8, 64 x k per row), m_samp_log_prob, m_samp_margin [R, 64], m_samp_row [R]
rows: the number of rows of the whole fixture.  A second run writes the same bytes (fixed archive dates, sorted keys).
"""
import argparse
import io
import os
import sys
import time
import warnings
import zipfile
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import metmhn_amd.model as model_mod                                                            # noqa: E402
import order_common as oc                                                                       # noqa: E402
from test_order_samples import MARGIN, MAX_EXCLUDED                                             # noqa: E402

DIAG_ORDERS = (0, 1, 2, -99)
_state = {}


def rows_of(name, n):
    """(dat, index): the fixture's rows of one model, and their indices in the LUAD-28 cohort (None for the synthetic ones)."""
    if name == "luad":
        dat = np.load(os.path.join(GOLDEN, "luad28.npz"))["dat"]
        k, typ = dat[:, :-2].astype(int).sum(1), dat[:, -1]
        one, met = np.flatnonzero((k >= 15) & (typ == 1)), np.flatnonzero((k >= 15) & (typ == 2))
        assert len(one) == 1 and len(met) == 6 and not ((k >= 15) & (typ == 0)).any()
        index = list(one) + list(met[:2])
        for kk in (18, 19, 20):
            both = np.flatnonzero((k == kk) & (typ == 3))
            assert len(both) >= 2
            index += list(both[:2])
        top = np.flatnonzero(k == 21)
        assert len(top) == 1 and typ[top[0]] == 3 and k.max() == 21
        index = np.array(index + list(top))
        return dat[index], index
    base = oc.large_rows(n)
    k = base[:, :-2].astype(int).sum(1)
    rows = []
    for r in base[k >= 15]:
        for d in DIAG_ORDERS if r[-1] == 3 else (r[-2],):
            rows.append(r.copy())
            rows[-1][-2] = d
    if n == 16:
        for d in DIAG_ORDERS:
            rows.append(oc.paired(n, range(0, 14, 2), range(1, 14, 2), d))      # k = 15, no joint event
        for d in DIAG_ORDERS:
            rows.append(oc.paired(n, range(8), range(7, 14), d))                # k = 16, PT slots 0 ... 14, MT slots 15 ... 27
    return np.array(rows), None


def models():
    """{name: (MetMHN, n, dat, index)}, built once per process."""
    if not _state:
        model_mod._kronvec = oc.OracleDiag                   # the host_only fixture's replacement
        warnings.simplefilter("ignore", DeprecationWarning)
        for name, n, seed in oc.BIG_MODELS:
            if seed is None:
                g = np.load(os.path.join(GOLDEN, "luad28.npz"))
                mod = oc.MetMHN(g["fit_theta"], g["fit_dp"], g["fit_dm"])
            else:
                mod = oc.model(n, seed=seed)
            _state[name] = (mod, n) + rows_of(name, n)
    return _state


def snapshot_with_gap(mod, args):
    """order_snapshot, and (best - second best) / best of the masses it chose from: the passes of the one call are kept and
    _snapshot_paired's masses formed once more."""
    kept = {}
    passes = mod._paired_passes

    def once(state, first_obs):
        kept["passes"] = passes(state, first_obs)
        return kept["passes"]
    mod._paired_passes = once
    try:
        res = mod.order_snapshot(*args)
    finally:
        del mod._paired_passes
    if res.map_first < 0:
        return res, np.nan
    T, F, Z, B = kept["passes"]
    k = T.k
    top, full = 1 << (k - 1), (1 << k) - 1
    best, second = (-1.0, -1, 0), -1.0
    for r, (possible, own, o, den, comp) in enumerate(((T.pt_first, T.pt_mask, T.o1, getattr(T, "den_mt", None), 1),
                                                       (T.mt_first, T.mt_mask, T.o2, getattr(T, "den_pt", None), 2))):
        if not possible:
            continue
        for x in range(top, full + 1):
            if x & own == own:
                s = F[x][0] * o[x] / den[x] * B[x][comp]
                if s > best[0]:
                    best, second = (s, r, x), best[0]
                elif s > second:
                    second = s
    assert best[1] == res.map_first and min(best[0] / Z, 1.0) == res.map_prob
    assert [best[2] >> d & 1 for d in range(k)] == res.map_state[T.slots].tolist()
    return res, (best[0] - max(second, 0.0)) / best[0]


def task(job):
    name, i, entry = job
    mod, n, dat, _ = models()[name]
    w = oc.Row(dat[i], n)
    args = mod._row_args(dat, i)
    t0 = time.perf_counter()
    if entry == "sample_orders":
        s = mod.sample_order(*args, n_samples=oc.BIG_SAMPLES, key=oc.KEY + n, first=oc.FIRST, row=i)
        k = len(w.codes)
        assert np.all(s.orders[:, k:] == -1) and np.all(s.orders[:, :k] >= 0)
        out = {"le": s.log_evidence, "orders": s.orders[:, :k].copy(), "log_prob": s.log_prob, "margin": s.margin, "row": i}
    else:
        single = oc.BIG_ENTRIES[entry][1]
        res, gap = snapshot_with_gap(mod, args) if entry == "order_snapshots" else (getattr(mod, single)(*args), None)
        block = oc.big_pack(entry, w, res)
        out = {"le": res.log_evidence, "val": block}
        extra = ()
        if entry == "order_snapshots":
            out["state"] = np.asarray(res.map_state)[w.codes].astype(np.int8) if w.typ == 3 else np.zeros(0, dtype=np.int8)
            out["first"], out["gap"] = int(res.map_first), gap
            extra = (out["state"], out["first"])
        # the block and the row's structure give the whole result back
        back = oc.big_unpack(entry, w, block, *extra)
        for f in oc.BIG_ENTRIES[entry][3]:
            assert np.array_equal(back[f], np.asarray(getattr(res, f)), equal_nan=back[f].dtype.kind == "f"), (name, i, entry, f)
    return job, out, time.perf_counter() - t0, len(w.codes)


def save(path, arrays):
    """An .npz whose bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            z.writestr(info, buf.getvalue())
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workers", type=int, default=8)
    a = ap.parse_args()
    assert 1 <= a.workers <= 8
    mods = models()
    entries = list(oc.BIG_ENTRIES) + ["sample_orders"]
    jobs = []
    for name, n, seed in oc.BIG_MODELS:
        dat = mods[name][2]
        k = dat[:, :-2].astype(int).sum(1)
        assert k.min() >= 15
        for i in range(len(dat)):
            for entry in entries:
                if entry != "sample_orders" or seed is not None:
                    jobs.append((name, i, entry, int(k[i]) + (2 if entry == "order_precedences" else 0) + (n == 28)))
    jobs.sort(key=lambda j: -j[3])                                       # the long ones first
    t0 = time.perf_counter()
    done, seconds = {}, {}
    with Pool(a.workers) as pool:
        for job, out, sec, k in pool.imap_unordered(task, [j[:3] for j in jobs]):
            done[job] = out
            s = seconds.setdefault((job[2], k), [0, 0.0])
            s[0], s[1] = s[0] + 1, s[1] + sec
    wall = time.perf_counter() - t0
    for (entry, k), (count, sec) in sorted(seconds.items()):
        print(f"{entry:18s} k = {k:2d}: {count:2d} rows, {sec:8.1f} s in all, {sec / count:7.2f} s per row")
    print(f"{len(jobs)} host calls in {wall:.0f} s on {a.workers} workers")

    common, per_entry = {"rows": np.int64(sum(len(m[2]) for m in mods.values()))}, {e: {} for e in entries}
    excluded = total = 0
    for name, n, seed in oc.BIG_MODELS:
        mod, _, dat, index = mods[name]
        common[name + "_n"], common[name + "_dat"] = np.int64(n), dat
        if seed is None:
            common[name + "_prefix"], common[name + "_index"] = np.array("fit"), index.astype(np.int64)
        else:
            common[name + "_seed"] = np.int64(seed)
        R = range(len(dat))
        for entry, (key, _, _, _) in oc.BIG_ENTRIES.items():
            out = [done[name, i, entry] for i in R]
            d = per_entry[entry]
            d[f"{name}_{key}_le"] = np.array([o["le"] for o in out])
            d[f"{name}_{key}_val"] = np.concatenate([o["val"] for o in out])
            d[f"{name}_{key}_off"] = np.concatenate(([0], np.cumsum([len(o["val"]) for o in out]))).astype(np.int64)
            if entry == "order_snapshots":
                d[f"{name}_snap_state"] = np.concatenate([o["state"] for o in out])
                d[f"{name}_snap_first"] = np.array([o["first"] for o in out], dtype=np.int32)
                d[f"{name}_snap_gap"] = np.array([o["gap"] for o in out], dtype=np.float64)
                tied = int((d[f"{name}_snap_gap"] <= oc.BIG_GAP).sum())
                print(f"{name}: smallest gap between the two best snapshots {np.nanmin(d[f'{name}_snap_gap']):.3e}, {tied} tied")
        if seed is not None:
            out = [done[name, i, "sample_orders"] for i in R]
            d = per_entry["sample_orders"]
            d[f"{name}_samp_le"] = np.array([o["le"] for o in out])
            d[f"{name}_samp_orders"] = np.concatenate([o["orders"].ravel() for o in out])
            d[f"{name}_samp_log_prob"] = np.array([o["log_prob"] for o in out])
            d[f"{name}_samp_margin"] = np.array([o["margin"] for o in out])
            d[f"{name}_samp_row"] = np.array([o["row"] for o in out], dtype=np.int64)
            excluded += int((d[f"{name}_samp_margin"] < MARGIN).sum())
            total += d[f"{name}_samp_margin"].size
    print(f"samples: {excluded} of {total} under the margin {MARGIN:g}")
    assert excluded <= MAX_EXCLUDED * total, "change the key, not the cap"

    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("orders_big"))
    for f in os.listdir(GOLDEN):
        if f.startswith("orders_big"):
            os.remove(os.path.join(GOLDEN, f))
    whole = dict(common)
    for d in per_entry.values():
        whole.update(d)
    path = os.path.join(GOLDEN, "orders_big.npz")
    size = save(path, whole)
    written = {path: size}
    if size > limit:
        written = {path: save(path, common)}
        for entry, d in per_entry.items():
            p = os.path.join(GOLDEN, f"orders_big_{oc.BIG_ENTRIES.get(entry, ('samp',))[0]}.npz")
            written[p] = save(p, d)
    for p, size in written.items():
        print(f"{os.path.relpath(p, ROOT)}: {size} bytes (limit {limit})")
        assert size <= limit, p


if __name__ == "__main__":
    main()
