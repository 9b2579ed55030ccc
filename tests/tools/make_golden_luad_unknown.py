#!/usr/bin/env python3
"""The LUAD primary tumours of unknown metastatic status as cohort rows: tests/golden/luad28_unknown_rows.npy.

    python tests/tools/make_golden_luad_unknown.py REFERENCE_CHECKOUT

REFERENCE_CHECKOUT holds the reference's data/luad/G14_LUAD_Events.csv and G14_LUAD_sampleSelection.csv.  The file is data
only: int8 [n_unknown, 59], the rows of type 4 that `Utilityfunctions.load_cohort(..., keep_unknown=True)` yields for the
28-event selection of tests/golden/luad28.npz (every event column, examples/analysis.py:55), in the order of the CSV.  The
rows of known status of the same call must be the `dat` of luad28.npz: checked before anything is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)


def main(ref):
    from metmhn_amd import Utilityfunctions as U
    base = os.path.join(ref, "data", "luad")
    csvs = (os.path.join(base, "G14_LUAD_Events.csv"), os.path.join(base, "G14_LUAD_sampleSelection.csv"))
    known, events = U.load_cohort(*csvs)
    both, events2 = U.load_cohort(*csvs, keep_unknown=True)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "luad28.npz"))["dat"]
    assert events == events2 and known.shape == gold.shape and np.array_equal(known, gold), "the known rows are not luad28.npz's"
    unknown = both[:, -1] == 4
    assert np.array_equal(both[~unknown], known), "keep_unknown changed a row of known status"
    rows = np.ascontiguousarray(both[unknown], dtype=np.int8)
    n = (rows.shape[1] - 3) // 2
    assert rows[:, 1:2 * n:2].sum() == 0 and rows[:, 2 * n].sum() == 0 and set(np.unique(rows[:, :2 * n])) <= {0, 1}
    rows[:, -2] = 0                                           # (the order column of a type-4 row is ignored: no -99 in the file)
    out = os.path.join(ROOT, "tests", "golden", "luad28_unknown_rows.npy")
    np.save(out, rows)
    print(f"{out}: {rows.shape}, PT events per row: max {rows[:, 0:2 * n:2].sum(1).max()}, "
          f"histogram {np.bincount(rows[:, 0:2 * n:2].sum(1)).tolist()}")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "data", "luad")):
        sys.exit(__doc__)
    main(sys.argv[1])
