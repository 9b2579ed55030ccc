"""What the tests of the order family share (test_orders*.py, test_order_*.py): the random models, the rows and cohorts they
run on, what a row carries, the enumeration of a paired state's orders, the host stand-in for the one device call of the
host code, and the contract every cohort entry point keeps: ENTRIES and the check_* bodies that the tests of the entry
points' own files call (the checks without a part of their own are the tests of tests/test_order_contract.py), and the
host values of rows with 15 - 21 slots (tests/golden/orders_big.npz: big_rows, check_big_rows, check_big_samples).  Imported by
name (`from order_common import ...`); tests/ is on sys.path.  The bars are derived in tests/test_order_posteriors.py."""
import glob
import itertools
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import metmhn_amd.model as model_mod
from metmhn_amd.model import MetMHN, _ROW_ERRORS
from metmhn_amd.state import MetState
from oracle import metmhn_oracle as orc

KEY = 0x9E3779B97F4A7C15          # sample_orders: a seed with a non-zero high word
FIRST = 2 ** 32 - 100             # sample indices that cross the low counter word


class OracleDiag:
    @staticmethod
    def kron_diag(log_theta, state, n_state):
        return orc.kron_diag(np.asarray(log_theta), np.asarray(state), n_state)


@pytest.fixture
def host_only(monkeypatch):
    """The one device call of the host class (the restricted joint diagonal) from the oracle."""
    monkeypatch.setattr(model_mod, "_kronvec", OracleDiag)
    warnings.simplefilter("ignore", DeprecationWarning)


# ---------------------------------------------------------------------------------------------------- models and rows
def model(n=5, seed=0):
    rng = np.random.default_rng(seed)
    th = rng.normal(0.0, 0.5, (n + 1, n + 1))
    th[np.diag_indices(n + 1)] = rng.normal(-1.0, 0.5, n + 1)
    return MetMHN(th, 2 * rng.random(n + 1) + 1, 2 * rng.random(n + 1) + 1)


def luad(golden, prefix):
    d = golden("luad28")
    return MetMHN(d[prefix + "_theta"], d[prefix + "_dp"], d[prefix + "_dm"]), d["dat"]


def row(n, slots, typ, diag_order=-99):
    r = np.zeros(2 * n + 3, dtype=np.int8)
    r[list(slots)] = 1
    r[-2], r[-1] = diag_order, typ
    return r


def paired(n, pt, mt, diag_order):
    return row(n, [2 * i for i in pt] + [2 * i + 1 for i in mt] + [2 * n], 3, diag_order)


class Row:
    """What a dat row carries.  slots: its occupied slots; codes: its event codes as likeliest_order writes them; lineages:
    {"pt" / "mt": the event codes of that lineage} for the lineages it has; call(): the (state, met_status, first_obs) of
    the one-observation entry points."""

    def __init__(self, dat_row, n):
        self.n, self.typ, self.data = n, int(dat_row[-1]), dat_row
        pt = [2 * i for i in range(n) if dat_row[2 * i]]
        mt = [2 * i + 1 for i in range(n) if dat_row[2 * i + 1]]
        seed = [2 * n] if dat_row[2 * n] else []
        self.slots = set(int(s) for s in np.flatnonzero(dat_row[:2 * n + 1]))
        self.codes = {0: pt, 1: pt + seed, 2: mt + seed, 3: sorted(pt + mt) + seed}[self.typ]
        self.lineages = {0: {"pt": pt}, 1: {"pt": pt + seed}, 2: {"mt": mt + seed}, 3: {"pt": pt + seed, "mt": mt + seed}}[self.typ]

    def call(self):
        status = ["absent", "present", "isMetastasis", "isPaired"][self.typ]
        first = {0: "unknown", 1: "PT"}.get(int(self.data[-2]), "Met") if self.typ == 3 else None
        return MetState.from_seq(self.data[:2 * self.n + 1]), status, first

    def moments(self, order):
        """moments() of one of the row's orders: in a paired row the events before the seeding are joint ones."""
        s = order.index(2 * self.n) if 2 * self.n in order else len(order)
        return moments(order, s // 2 if self.typ == 3 else 0)


def split(order, n):
    """(PT lineage, MT lineage) of an order of event codes."""
    return [c for c in order if c % 2 == 0], [c for c in order if c % 2 == 1 or c == 2 * n]


def moments(order, joint_before):
    """code -> the moment it happened: the two codes of a joint event before the seeding share one."""
    t = {}
    for j, c in enumerate(order):
        t[c] = j // 2 if j < 2 * joint_before else j - joint_before
    return t


# ---------------------------------------------------------------------------------------------------- enumeration
def paired_orders(state: MetState):
    """Every order the chain can take to a seeded paired `state`, with the number of joint events before the seeding."""
    n = state.n
    both = [i for i in state.PT_events if i in state.MT_events]
    for r in range(len(both) + 1):
        for pre in itertools.permutations(both, r):
            head = [c for i in pre for c in (2 * i, 2 * i + 1)] + [2 * n]
            rest = [2 * i for i in state.PT_events if i not in pre] + [2 * i + 1 for i in state.MT_events if i not in pre]
            for tail in itertools.permutations(rest):
                yield tuple(head) + tail, r


def all_orders(state: MetState):
    """Every order the chain can take to a seeded `state`."""
    return (order for order, _ in paired_orders(state))


def random_paired_states(n, rng_seed, model_seeds, draws, max_k=7):
    """The random paired states of the enumeration tests: for every model seed `draws` states whose slots below the seeding
    are occupied with probability 0.45, those with more than max_k slots (the seeding counted) drawn again - k <= 7 is
    under 6! x 2^3 orders per state.  Yields (model, slots without the seeding, seen): seen counts the events drawn so far
    that are in the PT only, in the MT only and in both."""
    rng = np.random.default_rng(rng_seed)
    seen = {"pt_only": 0, "mt_only": 0, "joint": 0}
    for seed in model_seeds:
        mod = model(n, seed=seed)
        drawn = 0
        while drawn < draws:
            slots = [s for s in range(2 * n) if rng.random() < 0.45]
            if len(slots) + 1 > max_k:
                continue
            drawn += 1
            pt, mt = {s // 2 for s in slots if s % 2 == 0}, {s // 2 for s in slots if s % 2 == 1}
            seen["pt_only"] += len(pt - mt); seen["mt_only"] += len(mt - pt); seen["joint"] += len(pt & mt)
            yield mod, slots, seen


# ---------------------------------------------------------------------------------------------------- cohorts
def mixed_cohort(n=5):
    """Every status and every diagnosis order of a paired row (-99 reads as "Met", as in the objective)."""
    S = 2 * n
    rows = [row(n, [0, 4, 6], 0), row(n, [], 0), row(n, [2, 4, 8, S], 1), row(n, [S], 1),
            row(n, [1, 5, 9, S], 2), row(n, [S], 2)]
    for d in (0, 1, 2, -99):
        rows += [row(n, [0, 1, 2, 5, 6, 7, S], 3, d), row(n, [0, 1, 4, 5, 3, S], 3, d), row(n, [1, S], 3, d)]
    return np.array(rows)


def small_shapes_n8():
    """(model, dat): the smallest rows at which the kernels take another path.  Index bits of a target's move vector:
    k - 1 for one tumour, k - 2 paired; chunks of 6 bits below 8 index bits (256 threads), so k = 9 paired is the first row
    whose classes split between a chunk's number and its low bits."""
    n = 8
    S = 2 * n
    rows = []
    for d in (0, 1, 2, -99):
        rows += [paired(n, [], [], d),                                   # k = 1: the seeding alone
                 paired(n, [2], [3], d),                                 # k = 3: one PT-only and one MT-only event
                 paired(n, [2], [], d), paired(n, [], [3], d),           # k = 2
                 paired(n, [0], [0], d),                                 # k = 3: the smallest joint row
                 paired(n, [0, 1, 3], [0, 2], d),                        # k = 6: a chunk narrower than a wave
                 paired(n, [0, 2, 4], [0, 2, 5], d),                     # k = 7
                 paired(n, [0, 1, 2, 3], [0, 1, 4], d),                  # k = 8: one chunk
                 paired(n, [0, 1, 2, 3, 4], [0, 5, 6], d),               # k = 9: two chunks
                 paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 3], d),            # k = 10
                 paired(n, [0, 1, 2, 3, 4], [0, 1, 2, 5, 6], d),         # k = 11
                 paired(n, [0, 1, 2], [3, 4, 5], d),      # k = 7, no joint event, PT slots low and MT slots high: the
                                                          # MT mask has no low bit, the PT mask no high one
                 paired(n, [0, 1, 2, 3], [0, 1, 2, 3], d)]               # k = 9, only joint events
    ev = lambda k, odd: [2 * i + odd for i in range(k)]
    rows += [row(n, ev(k, 0), 0) for k in (0, 1, 6, 7, 8)]               # "absent"
    rows += [row(n, ev(k - 1, 0) + [S], 1) for k in (1, 6, 7, 8)]        # "present"
    rows += [row(n, ev(k - 1, 1) + [S], 2) for k in (1, 6, 7, 8)]        # "isMetastasis"
    return model(n, seed=21), np.array(rows)


def large_rows(n):
    """Paired rows with k = 14 ... 17 (n = 9; n = 9 has room for 10 slots of one tumour, those rows are here too) or
    one-tumour rows with k = 14 ... 17 (n = 16): both sides of the 1024-thread switch at 15 slots."""
    rows = []
    if n == 9:
        for j, k in enumerate((14, 15, 16, 17)):
            # k - 1 = 2 joint + PT-only + MT-only
            nj = (5, 5, 6, 7)[j]
            rest = k - 1 - 2 * nj
            pt_only = list(range(nj, nj + (rest + 1) // 2))
            mt_only = list(range(nj + (rest + 1) // 2, nj + rest))
            assert nj + rest <= n
            rows.append(paired(n, list(range(nj)) + pt_only, list(range(nj)) + mt_only, (0, 1, 2, -99)[j]))
        rows += [paired(n, range(8), range(8), 0),                                  # k = 17, only joint events
                 paired(n, [0, 1, 2, 3, 4, 5, 6], [7, 8, 0, 1, 2, 3, 4], 1),        # k = 15
                 row(n, list(range(0, 18, 2)) + [18], 1), row(n, list(range(1, 18, 2)) + [18], 2),
                 row(n, list(range(0, 18, 2)), 0), row(n, [0, 4, 18], 1), row(n, [18], 2)]
    else:
        for k in (14, 15, 16, 17):
            rows += [row(n, [2 * i for i in range(k - 1)] + [2 * n], 1), row(n, [2 * i + 1 for i in range(k - 1)] + [2 * n], 2)]
            if k <= n:
                rows.append(row(n, [2 * i for i in range(k)], 0))
    return np.array(rows)


def luad_selection(dat):
    """The LUAD-28 rows of the tests of large rows: the indices of the 71 rows with k >= 15, of 300 rows with k <= 12 and of
    up to 200 with k = 13, 14."""
    k = dat[:, :-2].astype(int).sum(1)
    small = np.flatnonzero(k <= 12)
    return np.concatenate((np.flatnonzero(k >= 15), small[np.linspace(0, len(small) - 1, 300).astype(int)],
                           np.flatnonzero((k >= 13) & (k <= 14))[:200]))


def error_rows(n):
    """(good, bad): a valid cohort and one row per MMHN_ORD_* reason, in the order of the enum (1 ... 7)."""
    S = 2 * n
    good = np.array([row(n, [0, 4, 6], 0), row(n, [], 0), row(n, [2, 4, 8, S], 1), row(n, [1, 5, 9, S], 2),
                     row(n, [0, 1, 2, 5, 6, 7, S], 3, 0), row(n, [0, 1, 4, 5, 3, S], 3, 1), row(n, [1, S], 3, 2)])
    bad = [row(n, [0], 5), row(n, [0, 3], 3, 1), row(n, [0, 1], 3, 0), row(n, [0, 1, 2 * n], 2), row(n, [1, 3], 2),
           row(n, [1], 0), row(n, [0, 1, 2 * n], 1)]
    return good, bad


def too_large_cohort_k14(n=9):
    """A paired row with k = 14 (1.2 MiB, over a workspace of 1 MiB) in front of three small rows."""
    S = 2 * n
    wide = paired(n, [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 3, 7, 8], 0)
    return np.vstack((wide[None], [row(n, [0, 1, 2, 3, 6, S], 3, 1), row(n, [0, 2, S], 1), row(n, [0, 2], 0)]))


def too_large_cohort_k17(n=9):
    """The same with a paired row with k = 17 (9.5 MiB, over a workspace of 8 MiB): the cohort of order_posteriors."""
    S = 2 * n
    wide = row(n, list(range(16)) + [S], 3, 0)
    return np.vstack((wide[None], [row(n, [0, 1, 2, 3, 6, S], 3, 1), row(n, [0, 2, S], 1), row(n, [0, 2], 0)]))


# ---------------------------------------------------------------------------------------------------- rows of 15 - 21 slots
# tests/golden/orders_big*.npz (tests/tools/make_golden_orders_big.py): the host values of rows with k = 15 ... 21, which
# run on the 1 024-thread kernels and take the host code seconds to minutes each.  One layout, used by the generator
# (big_pack), the loader (big_rows, big_host) and the comparators (check_big_rows, check_big_samples).
BIG_MODELS = (("n9", 9, 31), ("n16", 16, 32), ("luad", 28, None))      # name, n, the seed of model() - None: LUAD-28 "fit"
BIG_ENTRIES = {            # cohort method -> (key in the fixture, one-observation method, result class, fields)
    "order_posteriors": ("post", "order_posterior", model_mod.OrderPosteriors, ("pre", "seed_pos")),
    "order_precedences": ("prec", "order_precedence", model_mod.OrderPrecedences, ("prec",)),
    "order_positions": ("pos", "order_position", model_mod.OrderPositions, ("pos_pt", "pos_mt")),
    "order_times": ("time", "order_time", model_mod.OrderTimes, ("time", "obs", "pt_first")),
    "order_snapshots": ("snap", "order_snapshot", model_mod.OrderSnapshots,
                        ("held", "late", "map_state", "map_first", "map_prob"))}
BIG_SAMPLES = 64           # samples per synthetic row, key = KEY + n, first = FIRST
BIG_GAP = 1e-12            # two best snapshots closer than this (relative): map_first / map_state are not compared


def _big_cells(entry, w):
    """[(field, index into that field's array of one row)]: the cells of a row's block of doubles, in the block's order -
    the entries over the row's own codes (k; k x k; one L x L per lineage; k + 3; 4 k + 3, less where late is narrower)."""
    n, codes = w.n, w.codes
    if entry == "order_posteriors":
        ev = sorted({c // 2 for c in codes if c != 2 * n})
        return [] if w.typ == 0 else [("pre", (ev,)), ("seed_pos", (slice(0, len(ev) + 1),))]
    if entry == "order_precedences":
        return [("prec", np.ix_(codes, codes))]
    if entry == "order_positions":
        return [("pos_" + name, np.ix_([c // 2 for c in w.lineages[name]], range(len(w.lineages[name]))))
                for name in ("pt", "mt") if name in w.lineages]
    if entry == "order_times":
        return [("time", (codes,)), ("obs", (slice(None),)), ("pt_first", ())]
    if w.typ != 3:
        return []
    return [("held", np.ix_((0, 1), codes)), ("late", (slice(None), slice(0, min(len(codes), n + 1)))), ("map_prob", ())]


def _big_blank(entry, w):
    """{field: one row's array} with what a row has outside its block: NaN / -1 where it does not carry a code, 0 where it
    does and the entry is one by construction (pre of an event only one tumour has, positions past a lineage's length, late
    past the other tumour's events)."""
    n = w.n
    L, N = 2 * n + 1, n + 1
    nan = lambda *shape: np.full(shape, np.nan)
    if entry == "order_posteriors":
        return {"pre": nan(n), "seed_pos": nan(N)} if w.typ == 0 else {"pre": np.zeros(n), "seed_pos": np.zeros(N)}
    if entry == "order_precedences":
        return {"prec": nan(L, L)}
    if entry == "order_positions":
        out = {"pos_pt": nan(N, N), "pos_mt": nan(N, N)}
        for name, codes in w.lineages.items():
            out["pos_" + name][[c // 2 for c in codes]] = 0.0
        return out
    if entry == "order_times":
        return {"time": nan(L), "obs": nan(2), "pt_first": nan()}
    return {"held": nan(2, L), "late": np.zeros((2, N)) if w.typ == 3 else nan(2, N),
            "map_state": np.full(L, -1, dtype=np.int8), "map_first": np.array(-1, dtype=np.int32), "map_prob": nan()}


def big_pack(entry, w, res):
    """The block of doubles of one host result (of BIG_ENTRIES[entry]'s one-observation method) of the row w."""
    return np.concatenate([np.zeros(0)] + [np.asarray(getattr(res, f), dtype=np.float64)[ix].ravel()
                                           for f, ix in _big_cells(entry, w)])


def big_unpack(entry, w, block, map_state=None, map_first=-1):
    """{field: one row's array in the shape and with the NaN / -1 padding of the API} from a block of big_pack (snapshots:
    and the chosen snapshot over the row's codes)."""
    out, at = _big_blank(entry, w), 0
    for f, ix in _big_cells(entry, w):
        size = out[f][ix].size
        out[f][ix] = block[at:at + size].reshape(out[f][ix].shape)
        at += size
    assert at == len(block), (entry, at, len(block))
    if entry == "order_snapshots" and w.typ == 3:
        out["map_state"][w.codes] = map_state
        out["map_first"][()] = map_first
    return out


def _big_files():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return sorted(glob.glob(os.path.join(here, "orders_big*.npz")))


_big_cache = {}


def big_rows():
    """{name: (mod: the MetMHN, n, dat: the rows in the fixture's order, index: their indices in the LUAD-28 cohort or
    None, raw: the fixture's arrays of this model without the name's prefix)} of the models of BIG_MODELS, and under
    "rows" the number of rows of the whole fixture.  Loaded once; nothing in it may be written to."""
    if not _big_cache:
        raw = {}
        for path in _big_files():
            with np.load(path) as z:
                raw.update({key: z[key] for key in z.files})
        assert raw, "tests/golden/orders_big*.npz is missing: tests/tools/make_golden_orders_big.py writes it"
        for name, n, seed in BIG_MODELS:
            if seed is None:
                luad28 = np.load(os.path.join(os.path.dirname(_big_files()[0]), "luad28.npz"))
                prefix = str(raw[name + "_prefix"])
                mod = MetMHN(luad28[prefix + "_theta"], luad28[prefix + "_dp"], luad28[prefix + "_dm"])
                np.testing.assert_array_equal(luad28["dat"][raw[name + "_index"]], raw[name + "_dat"])
            else:
                assert int(raw[name + "_seed"]) == seed
                mod = model(n, seed=seed)
            mine = {key[len(name) + 1:]: a for key, a in raw.items() if key.startswith(name + "_")}
            for a in mine.values():
                a.setflags(write=False)
            _big_cache[name] = SimpleNamespace(mod=mod, n=n, dat=mine["dat"], index=mine.get("index"), raw=mine)
        _big_cache["rows"] = int(raw["rows"])
        assert _big_cache["rows"] == sum(len(_big_cache[name].dat) for name, _, _ in BIG_MODELS)
    return _big_cache


def big_models(synthetic_only=False):
    """(name, what big_rows() holds under it) of the fixture's models, or of those with rows made up for it alone."""
    return [(name, big_rows()[name]) for name, _, seed in BIG_MODELS if seed is not None or not synthetic_only]


def big_host(entry, name, rows=None):
    """The host result of a cohort entry point on the fixture's rows of one model (all of them, or those of `rows`), in the
    API's shapes: an object of the entry point's result class."""
    m = big_rows()[name]
    key, _, cls, fields = BIG_ENTRIES[entry]
    off = m.raw[key + "_off"]
    rows = range(len(m.dat)) if rows is None else rows
    per_row, so = [], 0
    if entry == "order_snapshots":
        so = np.concatenate(([0], np.cumsum([len(Row(r, m.n).codes) if r[-1] == 3 else 0 for r in m.dat])))
    for i in rows:
        w = Row(m.dat[i], m.n)
        extra = (m.raw["snap_state"][so[i]:so[i + 1]], m.raw["snap_first"][i]) if entry == "order_snapshots" else ()
        per_row.append(big_unpack(entry, w, m.raw[key + "_val"][off[i]:off[i + 1]], *extra))
    return cls(m.raw[key + "_le"][list(rows)].copy(), *(np.array([r[f] for r in per_row]) for f in fields))


def _over(d, bar):
    """Largest entry of d over the bar, NaN (in both operands: the patterns are compared first) left out."""
    d = np.asarray(d, dtype=np.float64)
    return float(np.max(np.where(np.isnan(d), 0.0, d), initial=0.0)) / bar


def check_big_rows(entry, device, bar):
    """device: {name: the result of the cohort method `entry` on big_rows()[name].dat} against the fixture's host values.
    The NaN / -1 patterns are equal; every field is within the entry point's own device-against-host bar `bar` (absolute on
    probabilities; times and observation times over the row's last observation time, as tests/test_order_times.py has it);
    exp(log_evidence) within 1e-12 relative; map_first / map_state equal except where the host's two best snapshots are
    within BIG_GAP of each other, at most one row.  Prints the worst error over its bar per field before it asserts, and
    asserts that every row of the fixture (all have k >= 15) was compared.  Returns {field: worst error over its bar}."""
    big = big_rows()
    fields = BIG_ENTRIES[entry][3]
    worst, bad, compared, exempt = {"log_evidence": 0.0}, [], 0, 0
    for name, _, _ in BIG_MODELS:
        m, dev, host = big[name], device[name], big_host(entry, name)
        k = m.dat[:, :-2].astype(int).sum(1)
        if np.shape(dev.log_evidence) != host.log_evidence.shape:
            bad.append(f"{name}: {np.shape(dev.log_evidence)} evidences for {len(m.dat)} rows")
            continue
        compared += int((k >= 15).sum())
        zd, zh = np.exp(dev.log_evidence), np.exp(host.log_evidence)
        worst["log_evidence"] = max(worst["log_evidence"], _over(np.abs(zd - zh) / zh, 1e-12))
        if not np.all(np.isfinite(dev.log_evidence)):
            bad.append(f"{name}: log_evidence not finite")
        scale = 1.0
        if entry == "order_times":
            scale = np.where(np.isnan(host.obs[:, 1]), host.obs[:, 0], host.obs[:, 1])
        tied = np.zeros(len(m.dat), dtype=bool)
        if entry == "order_snapshots":
            tied = m.raw["snap_gap"] <= BIG_GAP                    # (NaN, a row without a first observation: compared)
            exempt += int(tied.sum())
        for f in fields:
            d, h = np.asarray(getattr(dev, f)), getattr(host, f)
            if d.shape != h.shape:
                bad.append(f"{name}: {f} has shape {d.shape}, not {h.shape}")
            elif f in ("map_state", "map_first"):
                rows = np.flatnonzero((d != h).reshape(len(h), -1).any(axis=1) & ~tied)
                worst[f] = max(worst.get(f, 0.0), float(len(rows)))
                if len(rows):
                    bad.append(f"{name}: {f} differs in rows {rows.tolist()}")
            else:
                if not np.array_equal(np.isnan(d), np.isnan(h)):
                    bad.append(f"{name}: NaN pattern of {f} differs in rows "
                               f"{np.flatnonzero((np.isnan(d) != np.isnan(h)).reshape(len(h), -1).any(axis=1)).tolist()}")
                s = scale if f in ("time", "obs") else 1.0
                s = np.reshape(s, np.shape(s) + (1,) * (h.ndim - np.ndim(s)))
                worst[f] = max(worst.get(f, 0.0), _over(np.abs(d - h) / s, bar))
    print(f"rows of 15 - 21 slots against the host values, {entry}: {compared} rows with k >= 15 compared (the fixture has "
          f"{big['rows']}), worst error over its bar (log_evidence: 1e-12 relative, the others {bar:g}; map_*: rows that "
          f"differ) {({f: float(f'{v:.3g}') for f, v in worst.items()})}, {exempt} rows with tied snapshots")
    assert compared == big["rows"], (compared, big["rows"])
    assert not bad, bad
    assert exempt <= 1
    for f, v in worst.items():
        assert v <= (0.0 if f in ("map_state", "map_first") else 1.0), (f, v)
    return worst


def big_host_samples(name):
    """The host's samples of the fixture's rows of a synthetic model: (log_evidence [R], orders [R, BIG_SAMPLES, 2n+1]
    padded with -1, log_prob, margin [R, BIG_SAMPLES])."""
    m = big_rows()[name]
    ks = [len(Row(r, m.n).codes) for r in m.dat]
    orders = np.full((len(m.dat), BIG_SAMPLES, 2 * m.n + 1), -1, dtype=np.int8)
    at = 0
    for i, k in enumerate(ks):
        orders[i, :, :k] = m.raw["samp_orders"][at:at + BIG_SAMPLES * k].reshape(BIG_SAMPLES, k)
        at += BIG_SAMPLES * k
    assert at == len(m.raw["samp_orders"]) and np.array_equal(m.raw["samp_row"], np.arange(len(m.dat)))
    return m.raw["samp_le"], orders, m.raw["samp_log_prob"], m.raw["samp_margin"]


def check_big_samples(device, margin, max_excluded):
    """device: {name: sample_orders(big_rows()[name].dat, BIG_SAMPLES, key=KEY + n, first=FIRST)} of the synthetic models
    against the host's samples, with the comparison of test_order_samples.test_device_against_host_small_shapes: the orders
    equal wherever the host margin is at least `margin`, log_prob within 1e-10 there, at most max_excluded of the samples
    set aside, exp(log_evidence) within 1e-12 relative."""
    total = excluded = differ = rows = 0
    d_lp = rel = 0.0
    least = np.inf
    for name, n, seed in BIG_MODELS:
        if seed is None:
            continue
        le, orders, log_prob, mg = big_host_samples(name)
        dev = device[name]
        assert dev.orders.shape == orders.shape and dev.orders.dtype == np.int8 and dev.log_prob.shape == log_prob.shape
        safe = mg >= margin
        same = (dev.orders == orders).all(axis=2)
        total, excluded, rows = total + safe.size, excluded + int((~safe).sum()), rows + len(le)
        differ += int((~same & safe).sum())
        d_lp = max(d_lp, float(np.abs(dev.log_prob - log_prob)[safe].max()))
        rel = max(rel, float((np.abs(np.exp(dev.log_evidence) - np.exp(le)) / np.exp(le)).max()))
        least = min(least, float(mg.min()))
    print(f"rows of 15 - 17 slots against the host's samples: {rows} rows x {BIG_SAMPLES} samples, {excluded} set aside "
          f"(smallest margin {least:.2e}), {differ} of the others differ, worst |log_prob| difference {d_lp:.2e}, rel. "
          f"evidence {rel:.2e}")
    assert rows == sum(len(big_rows()[name].dat) for name, _, seed in BIG_MODELS if seed is not None)
    assert excluded <= max_excluded * total
    assert differ == 0
    assert d_lp <= 1e-10
    assert rel <= 1e-12


# ---------------------------------------------------------------------------------------------------- the shared contract
# One entry per cohort entry point.  cohort / single / engine: the methods of MetMHN (a cohort, one observation) and of
# Engine; symbol, n_args: the C function and the length of its _lib.SIGNATURES entry; fallback: the MetMHN counter of the
# rows the device turned away; fields: the outputs after log_evidence; extra: what a call takes after dat (sample_orders:
# n_samples, key, first).  The inputs on which the entry points differ - error_good: the valid rows of the row-error test;
# too_large, workspace: a cohort whose first row does not fit that workspace; luad: the parameter point and the rows of
# LUAD-28 of the batching test (sample_orders, whose samples depend on the index of their row, has none).
whole = lambda dat: np.arange(len(dat))
ENTRIES = {e.cohort: e for e in (
    SimpleNamespace(cohort="order_posteriors", single="order_posterior", engine="order_posteriors",
                    symbol="mmhn_order_posteriors", n_args=11, fallback="posteriors_fallback_rows",
                    fields=("pre", "seed_pos"), extra=lambda *a: (), error_good=mixed_cohort,
                    too_large=too_large_cohort_k17, workspace=8 << 20, luad=("indep", whole)),
    SimpleNamespace(cohort="order_precedences", single="order_precedence", engine="order_precedences",
                    symbol="mmhn_order_precedences", n_args=10, fallback="precedences_fallback_rows",
                    fields=("prec",), extra=lambda *a: (), error_good=lambda n: error_rows(n)[0],
                    too_large=too_large_cohort_k14, workspace=1 << 20, luad=("fit", luad_selection)),
    SimpleNamespace(cohort="order_positions", single="order_position", engine="order_positions",
                    symbol="mmhn_order_positions", n_args=11, fallback="positions_fallback_rows",
                    fields=("pos_pt", "pos_mt"), extra=lambda *a: (), error_good=lambda n: error_rows(n)[0],
                    too_large=too_large_cohort_k14, workspace=1 << 20, luad=("fit", luad_selection)),
    SimpleNamespace(cohort="sample_orders", single="sample_order", engine="order_samples",
                    symbol="mmhn_order_samples", n_args=14, fallback="samples_fallback_rows",
                    fields=("orders", "log_prob"), extra=lambda *a: a, error_good=lambda n: error_rows(n)[0],
                    too_large=too_large_cohort_k14, workspace=1 << 20, luad=None))}


def check_arguments_before_the_library(e, monkeypatch):
    """The shape of dat and the backend with the messages of order_posteriors, the one-observation arguments with those of
    order_precedence; the library is not reached.  Returns the model."""
    import metmhn_amd.jx as jx

    def no_engine(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(jx, "engine", no_engine)
    mod = model()
    cohort, single, extra = getattr(mod, e.cohort), getattr(mod, e.single), e.extra(4)
    dat = mixed_cohort(mod.n)
    for bad in (dat[0], dat[:, :-1], np.zeros((2, 3, 4))):
        with pytest.raises(ValueError, match=r"dat must have shape \[n_pat, 13\]") as e1:
            cohort(bad, *extra)
        with pytest.raises(ValueError) as e2:
            mod.order_posteriors(bad)
        assert str(e1.value) == str(e2.value)
    with pytest.raises(ValueError, match="backend must be 'device' or 'host'") as e1:
        cohort(dat, *extra, backend="cpu")
    with pytest.raises(ValueError) as e2:
        mod.order_posteriors(dat, backend="cpu")
    assert str(e1.value) == str(e2.value)
    state = MetState([0, 1, 10], size=11)
    for args, message in (((state, "paired"), "met_status must be one of"),
                          ((state, "isPaired", "first"), "first_obs must be one of"),
                          ((MetState([0, 10], size=11), "absent"),
                           "Met part of the state was not empty, but met_status is 'absent'")):
        with pytest.raises(ValueError, match=message) as e1:
            single(*args)
        with pytest.raises(ValueError) as e2:
            mod.order_precedence(*args)
        assert str(e1.value) == str(e2.value)
    return mod


def check_errors_name_the_row(e):
    """One bad row per MMHN_ORD_* reason: the error of likeliest_orders, from the device and from the host; fp64 only.
    Returns the model and the valid rows."""
    from metmhn_amd.engine import Engine
    mod = model()
    n = mod.n
    cohort, extra = getattr(mod, e.cohort), e.extra(8)
    good, bad = e.error_good(n), error_rows(n)[1]
    for reason, b in enumerate(bad, start=1):
        dat = np.vstack((good[:3], b[None], good[3:]))
        with pytest.raises(ValueError) as lo_err:
            mod.likeliest_orders(dat)
        with pytest.raises(ValueError) as dev_err:
            cohort(dat, *extra)
        assert str(dev_err.value) == str(lo_err.value) == f"row 3: {_ROW_ERRORS[reason]}"
        with pytest.raises(ValueError, match=r"^row 3: "):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", DeprecationWarning)
                cohort(dat, *extra, backend="host")
    with Engine(n, dtype="f32") as e32:
        with pytest.raises(RuntimeError, match="fp64"):
            getattr(e32, e.engine)(mod.log_theta, mod.obs1, mod.obs2, good, *extra)
    return mod, good


def check_too_large_rows_get_the_host_value(e, monkeypatch):
    """The Python layer recomputes MMHN_ORD_TOO_LARGE rows with the one-observation method and counts them.  Returns
    (model, dat, ref: the device's result with room for every row, raw: the outputs of the Engine that turned row 0 away,
    host: the one-observation result of row 0) for what an entry point checks further."""
    import metmhn_amd.jx as jx
    from metmhn_amd.engine import Engine
    n = 9
    mod = model(n, seed=11)
    cohort, extra = getattr(mod, e.cohort), e.extra(64, KEY, FIRST)
    dat = e.too_large(n)
    ref = cohort(dat, *extra)
    assert getattr(mod, e.fallback) == 0
    with Engine(n, workspace_bytes=e.workspace) as small:
        raw = getattr(small, e.engine)(mod.log_theta, mod.obs1, mod.obs2, dat, *extra)
        assert raw[-1].tolist() == [3, 0, 0, 0]
        monkeypatch.setattr(jx, "engine", lambda n_mut: small)
        got = cohort(dat, *extra)
    assert getattr(mod, e.fallback) == 1
    host = getattr(mod, e.single)(MetState.from_seq(dat[0, :2 * n + 1]), "isPaired", "unknown", *extra)
    for name in ("log_evidence",) + e.fields:
        np.testing.assert_array_equal(getattr(got, name)[0], getattr(host, name))
        np.testing.assert_array_equal(getattr(got, name)[1:], getattr(ref, name)[1:])
    return mod, dat, ref, raw, host


# ---------------------------------------------------------------------------------------------------- device against host
# What the tests of one entry point and tests/test_limits.py (the same entry points at n = 31) both use.
BAR = 1e-12                       # device against host (tests/test_order_posteriors.py derives it)
MARGIN = 1e-9                     # a sample whose closest draw is nearer than this to a boundary is not compared
MAX_EXCLUDED = 1e-3               # share of one test's samples that may be set aside


def same_or_tie(mod, row, got, want, rel=1e-12):
    """(order, probability) of the device against the host's: the same probability, and the same order or one as likely."""
    (go, gp), (wo, wp) = got, want
    assert abs(gp - wp) <= rel * wp, (row, gp, wp)
    if go != wo:                                               # a tie: the device's order is as likely as the host's
        _, status, first = Row(row, mod.n).call()
        assert abs(mod.likelihood(go, status, first) - wp) <= rel * wp, (row, go, wo)


def worst_entry(d):
    """Largest entry of d, the NaN ones (NaN in both operands, which the callers assert first) left out."""
    d = np.asarray(d, dtype=float)
    return float(np.max(np.where(np.isnan(d), 0.0, d), initial=0.0))


def last_observation(obs):
    """The last observation time of rows of obs [..., 2]."""
    return np.where(np.isnan(obs[..., 1]), obs[..., 0], obs[..., 1])


def times_diff(got, want):
    """order_times: (relative difference of the evidence, worst difference of time and obs over the last observation time,
    absolute difference of pt_first - 0 where both are NaN); the NaN patterns are asserted equal."""
    np.testing.assert_array_equal(np.isnan(got.time), np.isnan(want.time))
    np.testing.assert_array_equal(np.isnan(got.obs), np.isnan(want.obs))
    np.testing.assert_array_equal(np.isnan(got.pt_first), np.isnan(want.pt_first))
    zg, zw = np.exp(got.log_evidence), np.exp(want.log_evidence)
    last = last_observation(np.asarray(want.obs))
    d_t = worst_entry(np.abs(np.asarray(got.time) - want.time) / last[..., None])
    d_o = worst_entry(np.abs(np.asarray(got.obs) - want.obs) / last[..., None])
    d_p = worst_entry(np.abs(np.asarray(got.pt_first, dtype=float) - want.pt_first))
    return float(np.max(np.abs(zg - zw) / zw)), max(d_t, d_o), d_p


def times_orderings(time, obs, dat, n):
    """order_times: worst violation, over the last observation time, of: seeding <= first observation <= second observation;
    a code of one tumour alone >= the seeding (paired rows); every time <= the last observation."""
    worst = 0.0
    for i, r in enumerate(dat):
        w = Row(r, n)
        last = last_observation(obs[i])
        gaps = [t - last for t in time[i, w.codes]]
        if r[2 * n]:
            gaps.append(time[i, 2 * n] - obs[i, 0])
        if w.typ == 3:
            gaps.append(obs[i, 0] - obs[i, 1])
            both = set(w.lineages["pt"]) & set(c - 1 for c in w.lineages["mt"])
            gaps += [time[i, 2 * n] - time[i, c] for c in w.codes if c != 2 * n and c - c % 2 not in both]
        worst = max([worst] + [g / last for g in gaps])
    return worst


def snapshots_diff(got, want):
    """order_snapshots: (relative difference of the evidence, worst absolute difference of held, of late, of map_prob); the
    NaN patterns, map_first and map_state are asserted equal."""
    for name in ("held", "late", "map_prob"):
        np.testing.assert_array_equal(np.isnan(getattr(got, name)), np.isnan(getattr(want, name)), err_msg=name)
    np.testing.assert_array_equal(got.map_first, want.map_first)
    np.testing.assert_array_equal(got.map_state, want.map_state)
    zg, zw = np.exp(got.log_evidence), np.exp(want.log_evidence)
    return (float(np.max(np.abs(zg - zw) / zw)),) + tuple(
        worst_entry(np.abs(np.asarray(getattr(got, name), dtype=float) - getattr(want, name))) for name in ("held", "late", "map_prob"))


def snapshots_patterns(run, dat, n):
    """order_snapshots: the NaN / -1 patterns of a device result: codes carried, paired rows."""
    paired_rows = dat[:, -1] == 3
    carried = np.zeros((len(dat), 2 * n + 1), dtype=bool)
    for i, r in enumerate(dat):
        if paired_rows[i]:
            carried[i, Row(r, n).codes] = True
    np.testing.assert_array_equal(~np.isnan(run.held), np.repeat(carried[:, None], 2, axis=1))
    np.testing.assert_array_equal(~np.isnan(run.late), np.broadcast_to(paired_rows[:, None, None], run.late.shape))
    np.testing.assert_array_equal(run.map_state >= 0, carried)
    np.testing.assert_array_equal(run.map_first >= 0, paired_rows)
    np.testing.assert_array_equal(~np.isnan(run.map_prob), paired_rows)
    assert np.all(np.isfinite(run.log_evidence)), "log_evidence is not finite"
