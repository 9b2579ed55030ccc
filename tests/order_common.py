"""What the tests of the order family share (test_orders*.py, test_order_*.py): the random models, the rows and cohorts they
run on, what a row carries, the enumeration of a paired state's orders, the host stand-in for the one device call of the
host code, and the contract every cohort entry point keeps: ENTRIES and the check_* bodies that the tests of the entry
points' own files call (the checks without a part of their own are the tests of tests/test_order_contract.py).  Imported by
name (`from order_common import ...`); tests/ is on sys.path.  The bars are derived in tests/test_order_posteriors.py."""
import itertools
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
