"""The refusals of the C ABI (include/metmhn_amd.h), called through ctypes as `engine.lib.mmhn_*` with mmhn_last_error() read
after each: which text a caller gets, and in which order an entry point makes its checks.  Every call here is turned away
before a kernel is launched, except the evaluations of the split-evaluation cases and the six primitives at the end, which
anchor the zero log-theta of the entry points that take observation rates only.  The texts are data: copied from the library's
source, one table row per entry point."""
import ctypes as C

import numpy as np
import pytest

from eval_common import TIGHT, close, paired, row
from metmhn_amd._lib import f64p, i8p, i32p

pytestmark = pytest.mark.gpu

N_MUT = 2
NN = N_MUT + 1                    # events with the seeding
LL = 2 * N_MUT + 1                # event codes of a row
SENTINEL = {np.dtype(np.float64): -7.25, np.dtype(np.int8): 77, np.dtype(np.int32): 777777}
PTR = {np.dtype(np.float64): f64p, np.dtype(np.int8): i8p, np.dtype(np.int32): i32p}
F64, I8, I32 = np.float64, np.int8, np.int32


def out(kind, *shape):
    """An output buffer of one row (R = 1) per table entry: (dtype, shape behind the row index)."""
    return ("out", np.dtype(kind), shape)


# name, name of its row count (None: it has none), family ("order": pointers, dat, count, fp64 - "lattice": count, pointers,
# fp64), the text of its fp64 refusal, its arguments behind the handle.  "lt" is the first required pointer of every entry.
ORDER_HEAD = ["lt", "o1", "o2", "dat", "count", "ncols"]
ENTRY_POINTS = [
    ("mmhn_likeliest_orders", "n_pat", "order", "likeliest orders need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [0, out(I8, 2 * NN - 1), out(F64), out(I32)]),
    ("mmhn_order_posteriors", "n_pat", "order", "order posteriors need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [out(F64), out(F64, N_MUT), out(F64, NN), out(I32)]),
    ("mmhn_order_precedences", "n_pat", "order", "order precedences need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [out(F64), out(F64, LL, LL), out(I32)]),
    ("mmhn_order_positions", "n_pat", "order", "order positions need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [out(F64), out(F64, NN, NN), out(F64, NN, NN), out(I32)]),
    ("mmhn_order_times", "n_pat", "order", "order times need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [out(F64), out(F64, LL), out(F64, 2), out(F64), out(I32)]),
    ("mmhn_order_snapshots", "n_pat", "order", "order snapshots need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [out(F64), out(F64, 2, LL), out(F64, 2, NN), out(I8, LL), out(I32), out(F64), out(I32)]),
    ("mmhn_order_samples", "n_pat", "order", "order samples need an fp64 engine (MMHN_F64)",
     ORDER_HEAD + [0, 2, 5, out(F64), out(I8, 2, LL), out(F64, 2), out(I32)]),
    ("mmhn_seeding_forecasts", "n_rows", "lattice", "seeding forecasts need an fp64 engine (MMHN_F64)",
     ["lt", "o1", "geno", "count", 0, out(F64), out(F64), out(F64, N_MUT), out(F64, N_MUT), out(F64, NN), out(I32)]),
    ("mmhn_seeding_landscape", "n_rows", "lattice", "the seeding landscape needs an fp64 engine (MMHN_F64)",
     ["lt", "o1", 0, "geno", "count", out(F64, 4), out(I32), None]),
    ("mmhn_genotype_distribution", "n_rows", "lattice", "the genotype distribution needs an fp64 engine (MMHN_F64)",
     ["lt", "o1", "geno", "count", out(F64, 2), out(I32), None, None]),
    ("mmhn_metastasis_distribution", "n_rows", "lattice", "the metastasis distribution needs an fp64 engine (MMHN_F64)",
     ["lt", "o1", "o2", "geno", "count", out(F64, 3), out(I32), None, None]),
    ("mmhn_partner_distributions", "n_rows", "lattice", "the partner distribution needs an fp64 engine (MMHN_F64)",
     ["lt", "o1", "o2", 0, "geno", None, "count", out(F64, 3), out(I32), None, None]),
    ("mmhn_cross_table", None, "lattice", "the cross table needs an fp64 engine (MMHN_F64)",
     ["lt", "o1", "o2", 1, out(F64, 1 + 2 * N_MUT + N_MUT * N_MUT + NN * NN + 2 * N_MUT * NN)]),
]
IDS = [e[0] for e in ENTRY_POINTS]
COUNTED = [e for e in ENTRY_POINTS if e[1]]
WITH_DAT = [e for e in ENTRY_POINTS if e[2] == "order"]


@pytest.fixture(scope="module")
def engines():
    from metmhn_amd import Engine
    pool = {dt: Engine(N_MUT, dtype=dt) for dt in ("f64", "f32")}
    yield pool
    for e in pool.values():
        e.close()


def last_error(e):
    return e.lib.mmhn_last_error().decode()


def refused(e, entry, count=1, null=()):
    """Calls the entry point of a table row on engine `e` with valid arguments of one row, except: the row count `count`, and a
    null pointer for every argument named in `null`.  Asserts status 1 and that no output buffer was written; returns the text."""
    name, _, _, _, spec = entry
    inputs = {"lt": np.zeros((NN, NN)), "o1": np.zeros(NN), "o2": np.zeros(NN),
              "dat": paired(N_MUT, [0], [1], 0)[None, :].copy(), "geno": np.array([[1, 0]], dtype=np.int8)}
    args, outs = [], []
    for a in spec:
        if isinstance(a, str) and a in inputs:
            args.append(None if a in null else inputs[a].ctypes.data_as(PTR[inputs[a].dtype]))
        elif a == "count":
            args.append(count)
        elif a == "ncols":
            args.append(2 * N_MUT + 3)
        elif isinstance(a, tuple):
            buf = np.full((1,) + a[2], SENTINEL[a[1]], dtype=a[1])
            outs.append(buf)
            args.append(buf.ctypes.data_as(PTR[a[1]]))
        else:
            args.append(a)
    status = getattr(e.lib, name)(e.h, *args)
    text = last_error(e)
    assert status == 1, f"{name}: status {status} ({text!r})"
    for buf in outs:
        assert (buf == SENTINEL[buf.dtype]).all(), f"{name}: an output buffer was written by a refused call"
    return text


# ---------------------------------------------------------------------------------------------------- the fp64-only entry points
@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=IDS)
def test_fp32_engine_is_refused(engines, entry):
    assert refused(engines["f32"], entry) == entry[3]


@pytest.mark.parametrize("count", [-1, 2 ** 31])
@pytest.mark.parametrize("entry", COUNTED, ids=[e[0] for e in COUNTED])
def test_row_count_out_of_range(engines, entry, count):
    assert refused(engines["f64"], entry, count=count) == f"{entry[1]} out of range"


@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=IDS)
def test_first_pointer_null(engines, entry):
    assert refused(engines["f64"], entry, null=("lt",)) == "null pointer"


@pytest.mark.parametrize("entry", WITH_DAT, ids=[e[0] for e in WITH_DAT])
def test_null_dat_with_a_row(engines, entry):
    assert refused(engines["f64"], entry, count=1, null=("dat",)) == "null dat"


@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=IDS)
def test_precedence_of_two_faults(engines, entry):
    """Two faults at once: the row count is checked before the engine's dtype everywhere; the order entry points check their
    pointers before the row count, the lattice ones the row count before their pointers."""
    name, count_name, family, _, _ = entry
    if count_name is None:                                      # (mmhn_cross_table has no count: pointers before the dtype)
        assert refused(engines["f32"], entry, null=("lt",)) == "null pointer"
        return
    assert refused(engines["f32"], entry, count=-1) == f"{count_name} out of range"
    want = "null pointer" if family == "order" else f"{count_name} out of range"
    assert refused(engines["f64"], entry, count=-1, null=("lt",)) == want


# ---------------------------------------------------------------------------------------------------- a null handle
def test_null_handle(engines):
    """One entry point of each family: cohort, primitive, order, lattice, sampler, counters."""
    lib = engines["f64"].lib
    z = np.zeros(64)
    p = z.ctypes.data_as(f64p)
    b = np.zeros(64, dtype=np.int8).ctypes.data_as(i8p)
    s = np.zeros(8, dtype=np.int32).ctypes.data_as(i32p)
    from metmhn_amd._lib import Counters
    calls = {
        "mmhn_cohort_sums": (p, p, p, 0, p),
        "mmhn_kronvec": (p, b, p, p, 1, 0),
        "mmhn_order_posteriors": (p, p, p, b, 1, 2 * N_MUT + 3, p, p, p, s),
        "mmhn_seeding_landscape": (p, p, 0, b, 1, p, s, None),
        "mmhn_simulate": (p, p, p, 1, 0, b, None),
        "mmhn_get_counters": (C.byref(Counters()),),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == 1, name
        assert lib.mmhn_last_error().decode() == "null handle", name
    assert (z == 0).all()


# ---------------------------------------------------------------------------------------------------- the split evaluation
def test_split_evaluation_error_order(engines):
    from metmhn_amd import synthetic
    e = engines["f64"]
    lt, dp, dm = synthetic.random_params(N_MUT)
    ptr = [np.ascontiguousarray(a).ctypes.data_as(f64p) for a in (lt, dp, dm)]
    e.set_cohort(np.array([paired(N_MUT, [0], [0, 1], 1), row(N_MUT, [1], [], 0, -99, 0), row(N_MUT, [], [0], 1, -99, 2)]))
    want = e.cohort_sums(lt, dp, dm)
    sums, wsums = np.zeros(4 + 2 * NN * NN + 3 * NN), np.full(1 + NN * NN + 2 * NN, SENTINEL[np.dtype(F64)])

    def pair_matches():
        sums[:] = SENTINEL[sums.dtype]
        assert e.lib.mmhn_cohort_sums_begin(e.h, *ptr, 1) == 0, last_error(e)
        assert e.lib.mmhn_cohort_sums_end(e.h, sums.ctypes.data_as(f64p)) == 0, last_error(e)
        np.testing.assert_array_equal(sums, want)

    assert e.lib.mmhn_cohort_sums_end(e.h, sums.ctypes.data_as(f64p)) == 1
    assert last_error(e) == "mmhn_cohort_sums_end without mmhn_cohort_sums_begin"
    pair_matches()

    assert e.lib.mmhn_cohort_sums_begin(e.h, *ptr, 1) == 0, last_error(e)
    assert e.lib.mmhn_cohort_wsums_end(e.h, wsums.ctypes.data_as(f64p)) == 1
    assert last_error(e) == "mmhn_cohort_sums_end / mmhn_cohort_wsums_end does not match the _begin call"
    assert (wsums == SENTINEL[wsums.dtype]).all()
    # (the refused _end left the evaluation pending: its own _end collects it)
    assert e.lib.mmhn_cohort_sums_end(e.h, sums.ctypes.data_as(f64p)) == 0, last_error(e)
    np.testing.assert_array_equal(sums, want)
    pair_matches()

    assert e.lib.mmhn_set_reduce_flag(e.h, float("nan")) == 1
    assert last_error(e) == "the flag must be finite"
    pair_matches()


# ---------------------------------------------------------------------------------------------------- zero log-theta
def test_rate_only_primitives_use_a_zero_log_theta():
    """The six primitives that take observation rates and no log-theta, at n_mut = 3 on a state of k = 3 active slots with the
    seeding, against their NumPy definitions (oracle/metmhn_oracle.py) at the bar of the golden cases (TIGHT)."""
    from metmhn_amd import Engine, synthetic
    from oracle import metmhn_oracle as O
    n = 3
    _, dp, dm = synthetic.random_params(n, seed=3)
    rng = np.random.default_rng(7)
    p, x = rng.normal(size=8), rng.normal(size=8)
    st = np.array([1, 0, 0, 1, 0, 0, 1], dtype=np.int8)         # joint: PT of event 0, MT of event 1, the seeding
    sv = np.array([1, 0, 1, 1], dtype=np.int8)                  # single tumour: events 0 and 2, the seeding
    with Engine(n) as e:
        close("diag_scal p", e.diag_scal(dp, st, p, 0), O.diag_scal_p(dp, st, p), *TIGHT)
        close("diag_scal m", e.diag_scal(dm, st, p, 1), O.diag_scal_m(dm, st, p), *TIGHT)
        for got, ref, nm in zip(e.x_partial_D_y(dp, dm, st, x, p), O.x_partial_D_y(dm, dp, st, x, p), ("dp", "dm")):
            close("x_partial_D_y " + nm, got, ref, *TIGHT)
        for i in range(n + 1):
            close(f"partial_diag_scal p {i}", e.partial_diag_scal(dp, st, p, i, 0), O.partial_diag_scal_p(dp, st, p, i), *TIGHT)
            close(f"partial_diag_scal m {i}", e.partial_diag_scal(dm, st, p, i, 1), O.partial_diag_scal_m(dm, st, p, i), *TIGHT)
        for got, ref, nm in zip(e.v_scal_d_pt(dp, dm, sv, p), O.v_scal_d_pt(dp, dm, sv, p), ("p", "m")):
            close("v_scal_d_pt " + nm, got, ref, *TIGHT)
        for i in range(n + 1):
            for got, ref, nm in zip(e.v_d_scal_d_pt(dp, dm, sv, p, i), O.v_d_scal_d_pt(dp, dm, sv, p, i), ("p", "m")):
                close(f"v_d_scal_d_pt {nm} {i}", got, ref, *TIGHT)
        for got, ref, nm in zip(e.v_x_partial_D_y(dp, dm, sv, x, p), O.v_x_partial_D_y(dp, dm, sv, x, p), ("dp", "dm")):
            close("v_x_partial_D_y " + nm, got, ref, *TIGHT)
