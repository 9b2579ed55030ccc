"""The cohort reduction (csrc/assemble.h: k_reduce_rows, k_reduce_parts, k_reduce_parts_pack, k_pack_sums / k_pack_wsums), both
packed layouts of include/metmhn_amd.h and the reduce flag behind the pre-combined one, with the host code that moves them
(Engine::cohort_sums_begin / _end).

Reference of a cohort buffer: the engine's own per-patient rows (Engine.patient_grads: a separate download of the same rows,
through none of the four kernels), summed per class with math.fsum (correctly rounded) and laid out as the header documents.

Bound per element: plain recursive summation.  With u = 2^-53, a class of P_cls rows and S = sum over its rows of |v|,
any order of adding the rows - any chunking, any number of batches - is a summation tree with at most P_cls - 1 inexact
additions on the path of a row (adding to a zero accumulator is exact), so the computed sum is within (P_cls - 1) u S of the
true one; the reference adds one rounding (u |sum| <= u S).  Raw buffer: |got - ref| <= (P_cls + 2) u S.  Pre-combined
buffer: the product with w and the addition of the two classes round once each on the device and once each in the float64
reference: |got - ref| <= (P + 4) u (|w| S_EM + S_NM).  (The d_dm block has no NM part, there the bound is (P + 4) u |w|
S_EM.)  Where S = 0 the bound is 0 and the comparison exact, as it is for the two counts.

The bound presupposes that two patient_grads calls return the same bits; the GPU tests assert that first, and add the spread
between the two calls, summed over the rows, to the bound (0 when the precondition holds)."""
import os

import numpy as np
import pytest

import reduction_common as RC
from eval_common import engine_pool, free_port
from reduction_common import (MULTI_BATCH, MULTI_BATCH_WS, PERC_MET, Reference, U, check_raw, check_wsums, raw_layout, raw_len, red_per, stride,
                              wsums_layout)

W = 0.37


# ---- the kernels' order of additions, in float64 NumPy ------------------------------------------------------------------

DEFECTS = ("drop_last_row", "zero_row_em", "dm_weighted", "shift", "flag_slot")


def replay(rows, kinds, batches, N, mode, a, b, defect=None, before=None):
    """What the device writes for a cohort of rows [P, st] with planner kinds [P] (0 .. 4) cut into consecutive `batches`
    (row counts): per batch chunks of red_per(rows of the batch) consecutive rows added in index order (k_reduce_rows), the
    chunk sums in chunk order (k_reduce_parts / k_reduce_parts_pack), the batches in order, the pack of the last (mode 1:
    a = n_em, b = n_pat, 4 + 2 N^2 + 3 N doubles; mode 2: a = w, b = the flag, 1 + N^2 + 2 N doubles and the flag's slot).
    before: what the destination held (default NaN).  defect: one of DEFECTS, a kernel that is wrong in that way."""
    assert defect is None or defect in DEFECTS
    st, NN = stride(N), N * N
    assert sum(batches) == rows.shape[0] and all(nb > 0 for nb in batches)
    sums = np.zeros((2, st))
    r0 = 0
    for npat in batches:
        per = red_per(npat)
        acc = np.zeros((2, st))
        for c in range((npat + per - 1) // per):
            i0, i1 = r0 + c * per, r0 + min(npat, (c + 1) * per)
            if defect == "drop_last_row":
                i1 -= 1
            part = np.zeros((2, st))
            for i in range(i0, i1):
                nm = kinds[i] == 0 or (kinds[i] == 4 and defect != "zero_row_em")
                part[1 if nm else 0] += rows[i]
            acc += part
        sums += acc
        r0 += npat
    em, nm = sums
    if mode == 1:
        packed = raw_layout(em, nm, a, b, N)
    else:
        packed = a * em + nm if defect == "dm_weighted" else wsums_layout(em, nm, a, N)
    size = len(packed) + (1 if mode == 2 else 0)
    o = np.full(size, np.nan) if before is None else np.array(before, dtype=np.float64)
    assert o.shape == (size,)
    if defect == "shift":
        o[1:len(packed)] = packed[:-1]
    else:
        o[:len(packed)] = packed
    if mode == 2:
        if defect == "flag_slot":
            o[st - 1] = b
        else:
            o[st] = b
    return o


# ---- the shapes ------------------------------------------------------------------------------------------------------------
# P: 32 is red_per's floor; 4096 -> 4097 takes it from 32 to 33, and the last chunk of 4097 rows holds 5.  n: the row has
# (N + 1)^2 doubles with N = n + 1: 36 at n = 4, 256 at n = 14 (one workgroup of k_reduce_parts_pack: the flag's slot is the first
# element past it), 289 at n = 15 (one workgroup and 33 threads).
SHAPES = [(4, P, "mixed") for P in (0, 1, 31, 32, 33, 4096, 4097)] + [(4, 33, "all_nm"), (4, 33, "all_em")] + \
         [(n, P, "mixed") for n in (14, 15) for P in (0, 33, 4097)]
SHAPE_IDS = [f"n{n}-P{P}-{kind}" for n, P, kind in SHAPES]


def _random_rows(N, P, kind, seed):
    """Signed rows over six decades with planner kinds; the NM rows' d_dm is not zero here, so that a pack that adds it shows."""
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((P, stride(N))) * 10.0 ** rng.uniform(-3, 3, size=(P, stride(N)))
    if kind == "all_nm":
        kinds = rng.choice([0, 4], size=P)
    elif kind == "all_em":
        kinds = rng.integers(1, 4, size=P)
    else:
        kinds = rng.integers(0, 5, size=P)
    if P >= 4 and kind != "all_em":
        kinds[[P - 1, min(red_per(P), P) - 2]] = 4            # all-zero rows at a chunk's end and before it
    return rows, kinds


def _replay_case(N, P, kind, batches, defect=None, seed=0):
    """Both layouts of one replayed cohort through the checks of the GPU tests; the worst error / bound of the two."""
    rows, kinds = _random_rows(N, P, kind, seed)
    n_seed = float(((kinds >= 1) & (kinds <= 3)).sum())
    ref = Reference(rows, (kinds == 0) | (kinds == 4), n_seed, N)
    good1 = replay(rows, kinds, batches, N, 1, n_seed, float(P))
    good2 = replay(rows, kinds, batches, N, 2, W, 3.0)
    before1, before2 = (good1, good2) if defect == "shift" else (None, None)     # (a destination that still holds the last result)
    r1 = check_raw(replay(rows, kinds, batches, N, 1, n_seed, float(P), defect, before1), ref)
    r2 = check_wsums(replay(rows, kinds, batches, N, 2, W, 3.0, defect, before2), ref, W, 3.0)
    return max(r1, r2)


@pytest.mark.parametrize("n,P,kind", SHAPES, ids=SHAPE_IDS)
def test_replayed_kernel_order_is_within_the_bound(n, P, kind):
    """The reference and the bound alone: the additions in the kernels' order, in float64, pass at every shape of the GPU tests."""
    ratio = _replay_case(n + 1, P, kind, [P] if P else [], seed=100 + P)
    print(f"replay n={n} P={P} {kind}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("batches", ([1400, 1400, 1297], [33, 4000, 64], [1] * 5 + [4092]), ids=("thirds", "uneven", "single_rows"))
def test_replayed_batches_are_within_the_bound(batches):
    n, P = MULTI_BATCH
    assert sum(batches) == P
    assert _replay_case(n + 1, P, "mixed", batches, seed=7) <= 1.0


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("n,P", ((4, 33), (4, 4097), (14, 33), (15, 4097)))
def test_injected_defects_break_the_bound(n, P, defect):
    """A reduction that is wrong in one of five small ways does not pass the checks the GPU tests apply."""
    assert _replay_case(n + 1, P, "mixed", [P], seed=5) <= 1.0
    with pytest.raises(AssertionError):
        _replay_case(n + 1, P, "mixed", [P], defect=defect, seed=5)


def test_layouts_and_chunk_sizes():
    """The helpers themselves: red_per at the edges the GPU cases sit on, and the two layouts on a row of distinct numbers."""
    assert [red_per(P) for P in (0, 1, 32, 33, 4096, 4097, 4224, 4225)] == [32, 32, 32, 32, 32, 33, 33, 34]
    assert (4097 + 32) // 33 == 125 and 4097 - 124 * 33 == 5
    assert [stride(n + 1) for n in (4, 14, 15)] == [36, 256, 289]
    N = 2
    em, nm = np.arange(1.0, 10.0), np.arange(11.0, 20.0)      # [lp, G (4), d_dp (2), d_dm (2)]
    np.testing.assert_array_equal(raw_layout(em, nm, 7.0, 9.0, N),
                                  [1, 11, 7, 9, 2, 3, 4, 5, 12, 13, 14, 15, 6, 7, 16, 17, 8, 9])
    np.testing.assert_array_equal(wsums_layout(em, nm, 2.0, N), [13, 16, 19, 22, 25, 28, 31, 16, 18])
    assert len(raw_layout(em, nm, 0, 0, N)) == raw_len(N)


# ---- GPU: cohorts -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def make_engine():
    yield from engine_pool()


def _references(e, dat, lt, dp, dm):
    """(reference of a gradient evaluation, reference of a score-only one, did two downloads agree bit for bit)."""
    nm_rows = dat[:, -1] == 0
    n_seed = float(dat[:, -3].sum())
    r1, r2 = RC.rows_of(e, lt, dp, dm), RC.rows_of(e, lt, dp, dm)
    s1, s2 = RC.rows_of(e, lt, dp, dm, False), RC.rows_of(e, lt, dp, dm, False)
    same = np.array_equal(r1, r2) and np.array_equal(s1, s2)
    assert np.isfinite(r1).all() and np.isfinite(s1).all()
    assert not r1[nm_rows][:, 1 + e.N * e.N + e.N:].any(), "a type-0 row has a d_dm entry: the raw layout has no slot for it"
    return (Reference(r1, nm_rows, n_seed, e.N, np.abs(r1 - r2)), Reference(s1, nm_rows, n_seed, e.N, np.abs(s1 - s2)), same)


def _wsums(e, lt, dp, dm, w, with_grad=True, flag=None):
    """One weighted evaluation: the buffer with the summed flag appended as its last element."""
    e.cohort_wsums_begin(lt, dp, dm, w, with_grad=with_grad, flag=flag)
    ws = e.cohort_wsums_end()
    return np.append(ws, e.reduce_flag)


def _close(a, b, what):
    """8 u relative per element plus 8 u of the block's largest entry; NaN (the objective of an empty cohort, 0 / 0) matches NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what
    if nan.all():
        return
    tol = 8 * U * np.abs(b) + 8 * U * np.abs(b[~nan]).max()
    assert (np.abs(a - b)[~nan] <= tol[~nan]).all(), f"{what}: {np.abs(a - b)[~nan].max():.3e}"


def _evaluate_and_check(e, dat, lt, dp, dm, tag):
    """Both layouts of engine `e` against its own rows, with and without gradients; (sums, wsums + flag, worst ratios, precondition)."""
    ref, ref0, same = _references(e, dat, lt, dp, dm)
    assert same, f"{tag}: two patient_grads calls differ - the bound presupposes reproducible rows"
    s = e.cohort_sums(lt, dp, dm)
    ratio_raw = check_raw(s, ref, tag + " cohort_sums")
    s0 = e.cohort_sums(lt, dp, dm, with_grad=False)           # straight after a gradient evaluation
    check_raw(s0, ref0, tag + " cohort_sums(with_grad=False)")
    assert not s0[4:].any(), f"{tag}: gradient entries of a score-only evaluation"
    ws = _wsums(e, lt, dp, dm, W)
    ratio_w = check_wsums(ws, ref, W, 0.0, tag + " cohort_wsums")
    ws0 = _wsums(e, lt, dp, dm, W, with_grad=False)
    check_wsums(ws0, ref0, W, 0.0, tag + " cohort_wsums(with_grad=False)")
    assert not ws0[1:].any(), f"{tag}: gradient entries of a score-only weighted evaluation"
    print(f"{tag}: worst error / bound: raw {ratio_raw:.3f}, pre-combined {ratio_w:.3f}; rows reproducible: {same}")
    return s, ws, s0, ws0


@pytest.mark.gpu
@pytest.mark.parametrize("n,P,kind", SHAPES, ids=SHAPE_IDS)
def test_reduction_edges(make_engine, n, P, kind):
    """Both buffers at the chunk edges and at row lengths around one workgroup of the packing kernel: within the bound of their own
    rows, zero gradients in a score-only evaluation, and the same bits from the two-call form, a second evaluation,
    MMHN_ZEROCOPY=0 and an attached one-rank communicator; the ABI's own combination against distributed.py's."""
    from metmhn_amd import distributed as D
    N = n + 1
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, P, kind)
    engines = {"default": make_engine(n), "zerocopy0": make_engine(n, zerocopy=False), "comm": make_engine(n, comm=True)}
    if P == 0:                                                # the handle held 33 rows and an evaluation of them before
        for e in engines.values():
            e.set_cohort(RC.cohort(n, 33))
            assert e.cohort_sums(lt, dp, dm)[3] == 33.0 and np.isfinite(_wsums(e, lt, dp, dm, W)).all()
    for e in engines.values():
        e.set_cohort(dat)
    e = engines["default"]
    tag = f"n={n} P={P} {kind}"
    s, ws, s0, ws0 = _evaluate_and_check(e, dat, lt, dp, dm, tag)
    if P == 0:
        assert not s.any() and not ws.any() and not s0.any() and not ws0.any()
    assert s[2] == float(dat[:, -3].sum()) and s[3] == float(P)
    # the same bits: two-call form, second evaluation, the copy-engine path, the all-reduce of one rank
    e.cohort_sums_begin(lt, dp, dm)
    np.testing.assert_array_equal(e.cohort_sums_end(), s)
    np.testing.assert_array_equal(e.cohort_sums(lt, dp, dm), s)
    np.testing.assert_array_equal(_wsums(e, lt, dp, dm, W), ws)
    for name in ("zerocopy0", "comm"):
        x = engines[name]
        np.testing.assert_array_equal(x.cohort_sums(lt, dp, dm), s, err_msg=name)
        np.testing.assert_array_equal(x.cohort_sums(lt, dp, dm, with_grad=False), s0, err_msg=name)
        np.testing.assert_array_equal(_wsums(x, lt, dp, dm, W), ws, err_msg=name)
        np.testing.assert_array_equal(_wsums(x, lt, dp, dm, W, with_grad=False), ws0, err_msg=name)
        x.cohort_sums_begin(lt, dp, dm)
        np.testing.assert_array_equal(x.cohort_sums_end(), s, err_msg=name)
    # mmhn_score_and_grad against the two Python combinations
    with np.errstate(all="ignore"):
        got = e.score_and_grad(lt, dp, dm, PERC_MET)
        via_sums = D.combine_sums(s, N, PERC_MET)
        w, n_full = D.em_weight(s[2], s[3], PERC_MET)
        via_wsums = D.split_wsums(_wsums(e, lt, dp, dm, w)[:-1], N, n_full)
    for name, a, b, c in zip(("score", "d_theta", "d_dp", "d_dm"), got, via_sums, via_wsums):
        _close(b, a, f"{tag} combine_sums {name}")
        _close(c, a, f"{tag} split_wsums {name}")


@pytest.mark.gpu
def test_empty_cohort_on_a_fresh_engine(make_engine):
    """k_pack_sums / k_pack_wsums on a handle that never held a row: zeros, zero counts, the flag behind the buffer."""
    n = 4
    lt, dp, dm = RC.params(n)
    e = make_engine(n, fresh=True)
    e.set_cohort(RC.cohort(n, 0))
    for grad in (True, False):
        assert not e.cohort_sums(lt, dp, dm, with_grad=grad).any()
        ws = _wsums(e, lt, dp, dm, W, with_grad=grad, flag=2.0)
        assert not ws[:-1].any() and ws[-1] == 2.0


@pytest.mark.gpu
def test_multi_batch_reduction(make_engine):
    """4 097 rows under the smallest workspace limit the library takes, 1 MiB (k_reduce_parts on every batch but the last).
    The engine does not report its batch count, so the least it can be follows from plan.h: footprint() charges every row
    (stride + 1) doubles of results and two T of dots, and every row that is not all-zero has at least one single-tumour
    problem: N^2 + 65 T of results and four vectors of at least one state.  split_into_batches closes a batch of several
    rows before its footprint passes the limit, so the batches are at least the sum of these charges over the limit."""
    n, P = MULTI_BATCH
    N = n + 1
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, P)
    all_zero = (dat[:, -1] == 0) & (dat[:, 0:2 * n + 1:2].sum(axis=1) == 0)
    charged = P * ((stride(N) + 1) * 8 + 2 * 8) + int((~all_zero).sum()) * ((N * N + 65) * 8 + 4 * 8)
    assert -(-charged // MULTI_BATCH_WS) >= 3
    e = make_engine(n, workspace=MULTI_BATCH_WS)
    e.set_cohort(dat)
    s, ws, _, _ = _evaluate_and_check(e, dat, lt, dp, dm, f"n={n} P={P} multi-batch")
    one = make_engine(n)                                      # one batch: another tree over the same rows
    one.set_cohort(dat)
    ref = Reference(RC.rows_of(one, lt, dp, dm), dat[:, -1] == 0, float(dat[:, -3].sum()), n + 1)
    check_raw(s, ref, "multi-batch sums against the one-batch engine's rows")
    check_wsums(ws, ref, W, 0.0, "multi-batch wsums against the one-batch engine's rows")


@pytest.mark.gpu
@pytest.mark.parametrize("P", (33, 4097))
def test_fp32_engine_reduction(make_engine, P):
    """The rows and the reduction are double in the fp32 engine too: the same bound against its own rows."""
    n = 4
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, P)
    e = make_engine(n, dtype="f32")
    e.set_cohort(dat)
    _evaluate_and_check(e, dat, lt, dp, dm, f"n={n} P={P} fp32")


# ---- GPU: the reduce flag ----------------------------------------------------------------------------------------------------

FLAG_RUNS = [(4, True, False), (4, False, False), (4, True, True), (4, False, True), (14, False, True)]
FLAG_IDS = [f"n{n}-{'zerocopy' if zc else 'zerocopy0'}-{'comm' if comm else 'nocomm'}" for n, zc, comm in FLAG_RUNS]


def _get_flag(e):
    import ctypes as C
    from metmhn_amd import _lib
    out = C.c_double(-1.0)
    _lib.check(e.lib.mmhn_get_reduce_flag(e.h, C.byref(out)))
    return out.value


def _set_flag(e, value):
    from metmhn_amd import _lib
    _lib.check(e.lib.mmhn_set_reduce_flag(e.h, float(value)))


@pytest.mark.gpu
@pytest.mark.parametrize("n,zerocopy,comm", FLAG_RUNS, ids=FLAG_IDS)
def test_reduce_flag_rides_behind_the_weighted_buffer(make_engine, n, zerocopy, comm):
    """mmhn_set_reduce_flag / mmhn_get_reduce_flag: the value comes back from the weighted evaluation it was set for and from
    no other, leaves the buffer as it was, and a plain evaluation reads 0."""
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, 33)
    e = make_engine(n, zerocopy=zerocopy, comm=comm)
    e.set_cohort(dat)
    plain = _wsums(e, lt, dp, dm, W)
    assert plain[-1] == 0.0
    flagged = _wsums(e, lt, dp, dm, W, flag=3.0)
    assert flagged[-1] == 3.0
    np.testing.assert_array_equal(flagged[:-1], plain[:-1])
    assert _wsums(e, lt, dp, dm, W)[-1] == 0.0                # the next one without a flag
    assert _wsums(e, lt, dp, dm, W, flag=-2.5)[-1] == -2.5
    assert _wsums(e, lt, dp, dm, W, flag=0.0)[-1] == 0.0
    score_only = _wsums(e, lt, dp, dm, W, with_grad=False, flag=7.0)
    assert score_only[-1] == 7.0 and np.isfinite(score_only[0]) and not score_only[1:-1].any()
    assert _get_flag(e) == 7.0
    e.cohort_sums_begin(lt, dp, dm)
    e.cohort_sums_end()
    assert _get_flag(e) == 0.0                                # a plain evaluation has no flag
    e.set_cohort(RC.cohort(n, 0))                               # k_pack_wsums
    empty = _wsums(e, lt, dp, dm, W, flag=4.0)
    assert empty[-1] == 4.0 and not empty[:-1].any()
    assert _wsums(e, lt, dp, dm, W)[-1] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n,zerocopy,comm", FLAG_RUNS, ids=FLAG_IDS)
def test_reduce_flag_waits_for_the_next_weighted_evaluation(make_engine, n, zerocopy, comm):
    """include/metmhn_amd.h: the value "travels with the NEXT mmhn_cohort_wsums_begin" - a plain mmhn_cohort_sums and a
    mmhn_patient_grads in between, and a _begin refused while an evaluation is pending, leave it where it is."""
    lt, dp, dm = RC.params(n)
    dat = RC.cohort(n, 33)
    e = make_engine(n, zerocopy=zerocopy, comm=comm)
    e.set_cohort(dat)
    plain = _wsums(e, lt, dp, dm, W)
    _set_flag(e, 5.0)
    sums = e.cohort_sums(lt, dp, dm)
    assert _get_flag(e) == 0.0
    e.patient_grads(lt, dp, dm)
    got = _wsums(e, lt, dp, dm, W)
    assert got[-1] == 5.0
    np.testing.assert_array_equal(got[:-1], plain[:-1])
    assert _wsums(e, lt, dp, dm, W)[-1] == 0.0                # consumed: the evaluation after that reads 0
    # a call refused on the host before anything is issued is not the next weighted evaluation
    e.cohort_sums_begin(lt, dp, dm)
    with pytest.raises(RuntimeError):
        e.cohort_wsums_begin(lt, dp, dm, W, flag=6.0)
    np.testing.assert_array_equal(e.cohort_sums_end(), sums)
    assert _wsums(e, lt, dp, dm, W)[-1] == 6.0
    assert _wsums(e, lt, dp, dm, W)[-1] == 0.0


# ---- GPU: a stale cohort on one of two ranks --------------------------------------------------------------------------------

STALE_N, STALE_ROWS, STALE_SEED = 6, 300, 11


def _stale_edit(dat):
    """The in-place edit of the two-rank test: the first paired row becomes an all-zero type-0 row (the global counts change too)."""
    r = int(np.flatnonzero(dat[:, -1] == 3)[0])
    dat[r] = 0
    dat[r, -2] = -99
    return dat


def _stale_worker(rank, world, port, q, reduce_mode, stale_ranks):
    """One rank: evaluate, edit the array in place, keep the guard of the ranks outside `stale_ranks` silent, evaluate again."""
    import sys
    import traceback
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        if reduce_mode:
            os.environ["MMHN_REDUCE"] = reduce_mode
        else:
            os.environ.pop("MMHN_REDUCE", None)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import metmhn_amd.regularized_optimization as ro
        from metmhn_amd import synthetic
        ro.configure(device=0)
        lt, dp, dm = synthetic.random_params(STALE_N)
        dat = synthetic.mixed_cohort(STALE_N, STALE_ROWS, seed=STALE_SEED)
        before = [np.asarray(r) for r in ro.score_and_grad(lt, dp, dm, dat, PERC_MET)]
        _stale_edit(dat)
        eng = ro._engine_for(dat, check=False)
        assert eng._sharded and eng.world_size_hint == world and 0 < eng.n_pat < STALE_ROWS
        if rank not in stale_ranks:
            eng._sample_crc = ro._sample_crc(dat)             # this rank's guard stays silent
        calls = []
        load_rows = ro._load_rows

        def counting(*args, **kwargs):
            calls.append(args[0] is eng)
            return load_rows(*args, **kwargs)
        ro._load_rows = counting
        try:
            after = [np.asarray(r) for r in ro.score_and_grad(lt, dp, dm, dat, PERC_MET)]
        finally:
            ro._load_rows = load_rows
        q.put((rank, calls, before, after))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:                                         # noqa: BLE001 (the parent fails with this text instead of waiting)
        q.put((rank, "error", traceback.format_exc(), None))


@pytest.fixture(scope="module")
def stale_expected():
    """One process, no sharding: the result before the edit and on a copy of the edited array."""
    import metmhn_amd.regularized_optimization as ro
    from metmhn_amd import synthetic
    lt, dp, dm = synthetic.random_params(STALE_N)
    dat = synthetic.mixed_cohort(STALE_N, STALE_ROWS, seed=STALE_SEED)
    edited = _stale_edit(dat.copy())
    assert not np.array_equal(dat, edited)
    before = [np.asarray(r) for r in ro.score_and_grad(lt, dp, dm, dat, PERC_MET)]
    after = [np.asarray(r) for r in ro.score_and_grad(lt, dp, dm, edited, PERC_MET)]
    ro.invalidate(dat)
    ro.invalidate(edited)
    assert abs(before[0] - after[0]) > 1e-6
    return before, after


@pytest.mark.gpu
@pytest.mark.parametrize("reduce_mode,stale_ranks", (("", (1,)), ("host_fixed_order", (1,)), ("", (0, 1))),
                         ids=("default-rank1", "host_fixed_order-rank1", "default-both"))
def test_stale_cohort_on_one_of_two_ranks(stale_expected, reduce_mode, stale_ranks):
    """regularized_optimization._result with two ranks (gloo, both engines on device 0): the "edited in place" bit of one rank
    (or of both: the sum is 2) crosses in the evaluation's own all-reduce, both ranks rebuild their shard once and return
    the edited cohort's value."""
    import torch.multiprocessing as mp
    port = free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stale_worker, args=(r, 2, port, q, reduce_mode, stale_ranks)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=180) for _ in range(2)]
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():                                  # (a rank waiting in a collective ends the test, not the run)
                p.terminate()
                p.join(timeout=10)
    for rank, calls, before, after in got:
        assert calls != "error", f"rank {rank}:\n{before}"
    assert all(p.exitcode == 0 for p in procs)
    assert sorted(r[0] for r in got) == [0, 1]
    want_before, want_after = stale_expected
    for rank, calls, before, after in got:
        assert calls == [True], f"rank {rank} rebuilt {len(calls)} times"
        for b, a, wb, wa in zip(before, after, want_before, want_after):
            np.testing.assert_allclose(b, wb, rtol=1e-12, atol=1e-12, err_msg=f"rank {rank} before the edit")
            np.testing.assert_allclose(a, wa, rtol=1e-12, atol=1e-12, err_msg=f"rank {rank} after the edit")
        assert abs(after[0] - before[0]) > 1e-6 and not np.allclose(after[1], before[1], rtol=1e-9, atol=1e-12)
