"""What the tests of the evaluation path share (set_cohort, patient_grads, cohort_sums, score_and_grad: test_gpu_parity.py,
test_parity_*.py, the window tests, test_limits.py, the reduction tests): the rows and cohorts they build, one evaluation on
an engine that never outlives it, the engine pools behind the module-scoped fixtures, and the comparisons with the bars that recur.  Imported by name
(`from eval_common import ...`); tests/ is on sys.path.  pytest does not rewrite the asserts of this module, so each carries
its message."""
import os
import socket

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("lp", "d_theta", "d_dp", "d_dm")

# ---------------------------------------------------------------------------------------------------- the bars that recur
NORTH_STAR = 1e-6                            # BASELINE.json north_star: fp64 likelihoods and gradients, relative
TIGHT = (1e-9, 1e-11)                        # (rtol, atol): what the fp64 kernels deliver on the small golden cases
FP32_BAR = (2e-3, 2e-5)                      # (rtol, atol) of every fp32 gradient component against fp64 (looser than 1e-6 by construction)
WINDOW_TOL = {"f64": 1e-12, "f32": 2e-4}     # two orders of the same sums, relative to the largest entry: rounding of the dtype times the terms of a row sum


# ---------------------------------------------------------------------------------------------------- rows
def row(n, pt, mt, seeding, order, typ):
    """One dat row of n events: the events `pt` in the primary tumour, `mt` in the metastasis, then seeding, order, type."""
    r = np.zeros(2 * n + 3, dtype=np.int8)
    for j in pt:
        r[2 * j] = 1
    for j in mt:
        r[2 * j + 1] = 1
    r[2 * n], r[2 * n + 1], r[2 * n + 2] = seeding, order, typ
    return r


def paired(n, pt, mt, order):
    """A paired row (type 3, seeded)."""
    return row(n, pt, mt, 1, order, 3)


def shape_rows(n, kr, kc, rows_p, count, seed, fixed=()):
    """`count` paired rows whose joint space has kr row-class and kc column-class bits (rows_p: the PT class is the rows),
    orders 0 / 1 / 2 in turn.  Per row the generator draws the row class, then the column class.  fixed = (row-class events,
    column-class events): every row carries them, and the drawn events lie below the smallest of them."""
    rng = np.random.default_rng(seed)
    fr, fc = (list(f) for f in fixed) if fixed else ([], [])
    below = min(fr + fc) if fixed else n
    out = []
    for i in range(count):
        a = np.concatenate((fr, rng.choice(below, size=kr - len(fr), replace=False))).astype(int)
        b = np.concatenate((fc, rng.choice(below, size=kc - len(fc), replace=False))).astype(int)
        pt, mt = (a, b) if rows_p else (b, a)
        out.append(paired(n, pt, mt, i % 3))
    return out


def _typed_row(bits, typ, order):
    """bits [2n] as a row of type `typ`: the slots the type does not read cleared, `order` on a paired row."""
    if typ in (0, 1):
        bits[1::2] = 0
        return np.concatenate((bits, [typ, -99, typ]))
    if typ == 2:
        bits[0::2] = 0
        return np.concatenate((bits, [1, -99, 2]))
    return np.concatenate((bits, [1, order(), 3]))


# The two generators below differ in what they draw: random_rows draws the type and the order code of every row from the
# generator and fills every slot at one density; top_rows deals types and order codes in turn (so nothing but the genotype is
# drawn), fills the slots of the events 27 .. 30 at the density and the others at 0.03, and keeps rows of at most 12 slots.
ORDER_CODES = [0, 1, 2, -99, 3]              # (3: an invalid order value on a paired row)


def random_rows(rng, n, count):
    """Rows of every type and order code, dense and sparse genotypes, empty and full rows."""
    rows = []
    for _ in range(count):
        dens = rng.choice([0.0, 0.15, 0.5, 0.85, 1.0])
        bits = (rng.random(2 * n) < dens).astype(np.int8)
        rows.append(_typed_row(bits, int(rng.integers(0, 4)), lambda: int(rng.choice(ORDER_CODES))))
    return rows


def top_rows(rng, count, n=31):
    """Rows of every type and order code with the slots biased to the events 27 .. 30 and k <= 12."""
    rows = []
    while len(rows) < count:
        dens = rng.choice([0.0, 0.15, 0.5, 0.85, 1.0])
        prob = np.full(2 * n, 0.03 * (dens > 0))
        prob[2 * 27:] = dens
        bits = (rng.random(2 * n) < prob).astype(np.int8)
        r = _typed_row(bits, len(rows) % 4, lambda: ORDER_CODES[(len(rows) // 4) % 5])
        if int(r[:2 * n + 1].sum()) <= 12:
            rows.append(r)
    return rows


# ---------------------------------------------------------------------------------------------------- engines
def _engine(*args, **kwargs):
    from metmhn_amd import Engine
    return Engine(*args, **kwargs)


def one_rank_comm(e):
    """In-library RCCL all-reduce with a one-rank communicator (what MMHN_FORCE_ALLREDUCE=1 attaches): the collective
    code path of the sharded engine on a single GPU."""
    from metmhn_amd.engine import unique_id
    e.comm_init(unique_id(), 0, 1)


def patient_grads(monkeypatch, n, dat, params, dtype="f64", workspace=None, counters=False, **env):
    """One evaluation on an engine of its own, created with the MMHN_* variables of `env` set through `monkeypatch` (None:
    unset) and closed before anything is compared: (lp, d_theta, d_dp, d_dm) of the cohort at params = (lt, dp, dm); with
    counters=True the pair (those, Engine.counters()).  The variables stay set until `monkeypatch` undoes them: pass
    `monkeypatch.context()`'s where the next engine must not see them."""
    for name, value in env.items():
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    with _engine(n, dtype=dtype, workspace_bytes=workspace) as e:
        e.set_cohort(dat)
        got = e.patient_grads(*params)
        return (got, e.counters()) if counters else got


def engine_pool(limit=4, poison=True):
    """Generator behind the `make_engine` fixtures: yields get(n, zerocopy=True, comm=False, dtype="f64", workspace=None, tag=0,
    fresh=False), which keeps at most `limit` engines alive (the least recently used is closed) and closes all of them at the
    end.  Engines are created under MMHN_POISON=1 (poison) and, with zerocopy=False, MMHN_ZEROCOPY=0; comm=True attaches a
    one-rank communicator; fresh=True closes the engine of the key and creates it anew; tag tells engines of one shape apart."""
    live = {}

    def get(n, zerocopy=True, comm=False, dtype="f64", workspace=None, tag=0, fresh=False):
        key = (n, zerocopy, comm, dtype, workspace, tag)
        if fresh and key in live:
            live.pop(key).close()
        if key not in live:
            while len(live) >= limit:
                live.pop(next(iter(live))).close()
            with pytest.MonkeyPatch.context() as mp:
                if poison:
                    mp.setenv("MMHN_POISON", "1")
                if zerocopy:
                    mp.delenv("MMHN_ZEROCOPY", raising=False)
                else:
                    mp.setenv("MMHN_ZEROCOPY", "0")
                e = _engine(n, dtype=dtype, workspace_bytes=workspace)
            if comm:
                one_rank_comm(e)
            live[key] = e
        live[key] = live.pop(key)                             # (most recently used last: a test's own engines are never the oldest)
        return live[key]
    try:
        yield get
    finally:
        for e in live.values():
            e.close()


def engines_by_n():
    """Generator behind the `engines` fixtures: yields get(n), one default engine per event count, all closed at the end."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _engine(n)
        return cache[n]
    try:
        yield get
    finally:
        for e in cache.values():
            e.close()


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------- comparisons
def close(tag, got, ref, rtol, atol=0.0):
    """numpy's assert_allclose bar |got - ref| <= atol + rtol |ref| on arrays of one shape, `got` finite; the worst ratio to
    the bar and its position are printed first."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{tag}: shape {got.shape} against {ref.shape}"
    assert np.isfinite(got).all(), f"{tag}: {int((~np.isfinite(got)).sum())} non-finite entries"
    bar = atol + rtol * np.abs(ref)
    err = np.abs(got - ref)
    ratio = np.where(err == 0.0, 0.0, err / np.where(bar > 0, bar, np.finfo(float).tiny))
    i = tuple(int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape)) if ratio.size else ()
    print(f"[close] {tag}: worst error / bar = {ratio.max(initial=0.0):.3g}" + (f" at {i}: {float(got[i])!r} against {float(ref[i])!r}" if ratio.size else ""))
    assert (err <= bar).all(), f"{tag}: {int((~(err <= bar)).sum())} of {err.size} entries over the bar, worst ratio {ratio.max():.3g} at {i}"


def close_grads(tag, got, ref, lp, grads):
    """(lp, d_theta, d_dp, d_dm) against a reference: lp = (rtol, atol) for the first array, grads = (rtol, atol) for the others"""
    assert len(got) == len(ref) == 4, f"{tag}: {len(got)} arrays against {len(ref)}"
    for x, y, nm, bar in zip(got, ref, NAMES, (lp, grads, grads, grads)):
        close(f"{tag} {nm}", x, y, *bar)


def close_to_largest(tag, got, ref, rtol):
    """Each of the four arrays within rtol of its reference, relative and of the reference's largest entry: two orders of the
    same sums (WINDOW_TOL)."""
    assert len(got) == len(ref) == 4, f"{tag}: {len(got)} arrays against {len(ref)}"
    for x, y, nm in zip(got, ref, NAMES):
        close(f"{tag} {nm}", x, y, rtol, rtol * np.abs(y).max())


def window_against(monkeypatch, n, dat, other, dtype, tag):
    """The window route (MMHN_WSOLVE=1) against MMHN_WSOLVE=`other` (0: the tile route, 2: the same solves converted to index
    order) on one cohort at synthetic.random_params(n), buffers NaN-poisoned, at WINDOW_TOL; the two results."""
    from metmhn_amd import synthetic
    params = synthetic.random_params(n)
    monkeypatch.setenv("MMHN_PSOLVE_MIN", "1")          # (also the window route's minimum: a few patients take it)
    monkeypatch.setenv("MMHN_POISON", "1")
    win = patient_grads(monkeypatch, n, dat, params, dtype=dtype, MMHN_WSOLVE="1")
    ref = patient_grads(monkeypatch, n, dat, params, dtype=dtype, MMHN_WSOLVE=other)
    close_to_largest(tag, win, ref, WINDOW_TOL[dtype])
    return win, ref


def fp32_close(tag, x32, x64):
    """Every component of an fp32 gradient against fp64 at FP32_BAR."""
    close(f"fp32 {tag}", x32, x64, *FP32_BAR)


def fp32_grads(tag, got32, ref64, lp_rtol=1e-4, lp_atol=0.0):
    """The fp32 bar of a per-patient result: log-probabilities 1e-4 relative, every gradient component at FP32_BAR."""
    close_grads(f"fp32 {tag}", got32, ref64, (lp_rtol, lp_atol), FP32_BAR)
