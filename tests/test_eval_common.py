"""The helpers of tests/eval_common.py themselves, on the CPU: the comparisons at and around their bar, the row builders
against rows written out, and the engine pool and the one-evaluation helper with a stand-in engine (no GPU, no library)."""
import os

import numpy as np
import pytest

import eval_common as EC


# ---------------------------------------------------------------------------------------------------- comparisons
def test_close_at_and_over_the_bar():
    ref = np.array([[1.0, -2.0, 0.0], [4.0, 8.0, 16.0]])
    got = ref.copy()
    got[1, 1] = 8.0 + (0.5 + 0.25 * 8.0)                     # exactly atol + rtol |ref|: every term is a binary fraction
    EC.close("on the bar", got, ref, 0.25, 0.5)
    got[1, 1] = np.nextafter(got[1, 1], np.inf)
    with pytest.raises(AssertionError, match=r"just over: 1 of 6 entries over the bar.* at \(1, 1\)"):
        EC.close("just over", got, ref, 0.25, 0.5)
    got[1, 1] = np.nan
    with pytest.raises(AssertionError, match="a NaN: 1 non-finite"):
        EC.close("a NaN", got, ref, 0.25, 0.5)
    with pytest.raises(AssertionError, match=r"shapes: shape \(3,\) against \(2, 3\)"):
        EC.close("shapes", ref[0], ref, 0.25, 0.5)
    EC.close("scalars", 1.0, np.float64(1.0), 0.0)
    EC.close("empty", np.zeros((0, 3)), np.zeros((0, 3)), 0.0)
    with pytest.raises(AssertionError, match="zero bar"):
        EC.close("zero bar", [0.0, 1e-300], [0.0, 0.0], 1.0)


def test_close_grads_pairs_the_bars():
    ref = (np.array([1.0, 2.0]), np.ones((2, 3, 3)), np.ones((2, 3)), np.ones((2, 3)))
    got = (ref[0] * (1 + 1e-3), ref[1] * (1 + 1e-6), ref[2] * (1 + 1e-6), ref[3] + 1e-6)
    EC.close_grads("lp loose, gradients tight", got, ref, lp=(2e-3, 0.0), grads=(2e-6, 0.0))
    with pytest.raises(AssertionError, match="swapped lp:"):
        EC.close_grads("swapped", got, ref, lp=(2e-6, 0.0), grads=(2e-3, 0.0))
    for k in (1, 2, 3):                                      # each gradient array is held to the tight pair
        bad = list(got)
        bad[k] = ref[k] * (1 + 1e-4)
        with pytest.raises(AssertionError, match=f"array {k} {EC.NAMES[k]}:"):
            EC.close_grads(f"array {k}", bad, ref, lp=(2e-3, 0.0), grads=(2e-6, 0.0))
    with pytest.raises(AssertionError, match="three: 3 arrays"):
        EC.close_grads("three", got[:3], ref, lp=(1, 0), grads=(1, 0))


def test_fp32_and_window_bars():
    x = np.array([1.0, 0.0, -3.0])
    EC.fp32_close("on the bar", x + np.array([2e-3 + 2e-5, 2e-5, 0.0]) * (1 - 1e-12), x)
    with pytest.raises(AssertionError, match="fp32 over"):
        EC.fp32_close("over", x + np.array([0.0, 2.1e-5, 0.0]), x)
    four = [np.array([1.0, 100.0])] * 4
    EC.close_to_largest("of the largest", [a + np.array([9e-11, 0.0]) for a in four], four, 1e-12)    # 1e-12 * 100 carries the small entry
    with pytest.raises(AssertionError, match="too far d_dm"):
        EC.close_to_largest("too far", four[:3] + [four[3] + np.array([2.1e-10, 0.0])], four, 1e-12)
    assert EC.TIGHT == (1e-9, 1e-11) and EC.FP32_BAR == (2e-3, 2e-5) and EC.NORTH_STAR == 1e-6 and EC.WINDOW_TOL == {"f64": 1e-12, "f32": 2e-4}


# ---------------------------------------------------------------------------------------------------- rows
def test_rows_written_out():
    #                                  PT0 MT0 PT1 MT1 seeding order type
    assert EC.row(2, [0], [1], 1, 2, 3).tolist() == [1, 0, 0, 1, 1, 2, 3]
    assert EC.row(2, [0, 1], [], 0, -99, 0).tolist() == [1, 0, 1, 0, 0, -99, 0]
    assert EC.row(2, [], [0], 1, -99, 2).tolist() == [0, 1, 0, 0, 1, -99, 2]
    assert EC.paired(2, [1], [0, 1], 0).tolist() == [0, 1, 1, 1, 1, 0, 3]
    assert EC.paired(2, range(2), np.array([1]), 1).tolist() == [1, 0, 1, 1, 1, 1, 3]
    assert EC.row(2, [], [], 0, -99, 0).dtype == np.int8 and EC.paired(2, [], [], 0).tolist() == [0, 0, 0, 0, 1, 0, 3]


@pytest.mark.parametrize("rows_p", (True, False))
def test_shape_rows(rows_p):
    n, kr, kc = 12, 7, 4
    rows = EC.shape_rows(n, kr, kc, rows_p, 5, seed=3)
    assert len(rows) == 5 and all(r.dtype == np.int8 and r.shape == (2 * n + 3,) for r in rows)
    for i, r in enumerate(rows):
        assert (int(r[0:2 * n:2].sum()), int(r[1:2 * n:2].sum())) == ((kr, kc) if rows_p else (kc, kr))
        assert r[2 * n:].tolist() == [1, i % 3, 3]
    other = EC.shape_rows(n, kr, kc, not rows_p, 5, seed=3)   # the same draws with the classes swapped
    for r, o in zip(rows, other):
        assert np.array_equal(r[0:2 * n:2], o[1:2 * n:2]) and np.array_equal(r[1:2 * n:2], o[0:2 * n:2])
    assert all(np.array_equal(a, b) for a, b in zip(rows, EC.shape_rows(n, kr, kc, rows_p, 5, seed=3)))


@pytest.mark.parametrize("rows_p", (True, False))
def test_shape_rows_with_fixed_events(rows_p):
    n, kr, kc = 31, 12, 7
    rows = EC.shape_rows(n, kr, kc, rows_p, 3, seed=71, fixed=((28, 30), (29, 30)))
    for i, r in enumerate(rows):
        pt, mt = r[0:2 * n:2], r[1:2 * n:2]
        rc, cc = (pt, mt) if rows_p else (mt, pt)
        assert int(rc.sum()) == kr and int(cc.sum()) == kc and r[2 * n:].tolist() == [1, i, 3]
        assert rc[[28, 29, 30]].tolist() == [1, 0, 1] and cc[[28, 29, 30]].tolist() == [0, 1, 1]


def test_random_generators_give_every_type_and_order():
    for rows, n in ((EC.random_rows(np.random.default_rng(1), 5, 200), 5), (EC.top_rows(np.random.default_rng(1), 60), 31)):
        dat = np.array(rows, dtype=np.int8)
        assert dat.shape == (len(rows), 2 * n + 3) and set(dat[:, -1]) == {0, 1, 2, 3}
        assert set(dat[dat[:, -1] == 3, -2]) == set(EC.ORDER_CODES) and set(dat[dat[:, -1] != 3, -2]) == {-99}
        assert not dat[dat[:, -1] < 2][:, 1:2 * n:2].any() and not dat[dat[:, -1] == 2][:, 0:2 * n:2].any()
        assert (dat[:, -3] == (dat[:, -1] != 0)).all()
    assert dat[:, :63].astype(int).sum(1).max() <= 12 and dat[:, -1].tolist() == [i % 4 for i in range(60)]


# ---------------------------------------------------------------------------------------------------- engines
class StandIn:
    """What the helpers use of an Engine, with the environment it was created under."""
    made = []

    def __init__(self, n, dtype="f64", workspace_bytes=None):
        self.n, self.dtype, self.workspace = n, dtype, workspace_bytes
        self.env = {k: os.environ.get(k) for k in ("MMHN_POISON", "MMHN_ZEROCOPY", "MMHN_WSOLVE", "MMHN_COOP")}
        self.closed, self.comm, self.fail = False, False, None
        StandIn.made.append(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        self.closed = True

    def set_cohort(self, dat):
        if dat is None:
            raise ValueError("no cohort")
        self.dat = dat

    def patient_grads(self, lt, dp, dm):
        if lt is None:
            raise RuntimeError("no parameters")
        return ("lp", "d_theta", "d_dp", "d_dm")

    def counters(self):
        return {"evals": 1}


@pytest.fixture
def stand_in(monkeypatch):
    StandIn.made = []
    monkeypatch.setattr(EC, "_engine", StandIn)
    monkeypatch.setattr(EC, "one_rank_comm", lambda e: setattr(e, "comm", True))
    monkeypatch.setenv("MMHN_ZEROCOPY", "7")                 # (the caller's own value comes back)
    monkeypatch.delenv("MMHN_POISON", raising=False)
    return StandIn


def test_engine_pool(stand_in):
    pool = EC.engine_pool()
    get = next(pool)
    a = get(4)
    assert get(4) is a and len(stand_in.made) == 1
    assert a.env["MMHN_POISON"] == "1" and a.env["MMHN_ZEROCOPY"] is None
    assert os.environ.get("MMHN_POISON") is None and os.environ["MMHN_ZEROCOPY"] == "7"     # set only while it is created
    b = get(4, zerocopy=False)
    assert b is not a and b.env["MMHN_ZEROCOPY"] == "0" and os.environ["MMHN_ZEROCOPY"] == "7"
    c = get(4, comm=True, dtype="f32", workspace=1 << 20)
    assert (c.comm, c.dtype, c.workspace, a.comm) == (True, "f32", 1 << 20, False)
    d = get(4, tag=1)
    assert len({id(x) for x in (a, b, c, d)}) == 4 and not any(x.closed for x in (a, b, c, d))
    assert get(4) is a                                       # a is now the most recently used, b the least
    e = get(5)
    assert b.closed and not any(x.closed for x in (a, c, d, e))
    a2 = get(4, fresh=True)
    assert a.closed and a2 is not a and get(4) is a2 and not any(x.closed for x in (c, d, e, a2))
    pool.close()
    assert all(x.closed for x in stand_in.made) and len(stand_in.made) == 6


def test_engine_pool_limit_and_poison(stand_in):
    pool = EC.engine_pool(limit=1, poison=False)
    get = next(pool)
    a = get(3)
    b = get(4)
    assert a.closed and not b.closed and a.env["MMHN_POISON"] is None
    with pytest.raises(StopIteration):
        next(pool)
    assert b.closed


def test_engines_by_n(stand_in):
    cache = EC.engines_by_n()
    get = next(cache)
    assert get(3) is get(3) and get(4) is not get(3) and len(stand_in.made) == 2
    cache.close()
    assert all(x.closed for x in stand_in.made)


def test_patient_grads_closes_its_engine(stand_in, monkeypatch):
    monkeypatch.setenv("MMHN_COOP", "0")
    with monkeypatch.context() as mp:
        got = EC.patient_grads(mp, 6, "dat", (1, 2, 3), dtype="f32", workspace=99, MMHN_WSOLVE="2", MMHN_COOP=None)
        assert os.environ["MMHN_WSOLVE"] == "2" and "MMHN_COOP" not in os.environ
    e = stand_in.made[-1]
    assert got == ("lp", "d_theta", "d_dp", "d_dm") and e.closed and (e.n, e.dtype, e.workspace, e.dat) == (6, "f32", 99, "dat")
    assert e.env["MMHN_WSOLVE"] == "2" and e.env["MMHN_COOP"] is None
    assert "MMHN_WSOLVE" not in os.environ and os.environ["MMHN_COOP"] == "0"
    got, counters = EC.patient_grads(monkeypatch, 6, "dat", (1, 2, 3), counters=True)
    assert got[0] == "lp" and counters == {"evals": 1} and stand_in.made[-1].closed
    with pytest.raises(ValueError, match="no cohort"):
        EC.patient_grads(monkeypatch, 6, None, (1, 2, 3))
    assert stand_in.made[-1].closed
    with pytest.raises(RuntimeError, match="no parameters"):
        EC.patient_grads(monkeypatch, 6, "dat", (None, 2, 3))
    assert stand_in.made[-1].closed and len(stand_in.made) == 4


def test_free_port():
    import socket
    port = EC.free_port()
    with socket.socket() as s:
        s.bind(("127.0.0.1", port))
