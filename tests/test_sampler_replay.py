"""The device Gillespie sampler (csrc/sampler.h: k_gillespie, k_gillespie_summary, gillespie_step) against an exact
replay of its documented random stream and step, oracle/sampler_replay.py: every trajectory event for event.

CPU part: the replay's Philox against the published Random123 answers, its distribution against the analytic
probabilities and oracle/gillespie.py (the bars of tests/test_montecarlo.py), its counts against host_counts of
tests/test_simulate_summary.py.  GPU part: dat, orders and summary counts of the device equal the replay's at
n_mut = 1 .. 30, three seeds (one with a high key word), indices past 2^32 and 2^40, and through the grid-stride
loop of the summary kernel.

Bit sets, event codes and counts are compared exactly.  Only `exp` can round differently on the two sides (<= 1 ulp
each), which moves a cumulative boundary by at most 62 x 2.2e-16 = 1.4e-14 of the total rate; a trajectory is set
aside iff the replay's own decision margin is <= 1e-11, and at most 1e-3 of a test's trajectories may be (expected:
2.5e-8 each).  Smallest margins measured on the CPU over the 4 001 trajectories of each case below, seeds 0 / 1234 /
0x9E37..15: random_params 7.6e-8 at n_mut = 8, 20 and 30; the stiff set 7.6e-8 at n_mut = 3, 8, 20 and 30 (the same
draw, u = (1 - 7.6e-8) total under seed 1234, against the last boundary), 2.2e-7 otherwise; the counter-word ranges
5.5e-9 (n_mut = 30 from 2^40 + 5).  Nothing was excluded anywhere.
"""
import numpy as np
import pytest

from metmhn_amd import synthetic
from oracle import sampler_replay as R
from sampler_common import N_SIM, cases, host_counts, sim  # noqa: F401  (sim: the module's parameters and NumPy samples)

MARGIN = 1e-11            # a trajectory whose closest draw is nearer than this to a boundary is not compared
MAX_EXCLUDED = 1e-3       # share of one test's trajectories that may be set aside
HIGH_SEED = 0x9E3779B97F4A7C15   # Engine.simulate takes the full uint64


def stiff_params(n_mut):
    """Rates over four orders of magnitude and strong, sparse effects: diag U[-8, 2], 30 % off-diagonals N(0, 1.5),
    dp / dm N(0, 1).  The generator's seed is one for which 20 - 75 % of the trajectories seed at every size used here
    (most seeds leave the seeding's base rate so low that the MT half of the kernel would hardly run)."""
    rng = np.random.default_rng(9700 + n_mut)
    N = n_mut + 1
    lt = np.diag(rng.uniform(-8.0, 2.0, size=N))
    off = rng.random((N, N)) < 0.3
    np.fill_diagonal(off, False)
    lt = lt + off * rng.normal(0.0, 1.5, size=(N, N))
    return lt, rng.normal(0.0, 1.0, size=N), rng.normal(0.0, 1.0, size=N)


PARAMS = {"random": synthetic.random_params, "stiff": stiff_params}


def kept(rep, what):
    """The trajectories that are compared; prints the exclusions and the smallest margin, asserts the cap."""
    keep = rep.margin > MARGIN
    n_ex = int((~keep).sum())
    print(f"{what}: {n_ex} of {keep.size} trajectories excluded, smallest margin {rep.margin.min():.3e}")
    assert n_ex <= MAX_EXCLUDED * keep.size, (n_ex, keep.size)
    return keep


def explain(params, ids, seed, rep, dat, orders, keep):
    """The first step of the first compared trajectory at which device and replay part, for the assertion message."""
    bad = np.nonzero(keep & ((orders != rep.orders).any(axis=1) | (dat != rep.dat).any(axis=1)))[0]
    if bad.size == 0:
        return ""
    row = int(bad[0])
    one = R.replay(*params, ids[row:row + 1], seed, trace=True)
    diff = np.nonzero(orders[row] != rep.orders[row])[0]
    step = int(diff[0]) if diff.size else 0
    return (f"{bad.size} trajectories differ; first: id {int(ids[row])}, step {step}: device event {orders[row, step]}, "
            f"replay event {rep.orders[row, step]}\ndevice orders {orders[row]}\nreplay orders {rep.orders[row]}\n"
            f"device dat {dat[row]}\nreplay dat {rep.dat[row]}\nreplay " + R.describe_step(one, 0, min(step, len(one.trace) - 1)))


# ---------------------------------------------------------------------------------------------- the oracle itself

def test_philox_known_answers():
    """Random123's published known answers for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, out in kat:
        assert tuple(int(v) for v in R.philox4x32_10(*ctr, *key)) == out
    ctr = np.array([k[0] for k in kat], dtype=np.uint64).T          # vectorised: the three at once
    key = np.array([k[1] for k in kat], dtype=np.uint64).T
    got = np.stack(R.philox4x32_10(*ctr, *key), axis=1)
    np.testing.assert_array_equal(got, np.array([k[2] for k in kat], dtype=np.uint64))
    assert R.uniform53(np.uint64(0xffffffff), np.uint64(0xffffffff)) == 1.0 - 2.0 ** -53
    assert R.uniform53(np.uint64(0x20), np.uint64(0)) == 2.0 ** -27 and R.uniform53(np.uint64(0), np.uint64(0x40)) == 2.0 ** -53


@pytest.fixture(scope="module")
def replayed(sim):  # noqa: F811
    lt, dp, dm, _ = sim
    return R.replay(lt, dp, dm, np.arange(N_SIM), 2024)


def test_replay_matches_analytic_probabilities(sim, replayed):  # noqa: F811
    """The nine rows of sampler_common.cases: replayed frequency against the oracle's probability, 4.5 sigma."""
    from oracle import metmhn_oracle as O
    lt, dp, dm, _ = sim
    for name, row, count in cases(replayed.dat):
        p = float(np.exp(O.score(lt, dp, dm, np.array([row], dtype=np.int8), 0)))
        sigma = np.sqrt(p * (1 - p) / N_SIM)
        assert count >= 25, f"{name}: too few samples ({count})"
        assert abs(count / N_SIM - p) < 4.5 * sigma, f"{name}: replayed {count / N_SIM:.5f} vs analytic {p:.5f}"


def test_replay_matches_numpy_sampler(sim, replayed):  # noqa: F811
    """Two-sample check against oracle/gillespie.py, every (genotype, order) row with pooled count >= 200: 5 sigma."""
    a, b = sim[3], replayed.dat
    assert a.shape == b.shape and b.dtype == np.int8
    keys = lambda d: (d.astype(np.int64) * (3 ** np.arange(d.shape[1]))).sum(axis=1)
    da, db = (dict(zip(*np.unique(keys(d), return_counts=True))) for d in (a, b))
    worst, n_rows = 0.0, 0
    for k in set(da) | set(db):
        x, y = int(da.get(k, 0)), int(db.get(k, 0))
        if x + y < 200:
            continue
        p = (x + y) / (2 * N_SIM)
        worst = max(worst, abs(x - y) / np.sqrt(2 * N_SIM * p * (1 - p)))
        n_rows += 1
    assert n_rows > 20 and worst < 5.0, (n_rows, worst)


@pytest.mark.parametrize("n_mut, n_sim", [(3, 20_000), (30, 3_000)])
def test_replay_counts_equal_host_reductions(n_mut, n_sim):
    """counts of the replay = the reference's reductions (extract_bse / preseeding_probs) of its own dat and orders."""
    lt, dp, dm = synthetic.random_params(n_mut)
    rep = R.replay(lt, dp, dm, np.arange(n_sim), 1234)
    assert rep.counts.dtype == np.int64 and rep.counts.shape == (4 + 5 * n_mut,)
    np.testing.assert_array_equal(rep.counts, host_counts(rep.dat, rep.orders, n_mut))
    assert 0 < rep.counts[1] < n_sim and rep.counts[4:4 + n_mut].sum() > 0
    assert rep.orders.shape == (n_sim, 2 * n_mut + 4) and np.isfinite(rep.margin).all() and (rep.margin >= 0).all()


# ---------------------------------------------------------------------------------------------- device = replay

_engines = {}


def engine(n_mut):
    from metmhn_amd import Engine
    if n_mut not in _engines:
        _engines[n_mut] = Engine(n_mut)
    return _engines[n_mut]


def assert_reaches_the_edges(rep, n_mut):
    """The inputs exercise bit 31 of the state sets, both diagnosis codes and both kinds of trajectory."""
    N = n_mut + 1
    d, od = rep.dat, rep.orders
    assert d[:, 0:2 * n_mut:2].any(axis=0).all() and d[:, 1:2 * n_mut:2].any(axis=0).all()   # every mutation, PT and MT
    assert (od == N).any() and (od == 2 * N + 1).any()              # both diagnosis flags (bit N of either set)
    assert od.max() == 2 * N + 1 == 2 * n_mut + 3
    seeded = d[:, -2].mean()
    assert 0.1 <= seeded <= 0.9, seeded
    for lo, hi in ((16, N), (N + 1 + 16, 2 * N + 1)):               # events above bit 15, in either tumour
        assert ((od >= lo) & (od < hi)).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "stiff"])
@pytest.mark.parametrize("seed", [0, 1234, HIGH_SEED])
@pytest.mark.parametrize("n_mut", [1, 3, 8, 20, 30])
def test_device_trajectories_equal_replay(n_mut, seed, kind):
    n_sim = 4001                                                    # the last workgroup is partly filled
    params = PARAMS[kind](n_mut)
    ids = np.arange(n_sim)
    rep = R.replay(*params, ids, seed)
    assert 0.1 <= rep.dat[:, -2].mean() <= 0.9                      # seeded and unseeded, at least 10 % each
    if n_mut == 30 and kind == "random":                            # (the stiff set's slowest mutations never fire)
        assert_reaches_the_edges(rep, n_mut)
    e = engine(n_mut)
    dat, orders = e.simulate(*params, n_sim, seed, orders=True)
    counts = e.simulate_summary(*params, n_sim, seed)
    keep = kept(rep, f"n_mut {n_mut} seed {seed:#x} {kind}")
    assert dat.shape == rep.dat.shape and orders.shape == rep.orders.shape and dat.dtype == orders.dtype == np.int8
    msg = explain(params, ids, seed, rep, dat, orders, keep)
    np.testing.assert_array_equal(orders[keep], rep.orders[keep], err_msg=msg)
    np.testing.assert_array_equal(dat[keep], rep.dat[keep], err_msg=msg)
    assert keep.all()                                               # these seeds exclude nothing: the counts are exact
    np.testing.assert_array_equal(counts, rep.counts)


def key_to_seed(key):
    """The documented fold of `original_key` into the 64-bit Philox key, in Python integers."""
    s, M = 0x9E3779B97F4A7C15, 2 ** 64 - 1
    for v in np.atleast_1d(key).ravel():
        s = ((s ^ int(v)) * 0xBF58476D1CE4E5B9) & M
        s ^= s >> 31
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("key", [1234, (7, 2 ** 40 + 3)])
def test_python_layer_equals_replay(key):
    """simulations.simulate_dat / simulate_orders / simulate_summary: the key-to-seed mapping and the call surface."""
    from metmhn_amd import simulations as S
    n_mut, n_sim = 8, 4001
    params = synthetic.random_params(n_mut)
    seed = key_to_seed(key)
    assert seed >> 32 and seed == S._seed(key)
    rep = R.replay(*params, np.arange(n_sim), seed)
    keep = kept(rep, f"key {key}")
    np.testing.assert_array_equal(S.simulate_dat(*params, n_sim, key)[keep], rep.dat[keep])
    np.testing.assert_array_equal(S.simulate_orders(*params, n_sim, key)[keep], rep.orders[keep])
    assert keep.all()
    np.testing.assert_array_equal(S.simulate_summary(*params, n_sim, key).counts, rep.counts)
    first = 2 ** 33 + 17
    part = R.replay(*params, first + np.arange(1500, dtype=np.uint64), seed)
    assert kept(part, f"key {key} first {first}").all()
    np.testing.assert_array_equal(S.simulate_summary(*params, 1500, key, first=first).counts, part.counts)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [2 ** 32 - 1000, 2 ** 40 + 5])
@pytest.mark.parametrize("n_mut", [8, 30])
def test_counter_words(n_mut, first):
    """Both 32-bit words of the trajectory index reach the Philox counter: ranges that cross 2^32 and lie past 2^40."""
    n_sim, seed = 2000, 1234
    params = synthetic.random_params(n_mut)
    ids = np.uint64(first) + np.arange(n_sim, dtype=np.uint64)
    rep = R.replay(*params, ids, seed)
    assert kept(rep, f"n_mut {n_mut} first {first}").all()
    e = engine(n_mut)
    counts = e.simulate_summary(*params, n_sim, seed, first=first)
    np.testing.assert_array_equal(counts, rep.counts)
    low = R.replay(*params, ids & np.uint64(0xFFFFFFFF), seed)      # what a dropped high word would draw
    assert (counts != low.counts).any()
    assert (counts != e.simulate_summary(*params, n_sim, seed)).any()
    if first >= 2 ** 32:
        assert (counts != e.simulate_summary(*params, n_sim, seed, first=first % 2 ** 32)).any()


@pytest.mark.gpu
def test_summary_grid_stride_loop(monkeypatch):
    """One launch of k_gillespie_summary covers 8 x CUs x 256 samples per pass; more than two passes here."""
    import torch
    from metmhn_amd import Engine
    n_mut, seed = 3, 1234
    params = synthetic.random_params(n_mut)
    one_pass = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256
    n_sim = max(700_000, 2 * one_pass + 1234)
    assert n_sim > one_pass
    e = engine(n_mut)
    whole = e.simulate_summary(*params, n_sim, seed)
    assert whole[0] == n_sim
    piece = min(100_000, one_pass)                                  # each of these calls is a single pass
    parts = sum(e.simulate_summary(*params, min(piece, n_sim - f), seed, first=f) for f in range(0, n_sim, piece))
    np.testing.assert_array_equal(whole, parts)
    for first in (0, one_pass + 4321):                              # one slice in the first pass, one past it
        assert first + 20_000 <= n_sim
        rep = R.replay(*params, first + np.arange(20_000), seed)
        assert kept(rep, f"slice at {first}").all()
        np.testing.assert_array_equal(e.simulate_summary(*params, 20_000, seed, first=first), rep.counts)
    chunk = n_sim - 100_001                                         # two launches: one that loops, one that does not
    chunk -= chunk % 256 == 0
    assert one_pass < chunk < n_sim and chunk % 256
    monkeypatch.setenv("MMHN_SIM_CHUNK", str(chunk))
    np.testing.assert_array_equal(Engine(n_mut).simulate_summary(*params, n_sim, seed), whole)
